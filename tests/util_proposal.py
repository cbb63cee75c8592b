"""Plain restatement of proposal drafts (include/ttx.h: "Proposal drafts"; csrc/ttx_proposal.hip.h: k_proposal_drafts) for the tests,
built on tests/util_prefix.py, tests/util_sample_spec.py and tests/util_sample_pool.py.  No GPU call and no test in here.
tests/test_proposal_host.py shows on the CPU that the restatement, driven through the restated loop and the restated pool, returns
position-by-position sampling whatever the proposals hold, that perfect proposals meet the step bound, and that the checker flags
each single defect; the GPU modules hold the kernel to it.

The rule is restated from the contract in include/ttx.h, in NumPy, not from the kernel.

  Proposals          util_prefix.Prefixes: the table [sources, ld], the sources' lengths
  agreement          c(d) of one row for one shift
  choose_shift       the eligible shift with the largest c, ties to the smaller |d|, then to d >= 0; None when none is eligible
  proposal_drafts    k_proposal_drafts: draft 0 of every active row for the step that starts at the rows' fronts
  run_loop, run_pool util_sample_spec.run_loop and util_sample_pool.run_pool, proposed: nothing is forced
  perturbed          a proposal with one substitution, insertion or deletion
"""
from __future__ import annotations

import numpy as np

import util_loop_checks as U
import util_prefix as F
import util_sample_checks as S
import util_sample_pool as P
import util_sample_spec as X

PAD, BOS, EOS = U.PAD, U.BOS, U.EOS
REPL = F.REPL
CTX = 2                                    # context tokens compared per shift (the library's PROPOSAL_CTX)
SHIFTS = range(-32, 32)                    # one lane of a wave per shift: d = lane - 32
Proposals = F.Prefixes


def agreement(g, f: int, q, length: int, d: int, ctx: int = CTX, bos: int = BOS) -> int:
    """c(d): the number of a in 0 .. ctx-1 with f - a >= 0, -1 <= f-1-a+d < length and q[f-1-a+d] == g[f-a], where q[-1] = BOS."""
    c = 0
    for a in range(ctx):
        i = f - 1 - a + d
        if f - a >= 0 and -1 <= i < length:
            c += int((bos if i == -1 else int(q[i])) == int(g[f - a]))
    return c


def choose_shift(g, f: int, q, length: int, ctx: int = CTX, bos: int = BOS):
    """The shift of a row with tokens g[0 .. f] and proposal q[0 .. length-1], or None: among the shifts with c(d) >= 1 and
    0 <= f + d < length the one with the largest c; ties go to the smaller |d|, then to d >= 0."""
    best = None
    for d in SHIFTS:
        c = agreement(g, f, q, length, d, ctx, bos)
        if c >= 1 and 0 <= f + d < length:
            rank = (c, -abs(d), 1 if d >= 0 else 0)
            if best is None or rank > best[0]:
                best = (rank, d)
    return None if best is None else best[1]


def proposal_drafts(drafts: np.ndarray, draft0: np.ndarray, act_idx, n_active: int, front, gen: np.ndarray, prop: Proposals, src_of,
                    ctx: int = CTX, bos: int = BOS, eos: int = EOS, pad: int = PAD, repl: int = REPL) -> np.ndarray:
    """k_proposal_drafts.  drafts [B, N, D] -> a copy in which, for every active row b = act_idx[slot], slot < n_active, draft 0 is:
    with d the row's shift, token j = q[front + d + j] while that index is below the proposal's length (EOS and PAD as ``repl``),
    else draft0[b, j]; draft0[b] whole when no shift is eligible.  ``gen`` [B, >= front + 1] holds the rows' tokens, ``src_of`` [B]
    maps rows to sources.  Nothing else changes."""
    out = np.array(drafts, copy=True)
    D = out.shape[2]
    for slot in range(n_active):
        b = int(act_idx[slot])
        s, f = int(src_of[b]), int(front[b])
        q, length = prop.table[s], int(prop.length[s])
        d = choose_shift(gen[b], f, q, length, ctx, bos)
        for j in range(D):
            i = length if d is None else f + d + j
            if i < length:
                t = int(q[i])
                out[b, 0, j] = repl if t in (eos, pad) else t
            else:
                out[b, 0, j] = draft0[b, j]
    return out


def run_loop(drafts: np.ndarray, max_len: int, logits_of, key, sample, seed: int, p: S.Params, prop: Proposals, src_of=None,
             drafts_fn=proposal_drafts, steps: list | None = None, ctx: int = CTX) -> U.LoopState:
    """util_sample_spec.run_loop, proposed: draft 0 of every active row is rewritten before every step (before the first one here,
    after every accept step through the loop's ``step_fn`` hook: the rewrite is stateless, so that is the head of the next step).
    The draws and the accept step are the unproposed loop's."""
    B = drafts.shape[0]
    src_of = np.arange(B) if src_of is None else np.asarray(src_of)
    draft0 = np.array(drafts[:, 0, :], copy=True)
    gen0 = np.full((B, 1), BOS, dtype=np.int64)
    first = drafts_fn(drafts, draft0, np.arange(B), B, np.zeros(B, dtype=np.int64), gen0, prop, src_of, ctx=ctx)

    def step(s, pred):
        if steps is not None:
            steps.append(int(s.words["n_active"]))
        t = X.sample_accept_step(s, pred)
        t.drafts = drafts_fn(t.drafts, draft0, t.act_idx, int(t.words["n_active"]), t.front, t.gen, prop, src_of, ctx=ctx)
        return t
    return X.run_loop(first, max_len, logits_of, key, sample, seed, p, step_fn=step)


def run_pool(src_drafts: np.ndarray, keys, n: int, C: int, max_len: int, logits_of, seed: int, p: S.Params, prop: Proposals,
             sub_chunk: int = 0, drafts_fn=proposal_drafts, ctx: int = CTX) -> np.ndarray:
    """util_sample_pool.run_pool, proposed, as util_prefix.run_pool is prompted: a slot's source is what the pool hands the host
    model for the slot's rows; new slots start from their source's draft 0 rewritten for front 0, and after every accept step draft
    0 of the rows that go on is rewritten for the next step."""
    S_total, N, D = src_drafts.shape
    R = U.rps(N, D)
    first = np.array(src_drafts, copy=True)
    bos_row = np.full((1, 1), BOS, dtype=np.int64)
    for s in range(S_total):
        one = drafts_fn(src_drafts[s:s + 1], src_drafts[s:s + 1, 0, :], np.zeros(1, dtype=np.int64), 1, np.zeros(1, dtype=np.int64),
                        bos_row, prop, np.array([s]), ctx=ctx)
        first[s] = one[0]
    seen = []

    def model(src, prefix):
        seen.append(int(src))
        return logits_of(src, prefix)

    def accept(st, pred):
        n_act = int(st.words["n_active"])
        assert len(seen) == n_act * R
        src_of = np.zeros(st.B, dtype=np.int64)
        for slot in range(n_act):
            src_of[int(st.act_idx[slot])] = seen[slot * R]
        seen.clear()
        t = X.sample_accept_step(st, pred)
        draft0 = np.stack([src_drafts[min(int(s), S_total - 1), 0] for s in src_of])
        t.drafts = drafts_fn(t.drafts, draft0, t.act_idx, int(t.words["n_active"]), t.front, t.gen, prop, src_of, ctx=ctx)
        st.drafts[...] = t.drafts                      # the pool keeps its own drafts array: the one this state was built on
        return t
    return P.run_pool(first, keys, n, C, max_len, model, seed, p, sub_chunk=sub_chunk, accept_fn=accept)


def row_tokens(row, pad: int = PAD, eos: int = EOS) -> list:
    """The proposal a finished output row makes: its tokens behind BOS up to and including the first EOS (or PAD, excluded)."""
    out = []
    for t in [int(x) for x in row[1:]]:
        if t == pad:
            break
        out.append(t)
        if t == eos:
            break
    return out


def perturbed(tokens: list, kind: str, at: int, other: int) -> list:
    """``tokens`` with one edit at index ``at``: "sub" replaces the token by ``other``, "ins" inserts ``other`` before it, "del"
    removes it.  ``at`` is clipped into the list; an empty list stays empty (or receives the insertion)."""
    t = list(tokens)
    if not t:
        return [other] if kind == "ins" else t
    at = min(max(at, 0), len(t) - 1)
    if kind == "sub":
        t[at] = other
    elif kind == "ins":
        t.insert(at, other)
    elif kind == "del":
        del t[at]
    else:
        raise ValueError(kind)
    return t
