"""Plain restatement of forced target prefixes (include/ttx.h: "Forced target prefixes"; csrc/ttx_sample.hip.h: k_prefix_drafts and
the forced position of k_sample / k_sample_step) for the tests, built on tests/util_sample_spec.py and tests/util_sample_pool.py.  No
GPU call and no test in here.  tests/test_prefix_host.py shows on the CPU that the restatement, driven through the restated loop and
the restated pool, returns position-by-position sampling with the same positions forced, and that the checker flags each single
defect; the GPU modules hold the kernels to it.

The rules are restated from the contract in include/ttx.h, in NumPy, not from the kernels.

  Prefixes           the table [sources, ld], the sources' lengths, and the row (slot) -> source map of a loop
  prefix_drafts      k_prefix_drafts: draft 0 of every active row for the step that starts at the rows' fronts
  force_pred         the forced position: the draws of a step with the prefix tokens where the position lies inside the prefix
  force_logits       a host model whose forced positions can only emit the prefix token (for util_sample_spec.sequential)
  sequential         util_sample_spec.sequential on that model: what every prompted call has to return
  run_loop, run_pool util_sample_spec.run_loop and util_sample_pool.run_pool, prompted
"""
from __future__ import annotations

import numpy as np

import util_loop_checks as U
import util_sample_checks as S
import util_sample_pool as P
import util_sample_spec as X

PAD, BOS, EOS = U.PAD, U.BOS, U.EOS
REPL = 3                                   # the replace token of the host loops (util_loop_checks' drafts hold tokens >= 3)


class Prefixes:
    """``table`` int [sources, ld] (columns at or beyond a source's length hold anything), ``length`` int [sources]."""

    def __init__(self, table, length):
        self.table = np.asarray(table, dtype=np.int64)
        self.length = np.asarray(length, dtype=np.int64)
        assert self.table.ndim == 2 and self.length.shape == (self.table.shape[0],)
        assert (self.length >= 0).all() and (self.length <= self.table.shape[1]).all()

    @classmethod
    def of_rows(cls, rows, ld: int | None = None) -> "Prefixes":
        """From a list of token lists (without BOS)."""
        ld = max([len(r) for r in rows] + [1]) if ld is None else ld
        t = np.full((len(rows), ld), PAD, dtype=np.int64)
        for i, r in enumerate(rows):
            t[i, :len(r)] = r
        return cls(t, [len(r) for r in rows])

    def token(self, src: int, pos: int, V: int | None = None) -> int:
        """The forced token of position ``pos`` (1-based, pos <= length[src]); an id outside [0, V) is emitted as 0."""
        t = int(self.table[src, pos - 1])
        return t if V is None or 0 <= t < V else 0


def prefix_drafts(drafts: np.ndarray, draft0: np.ndarray, act_idx, n_active: int, front, pre: Prefixes, src_of, eos: int = EOS,
                  pad: int = PAD, repl: int = REPL) -> np.ndarray:
    """k_prefix_drafts.  drafts [B, N, D] -> a copy in which, for every active row b = act_idx[slot], slot < n_active, and
    j = 0 .. D-1, draft 0's token j is: with c = front[b] + 1 + j, the prefix token of column c if c <= length (EOS and PAD as
    ``repl``), else draft0[b, j], the row's own source draft 0.  Nothing else changes; ``src_of`` [B] maps rows to sources."""
    out = np.array(drafts, copy=True)
    D = out.shape[2]
    for slot in range(n_active):
        b = int(act_idx[slot])
        s, f = int(src_of[b]), int(front[b])
        for j in range(D):
            c = f + 1 + j
            if c <= pre.length[s]:
                t = int(pre.table[s, c - 1])
                out[b, 0, j] = repl if t in (eos, pad) else t
            else:
                out[b, 0, j] = draft0[b, j]
    return out


def force_pred(pred: np.ndarray, b: np.ndarray, pos: np.ndarray, pre: Prefixes, src_of, V: int | None = None) -> np.ndarray:
    """The forced position on the draws of a step: row i (decoder row b[i], predicting position pos[i]) holds the prefix token when
    pos[i] <= the length of the row's source, else what it held.  Rows beyond len(b) stay."""
    out = np.array(pred, copy=True)
    for i in range(len(b)):
        s = int(src_of[int(b[i])])
        if pos[i] <= pre.length[s]:
            out[i] = pre.token(s, int(pos[i]), V)
    return out


def force_logits(logits_of, pre: Prefixes, src_of_row=lambda r: r):
    """logits(r, prefix) of a host model whose forced positions can emit the prefix token alone (every other logit -inf), so that
    util_sample_spec.sequential, which samples every position, emits it there whatever the uniform is.  The position being
    sampled is len(prefix) (prefix holds BOS)."""
    def forced(r, prefix):
        s, pos = src_of_row(r), len(prefix)
        x = logits_of(r, prefix)
        if pos <= pre.length[s]:
            y = np.full(len(x), -np.inf)
            y[pre.token(s, pos, len(x))] = 0.0
            return y
        return x
    return forced


def sequential(B: int, max_len: int, logits_of, key, sample, seed: int, p: S.Params, pre: Prefixes, src_of_row=lambda r: r) -> np.ndarray:
    """Position-by-position sampling with the prefix positions forced: what every prompted call has to return."""
    return X.sequential(B, max_len, force_logits(logits_of, pre, src_of_row), key, sample, seed, p)


def run_loop(drafts: np.ndarray, max_len: int, logits_of, key, sample, seed: int, p: S.Params, pre: Prefixes, src_of=None,
             drafts_fn=prefix_drafts, force_fn=force_pred, steps: list | None = None) -> U.LoopState:
    """util_sample_spec.run_loop, prompted: draft 0 of every active row is rewritten before every step (before the first one here,
    after every accept step through the loop's ``step_fn`` hook: the rewrite is stateless, so that is the head of the next step), and
    the step's draws pass through the forced position before the accept step, whose rule is untouched."""
    B = drafts.shape[0]
    src_of = np.arange(B) if src_of is None else np.asarray(src_of)
    draft0 = np.array(drafts[:, 0, :], copy=True)
    first = drafts_fn(drafts, draft0, np.arange(B), B, np.zeros(B, dtype=np.int64), pre, src_of)

    def step(s, pred):
        n = int(s.words["n_active"])
        b, pos = X.step_rows(s.act_idx, s.front, n, s.N, s.D)
        t = X.sample_accept_step(s, force_fn(pred, b, pos, pre, src_of))
        if steps is not None:
            steps.append(n)
        t.drafts = drafts_fn(t.drafts, draft0, t.act_idx, int(t.words["n_active"]), t.front, pre, src_of)
        return t
    return X.run_loop(first, max_len, logits_of, key, sample, seed, p, step_fn=step)


def run_pool(src_drafts: np.ndarray, keys, n: int, C: int, max_len: int, logits_of, seed: int, p: S.Params, pre: Prefixes,
             sub_chunk: int = 0, drafts_fn=prefix_drafts, force_fn=force_pred, by_slot: bool = False) -> np.ndarray:
    """util_sample_pool.run_pool, prompted.  A slot's source is what the pool hands the host model for the slot's rows (its
    ``logits_of`` is called row by row, in order, with the source of the row's slot), which is how the hooks learn it: the pool
    itself knows nothing of prefixes.  New slots start from their source's draft 0 rewritten for front 0 (the prefix and the source
    draft are both the source's); after every accept step draft 0 of the rows that go on is rewritten for the next step.
    ``by_slot``: the defect of indexing the prefix by slot instead of source."""
    S_total, N, D = src_drafts.shape
    R = U.rps(N, D)
    first = np.array(src_drafts, copy=True)
    for s in range(S_total):
        one = drafts_fn(src_drafts[s:s + 1], src_drafts[s:s + 1, 0, :], np.zeros(1, dtype=np.int64), 1, np.zeros(1, dtype=np.int64), pre,
                        np.array([s]))
        first[s] = one[0]
    seen = []                                          # the sources of the rows of the step being drawn, in row order

    def model(src, prefix):
        seen.append(int(src))
        return logits_of(src, prefix)

    def accept(st, pred):
        n_act = int(st.words["n_active"])
        assert len(seen) == n_act * R
        src_of = np.zeros(st.B, dtype=np.int64)
        for slot in range(n_act):
            src_of[int(st.act_idx[slot])] = slot if by_slot else seen[slot * R]
        seen.clear()
        b, pos = X.step_rows(st.act_idx, st.front, n_act, N, D)
        t = X.sample_accept_step(st, force_fn(pred, b, pos, pre, src_of))
        draft0 = np.stack([src_drafts[min(int(s), S_total - 1), 0] for s in src_of])
        t.drafts = drafts_fn(t.drafts, draft0, t.act_idx, int(t.words["n_active"]), t.front, pre, src_of)
        st.drafts[...] = t.drafts                      # the pool keeps its own drafts array: the one this state was built on
        return t
    return P.run_pool(first, keys, n, C, max_len, model, seed, p, sub_chunk=sub_chunk, accept_fn=accept)

