"""Plain restatement of the bookkeeping kernels of the beam-speculative batch pool (csrc/ttx_loop_kernels.hip.h "Beam-speculative
BATCH POOL": k_bsp_init, k_bsp_admit, k_bsp_fill, k_bsp_prep, k_bsp_select, k_bsp_batches, k_bsp_retire, k_bsp_publish), a synthetic
stand-in for the verify step, a per-batch loop written from the reference's scalars, and the driver that chains the eight rules
over a work list.  No GPU call in here: tests/test_bsp_checks_host.py shows that the chained restatement gives what the per-batch
loop gives, that the scenarios reach the branches a trained model seldom reaches, and that the checker can fail;
tests/test_gpu_bsp_kernels.py holds the kernels to the restatement, one launch at a time (ttx_debug_bsp).

A State is every array of the kernels' argument block (BeamPoolArgs, the caller-side arrays of BeamPoolIo, the operands of init /
admit / fill), by the kernels' names, plus the 12 words of ttx_debug_bsp (8 BeamCounters, then steps_done, n_live, n_running, error
of BeamPoolHost).  Each rule maps a State to the State its launch leaves behind; a State that starts sentinel-filled (blank) keeps
the sentinel wherever no rule wrote.  Every output of this family is an integer, a flag or a bit copy (logp_next is a leaf's own
score), so `compare` is bit equality of everything.

The rules, from the kernels' header comment and the reference (src/decoding/speculative_decoding.py):
  * a given batch is admitted as a whole, into the lowest free source slots and the lowest free batch slot; its draft length
    starts at min(D0, max_len - 2) (:457, :476 with one <BOS> column);
  * in a batch's first iteration a source has ONE candidate, afterwards K (:447-459); a slot without a source is dead;
  * smart mode: the library of a source is every stride-1 window of D0 + 1 tokens of its row padded to the GIVEN width, given - 5
    of them (:603-615), EOS / PAD replaced; a candidate takes the first N windows that start with its last token, window 0 if
    there is none (:417-419); the batch's group width is the largest count among its candidates (:779-784), a finished source
    counting 1;
  * the K best leaves of a source, best first, equal scores in enumeration order (util_beam_checks.best_leaves); fewer than K
    raise for the whole batch (:195 of the sampler);
  * after an iteration: longest row of the batch (finished sources included), room = max_len - longest - 1 (:596), the loop ends
    when room < 1 (:464) or every row holds EOS (:586, per source here: a finished source is a fixed point), the next draft
    length is min(room, draft length) (:476); max_steps is the library's guard;
  * a source whose K rows hold EOS retires at once; a running one follows its batch.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

import util_beam_checks as B
import util_loop_checks as U

PAD, BOS, EOS = U.PAD, U.BOS, U.EOS
REPL = 4
I16, I32, I64, F32, U8 = np.int16, np.int32, np.int64, np.float32, np.uint8
RUNNING, DONE, ERR_LEAVES, STOPPED, MAX_STEPS = 0, 1, 2, 3, 4           # BeamPoolStatus
OPS = ("init", "admit", "fill", "prep", "select", "batches", "retire", "publish")
CNT_WORDS, HOST_WORDS = 8, 4                                             # ttx_debug_bsp's words: BeamCounters, then BeamPoolHost
W_CALLS, W_STEPS, W_LIVE, W_RUNNING, W_ERROR = 0, 8, 9, 10, 11


def params(*, C, K, N, D0, Ls_cap, max_len, smart, T_cap, max_steps=0, ld=None) -> NS:
    return NS(C=C, K=K, N=N, D0=D0, Ls_cap=Ls_cap, max_len=max_len, ld=max_len + D0 + 2 if ld is None else ld, smart=int(bool(smart)),
              lib_ld=D0 + 1, pad=PAD, bos=BOS, eos=EOS, repl=REPL, max_steps=max_steps, T_cap=T_cap)


def scalars(p) -> dict:
    """The int32 scalars of ttx_debug_bsp_args that every op takes, as NativeTransformer.debug_bsp names them."""
    return dict(C_=p.C, K=p.K, n=p.N, D0=p.D0, Ls_cap=p.Ls_cap, max_len=p.max_len, ld=p.ld, smart=p.smart, lib_ld=p.lib_ld, pad=p.pad,
                bos=p.bos, eos=p.eos, repl=p.repl, max_steps=p.max_steps, T_cap=p.T_cap)


def shapes(p, rows: int, batches: int, kv_row: int) -> dict:
    """name -> (shape, dtype) of every array of a State."""
    C, K, MC, dl1 = p.C, p.K, p.C * p.K, p.D0 + 1
    s = {k: ((C,), I32) for k in ("row_of", "slot_batch", "src_state", "bat_id", "bat_iter", "bat_dl", "bat_grp", "bat_live", "bat_nfin",
                                  "bat_longest_fin", "bat_longest_cur", "bat_state", "bat_given", "new_slot")}
    s.update({k: ((MC,), I32) for k in ("len_next", "parent", "parent_draft", "front", "len", "per_cand", "cand_dl", "cand_batch",
                                        "cache_slot", "cache_slot_parent", "chosen_slot", "src_of", "cand_src_len")})
    s.update({k: ((MC,), U8) for k in ("fin_next", "active", "finished", "live")})
    s.update({k: ((MC,), F32) for k in ("logp_next", "logp")})
    s.update(src_acc=((C, 8), I32), tok=((C, p.Ls_cap), I32), drafts_all=((C, p.N, p.D0), I32), cand_next=((MC, p.ld), I64),
             gen=((MC, p.ld), I32), drafts32=((MC, p.N, p.D0), I32), chosen=((MC, p.D0), I64), leaf_score=((MC, dl1, K), F32),
             leaf_tok=((MC, dl1, K), I32), leaf_cnt=((MC, dl1), I32), dev_summary=((4,), I32),
             out=((rows, K, p.max_len), I64), trace_len=((rows, p.T_cap), I16), summary=((rows, 8), I32), len_all=((rows,), I32),
             batch_all=((rows,), I32), given_all=((batches,), I32), src_valid=((C, p.Ls_cap), U8), memkv=((C, p.Ls_cap, kv_row), F32))
    return s


STAGED = ("tok_new", "valid_new", "drafts_new", "memkv_new")             # the operands of one admission: not part of a State
STEP_OUT = ("chosen_slot", "chosen", "leaf_score", "leaf_tok", "leaf_cnt")      # what the verify step leaves for k_bsp_select


class State:
    def __init__(self, p, a: dict, words):
        self.p, self.a, self.w = p, a, [int(v) for v in words]

    def copy(self) -> "State":
        return State(self.p, {k: v.copy() for k, v in self.a.items()}, list(self.w))


def blank(p, rows: int, batches: int, kv_row: int = 128, words=None) -> State:
    """Every array sentinel-filled; the words hold values no rule produces."""
    a = {k: B.sent(shape, dt) for k, (shape, dt) in shapes(p, rows, batches, kv_row).items()}
    return State(p, a, [-3 - i for i in range(CNT_WORDS + HOST_WORDS)] if words is None else words)


def compare(got_arrays: dict, got_words, want: State, what: str) -> None:
    B.check_exact({k: got_arrays[k] for k in want.a}, want.a, what)
    assert [int(v) for v in got_words] == want.w, f"{what}: words {list(got_words)} expected {want.w}"


# ---------------------------------------------------------------------------------------------------------------------------
# the eight rules
def init(S: State) -> State:
    S = S.copy()
    p, a = S.p, S.a
    for k in ("slot_batch", "src_state", "bat_iter", "bat_grp", "bat_live", "bat_nfin", "bat_longest_fin", "bat_longest_cur", "bat_state",
              "bat_given", "src_acc", "parent_draft", "active", "live", "per_cand", "cand_batch", "dev_summary"):
        a[k][...] = 0
    a["row_of"][:], a["bat_id"][:], a["parent"][:] = -1, -1, -1
    a["bat_dl"][:], a["cand_dl"][:] = p.D0, p.D0
    a["len_next"][:], a["fin_next"][:], a["finished"][:], a["cand_src_len"][:] = 1, 1, 1, 1
    a["logp_next"][:] = F32(0)
    a["cache_slot"][:] = a["cache_slot_parent"][:] = np.arange(p.C * p.K)
    a["src_of"][:] = np.arange(p.C * p.K) // p.K
    S.w = [0] * (CNT_WORDS + HOST_WORDS)
    return S


def admit(S: State, R: int, first_row: int, cov: set | None = None) -> State:
    """Rows first_row .. first_row + R - 1 take the lowest free source slots in order, each new batch the lowest free batch slot.
    Running out of either sets the error words and leaves the remaining rows alone."""
    S = S.copy()
    p, a = S.p, S.a
    free_src = [int(s) for s in np.flatnonzero(a["row_of"] < 0)]
    free_bat = [int(b) for b in np.flatnonzero(a["bat_id"] < 0)]
    others_live = bool((a["bat_id"] >= 0).any())
    cur, slot = None, None
    for i in range(R):
        row = first_row + i
        batch = int(a["batch_all"][row])
        if not free_src or (batch != cur and not free_bat):
            a["dev_summary"][2] = 1
            S.w[W_ERROR] = 1
            break
        s = free_src.pop(0)
        if batch != cur:
            cur, slot = batch, free_bat.pop(0)
            if cov is not None and others_live and a["bat_iter"][slot] > 0:
                cov.add("batch slot reused while another batch is live")
            for k in ("bat_iter", "bat_grp", "bat_live", "bat_nfin", "bat_longest_fin", "bat_longest_cur", "bat_state"):
                a[k][slot] = 0
            a["bat_id"][slot], a["bat_given"][slot] = batch, a["given_all"][batch]
            a["bat_dl"][slot] = min(p.D0, p.max_len - 2)
        if cov is not None and others_live and a["src_acc"][s].any():
            cov.add("source slot reused while another batch is live")
        a["new_slot"][i], a["row_of"][s], a["slot_batch"][s], a["src_state"][s] = s, row, slot, RUNNING
        a["bat_live"][slot] += 1
        a["src_acc"][s] = 0
        own = slice(s * p.K, (s + 1) * p.K)
        a["cand_src_len"][own], a["cand_batch"][own] = a["len_all"][row], slot
        a["cache_slot"][own] = a["cache_slot_parent"][own] = np.arange(s * p.K, (s + 1) * p.K)
    return S


def fill(S: State, R: int, first_row: int, stage: dict) -> State:
    """New source i sits in slot new_slot[i]: one <BOS> candidate (the other K - 1 rows are PAD and not looked at before the second
    iteration), its tokens, validity bytes, drafts and cross K/V padded to the slot's width, and blank caller-side rows."""
    S = S.copy()
    p, a = S.p, S.a
    Ls_new = stage["tok_new"].shape[1]
    for i in range(R):
        s, row = int(a["new_slot"][i]), first_row + i
        own = slice(s * p.K, (s + 1) * p.K)
        a["cand_next"][own] = p.pad
        a["cand_next"][s * p.K, 0] = p.bos
        a["len_next"][own], a["fin_next"][own], a["logp_next"][own], a["parent"][own], a["parent_draft"][own] = 1, 0, F32(0), -1, 0
        a["tok"][s], a["src_valid"][s] = p.pad, 0
        a["tok"][s, :Ls_new], a["src_valid"][s, :Ls_new] = stage["tok_new"][i], stage["valid_new"][i]
        if stage.get("drafts_new") is not None:
            a["drafts_all"][s] = stage["drafts_new"][i]
        a["memkv"][s, :Ls_new] = stage["memkv_new"][i]
        a["out"][row], a["trace_len"][row], a["summary"][row] = p.pad, -1, 0
    return S


def library(p, tokens, given: int) -> np.ndarray:
    """[given - 5, D0 + 1]: the stride-1 windows of a source row padded to the given batch's width (the slot may be narrower: what
    lies beyond it is PAD all the same), EOS / PAD replaced."""
    n_lib = given - 5
    row = np.full(n_lib + p.D0 + 1, p.pad, I32)
    n = min(len(tokens), len(row))
    row[:n] = tokens[:n]
    row[(row == p.eos) | (row == p.pad)] = p.repl
    return np.stack([row[i:i + p.D0 + 1] for i in range(n_lib)])


def prep(S: State, cov: set | None = None) -> State:
    S = S.copy()
    p, a = S.p, S.a
    K = p.K
    grp = {}
    for s in range(p.C):
        row, b = int(a["row_of"][s]), int(a["slot_batch"][s])
        beam = 0 if row < 0 else (1 if a["bat_iter"][b] == 0 else K)
        dead = slice(s * K + beam, (s + 1) * K)
        a["active"][dead], a["finished"][dead], a["live"][dead], a["per_cand"][dead], a["len"][dead], a["front"][dead] = 0, 1, 0, 0, 1, 0
        if beam == 0:
            continue
        own = slice(s * K, s * K + beam)
        c = NS(max_cand=beam, n_cand=beam, beam=beam, ld=p.ld, N=p.N, dl=p.D0, smart=bool(p.smart), cand_next=a["cand_next"][own],
               len_next=a["len_next"][own], fin_next=a["fin_next"][own], logp_next=a["logp_next"][own],
               drafts_all=None if p.smart else a["drafts_all"][s][None], lib=library(p, a["tok"][s], int(a["bat_given"][b]))[None] if p.smart else None)
        for k, v in B.bs_prep(c).items():                                  # the per-batch kernel's rule, pinned in test_beam_checks_host.py
            a[k][own] = v
        a["live"][own], a["cand_dl"][own] = 1, a["bat_dl"][b]
        if p.smart:
            grp[b] = max(grp.get(b, 0), int(a["per_cand"][own].max()))
            if cov is not None and a["bat_given"][b] > p.Ls_cap:
                cov.add("given width above the slot width")
    for b, g in grp.items():
        a["bat_grp"][b] = max(int(a["bat_grp"][b]), g)
        if cov is not None and a["bat_grp"][b] > 1:
            cov.add("bat_grp > 1")
    return S


def cache_slots(old, par, fin):
    """The K new candidates share their parents' K cache slots: a parent's slot goes to its first running child, or to its first
    child if none runs (that child only appends); every other child, in order, copies into the slot of the lowest parent that
    has no child.  Returns (new slots, how the heirs were found: "running", "finished", "spare")."""
    K = len(par)
    new, how = [None] * K, set()
    for q in sorted(set(par)):
        kids = [r for r in range(K) if par[r] == q]
        running = [r for r in kids if not fin[r]]
        heir = running[0] if running else kids[0]
        how.add("running" if running else "finished")
        new[heir] = old[q]
    spare = [old[q] for q in range(K) if q not in set(par)]
    for r in range(K):
        if new[r] is None:
            new[r] = spare.pop(0)
            how.add("spare")
    return new, how


def select(S: State, cov: set | None = None) -> State:
    S = S.copy()
    p, a = S.p, S.a
    K, dl1 = p.K, p.D0 + 1
    for s in range(p.C):
        row = int(a["row_of"][s])
        if row < 0:
            continue
        b = int(a["slot_batch"][s])
        it = int(a["bat_iter"][b]) + 1
        beam = 1 if it == 1 else K
        c0 = s * K
        own = slice(c0, c0 + beam)
        win = B.best_leaves(a["leaf_score"][own].reshape(beam * dl1, K), a["leaf_cnt"][own].reshape(beam * dl1), K)
        running = a["finished"][own] == 0
        acc = a["src_acc"][s]
        acc[0] += a["per_cand"][own].sum()
        acc[1] += a["per_cand"][own][running].sum()
        acc[4] += running.sum()
        longest = n_eos = 0
        if win is not None:
            rows, par, fin = [], [], []
            for r, (seg, i) in enumerate(win):
                cl, pos = divmod(seg, dl1)
                cc = c0 + cl
                tok, lc = int(a["leaf_tok"][cc, pos, i]), int(a["len"][cc])
                new = a["gen"][cc].astype(I64)
                new[lc:lc + dl1] = p.pad
                new[lc:lc + pos] = a["chosen"][cc, :pos]
                new[lc + pos] = tok
                rows.append(new)
                eos = bool(a["finished"][cc]) or tok == p.eos
                real = lc + pos + (0 if tok == p.pad else 1)
                a["logp_next"][c0 + r] = a["leaf_score"][cc, pos, i]
                a["parent"][c0 + r], a["parent_draft"][c0 + r], a["len_next"][c0 + r], a["fin_next"][c0 + r] = cc, a["chosen_slot"][cc], real, eos
                n_eos += eos
                longest = max(longest, real)
                if not a["finished"][cc]:
                    acc[2] += pos
                    acc[3] += 1
                par.append(cl)
                fin.append(eos)
            a["cand_next"][c0:c0 + K] = np.stack(rows)
            old = [int(v) for v in a["cache_slot"][c0:c0 + K]]
            new_slots, how = cache_slots(old, par, fin)
            a["cache_slot"][c0:c0 + K] = new_slots
            a["cache_slot_parent"][c0:c0 + K] = [old[q] for q in par]
            a["bat_longest_cur"][b] = max(int(a["bat_longest_cur"][b]), longest)
            if cov is not None:
                cov.update(f"cache slot: {h}" for h in how)
        acc[5], acc[6] = longest, K - n_eos if win is not None else 0
        if it - 1 < p.T_cap:
            a["trace_len"][row, it - 1] = longest
        elif cov is not None:
            cov.add("it - 1 >= T_cap")
        a["src_state"][s] = ERR_LEAVES if win is None else (DONE if n_eos == K else RUNNING)
        if win is None:
            a["bat_state"][b] = max(int(a["bat_state"][b]), 2)
    return S


def batches(S: State, cov: set | None = None) -> State:
    S = S.copy()
    p, a = S.p, S.a
    for b in np.flatnonzero(a["bat_id"] >= 0):
        a["bat_iter"][b] += 1
        if a["bat_state"][b] == 2:                                          # the batch raised: nothing else is of interest
            continue
        room = p.max_len - max(int(a["bat_longest_fin"][b]), int(a["bat_longest_cur"][b])) - 1
        if room < 1:
            a["bat_state"][b] = 1
        elif p.max_steps > 0 and a["bat_iter"][b] >= p.max_steps:
            a["bat_state"][b] = 3
        if cov is not None and max(room, 1) < a["bat_dl"][b]:
            cov.add("bat_dl shrinks")
        a["bat_dl"][b] = min(max(room, 1), int(a["bat_dl"][b]))
        a["bat_longest_cur"][b] = 0
    return S


def retire(S: State, cov: set | None = None) -> State:
    S = S.copy()
    p, a = S.p, S.a
    K = p.K
    for s in range(p.C):
        row = int(a["row_of"][s])
        if row < 0:
            continue
        b = int(a["slot_batch"][s])
        st, bst = int(a["src_state"][s]), int(a["bat_state"][b])
        if st == RUNNING:
            st = {0: RUNNING, 1: STOPPED, 2: ERR_LEAVES, 3: MAX_STEPS}[bst]
        elif st == DONE and bst == 2:
            st = ERR_LEAVES
            if cov is not None:
                cov.add("BP_DONE turned into BP_ERR_LEAVES")
        if cov is not None:
            cov.add(f"status {st}")
            if st == DONE and bst == 3:
                cov.add("max_steps meets a source that finishes in the same iteration")
            if st == ERR_LEAVES and a["bat_nfin"][b] > 0:
                cov.add("a batch raises after a source of it retired")
        acc = a["src_acc"][s]
        if st == RUNNING:
            a["dev_summary"][0] += 1
            a["dev_summary"][1] += acc[6]
            continue
        if st in (DONE, STOPPED):
            a["out"][row] = a["cand_next"][s * K:(s + 1) * K, :p.max_len]
        a["summary"][row] = [a["bat_iter"][b], st, acc[0], acc[1], acc[2], acc[3], acc[5], acc[4]]
        a["row_of"][s] = -1
        a["bat_longest_fin"][b] = max(int(a["bat_longest_fin"][b]), int(acc[5]))
        a["bat_nfin"][b] += 1
        a["bat_live"][b] -= 1
        if a["bat_live"][b] == 0:
            a["bat_id"][b] = -1
    return S


def publish(S: State, cov: set | None = None) -> State:
    S = S.copy()
    a = S.a
    with_finished = (a["bat_id"] >= 0) & (a["bat_nfin"] > 0)
    if cov is not None and (with_finished & (a["bat_grp"] > 1)).any():
        cov.add("bat_grp reset to 1 after a source of the batch finished")
    a["bat_grp"][:] = with_finished
    S.w[W_LIVE], S.w[W_RUNNING] = int(a["dev_summary"][0]), int(a["dev_summary"][1])
    if a["dev_summary"][2]:
        S.w[W_ERROR] = 1
    a["dev_summary"][:2] = 0
    S.w[W_STEPS] = S.w[W_CALLS]
    return S


RULES = dict(init=init, admit=admit, fill=fill, prep=prep, select=select, batches=batches, retire=retire, publish=publish)


# ---------------------------------------------------------------------------------------------------------------------------
# the synthetic step: what the verify step, k_bs_hits and k_bs_leaves would leave for k_bsp_select, as a function of the source's
# row in the work list, the candidate's tokens, cand_dl and per_cand alone — never of the slot the source sits in
def knobs(*, seed=0, V=6, eos_rate=0.04, pad_leaf=True, tie=False, starve=None, finish=None, acc_cap=None) -> NS:
    """V: tokens are drawn from 5 .. 5 + V - 1; eos_rate: a leaf is EOS with probability eos_rate * (length of its root);
    pad_leaf: a finished root has its one PAD leaf (False: none, the source then runs short of leaves); tie: scores take few
    values, so the enumeration order decides often; starve {row: length}: candidates of that row at or beyond the length have no
    leaves; finish {row: length}: ... have EOS leaves only; acc_cap {row: n}: at most n draft tokens are accepted."""
    return NS(seed=seed, V=V, eos_rate=eos_rate, pad_leaf=pad_leaf, tie=tie, starve=starve or {}, finish=finish or {}, acc_cap=acc_cap or {})


def score_of(kn, row: int, toks) -> np.float32:
    """The score of a hypothesis: a function of its tokens, so the PAD leaf of a finished root repeats the root's own score."""
    h = 2166136261
    for v in (row, *toks):
        h = ((h ^ (int(v) & 0xFFFF)) * 16777619) & 0xFFFFFFFF
    if kn.tie:
        return F32(-(len(toks) // 2) - 0.5 * (h % 3))
    return F32(-0.37 * len(toks) - (h % 4096) / 2048.0)


def cand_leaves(kn, K: int, D0: int, row: int, toks, dl: int, per_cand: int):
    """-> chosen_slot, chosen [D0], leaf_cnt [D0 + 1], leaf_tok [D0 + 1, K], leaf_score [D0 + 1, K] of one live candidate.  A running
    candidate accepts n <= dl draft tokens; position n holds K leaves, an accepted position fewer (the accepted token is not among
    them).  Entries beyond a count hold values a kernel must not read (+3e38 would win every comparison)."""
    toks = [int(t) for t in toks]
    rng = np.random.default_rng([kn.seed, row, dl, per_cand, *toks])
    cnt, tok, score = np.zeros(D0 + 1, I32), np.full((D0 + 1, K), -7, I32), np.full((D0 + 1, K), 3e38, F32)
    chosen = rng.integers(5, 5 + kn.V, size=D0).astype(I64)
    slot = int(rng.integers(0, max(per_cand, 1)))
    L = len(toks)
    if EOS in toks:
        if kn.pad_leaf:
            cnt[0], tok[0, 0], score[0, 0] = 1, PAD, score_of(kn, row, toks)
        return slot, chosen, cnt, tok, score
    n_acc = int(rng.integers(0, min(dl, kn.acc_cap.get(row, dl)) + 1))
    if row in kn.starve and L >= kn.starve[row]:
        return slot, chosen, cnt, tok, score
    force = row in kn.finish and L >= kn.finish[row]
    for pos in range(n_acc + 1):
        cnt[pos] = K if (pos == n_acc or force) else rng.integers(0, K)
        for i in range(cnt[pos]):
            t = EOS if (force or rng.random() < kn.eos_rate * L) else int(rng.integers(5, 5 + kn.V))
            if pos < n_acc and t == chosen[pos]:
                t = 5 + (t - 5 + 1) % kn.V if kn.V > 1 else EOS
            tok[pos, i], score[pos, i] = t, score_of(kn, row, toks + [int(v) for v in chosen[:pos]] + [t])
    return slot, chosen, cnt, tok, score


def synth(S: State, kn) -> State:
    """The step of one pool iteration on the state k_bsp_prep left: STEP_OUT of every live candidate (dead ones: no leaves) and one
    model call more."""
    S = S.copy()
    p, a = S.p, S.a
    a["leaf_cnt"][...] = 0
    for c in np.flatnonzero(a["live"] == 1):
        row = int(a["row_of"][c // p.K])
        got = cand_leaves(kn, p.K, p.D0, row, a["gen"][c, :a["len"][c]], int(a["cand_dl"][c]), int(a["per_cand"][c]))
        for k, v in zip(STEP_OUT, (got[0], got[1], got[4], got[3], got[2])):
            a[k][c] = v
    S.w[W_CALLS] += 1
    return S


# ---------------------------------------------------------------------------------------------------------------------------
# work lists, admissions and the chain
def work_list(sizes, *, smart, seed=0, V=6, Ls=16, len_lo=6, wide=()) -> NS:
    """Batches of sizes[i] sources: rows <BOS> tokens <EOS> PAD.. of len_lo .. Ls tokens; given width = the batch's longest row,
    for the batches in ``wide`` 4 more (beyond the pool's slot width when the row is the longest of the list)."""
    rng = np.random.default_rng(seed)
    R = int(sum(sizes))
    w = NS(sizes=list(sizes), n_batches=len(sizes), R=R, Ls=Ls, smart=smart, tokens=np.full((R, Ls), PAD, I32), len_all=np.zeros(R, I32),
           batch_all=np.repeat(np.arange(len(sizes)), sizes).astype(I32), given_all=np.zeros(len(sizes), I32))
    w.first = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    for r in range(R):
        n = int(rng.integers(len_lo, Ls + 1))
        w.tokens[r, :n] = [BOS, *rng.integers(5, 5 + V, size=n - 2), EOS]
        w.len_all[r] = n
    for b in range(len(sizes)):
        w.given_all[b] = w.len_all[w.first[b]:w.first[b + 1]].max() + (4 if b in wide else 0)
    return w


def start(p, w, kv_row: int = 128) -> State:
    S = blank(p, w.R, w.n_batches, kv_row)
    S.a["len_all"], S.a["batch_all"], S.a["given_all"] = w.len_all.copy(), w.batch_all.copy(), w.given_all.copy()
    return S


def stage(p, w, first_row: int, R: int, kv_row: int = 128, Ls_new: int | None = None) -> dict:
    """The staged operands of one admission: functions of the rows alone."""
    rows = range(first_row, first_row + R)
    Ls_new = int(w.len_all[first_row:first_row + R].max()) if Ls_new is None else Ls_new
    tok = w.tokens[first_row:first_row + R, :Ls_new].astype(I32)
    kv = np.stack([np.random.default_rng(1000 + r).standard_normal((Ls_new, kv_row)).astype(F32) for r in rows])
    drafts = None if p.smart else np.stack([np.random.default_rng(2000 + r).integers(5, 11, size=(p.N, p.D0)) for r in rows]).astype(I32)
    return dict(tok_new=np.ascontiguousarray(tok), valid_new=(tok != PAD).astype(U8), drafts_new=drafts, memkv_new=kv)


def policy_batches(policy: str, it: int, free: int, sizes, pool_empty: bool) -> int:
    """How many of the next batches (sizes) the host admits before iteration ``it``: eager (all that fit), single (one), lazy (only
    into an empty pool, then all that fit), third (eager on every third iteration).  An empty pool always admits."""
    fit = 0
    for n in sizes:
        if n > free:
            break
        free -= n
        fit += 1
    if policy == "single":
        fit = min(fit, 1)
    elif policy == "lazy" and not pool_empty:
        fit = 0
    elif policy == "third" and it % 3 and not pool_empty:
        fit = 0
    return fit


def chain(p, w, kn, policy: str, apply=None, cov: set | None = None, max_iters: int = 400):
    """init, then per iteration: admit + fill when the policy says so, prep, the synthetic step, select, batches, retire, publish —
    until the work list is done.  ``apply(op, S_before, S_after, *operands)`` sees every step, "synth" included (the GPU test
    launches and compares there); the operands are (R, first_row) of admit and (R, first_row, staged arrays) of fill.  Returns the
    final State and a log {(batch, iteration): (bat_dl, bat_grp)} of the scalars in force after prep."""
    def step(op, S, *args):
        after = RULES[op](S, *args, **({"cov": cov} if op not in ("init", "fill") else {}))
        if apply is not None:
            apply(op, S, after, *args)
        return after

    S = step("init", start(p, w))
    nxt, log = 0, {}
    for it in range(max_iters):
        empty = not (S.a["row_of"] >= 0).any()
        if empty and nxt == w.n_batches:
            return S, log
        take = policy_batches(policy, it, int((S.a["row_of"] < 0).sum()), w.sizes[nxt:], empty)
        if take:
            first_row, R = int(w.first[nxt]), int(w.first[nxt + take] - w.first[nxt])
            st = stage(p, w, first_row, R)
            S = step("admit", S, R, first_row)
            S = step("fill", S, R, first_row, st)
            nxt += take
        S = step("prep", S)
        for b in np.flatnonzero(S.a["bat_id"] >= 0):
            log[(int(S.a["bat_id"][b]), int(S.a["bat_iter"][b]) + 1)] = (int(S.a["bat_dl"][b]), int(S.a["bat_grp"][b]))
        before, S = S, synth(S, kn)
        if apply is not None:
            apply("synth", before, S)
        prev = S
        S = step("select", S)
        check_cache_slots(prev, S)
        for op in ("batches", "retire", "publish"):
            S = step(op, S)
    raise AssertionError("the chain does not end")


def check_cache_slots(before: State, after: State) -> None:
    """After a select: a source's cache slots are a permutation of its own K slots, and a parent with a running child has handed
    its old slot to a running child of its."""
    p = before.p
    K = p.K
    for s in np.flatnonzero(before.a["row_of"] >= 0):
        own = slice(s * K, (s + 1) * K)
        new = after.a["cache_slot"][own]
        assert sorted(new) == list(range(s * K, (s + 1) * K)), f"source slot {s}: cache slots {list(new)}"
        if after.a["src_state"][s] == ERR_LEAVES:
            continue
        old = before.a["cache_slot"][own]
        for q in set(int(v) - s * K for v in after.a["parent"][own]):
            kids = [r for r in range(K) if after.a["parent"][s * K + r] == s * K + q]
            running = [r for r in kids if not after.a["fin_next"][s * K + r]]
            heirs = [r for r in kids if new[r] == old[q]]
            assert len(heirs) == 1 and (not running or heirs[0] in running), f"source slot {s}, parent {q}: heirs {heirs}, running {running}"
            assert all(after.a["cache_slot_parent"][s * K + r] == old[q] for r in kids)


# ---------------------------------------------------------------------------------------------------------------------------
# the per-batch loop: the reference's generate_* on ONE given batch, scalars as the reference keeps them (:457, :464, :476, :586,
# :596 and the library's max_steps guard), leaves from the same synthetic step, selection by util_beam_checks.beam_select
def window_count(p, tokens, given: int, last: int) -> int:
    """Smart mode: drafts of a candidate ending in ``last`` (:417-419: at least one, at most N)."""
    starts = [p.repl if t in (p.eos, p.pad) else int(t) for t in list(tokens) + [p.pad] * given][:given - 5]
    return min(p.N, max(1, sum(t == last for t in starts)))


def per_batch(p, w, kn, bi: int) -> NS:
    rows = list(range(int(w.first[bi]), int(w.first[bi + 1])))
    nb, K, D0, dl1 = len(rows), p.K, p.D0, p.D0 + 1
    given = int(w.given_all[bi])
    cand = [[[BOS]] for _ in rows]                                         # per source: token lists of its candidates
    res = NS(rows=rows, status=[RUNNING] * nb, iters=[0] * nb, trace=[[] for _ in rows], acc=np.zeros((nb, 8), np.int64), out=[None] * nb,
             scalars={}, width=1, model_calls=0, error=None)
    src_longest = [1] * nb
    longest = 1
    possible = p.max_len - longest - 1                                     # :457
    dl, it = D0, 0
    while possible >= 1 and longest <= p.max_len:                          # :464
        it += 1
        dl = min(possible, dl)                                             # :476
        res.width = max(res.width, longest + dl + 1)                       # :488-491
        res.model_calls += 1
        beam = len(cand[0])
        per = [[(window_count(p, w.tokens[r], given, c[-1]) if p.smart else p.N) for c in cand[i]] for i, r in enumerate(rows)]
        fin = [[EOS in c for c in cand[i]] for i in range(nb)]
        res.scalars[it] = (dl, max(max(1 if f else n for n, f in zip(per[i], fin[i])) for i in range(nb)) if p.smart else 0)
        ld = p.max_len + D0 + 2
        c = NS(B=nb, beam=beam, dl=D0, K=K, pad=PAD, eos=EOS, width=ld, ld_in=ld, ld_out=ld, summary=np.array([0, B.BIG, 0, 0, 0], I32),
               cand=np.full((nb * beam, ld), PAD, I32), len=np.zeros(nb * beam, I32), chosen=np.zeros((nb * beam, D0), I64),
               chosen_slot=np.zeros(nb * beam, I32), finished=np.zeros(nb * beam, U8), leaf_score=np.zeros((nb * beam, dl1, K), F32),
               leaf_tok=np.zeros((nb * beam, dl1, K), I32), leaf_cnt=np.zeros((nb * beam, dl1), I32))
        for i, r in enumerate(rows):
            for k, toks in enumerate(cand[i]):
                cc = i * beam + k
                c.cand[cc, :len(toks)], c.len[cc], c.finished[cc] = toks, len(toks), fin[i][k]
                c.chosen_slot[cc], c.chosen[cc], c.leaf_cnt[cc], c.leaf_tok[cc], c.leaf_score[cc] = cand_leaves(kn, K, D0, r, toks, dl, per[i][k])
        live = [i for i in range(nb) if res.status[i] == RUNNING]
        short = [i for i in live if c.leaf_cnt[i * beam:(i + 1) * beam].sum() < K]
        for i in live:
            res.iters[i] = it
            res.acc[i, 0] += sum(per[i])
            res.acc[i, 1] += sum(n for n, f in zip(per[i], fin[i]) if not f)
            res.acc[i, 7] += sum(not f for f in fin[i])
        if short:                                                          # the sampler asserts: the batch is lost, finished sources kept
            for i in live:
                res.status[i] = ERR_LEAVES
            res.error = "reference"
            return res
        o = B.beam_select(c)
        if beam == 1:
            cand = [c1 * K for c1 in cand]                                 # n_best rows per source from now on
        for i in live:                                                     # a finished source is a fixed point: its rows stay
            own = slice(i * K, (i + 1) * K)
            cand[i] = [[int(t) for t in o["new_cand"][i * K + r, :o["new_len"][i * K + r]]] for r in range(K)]
            running_parents = c.finished[o["parent"][own]] == 0
            res.acc[i, 2] += o["mark"][own][running_parents].sum()
            res.acc[i, 3] += running_parents.sum()
            res.acc[i, 6] = o["new_len"][own].max()
            res.trace[i].append(int(o["new_len"][own].max()))
            if o["new_finished"][own].all():
                res.status[i] = DONE
            res.out[i] = o["new_cand"][own, :p.max_len].copy()
            src_longest[i] = int(o["new_len"][own].max())
        longest = max(src_longest)
        if all(s == DONE for s in res.status):                             # :586
            break
        possible = p.max_len - longest - 1                                 # :596
        stop = STOPPED if possible < 1 else (MAX_STEPS if p.max_steps > 0 and it >= p.max_steps else RUNNING)
        if stop != RUNNING:
            for i in range(nb):
                if res.status[i] == RUNNING:
                    res.status[i] = stop
            if stop == MAX_STEPS:
                res.error = "max_steps"
            break
    return res


def expected_io(p, w, kn):
    """out, summary, trace_len of the whole work list as the pool must leave them, from the per-batch loop alone; and its results."""
    out = np.full((w.R, p.K, p.max_len), PAD, I64)
    summary = np.zeros((w.R, 8), I32)
    trace = np.full((w.R, p.T_cap), -1, I16)
    refs = []
    for bi in range(w.n_batches):
        r = per_batch(p, w, kn, bi)
        refs.append(r)
        for i, row in enumerate(r.rows):
            a = r.acc[i]
            summary[row] = [r.iters[i], r.status[i], a[0], a[1], a[2], a[3], a[6], a[7]]
            if r.status[i] in (DONE, STOPPED):
                out[row] = r.out[i]
            t = r.trace[i][:p.T_cap]
            trace[row, :len(t)] = t
    return out, summary, trace, refs


def check_against_per_batch(S: State, log: dict, p, w, kn) -> list:
    """The pooled run's caller-side arrays against the per-batch loop.  A source that was live when its batch raised has no
    counterpart in the reference beyond the raise itself: its status and iteration count are compared, and its hypotheses stay PAD."""
    out, summary, trace, refs = expected_io(p, w, kn)
    raised = summary[:, 1] == ERR_LEAVES
    B.same(S.a["out"], out, "out")
    B.same(S.a["summary"][:, :2], summary[:, :2], "summary: iterations and status")
    B.same(S.a["summary"][~raised], summary[~raised], "summary")
    B.same(S.a["trace_len"][~raised], trace[~raised], "trace_len")
    for bi, r in enumerate(refs):
        for it, sc in r.scalars.items():
            got = log[(bi, it)] if p.smart else (log[(bi, it)][0], 0)        # the group width is a smart-mode scalar
            assert got == sc, f"batch {bi} iteration {it}: draft length and group width {got}, the per-batch loop has {sc}"
        assert max(it for (b, it) in log if b == bi) == max(r.iters), f"batch {bi}: iterations"
    return refs


# ---------------------------------------------------------------------------------------------------------------------------
# the chained scenarios of tests/test_bsp_checks_host.py and tests/test_gpu_bsp_kernels.py
SIZES = [3, 1, 5, 2, 4, 1, 2, 3, 5]                                        # 9 batches of 1 - 5 sources


def scenarios() -> list:
    """name -> what it is built to reach.  plain: the common path, a given width beyond the slot width.  tight: max_len 12 under
    D0 5 (the draft length shrinks, batches stop for lack of room), T_cap 3 below the iteration count, tied scores.  raise: row 0
    finishes in the iteration in which its batch mate row 1 runs out of leaves; row 7 runs out later, after a mate finished.
    guard: max_steps 3, row 4 finishes exactly in iteration 3 while its mates are cut off."""
    base = dict(sizes=SIZES, K=3, N=3, D0=5, max_len=24, T_cap=40, max_steps=0, wide=(2, 5), seed=1, kn={})
    return [NS(name="plain", **base),
            NS(name="tight", **{**base, "max_len": 12, "T_cap": 3, "K": 4, "N": 2, "seed": 2, "kn": dict(tie=True, eos_rate=0.02)}),
            NS(name="raise", **{**base, "K": 2, "D0": 3, "seed": 3,
                                "kn": dict(finish={0: 1, 6: 2}, starve={1: 1, 7: 4}, eos_rate=0.05)}),
            NS(name="guard", **{**base, "K": 5, "D0": 2, "N": 1, "max_steps": 3, "seed": 4,
                                "kn": dict(finish={4: 3}, acc_cap={4: 0}, eos_rate=0.01)})]


def scenario_setup(sc, smart: bool, C: int):
    w = work_list(sc.sizes, smart=smart, seed=sc.seed, wide=sc.wide)
    p = params(C=C, K=sc.K, N=sc.N, D0=sc.D0, Ls_cap=int(w.len_all.max()), max_len=sc.max_len, smart=smart, T_cap=sc.T_cap,
               max_steps=sc.max_steps)
    return p, w, knobs(seed=sc.seed, **sc.kn)


# the chains the GPU test launches (scenario, smart, capacity, policy); the host test runs these and more, and asserts that THESE
# reach every condition of REQUIRED
CHAINS = [("plain", False, 5, "eager"), ("plain", True, 6, "single"), ("tight", False, 6, "third"), ("tight", True, 5, "eager"),
          ("raise", False, 6, "single"), ("raise", True, 5, "eager"), ("guard", False, 5, "lazy"), ("guard", True, 6, "third")]
REQUIRED = ["status 0", "status 1", "status 2", "status 3", "status 4", "BP_DONE turned into BP_ERR_LEAVES", "bat_dl shrinks",
            "source slot reused while another batch is live", "batch slot reused while another batch is live", "bat_grp > 1",
            "bat_grp reset to 1 after a source of the batch finished", "it - 1 >= T_cap", "cache slot: running", "cache slot: finished",
            "cache slot: spare", "max_steps meets a source that finishes in the same iteration", "a batch raises after a source of it retired",
            "given width above the slot width"]


def run_chain(name: str, smart: bool, C: int, policy: str, apply=None, cov: set | None = None):
    sc = next(x for x in scenarios() if x.name == name)
    p, w, kn = scenario_setup(sc, smart, C)
    S, log = chain(p, w, kn, policy, apply=apply, cov=cov)
    return S, log, p, w, kn


# ---------------------------------------------------------------------------------------------------------------------------
# constructed States for the single-launch cases of tests/test_gpu_bsp_kernels.py
def build(p, layout, *, rows: int, n_batches: int, seed=0, kv_row: int = 128, V: int = 6, row_len=None) -> State:
    """A State between two iterations.  ``layout``: one dict per live batch — slot (batch slot), id (batch in the work list), srcs
    (source slots), it (iterations done), and optionally dl, given, state, nfin, longest_fin, longest_cur, grp.  Everything the
    layout does not speak of stays blank; free source slots hold row_of -1, free batch slots bat_id -1.  Sources take the rows
    0, 1, .. of the work list in the order of the layout; a live source has K candidate rows of random tokens (one <BOS> row in
    its batch's first iteration), a random share of them finished, and a random permutation of its cache slots."""
    rng = np.random.default_rng(seed)
    S = blank(p, rows, n_batches, kv_row)
    a, K = S.a, p.K
    a["row_of"][:], a["bat_id"][:] = -1, -1
    a["dev_summary"][:] = 0
    a["batch_all"][:], a["len_all"][:], a["given_all"][:] = 0, 2, 6
    S.w = [7, 0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0]
    row = 0
    for bt in layout:
        b = bt["slot"]
        given = bt.get("given", p.Ls_cap)
        a["bat_id"][b], a["bat_iter"][b], a["bat_dl"][b], a["bat_grp"][b] = bt["id"], bt["it"], bt.get("dl", p.D0), bt.get("grp", 0)
        a["bat_live"][b], a["bat_nfin"][b], a["bat_state"][b], a["bat_given"][b] = len(bt["srcs"]), bt.get("nfin", 0), bt.get("state", 0), given
        a["bat_longest_fin"][b], a["bat_longest_cur"][b] = bt.get("longest_fin", 0), bt.get("longest_cur", 0)
        a["given_all"][bt["id"]] = given
        for s in bt["srcs"]:
            n = min(p.Ls_cap, given) if row_len is None else row_len
            a["row_of"][s], a["slot_batch"][s], a["src_state"][s] = row, b, RUNNING
            a["src_acc"][s] = rng.integers(0, 50, size=8)
            a["tok"][s] = p.pad
            a["tok"][s, :n] = [BOS, *rng.integers(5, 5 + V, size=n - 2), EOS]
            a["batch_all"][row], a["len_all"][row] = bt["id"], n
            if not p.smart:
                a["drafts_all"][s] = rng.integers(5, 5 + V, size=(p.N, p.D0))
            own = slice(s * K, (s + 1) * K)
            a["cand_batch"][own], a["cand_src_len"][own] = b, n
            a["cache_slot"][own] = s * K + rng.permutation(K)
            a["cache_slot_parent"][own] = s * K + rng.integers(0, K, size=K)
            a["cand_next"][own] = p.pad
            for k in range(K):
                c = s * K + k
                first = bt["it"] == 0
                lc = 1 if first else int(rng.integers(2, max(3, p.max_len - p.D0 - 1)))
                fin = (not first) and k > 0 and rng.random() < 0.3
                a["cand_next"][c, :lc] = [BOS, *rng.integers(5, 5 + V, size=lc - 1)]
                if fin:
                    a["cand_next"][c, lc - 1] = EOS
                a["len_next"][c], a["fin_next"][c], a["logp_next"][c] = lc, fin, F32(-rng.random() * 9)
                a["parent"][c], a["parent_draft"][c] = c, 0
            row += 1
    assert row <= rows
    return S


def plant_keys(S: State, s: int, n_lib: int, rng) -> list:
    """Smart mode: source slot s gets a row in which key 10 starts no window, 11 fewer than N, 12 exactly N and 13 more than N
    windows (the (N+1)-th beyond position 255 when the library has a second scan round); its K candidates end in the keys in turn."""
    p, a = S.p, S.a
    keys, N = [10, 11, 12, 13], p.N
    n = min(p.Ls_cap, n_lib + 5)
    a["tok"][s] = p.pad
    a["tok"][s, :n] = rng.integers(20, 40, size=n)
    free = [int(i) for i in rng.permutation(min(n, n_lib))]

    def take(k, pred=lambda i: True):
        got = [i for i in free if pred(i)][:k]
        for i in got:
            free.remove(i)
        return got
    a["tok"][s, take(min(N - 1, n_lib // 4))] = keys[1]
    if len(free) >= N:
        a["tok"][s, take(N)] = keys[2]
    if len(free) >= N + 1:
        more = take(N, lambda i: i < 256) + take(1, (lambda i: i >= 256) if min(n, n_lib) > 256 else (lambda i: True))
        a["tok"][s, more] = keys[3]
    for k in range(p.K):
        c = s * p.K + k
        if a["len_next"][c] < 2:
            a["len_next"][c] = 2
            a["cand_next"][c, 0] = BOS
        a["cand_next"][c, a["len_next"][c] - 1] = keys[k % 4]
        a["fin_next"][c] = 0
    return keys


def plant_leaves(S: State, s: int, pattern: str, rng) -> None:
    """The step's arrays of source slot s (after prep), by pattern: random; ties (few score values, inside and across segments);
    exact (K leaves in all); short (K - 1); done (EOS leaves only); one_parent (only candidate 0 has leaves); one_each (one
    leaf per candidate: one child per parent); fin_first (every candidate offers an EOS leaf that beats its other leaf: a
    finished child listed before a running child of the same parent).  Finished candidates keep their one PAD leaf unless the
    pattern gives the counts itself."""
    p, a = S.p, S.a
    K, dl1 = p.K, p.D0 + 1
    b = int(a["slot_batch"][s])
    beam = 1 if a["bat_iter"][b] == 0 else K
    own = slice(s * K, s * K + beam)
    cnt, tok, sc = a["leaf_cnt"][own], a["leaf_tok"][own], a["leaf_score"][own]
    cnt[...] = rng.integers(0, K + 1, size=cnt.shape)
    cnt[0, 0] = K
    tok[...] = rng.choice([EOS, 5, 6, 7, 8], size=tok.shape, p=[0.2, 0.2, 0.2, 0.2, 0.2])
    sc[...] = (-rng.random(sc.shape) * 20).astype(F32)
    a["chosen"][own] = rng.integers(5, 11, size=a["chosen"][own].shape)
    a["chosen_slot"][own] = rng.integers(0, p.N, size=beam)
    fin = a["finished"][own] == 1
    if pattern == "ties":
        sc[...] = F32(-3.25)
        sc[rng.random(sc.shape) < 0.3] = F32(-7.5)
    elif pattern in ("exact", "short"):
        cnt[...] = 0
        for _ in range(K if pattern == "exact" else K - 1):
            free = np.argwhere(cnt < K)
            i = free[rng.integers(len(free))]
            cnt[i[0], i[1]] += 1
    elif pattern == "done":
        tok[...] = EOS
    elif pattern == "one_parent":
        cnt[1:] = 0
    elif pattern == "one_each":
        cnt[...] = 0
        cnt[:, 0] = 1
        tok[:, 0, 0] = 7
        if beam < K:
            cnt[0, 0] = K
    elif pattern == "fin_first":
        cnt[...] = 0
        cnt[:, 0] = min(2, K)
        tok[:, 0, 0], sc[:, 0, 0] = EOS, -(1 + np.arange(beam)).astype(F32)
        if K > 1:
            tok[:, 0, 1], sc[:, 0, 1] = 6, -(1.5 + np.arange(beam)).astype(F32)
        if beam < K:
            cnt[0, 0] = K
    if pattern in ("random", "ties", "done"):
        for k in np.flatnonzero(fin):
            cnt[k], tok[k, 0, 0] = 0, PAD
            cnt[k, 0] = 1
