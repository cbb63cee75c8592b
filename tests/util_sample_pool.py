"""Plain restatement of the sampling slot pool (include/ttx.h: ttx_sample_speculative_generate_pool) for the tests, built on
tests/util_sample_spec.py and tests/util_loop_checks.py: the compacted rows of a draft pass under draft select, the accept step in
pool mode, one admission of sources x samples, and a host pool that admits sources in units of n under plan_admission's semantics
and runs a float64 sampler on a host model.  No GPU call and no test in here.  tests/test_sample_pool_host.py shows on the CPU that
the restated pool returns the position-by-position sampler's rows and that its checkers flag each single defect; the GPU modules
hold the kernels to it.

  select_row_map       draft masks of the slots of a pass -> compacted row -> layout row (k_probe_split's order)
  accept_pool_step     util_sample_spec.sample_accept_step with the pool's caller rows and executed-row count
  admit                one admission: slot scalars, gen, drafts, validity bytes, cross K/V, caller rows
  plan_admission       csrc/ttx_admit.h's rule, restated for one pool
  run_pool             the whole pool on the host
"""
from __future__ import annotations

import copy

import numpy as np

import util_loop_checks as U
import util_sample_checks as S
import util_sample_spec as X

PAD, BOS, EOS = U.PAD, U.BOS, U.EOS


def select_row_map(masks, N: int, D: int) -> np.ndarray:
    """Slot p of the pass has the drafts whose bit is set in masks[p]: its compacted rows are row 0, then the D rows of every present
    draft in ascending draft order; the slots follow each other in order.  Returns the layout row p * RPS + rs of every compacted row."""
    R = U.rps(N, D)
    out = []
    for p, m in enumerate(masks):
        out.append(p * R)
        for n in range(N):
            if (int(m) >> n) & 1:
                out.extend(p * R + 1 + n * D + j for j in range(D))
    return np.asarray(out, dtype=np.int32)


def accept_pool_step(state: U.LoopState, pred: np.ndarray, exec_rows: int | None = None) -> U.LoopState:
    """One accept step of the sampling pool: util_sample_spec.sample_accept_step, except that an ended row b goes to
    pool_out[row_of[b], :max_len] (there is no ``out``) and verified_positions grows by ``exec_rows`` when that is given."""
    s = state.clone()
    Bc = int(s.words["n_active"])
    if Bc == 0:
        return X.sample_accept_step(s, pred)
    rows = s.act_idx[:Bc].copy()
    s.out = np.zeros((s.B, s.max_len), dtype=np.int64)                    # scratch for the shared restatement
    t = X.sample_accept_step(s, pred)
    fin = t.rec[:Bc, 4] == 1
    t.pool_out[t.row_of[rows[fin]], :t.max_len] = t.gen[rows[fin], :t.max_len]
    t.out = None
    if exec_rows is not None:
        t.words["verified_positions"] += int(exec_rows) - Bc * U.rps(s.N, s.D)
    return t


def make_pool_state(B: int, N: int, D: int, max_len: int, fronts, n_active=None, seed: int = 0, V: int = 40) -> U.LoopState:
    """util_loop_checks.make_state in pool mode as the sampling pool holds it: a non-identity row_of, sentinels in the caller rows,
    haspad zero, no traces."""
    s = U.make_state(B, N, D, max_len, fronts, n_active=n_active, seed=seed, V=V, pool=True)
    s.rstep = s.pool_traj = s.pool_fin_step = None
    return s


def to_pool(s: U.LoopState, seed: int = 1) -> U.LoopState:
    """A single-session case of util_sample_spec (lengths_case, ending_case, ...) as a pool state: the same slots, fronts, drafts."""
    rng = np.random.default_rng(seed)
    t = s.clone()
    t.row_rule, t.pool = 1, 1
    t.pool_rows = s.B + 5
    t.row_of = rng.permutation(t.pool_rows)[:s.B].astype(np.int32)
    t.pool_out = U.sentinel_array((t.pool_rows, s.max_len), __import__("torch").int64)
    t.out = None
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# admission
class Pool:
    """The per-slot state of a sampling pool of C slots (NumPy), as k_pool_admit / k_pool_fill leave it."""

    def __init__(self, C: int, N: int, D: int, max_len: int, Ls_cap: int, kv_row: int, out_rows: int, rng=None):
        rng = rng or np.random.default_rng(0)
        self.C, self.N, self.D, self.max_len, self.Ls_cap, self.kv_row = C, N, D, max_len, Ls_cap, kv_row
        self.gen_ld = max_len + D + 2
        i32 = lambda *shape: rng.integers(-1000, -1, size=shape, dtype=np.int32)       # stale values of earlier occupants
        self.act_idx, self.front, self.haspad, self.rstep, self.row_of, self.src_len = (i32(C) for _ in range(6))
        self.key = rng.integers(-2 ** 62, 2 ** 62, size=C, dtype=np.int64)
        self.sample = i32(C)
        self.gen = i32(C, self.gen_ld)
        self.drafts = i32(C, N * D)
        self.src_valid = rng.integers(0, 255, size=(C, Ls_cap), dtype=np.uint8)
        self.memkv = rng.standard_normal((C, Ls_cap, kv_row)).astype(np.float32)
        self.out = np.full((out_rows, max_len), -7, dtype=np.int64)
        self.n_active = 0

    ARRAYS = ("act_idx", "front", "haspad", "rstep", "row_of", "src_len", "key", "sample", "gen", "drafts", "src_valid", "memkv", "out")

    def clone(self) -> "Pool":
        return copy.deepcopy(self)


def admit(pool: Pool, drafts_new: np.ndarray, valid_new: np.ndarray, memkv_new: np.ndarray, n: int, first_src: int, row_keys=None) -> dict:
    """One admission of S_chunk = len(drafts_new) staged sources x n samples, in place.  New decoder row i takes the lowest free slot:
    front 0, haspad 0, rstep 0, row_of = first_src * n + i, src_len = Ls_new, key of source first_src + i // n, sample i % n; gen row
    BOS then PAD; drafts, validity bytes (zero beyond Ls_new) and cross K/V of staged source i // n; caller row BOS then PAD.  More
    rows than free slots: error 4 (the slots that were free are handed out, nothing is filled)."""
    S_chunk, Ls_new = valid_new.shape
    R = S_chunk * n
    used = np.zeros(pool.C, dtype=bool)
    used[pool.act_idx[:pool.n_active]] = True
    free = np.nonzero(~used)[0]
    got = min(R, len(free))
    for i in range(got):
        b = int(free[i])
        src = first_src + i // n
        pool.act_idx[pool.n_active + i] = b
        pool.front[b], pool.haspad[b], pool.rstep[b] = 0, 0, 0
        pool.row_of[b] = first_src * n + i
        pool.src_len[b] = Ls_new
        pool.key[b] = src if row_keys is None else row_keys[src]
        pool.sample[b] = i % n
    pool.n_active += got
    error = 4 if got != R else 0
    if not error:
        for i in range(R):
            b, si = int(free[i]), i // n
            pool.gen[b] = PAD
            pool.gen[b, 0] = BOS
            pool.drafts[b] = drafts_new[si]
            pool.src_valid[b] = 0
            pool.src_valid[b, :Ls_new] = valid_new[si]
            pool.memkv[b, :Ls_new] = memkv_new[si]
            pool.out[first_src * n + i] = PAD
            pool.out[first_src * n + i, 0] = BOS
    return dict(n_active=pool.n_active, m_rows=pool.n_active * U.rps(pool.N, pool.D), error=error, host_n_active=pool.n_active)


# ---------------------------------------------------------------------------------------------------------------------------
# the pool on the host
def plan_admission(first, n_units: int, C: int, cursor: int, free_slots: int, n_live: int) -> int:
    """csrc/ttx_admit.h's plan_admission for a single pool (one job, not serial): units taken now."""
    min_admit = max(1, C // 4)
    if cursor >= n_units:
        return 0
    if n_live != 0 and free_slots < max(min_admit, first[cursor + 1] - first[cursor]):
        return 0
    take, end = 0, cursor
    while end < n_units:
        sz = first[end + 1] - first[end]
        if take + sz > free_slots:
            break
        take += sz
        end += 1
    return end - cursor


def run_pool(src_drafts: np.ndarray, keys, n: int, C: int, max_len: int, logits_of, seed: int, p: S.Params, sub_chunk: int = 0,
             defect: str | None = None, rows_fn=X.step_rows, accept_fn=None, admitted: dict | None = None) -> np.ndarray:
    """[S * n, max_len]: the sampling pool on the host.  Sources (their copy drafts ``src_drafts`` [S, N, D], in list order) are
    admitted in units of n rows into C slots under plan_admission; every step draws with the float64 sampler for (key[slot],
    sample[slot], position) on ``logits_of(source, prefix)`` and accepts under util_sample_spec's rule; ended rows go to
    out[row_of[slot]].  ``sub_chunk`` > 0 admits at most that many sources per k_pool_admit (the length buckets of an admission).
    ``defect`` plants one of the single defects tests/test_sample_pool_host.py lists.  ``admitted`` (a dict) receives every caller
    row as its admission left it (an ended row is later overwritten whole from its gen row)."""
    S_total, N, D = src_drafts.shape
    assert C >= n
    gen_ld = max_len + D + 2
    out = np.full((S_total * n, max_len), -7, dtype=np.int64)
    first = [s * n for s in range(S_total + 1)]
    act = np.zeros(C, dtype=np.int32)
    front = np.zeros(C, dtype=np.int32)
    key = np.full(C, -99, dtype=np.int64)
    sample = np.full(C, -99, dtype=np.int64)
    row_of = np.zeros(C, dtype=np.int32)
    src_of_slot = np.zeros(C, dtype=np.int64)          # which source's cross data a slot holds (the replicated K/V)
    gen = np.full((C, gen_ld), PAD, dtype=np.int32)
    drafts = np.zeros((C, N, D), dtype=np.int32)
    n_act, cursor, steps = 0, 0, 0
    while True:
        take = plan_admission(first, S_total, C, cursor, C - n_act, n_act)
        s0 = cursor
        while s0 < cursor + take:
            s1 = min(cursor + take, s0 + sub_chunk) if sub_chunk else cursor + take
            used = np.zeros(C, dtype=bool)
            used[act[:n_act]] = True
            free = np.nonzero(~used)[0]
            for i in range((s1 - s0) * n):
                b = int(free[i])
                src = s0 + i // n
                act[n_act + i] = b
                front[b] = 0
                gen[b] = PAD
                gen[b, 0] = BOS
                if defect != "stale_key":
                    key[b] = keys[src]
                    sample[b] = (i // n) if defect == "sample_div" else i % n
                elif key[b] == -99:
                    key[b], sample[b] = keys[src], i % n
                data_src = s0 + i if (defect == "data_of_row" and s0 + i < S_total) else src
                drafts[b] = src_drafts[data_src]
                src_of_slot[b] = data_src
                row_of[b] = s0 * n + i + (n if defect == "row_of_off" else 0)
                r = s0 * n + i
                out[r] = PAD
                if defect != "no_bos":
                    out[r, 0] = BOS
                if admitted is not None:
                    admitted[r] = out[r].copy()
            n_act += (s1 - s0) * n
            s0 = s1
        cursor += take
        if n_act == 0:
            break
        steps += 1
        assert steps <= (max_len + 2) * (S_total + 1), "the pool did not end by itself"
        st = U.LoopState(B=C, N=N, D=D, Ls=0, max_len=max_len, gen_ld=gen_ld, pad=PAD, bos=BOS, eos=EOS, V=0, row_rule=1, pool=1,
                         act_idx=act, front=front, gen=gen, drafts=drafts, rec=np.zeros((C, 5), dtype=np.int32),
                         out=np.zeros((C, max_len), dtype=np.int64), haspad=np.zeros(C, dtype=np.int32), traj=None, fin_step=None,
                         rstep=None, row_of=None, pool_out=None, pool_traj=None, pool_fin_step=None)
        st.words = dict.fromkeys(U.WORDS, 0)
        st.words.update(n_active=n_act, r_rows=n_act * N, m_rows=n_act * U.rps(N, D))
        pred = X.draw_step(st, lambda b, prefix: logits_of(int(src_of_slot[b]), prefix), key, sample, seed, p, rows_fn)
        rows = act[:n_act].copy()
        st = (accept_fn or X.sample_accept_step)(st, pred)
        act, front, gen = st.act_idx, st.front, st.gen
        fin = st.rec[:n_act, 4] == 1
        for b in rows[fin]:
            if 0 <= row_of[b] < len(out):
                out[row_of[b]] = gen[b, :max_len]
        n_act = int(st.words["n_active"])
    return out
