"""Plain restatement of the beam family of csrc/ttx_loop_kernels.hip.h (k_bs_prep, k_bs_list, k_bs_hits, k_bs_leaves /
beam_leaves_core, select_best_leaves / k_beam_select, k_beam_step, k_tree_cache), the operands of their kernel-level tests and the
checkers.  No GPU call in here: tests/test_beam_checks_host.py pins the restatement to the oracle (oracle/spec_beam.py:142-257,
oracle/drafting.py) and shows on the CPU that each checker fails when it should; tests/test_gpu_beam_loop_kernels.py holds the kernels
to it, one launch at a time (ttx_debug_bs_prep .. ttx_debug_tree_cache).

Every restatement returns the arrays a launch leaves behind, starting from sentinel-filled arrays (util_loop_checks.sentinel_array):
the rule's value in every element it writes, the sentinel in every element it does not.  A checker compares all of it; the guard
margins around the device arrays are util_loop_checks.Buf's.

EXACT (bit equality): everything k_bs_prep, k_bs_list, k_tree_cache and k_beam_select write (its scores are copied inputs, so the
order "higher score first, equal scores by enumeration order" is fully determined); of k_bs_leaves the best draft (a port of
ttxsel::topk1_index, pinned against torch.topk), best_n, chosen, the leaf counts, tokens and their ascending order (the top-K of a
row compares stored fp32 values, no arithmetic); of k_beam_step every integer given the (parent, token) pairs it names.

k_bs_hits: the reference is the float64 nucleus (sort, softmax, mass ranked above < 0.9975, at most K ranks).  A flag may differ
only where some rank's fp64 mass-above lies within HIT_MARGIN = 1e-5 of 0.9975 (the margin tests/test_gpu_beam_kernels.py uses for
the same arithmetic), such pairs may be at most HIT_CAP = 1 % of a case's pairs, and planted rows (plant_row: the mass crosses the
threshold at a chosen rank with margin >= PLANT_MARGIN = 1e-3, asserted) are never exempt.

SCORE BOUND (leaf scores of k_bs_leaves, new_score of k_beam_step).  The kernels evaluate, in fp32, per logits row x of V entries:
m = max x (exact); e_i = expf(x_i - m); z = sum of e_i, every lane adding n_l of them in sequence (n_l = VPL in topk_to_lanes,
ceil(V / 64) in k_beam_step) followed by 6 butterfly steps; l_i = logf(e_i / z).  With eps32 = 2^-23 (one ulp, relative), expf and
logf within 1 ulp, the division within 2.5 ulp (it is correctly rounded when the compiler's default holds), a rounding of eps32/2
per subtraction and addition, a_i = x_i - m and D = max |a_i| (D < 80 is asserted: no underflow):
    relative error of e_i   <=  eps32 * (|a_i| / 2 + 1)
    relative error of z     <=  eps32 * ((n_l + 6) / 2 + 1 + D / 2)          all terms positive: n_l + 6 additions, the worst e_i
    |error of l_i| = T_i    <=  eps32 * (|a_i| / 2 + 1 + 2.5 + |l_i|) + eps32 * ((n_l + 6) / 2 + 1 + D / 2)
A score is root + (((l_0 + l_1) + ..) + l_p), n_add sequential additions (p + 1 for a leaf at position p, 1 for k_beam_step), each
rounding at most eps32/2 of a partial sum no larger than S = |root| + sum |l_k|:
    bound  =  sum_k T_k  +  n_add * (eps32 / 2) * S
(score_bound).  The leaf of a finished candidate, root + logf(1 / (1 + (V-1) expf(-35))), has T = eps32 * 5.5.  The host test shows
for every test input that a numpy fp32 evaluation in this order stays inside the bound against float64, and that an error of four
bounds planted at one leaf is caught; on the GPU every case prints its largest error / bound.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np
import torch

import util_loop_checks as U

PAD, BOS, EOS = U.PAD, U.BOS, U.EOS
EPS32 = 2.0 ** -23
NUCLEUS, HIT_MARGIN, HIT_CAP, PLANT_MARGIN = 0.9975, 1e-5, 0.01, 1e-3
GAP = 1e-3                                   # separation of the planted k_beam_step totals
I32, I64, F32, U8 = np.int32, np.int64, np.float32, np.uint8
TORCH_OF = {np.dtype(U8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(I32): torch.int32, np.dtype(I64): torch.int64,
            np.dtype(F32): torch.float32}
BIG = 0x7FFFFFFF


def sent(shape, np_dtype) -> np.ndarray:
    return U.sentinel_array(shape if isinstance(shape, tuple) else (shape,), TORCH_OF[np.dtype(np_dtype)])


def bits(a: np.ndarray) -> np.ndarray:
    return a.view(I32) if a.dtype == F32 else a


def same(got: np.ndarray, want: np.ndarray, what: str) -> None:
    """Bit equality of two arrays (fp32 by its bit patterns, so sentinels and signed zeros count)."""
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    d = U.first_difference(bits(np.ascontiguousarray(got)), bits(np.ascontiguousarray(want)))
    assert d is None, f"{what}: {d}"


def upload(arrays: dict, device: str) -> dict:
    """name -> util_loop_checks.Buf holding the array (guard margins on either side)."""
    return {k: U.Buf(a.shape, TORCH_OF[a.dtype], device, a) for k, a in arrays.items()}


def download(bufs: dict, names) -> dict:
    out = {}
    for k in names:
        a = bufs[k].get()
        out[k] = a.view(F32) if bufs[k].dtype == torch.float32 else a
    return out


def check_margins(bufs: dict) -> None:
    for k, b in bufs.items():
        m = b.margins()
        assert m is None, f"{k}: {m}"


def check_inputs(bufs: dict, arrays: dict, names) -> None:
    for k in names:
        a = bufs[k].get()
        same(a.view(F32) if bufs[k].dtype == torch.float32 else a, arrays[k], f"input {k} was written")


def rps(N: int, D: int) -> int:
    return 1 + N * D


# ---------------------------------------------------------------------------------------------------------------------------
# ttxsel::topk1_index (csrc/ttx_select.h): which of several equal maxima torch.topk(1) on the CPU reports
def topk1_index(values) -> int:
    v = [int(x) for x in values]
    n = len(v)
    ix = list(range(n))
    if n <= 1:
        return 0

    def swap(a, b):
        v[a], v[b] = v[b], v[a]
        ix[a], ix[b] = ix[b], ix[a]

    def heap_select_one(lo, hi):
        for i in range(lo + 1, hi):
            if v[i] > v[lo]:
                swap(i, lo)

    if n >= 64:
        heap_select_one(0, n)
        return ix[0]
    lo, hi = 0, n
    depth = 2 * (n.bit_length() - 1)
    while hi - lo > 3:
        if depth == 0:
            heap_select_one(lo, hi)
            return ix[0]
        depth -= 1
        mid = lo + (hi - lo) // 2
        a, b, c = lo + 1, mid, hi - 1
        if v[a] > v[b]:
            med = b if v[b] > v[c] else (c if v[a] > v[c] else a)
        elif v[a] > v[c]:
            med = a
        elif v[b] > v[c]:
            med = c
        else:
            med = b
        swap(lo, med)
        first, last = lo + 1, hi
        while True:
            while v[first] > v[lo]:
                first += 1
            last -= 1
            while v[lo] > v[last]:
                last -= 1
            if not first < last:
                break
            swap(first, last)
            first += 1
        hi = first
    for i in range(lo + 1, hi):
        tv, ti = v[i], ix[i]
        if tv > v[lo]:
            for j in range(i, lo, -1):
                v[j], ix[j] = v[j - 1], ix[j - 1]
            v[lo], ix[lo] = tv, ti
        else:
            j = i
            while tv > v[j - 1]:
                v[j], ix[j] = v[j - 1], ix[j - 1]
                j -= 1
            v[j], ix[j] = tv, ti
    return ix[0]


# ---------------------------------------------------------------------------------------------------------------------------
# k_bs_prep
PREP_IN = ["cand_next", "len_next", "fin_next", "logp_next", "drafts_all", "lib"]
PREP_OUT = ["gen", "front", "len", "active", "finished", "logp", "per_cand", "drafts32"]


def bs_prep(c) -> dict:
    """Row -> the step's loop state and the candidate's draft slots.  All drafts: the N drafts of its source cut to dl tokens.
    Smart: the first N windows of the source's library whose first token equals the candidate's last token, in library order
    (window 0 if there is none, spec_beam.py:146-153); unused slots repeat the first.  Candidates at or beyond n_cand: active and
    per_cand 0, nothing else."""
    MC, ld, N, dl = c.max_cand, c.ld, c.N, c.dl
    o = dict(gen=sent((MC, ld), I32), front=sent(MC, I32), len=sent(MC, I32), active=sent(MC, U8), finished=sent(MC, U8),
             logp=sent(MC, F32), per_cand=sent(MC, I32), drafts32=sent((MC, N, dl), I32))
    for cc in range(MC):
        if cc >= c.n_cand:
            o["active"][cc], o["per_cand"][cc] = 0, 0
            continue
        lc, fin = int(c.len_next[cc]), int(c.fin_next[cc])
        o["gen"][cc] = c.cand_next[cc].astype(I32)
        o["len"][cc], o["front"][cc], o["finished"][cc], o["active"][cc] = lc, lc - 1, fin, 0 if fin else 1
        o["logp"][cc] = c.logp_next[cc]
        b = cc // c.beam
        if not c.smart:
            o["drafts32"][cc] = c.drafts_all[b, :, :dl]
            o["per_cand"][cc] = N
            continue
        match = np.flatnonzero(c.lib[b, :, 0] == c.cand_next[cc, lc - 1])
        if match.size == 0:
            match = np.array([0])
        match = match[:N]
        for n in range(N):
            o["drafts32"][cc, n] = c.lib[b, match[n] if n < len(match) else match[0], 1:dl + 1]
        o["per_cand"][cc] = len(match)
    return o


def check_exact(got: dict, want: dict, what: str) -> None:
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in want:
        same(got[k], want[k], f"{what}: {k}")


def prep_case(*, B, beam, n_cand, max_cand, dl, N, smart, V=40, n_lib=0, D0=0, seed=0):
    """Operands of one k_bs_prep launch.  Smart mode: the candidates of a source end, in turn, in a key without any window, with
    fewer than N, with exactly N and with more than N windows (the (N+1)-th in the library's next round of 256 when there is one)."""
    rng = np.random.default_rng(seed)
    ld = 9 + dl
    c = NS(B=B, beam=beam, n_cand=n_cand, max_cand=max_cand, dl=dl, N=N, smart=smart, pad=PAD, ld=ld, n_lib=n_lib, lib_ld=dl + 1, D0=D0)
    c.len_next = rng.integers(1, 8, size=max_cand).astype(I32)
    c.cand_next = np.full((max_cand, ld), PAD, dtype=I64)
    for cc in range(max_cand):
        c.cand_next[cc, :c.len_next[cc]] = rng.integers(20, V, size=c.len_next[cc])
        c.cand_next[cc, 0] = BOS
    c.fin_next = (rng.random(max_cand) < 0.3).astype(U8)
    c.logp_next = (-rng.random(max_cand) * 9).astype(F32)
    c.drafts_all = rng.integers(3, V, size=(B, N, max(D0, 1))).astype(I32) if not smart else np.zeros((1, 1, 1), I32)
    c.lib = np.zeros((1, 1, 1), I32)
    c.keys = None
    if smart:
        keys = [10, 11, 12, 13]                                            # none, fewer than N, exactly N, more than N windows
        c.lib = rng.integers(20, V, size=(B, n_lib, dl + 1)).astype(I32)
        for b in range(B):
            free = [int(i) for i in rng.permutation(n_lib)]

            def take(n, pred=lambda i: True):
                got = [i for i in free if pred(i)][:n]
                for i in got:
                    free.remove(i)
                return got
            c.lib[b, take(min(N - 1, n_lib // 4)), 0] = keys[1]
            if len(free) >= N:
                c.lib[b, take(N), 0] = keys[2]
            if len(free) >= N + 1:                                         # N windows, then the (N+1)-th in the next round of 256
                more = take(N, lambda i: i < 256)
                more += take(1, (lambda i: i >= 256) if n_lib > 256 else (lambda i: True))
                c.lib[b, more, 0] = keys[3]
        c.keys = keys
        for cc in range(n_cand):
            c.cand_next[cc, c.len_next[cc] - 1] = keys[cc % 4]
            if c.len_next[cc] == 1:                                        # keep <BOS> in front of the key
                c.len_next[cc] = 2
                c.cand_next[cc, 0], c.cand_next[cc, 1] = BOS, keys[cc % 4]
    return c


def prep_arrays(c) -> dict:
    a = {k: getattr(c, k) for k in PREP_IN}
    a.update(bs_prep(c))
    for k in PREP_OUT:
        a[k] = sent(a[k].shape, a[k].dtype)
    return a


# ---------------------------------------------------------------------------------------------------------------------------
# k_bs_list
LIST_OUT = ["act_idx", "slot_of", "prev_len", "summary"]


def bs_list(active, per_cand, length, n_cand: int, N: int, dl: int, counters, rows: int):
    """Compact list of the running candidates in candidate order, candidate -> slot (-1: not running), the lengths, the DecState
    of the verify step, the counters of the iteration added to ``counters`` (8 words; max_group is set, not added) and the reset of
    the selection summary.  Returns (arrays over ``rows`` elements, 8 counter words, 13 DecState words)."""
    act = np.flatnonzero(active[:n_cand] != 0)
    na = len(act)
    o = dict(act_idx=sent(rows, I32), slot_of=sent(rows, I32), prev_len=sent(rows, I32), summary=np.array([0, BIG, 0, 0, 0], I32))
    o["act_idx"][:na] = act
    o["slot_of"][:n_cand] = -1
    o["slot_of"][act] = np.arange(na)
    o["prev_len"][:n_cand] = length[:n_cand]
    pc = per_cand[:n_cand].astype(np.int64)
    run = int(pc[act].sum())
    cnt = [int(x) for x in counters]
    cnt[0] += 1
    cnt[1] += int(pc.sum())
    cnt[2] += run
    cnt[3] += na + run * dl
    cnt[4] += na * rps(N, dl)
    cnt[5] += int((length[act].astype(np.int64) - 1).sum())
    cnt[6] += na
    cnt[7] = int(pc.max()) if n_cand else 0
    state = [na, na * N, na * rps(N, dl)] + [0] * 10
    return o, cnt, state


# ---------------------------------------------------------------------------------------------------------------------------
# the nucleus (k_bs_hits) in float64
def order_desc(x: np.ndarray) -> np.ndarray:
    """Columns of every row by value, largest first, equal values by lower index (x: [rows, V] without NaN)."""
    return np.argsort(-x.astype(np.float64), axis=-1, kind="stable")


def nucleus64(rows: np.ndarray, K: int):
    """Per row: the kept tokens [rows, K] (-1 where a rank is not kept) and whether some rank's mass-above is within HIT_MARGIN of
    the threshold.  Rank 0 is always kept; rank r while the softmax mass of the ranks above it is below 0.9975; at most K."""
    x = rows.astype(np.float64)
    V = x.shape[1]
    k = min(K, V)
    order = order_desc(rows)[:, :k]
    p = np.exp(x - x.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    ps = np.take_along_axis(p, order, axis=1)
    above = np.concatenate([np.zeros((len(x), 1)), np.cumsum(ps, axis=1)[:, :-1]], axis=1)
    keep = above < NUCLEUS
    keep[:, 0] = True
    kept = np.where(keep, order, -1)
    near = (np.abs(above[:, 1:] - NUCLEUS) < HIT_MARGIN).any(axis=1)
    margin = np.abs(above[:, 1:] - NUCLEUS).min(axis=1) if k > 1 else np.full(len(x), np.inf)
    if k < K:
        kept = np.concatenate([kept, np.full((len(x), K - k), -1)], axis=1)
    return kept, near, margin


def plant_row(V: int, K: int, r: int, rng, dup_at: int | None = None):
    """A logits row whose kept set is exactly the ranks [0, r): r < K: the mass above rank r-1 is below and the mass above rank r
    is above the threshold by more than PLANT_MARGIN; r == K: every rank below K is kept by mass and rank K falls to n_best.
    ``dup_at`` = q: the tokens of ranks q and q + 1 hold the same logit, the lower id taking rank q.  Returns (row, tokens by rank)."""
    assert 1 <= r <= min(K, V)
    p = np.empty(V)
    if r < K and r < V:
        if r == 1:
            head = np.array([0.999])
        else:                                                             # ranks < r-1 share 0.989; rank r-1 lifts the mass to 0.999
            w = np.linspace(1.2, 1.0, r - 1)
            head = np.append(0.989 * w / w.sum(), 0.01)
        tail = np.linspace(2.0, 1.0, V - r)
        p[:r], p[r:] = head, tail / tail.sum() * 0.001
    else:                                                                 # slowly decreasing: ranks < K hold well under 0.9975
        w = np.linspace(2.0, 1.0, V)
        p = w / w.sum()
    assert (np.diff(p) < 0).all() or dup_at is not None
    if dup_at is not None:
        p[dup_at + 1] = p[dup_at]
    toks = rng.permutation(V)
    if dup_at is not None and toks[dup_at] > toks[dup_at + 1]:
        toks[[dup_at, dup_at + 1]] = toks[[dup_at + 1, dup_at]]
    row = np.empty(V, F32)
    row[toks] = (np.log(p) + 3.0).astype(F32)
    return row, toks


HITS_IN = ["logits", "finished", "slot_of", "per_cand", "drafts32", "dl_of"]


def hits_case(*, V, K, N, dl, n_cand, max_cand, pool=False, seed=0):
    """Operands of one k_bs_hits launch: random rows (randn * 4) and, spread over the pairs, planted rows with the draft token at
    rank r-1 (hit), r (miss), K-1 (hit), K (miss by n_best) and on either token of a duplicated logit at ranks K-1 / K."""
    rng = np.random.default_rng(seed)
    c = NS(V=V, K=K, N=N, dl=dl, n_cand=n_cand, max_cand=max_cand)
    c.finished = np.zeros(max_cand, U8)
    if n_cand > 2:
        c.finished[1] = 1
    run = [cc for cc in range(n_cand) if not c.finished[cc]]
    c.slot_of = np.full(max_cand, -1, I32)
    c.slot_of[run] = rng.permutation(len(run))                             # not the identity
    c.per_cand = np.zeros(max_cand, I32)
    c.per_cand[:n_cand] = N
    if n_cand > 1:
        c.per_cand[run[-1]] = max(1, N // 2)                               # smart mode's shorter groups
    c.drafts32 = rng.integers(0, V, size=(max_cand, N, dl)).astype(I32)
    c.dl_of = np.full(max_cand, dl, I32)
    if pool and dl > 1:
        c.dl_of[run[0]] = dl - 1
        c.dl_of[run[-1]] = max(dl // 2, 1)
    c.pool = pool
    R = rps(N, dl)
    c.logits = (rng.standard_normal((len(run) * R, V)) * 4).astype(F32)
    c.planted = np.zeros((max_cand, N * dl), bool)
    kk = min(K, V)
    spots = [(cc, i, j) for cc in run for i in range(int(c.per_cand[cc])) for j in range(int(c.dl_of[cc] if pool else dl)) if j > 0 or i == 0]
    plans = []
    for r in sorted({1, 2, max(kk // 2, 1), kk - 1} - {0}):
        if r < kk:
            plans += [(r, r - 1, None), (r, r, None)]                      # (kept ranks, rank of the draft token, duplicate)
    plans += [(kk, kk - 1, None)]
    if kk < V:
        plans += [(kk, kk, None)]
        if kk >= 1:
            plans += [(kk, kk - 1, kk - 1), (kk, kk, kk - 1)]              # equal logits at ranks K-1 and K: the lower id is inside
    if kk >= 3:
        plans += [(kk, 1, 1), (kk, 2, 1)]                                  # equal logits inside the kept set: both are hits
    c.plans = []
    assert len(spots) >= len(plans) or dl == 0, "too few pairs for the planted rows"
    for (r, at, dup), (cc, i, j) in zip(plans, [spots[t] for t in rng.permutation(len(spots))[:len(plans)]]):
        row, toks = plant_row(V, K, r, rng, dup)
        srow = 0 if j == 0 else 1 + i * dl + (j - 1)
        c.logits[c.slot_of[cc] * R + srow] = row
        c.drafts32[cc, i, j] = toks[at]
        c.planted[cc, i * dl + j] = True
        c.plans.append((r, at, dup, cc, i, j))
    return c


def bs_hits(c):
    """The flag of every (draft, position) pair a launch writes, with what the checker needs: ``want`` (sentinel where nothing is
    written), ``written``, ``near`` (a rank's fp64 mass-above within HIT_MARGIN of the threshold) and ``margin``."""
    N, dl, K, R = c.N, c.dl, c.K, rps(c.N, c.dl)
    want = sent((c.max_cand, N * dl), U8)
    written = np.zeros(want.shape, bool)
    near = np.zeros(want.shape, bool)
    margin = np.full(want.shape, np.inf)
    for cc in range(c.n_cand):
        if c.finished[cc]:
            continue
        pairs = [(i, j) for i in range(int(c.per_cand[cc])) for j in range(dl) if not c.pool or j < c.dl_of[cc]]
        if not pairs:
            continue
        rows = np.array([c.slot_of[cc] * R + (0 if j == 0 else 1 + i * dl + (j - 1)) for i, j in pairs])
        kept, nr, mg = nucleus64(c.logits[rows], K)
        for t, (i, j) in enumerate(pairs):
            p = i * dl + j
            want[cc, p] = 1 if (kept[t] == c.drafts32[cc, i, j]).any() else 0
            written[cc, p], near[cc, p], margin[cc, p] = True, nr[t], mg[t]
    return NS(want=want, written=written, near=near, margin=margin)


def check_hits(got: np.ndarray, c, ref, what: str) -> int:
    """Flags equal the fp64 nucleus except, at most, at pairs inside the margin that are not planted; those pairs are at most HIT_CAP
    of the case's; the planted rows keep PLANT_MARGIN; unwritten flags hold the sentinel.  Returns the number of flags that differ."""
    n = int(ref.written.sum())
    exempt = ref.near & ~c.planted & ref.written
    assert int(exempt.sum()) <= HIT_CAP * n, f"{what}: {int(exempt.sum())} of {n} pairs lie inside the margin (cap {HIT_CAP:.0%})"
    assert (ref.margin[c.planted] >= PLANT_MARGIN).all(), f"{what}: a planted row is closer than {PLANT_MARGIN} to the threshold"
    assert c.planted[ref.written].sum() == c.planted.sum(), f"{what}: a planted pair is not among the written ones"
    same(got[~ref.written], ref.want[~ref.written], f"{what}: flags outside the pairs of running candidates")
    diff = (got != ref.want) & ref.written
    bad = diff & ~exempt
    assert not bad.any(), (f"{what}: {int(bad.sum())} flags differ outside the margin, first at (candidate, pair) "
                           f"{tuple(int(v) for v in np.argwhere(bad)[0])}, margin {ref.margin[bad][0]:.3g}")
    return int(diff.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# log-softmax with its error bound; fp32 evaluation in the kernels' order
def lsm64(row: np.ndarray, n_l: int):
    """(l, T): log(exp(x - m) / z) in float64 and the bound T of the module docstring on the fp32 value of every element."""
    x = row.astype(np.float64)
    a = x - x.max()
    D = float(np.abs(a).max())
    assert D < 80.0, "the bound assumes no underflow of expf(x - m)"
    e = np.exp(a)
    l = np.log(e / e.sum())
    T = EPS32 * (np.abs(a) / 2 + 1 + 2.5 + np.abs(l)) + EPS32 * ((n_l + 6) / 2 + 1 + D / 2)
    return l, T


def lsm32(row: np.ndarray, n_l: int) -> np.ndarray:
    """The same in fp32 in the kernels' order: 64 lanes add n_l terms each in sequence, then 6 butterfly steps."""
    x = row.astype(F32)
    V = len(x)
    assert V <= 64 * n_l
    e = np.exp((x - x.max()).astype(F32)).astype(F32)
    pad = np.zeros(64 * n_l, F32)
    pad[:V] = e
    lanes = np.zeros(64, F32)
    for i in range(n_l):
        lanes = (lanes + pad[64 * i:64 * i + 64]).astype(F32)
    o = 32
    while o:
        lanes = (lanes + lanes[np.arange(64) ^ o]).astype(F32)
        o >>= 1
    return np.log((e / lanes[0]).astype(F32)).astype(F32)


def score_bound(root: float, ls, Ts) -> float:
    """Bound on root + (((l_0 + l_1) + ..) + l_p) evaluated in fp32 (module docstring)."""
    ls = np.abs(np.asarray(ls, np.float64))
    n_add = len(ls)
    return float(np.sum(Ts) + n_add * (EPS32 / 2) * (abs(float(root)) + ls.sum()))


def vpl_for(V: int) -> int:
    return 4 if V <= 256 else (8 if V <= 512 else 16)


# ---------------------------------------------------------------------------------------------------------------------------
# k_bs_leaves
LEAVES_IN = ["logits", "finished", "slot_of", "per_cand", "drafts32", "logp", "hit", "live", "dl_of", "grp_of", "cand_batch"]
LEAVES_OUT = ["best_n", "best_slot", "chosen", "leaf_score", "leaf_tok", "leaf_cnt"]


def leading(flags: np.ndarray, limit: int) -> int:
    n = 0
    while n < limit and flags[n]:
        n += 1
    return n


def best_draft(c, cc: int):
    """(best slot, its accepted length): leading hits of every draft of the candidate (none for a finished one), then topk(1) over the
    N drafts or, in smart mode, over the table padded with -1 to the longest group (of the batch, in the pool)."""
    pc = int(c.per_cand[cc])
    dl_c = int(c.dl_of[cc]) if c.pool else c.dl
    nok = [0 if c.finished[cc] else leading(c.hit[cc, i * c.dl:(i + 1) * c.dl], dl_c) for i in range(pc)]
    W = c.N if not c.smart else (int(c.grp_of[c.cand_batch[cc]]) if c.pool else c.max_group)
    best = topk1_index([nok[i] if i < pc else -1 for i in range(W)])
    return best, nok[best]


def bs_leaves(c, fp32: bool = False):
    """Everything a k_bs_leaves launch writes.  Scores: float64 with ``bound`` per leaf, or (``fp32``) the numpy fp32 evaluation in
    the kernel's order.  Leaf = (candidate, position p <= n_accepted along the chosen draft, token): the K largest logits of the
    position, minus the accepted token (p < n_accepted), minus <BOS> at the first rejected position (p == n_accepted < the draft
    length in force), minus logits that are exactly 0; ascending token id.  Score = log-prob of the root + log-softmax of the kept
    tokens in position order + log-softmax of the leaf token."""
    MC, N, dl, K, V = c.max_cand, c.N, c.dl, c.K, c.V
    dl1, R, n_l = dl + 1, rps(N, dl), c.vpl or vpl_for(V)
    o = dict(best_n=sent(MC, I32), best_slot=sent(MC, I32), chosen=sent((MC, dl), I64), leaf_score=sent((MC, dl1, K), F32),
             leaf_tok=sent((MC, dl1, K), I32), leaf_cnt=sent((MC, dl1), I32))
    score = np.full((MC, dl1, K), np.nan)
    bound = np.full((MC, dl1, K), np.nan)
    for cc in range(c.n_cand):
        if c.pool and not c.live[cc]:
            o["leaf_cnt"][cc] = 0
            continue
        best, nacc = best_draft(c, cc)
        o["best_slot"][cc], o["best_n"][cc] = best, nacc
        o["chosen"][cc] = c.drafts32[cc, best]
        o["leaf_cnt"][cc] = 0
        root = float(c.logp[cc])
        if c.finished[cc]:
            o["leaf_cnt"][cc, 0], o["leaf_tok"][cc, 0, 0] = 1, PAD
            score[cc, 0, 0] = root + np.log(1.0 / (1.0 + (V - 1) * np.exp(-35.0)))
            bound[cc, 0, 0] = EPS32 * 5.5 + (EPS32 / 2) * abs(root)
            o["leaf_score"][cc, 0, 0] = F32(root) + np.log(F32(1.0) / (F32(1.0) + F32(V - 1) * np.exp(F32(-35.0))))
            continue
        dl_c = int(c.dl_of[cc]) if c.pool else dl
        kept_l, kept_T, kept32 = [], [], []
        for p in range(nacc + 1):
            row = c.logits[c.slot_of[cc] * R + (0 if p == 0 else 1 + best * dl + (p - 1))]
            l, T = lsm64(row, n_l)
            l32 = lsm32(row, n_l) if fp32 else None
            order = [t for t in order_desc(row[None])[0] if row[t] > -np.inf][:K]
            excl = int(c.drafts32[cc, best, p]) if p < nacc else (BOS if p < dl_c else -1)
            toks = sorted(int(t) for t in order if t != excl and row[t] != 0.0)
            o["leaf_cnt"][cc, p] = len(toks)
            for i, t in enumerate(toks):
                o["leaf_tok"][cc, p, i] = t
                ls, Ts = kept_l + [l[t]], kept_T + [T[t]]
                score[cc, p, i] = root + sum(ls)
                bound[cc, p, i] = score_bound(root, ls, Ts)
                if fp32:
                    acc = F32(0.0)
                    for q, v in enumerate(kept32):
                        acc = v if q == 0 else F32(acc + v)
                    o["leaf_score"][cc, p, i] = F32(root) + (l32[t] if p == 0 else F32(acc + l32[t]))
            if p < nacc:
                tk = int(c.drafts32[cc, best, p])
                kept_l.append(l[tk]); kept_T.append(T[tk])
                if fp32:
                    kept32.append(l32[tk])
    return NS(out=o, score=score, bound=bound)


def check_leaves(got: dict, c, ref, what: str) -> float:
    """Exact: best_n, best_slot, chosen, counts, tokens and their order, sentinels everywhere else (scores beyond a count included).
    Scores: within the derived bound of float64.  Returns the largest error / bound."""
    for k in ("best_n", "best_slot", "chosen", "leaf_cnt", "leaf_tok"):
        same(got[k], ref.out[k], f"{what}: {k}")
    real = ~np.isnan(ref.score)
    same(got["leaf_score"][~real], sent(1, F32).repeat(int((~real).sum())), f"{what}: leaf_score beyond the leaves")
    g = got["leaf_score"][real].astype(np.float64)
    assert np.isfinite(g).all(), f"{what}: a leaf score is not finite"
    ratio = np.abs(g - ref.score[real]) / ref.bound[real]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, (f"{what}: leaf score off by {worst:.2f} bounds at (candidate, position, leaf) "
                          f"{tuple(int(v) for v in np.argwhere(real)[int(ratio.argmax())])}")
    return worst


def width_sensitive(N: int, rng):
    """Accepted lengths of pc < N drafts whose topk(1) over the table padded with -1 to width W differs from the choice at width pc
    (the reason the pool hands k_bs_leaves the batch's group width): (lengths, W)."""
    for _ in range(20000):
        pc = int(rng.integers(2, N))
        nok = rng.integers(0, 3, size=pc)
        own = topk1_index(nok)
        for W in range(pc + 1, N + 1):
            if topk1_index(list(nok) + [-1] * (W - pc)) != own:
                return [int(v) for v in nok], W
    raise AssertionError("no width-sensitive draft table found")


def leaves_case(*, V, K, N, dl, n_cand, max_cand, smart=False, pool=False, vpl=0, seed=0):
    """Operands of one k_bs_leaves launch.  The hit flags are the test's own (leading ones up to a planned accepted length, a zero,
    then noise), so that candidate cc's best draft accepts cc % (dl + 1) tokens and every length 0 .. dl occurs when there are
    enough candidates; the rows along the chosen draft carry, in turn: a logit that is exactly 0 inside the top K, <BOS> on top at
    the first rejected position (at position dl it stays a leaf), the accepted token on top."""
    rng = np.random.default_rng(seed)
    c = NS(V=V, K=K, N=N, dl=dl, n_cand=n_cand, max_cand=max_cand, smart=smart, pool=pool, vpl=vpl, bos=BOS, pad=PAD, max_group=0)
    c.finished = np.zeros(max_cand, U8)
    if n_cand > 2:
        c.finished[2] = 1
    c.live = np.ones(max_cand, U8)
    if pool and n_cand > 3:
        c.live[3] = 0
    c.live[n_cand:] = 0
    alive = [cc for cc in range(n_cand) if c.live[cc]]
    run = [cc for cc in alive if not c.finished[cc]]
    c.slot_of = np.full(max_cand, -1, I32)
    c.slot_of[run] = rng.permutation(len(run))
    c.per_cand = np.zeros(max_cand, I32)
    c.per_cand[alive] = N if not smart else rng.integers(1, N + 1, size=len(alive))
    c.drafts32 = rng.integers(3, V, size=(max_cand, N, dl)).astype(I32)
    c.logp = (-rng.random(max_cand) * 9).astype(F32)
    c.dl_of = np.full(max_cand, dl, I32)
    c.cand_batch = (np.arange(max_cand) % 2).astype(I32)
    c.grp_of = np.array([N, N], I32)
    if pool and dl > 1 and len(run) > 1:
        c.dl_of[run[1]] = dl - 1
    c.hit = (rng.random((max_cand, N * dl)) < 0.5).astype(U8)
    c.sensitive = None
    for cc in alive:
        pc = int(c.per_cand[cc])
        dl_c = int(c.dl_of[cc])
        top = cc % (dl_c + 1)
        lens = [top] + [int(rng.integers(max(top - 1, 0), top + 1)) for _ in range(pc - 1)]      # ties among the drafts
        lens = [lens[t] for t in rng.permutation(pc)]
        if smart and pool and c.sensitive is None and N >= 3 and dl >= 2 and not c.finished[cc]:
            lens, W = width_sensitive(N, rng)
            c.per_cand[cc], pc = len(lens), len(lens)
            c.grp_of[c.cand_batch[cc]] = W
            c.sensitive = (cc, W)
        for i in range(pc):
            c.hit[cc, i * dl:i * dl + lens[i]] = 1
            if lens[i] < dl:
                c.hit[cc, i * dl + lens[i]] = 0
    if smart and pool:
        for b in range(2):
            c.grp_of[b] = max(int(c.grp_of[b]) if c.sensitive and c.cand_batch[c.sensitive[0]] == b else 0,
                              max([int(c.per_cand[cc]) for cc in alive if c.cand_batch[cc] == b], default=1))
    c.max_group = int(c.per_cand[:n_cand].max()) if n_cand else 0
    R = rps(N, dl)
    c.logits = (rng.standard_normal((max(len(run), 1) * R, V)) * 4).astype(F32)
    c.features = set()
    for cc in run:                                                         # the rows along the chosen draft
        best, nacc = best_draft(c, cc)
        dl_c = int(c.dl_of[cc]) if pool else dl
        for p in range(nacc + 1):
            row = c.logits[c.slot_of[cc] * R + (0 if p == 0 else 1 + best * dl + (p - 1))]
            kind = (cc + p) % 3
            top = float(row.max())
            if p == nacc and (kind != 0 or nacc == dl_c):
                row[BOS] = top + 1.0                                       # excluded at the first rejected position, a leaf at dl
                c.features.add("bos_kept" if nacc == dl_c else "bos_excluded")
            elif p < nacc and kind == 1:
                row[c.drafts32[cc, best, p]] = top + 0.5                   # the accepted token inside the top K: excluded
                c.features.add("accepted_excluded")
            elif kind == 0:
                q = min(2, min(K, V) - 1)
                row -= np.sort(row)[::-1][q]                               # the rank-q logit becomes exactly 0: no leaf
                c.features.add("zero_logit")
    return c


def leaves_arrays(c) -> dict:
    a = {k: getattr(c, k) for k in LEAVES_IN}
    for k, v in bs_leaves(c).out.items():
        a[k] = sent(v.shape, v.dtype)
    return a


# ---------------------------------------------------------------------------------------------------------------------------
# select_best_leaves / k_beam_select
SELECT_IN = ["leaf_score", "leaf_tok", "leaf_cnt", "cand", "len", "chosen", "chosen_slot", "finished"]
SELECT_OUT = ["new_cand", "new_logp", "parent", "parent_draft", "mark", "summary", "new_len", "new_finished"]


def best_leaves(scores: np.ndarray, cnt: np.ndarray, K: int):
    """The K best of one source's leaves: scores [nseg, K], cnt [nseg] -> [(segment, i)] best first, equal scores in enumeration
    order (segment-major); None when there are fewer than K leaves."""
    leaves = [(seg, i) for seg in range(len(cnt)) for i in range(int(cnt[seg]))]
    if len(leaves) < K:
        return None
    order = sorted(range(len(leaves)), key=lambda e: (-float(scores[leaves[e]]), e))
    return [leaves[e] for e in order[:K]]


def beam_select(c) -> dict:
    """Everything k_beam_select writes: per source the K new rows (root tokens, the kept draft tokens, the leaf token, PAD up to
    column len + dl; columns < width only), their scores (the leaves' own bits), parents, the parents' chosen draft slot, accepted
    marks (-1 under a finished root) and the summary sums; a source with fewer than K leaves sets summary[4] and writes nothing."""
    B, beam, dl, K, dl1 = c.B, c.beam, c.dl, c.K, c.dl + 1
    nseg = beam * dl1
    o = dict(new_cand=sent((B * K, c.ld_out), I64), new_logp=sent(B * K, F32), parent=sent(B * K, I32), parent_draft=sent(B * K, I32),
             mark=sent(B * K, I32), summary=c.summary.copy(), new_len=sent(B * K, I32), new_finished=sent(B * K, U8))
    sc = c.leaf_score.reshape(B, nseg, K)
    tk = c.leaf_tok.reshape(B, nseg, K)
    cn = c.leaf_cnt.reshape(B, nseg)
    for b in range(B):
        win = best_leaves(sc[b], cn[b], K)
        if win is None:
            o["summary"][4] = 1
            continue
        for r, (seg, i) in enumerate(win):
            cl, p = divmod(seg, dl1)
            cc, out, tok = b * beam + cl, b * K + r, int(tk[b, seg, i])
            lc = int(c.len[cc])
            row = c.cand[cc, :c.width].astype(I64)
            for j in range(dl1):
                if lc + j < c.width:
                    row[lc + j] = c.chosen[cc, j] if j < p else (tok if j == p else c.pad)
            o["new_cand"][out, :c.width] = row
            o["new_logp"][out] = sc[b, seg, i]
            o["parent"][out], o["parent_draft"][out] = cc, c.chosen_slot[cc]
            fin = bool(c.finished[cc])
            o["mark"][out] = -1 if fin else p
            eos = fin or tok == c.eos
            real = lc + p if tok == c.pad else lc + p + 1
            o["new_len"][out], o["new_finished"][out] = real, 1 if eos else 0
            o["summary"][0] += 1 if eos else 0
            o["summary"][1] = min(int(o["summary"][1]), c.width - real)
            if not fin:
                o["summary"][2] += p
                o["summary"][3] += 1
    return o


def select_case(*, B, beam, K, dl, pattern="random", ld_extra=0, seed=0):
    """Operands of one k_beam_select launch.  ``pattern`` shapes the leaves of source 0 (the other sources stay random):
    random; ties (one score shared inside a segment, across the segments of a quarter and across the quarters, so only enumeration
    order decides); one_quarter (every winner in the last quarter of the strided entries); sparse (the first quarter holds fewer than
    K leaves); neg_inf (valid leaves with score -inf among the winners); exact (exactly K leaves); short (K - 1 leaves)."""
    rng = np.random.default_rng(seed)
    dl1 = dl + 1
    nseg, n_cand = beam * dl1, B * beam
    width = 6 + dl1
    c = NS(B=B, beam=beam, K=K, dl=dl, pad=PAD, eos=EOS, width=width, ld_in=width + ld_extra, ld_out=width + 2 * ld_extra, pattern=pattern)
    c.len = rng.integers(1, 6, size=n_cand).astype(I32)
    c.cand = np.full((n_cand, c.ld_in), PAD, I32)
    for cc in range(n_cand):
        c.cand[cc, :c.len[cc]] = rng.integers(3, 90, size=c.len[cc])
    c.cand[:, width:] = 77                                                 # beyond the logical width: never copied
    c.chosen = rng.integers(3, 90, size=(n_cand, dl)).astype(I64)
    c.chosen_slot = rng.integers(0, 64, size=n_cand).astype(I32)
    c.finished = (rng.random(n_cand) < 0.3).astype(U8)
    c.finished[::beam] = 0                                                 # a source keeps one running candidate
    c.leaf_cnt = rng.integers(0, K + 1, size=(n_cand, dl1)).astype(I32)
    for cc in np.flatnonzero(c.finished):
        c.leaf_cnt[cc] = 0
        c.leaf_cnt[cc, 0] = 1                                              # a finished root has its one PAD leaf
    c.leaf_score = (-rng.random((n_cand, dl1, K)) * 20).astype(F32)
    c.leaf_tok = rng.choice([PAD, EOS, 5, 6, 7, 8], size=(n_cand, dl1, K), p=[0.15, 0.2, 0.2, 0.15, 0.15, 0.15]).astype(I32)
    for cc in np.flatnonzero(c.finished):
        c.leaf_tok[cc, 0, 0] = PAD
    c.summary = np.array([0, BIG, 0, 0, 0], I32)
    cn, sc = c.leaf_cnt[:beam].reshape(nseg), c.leaf_score[:beam].reshape(nseg, K)      # views of source 0
    per_wave = (nseg * K + 3) // 4
    if pattern == "ties":
        cn[:] = rng.integers(1, K + 1, size=nseg)
        sc[:] = F32(-3.25)
        sc[rng.random((nseg, K)) < 0.3] = F32(-7.5)
    elif pattern == "one_quarter":
        cn[:] = K
        sc[:] = (-20 - rng.random((nseg, K)) * 5).astype(F32)
        flat = sc.reshape(-1)
        lo = 3 * per_wave if nseg * K > 3 * per_wave else 0
        flat[lo:] = (-rng.random(len(flat) - lo)).astype(F32)
    elif pattern == "sparse":
        first = [s for s in range(nseg) if s * K < per_wave]
        assert len(first) < nseg
        cn[:] = K
        cn[first] = 0
        if K > 1:
            cn[first[0]] = K - 1
            sc[first[0]] = (F32(-0.001) * (1 + np.arange(K))).astype(F32)   # the quarter's few leaves are the best ones
    elif pattern == "neg_inf":
        cn[:] = 0
        segs = rng.permutation(nseg)[:max(2, min(nseg, 4))]
        cn[segs] = K
        sc[segs] = F32(-np.inf)
        sc[segs[0], 0] = F32(-1.0)
    elif pattern in ("exact", "short"):
        want = K if pattern == "exact" else K - 1
        cn[:] = 0
        for _ in range(want):
            free = np.flatnonzero(cn < K)
            cn[free[rng.integers(len(free))]] += 1
    if pattern != "random":
        c.finished[:beam] = 0                                              # the pattern's counts are not "one PAD leaf"
    for b in range(0 if pattern == "random" else 1, B):                    # every other source has its K leaves
        own = c.leaf_cnt[b * beam:(b + 1) * beam]
        if own.sum() < K:
            free = [cl for cl in range(beam) if not c.finished[b * beam + cl]]
            own[free[0], 0] = K
    return c


def select_arrays(c) -> dict:
    a = {k: getattr(c, k) for k in SELECT_IN}
    for k, v in beam_select(c).items():
        a[k] = v.copy() if k == "summary" else sent(v.shape, v.dtype)
    a["summary"] = c.summary.copy()
    return a


# ---------------------------------------------------------------------------------------------------------------------------
# k_beam_step
STEP_IN = ["logits", "slot_of", "finished", "score", "gen"]
STEP_OUT = ["new_cand", "new_score", "parent", "new_len", "new_finished", "parent_draft", "summary"]


def step_rows(c) -> np.ndarray:
    """[n_cand, V] the distribution every candidate is expanded with: its logits row, or 35 on PAD and 0 elsewhere once finished."""
    x = np.zeros((c.B * c.beam, c.V), F32)
    for cc in range(c.B * c.beam):
        if c.finished[cc]:
            x[cc, c.pad] = 35.0
        else:
            x[cc] = c.logits[c.slot_of[cc]]
    return x


def step_totals(c, fp32: bool = False):
    """total[candidate, token] = score + log-softmax in float64 with the bound of every total (or the fp32 evaluation)."""
    x = step_rows(c)
    n_l = -(-c.V // 64)
    if fp32:
        return np.stack([(F32(c.score[cc]) + lsm32(x[cc], n_l)).astype(F32) for cc in range(len(x))])
    tot, bnd = np.empty(x.shape), np.empty(x.shape)
    for cc in range(len(x)):
        l, T = lsm64(x[cc], n_l)
        tot[cc] = float(c.score[cc]) + l
        bnd[cc] = T + (EPS32 / 2) * (abs(float(c.score[cc])) + np.abs(l))
    return tot, bnd


def step_outputs(c, picks, scores) -> dict:
    """The arrays of a k_beam_step launch that selected ``picks[b]`` = [(beam index, token)] with ``scores[b]``."""
    B, beam, K = c.B, c.beam, c.K
    o = dict(new_cand=sent((B * K, c.ld), I64), new_score=sent(B * K, F32), parent=sent(B * K, I32), new_len=sent(B * K, I32),
             new_finished=sent(B * K, U8), parent_draft=sent(B * K, I32), summary=c.summary.copy())
    for b in range(B):
        for r, (k, tok) in enumerate(picks[b]):
            cc, out = b * beam + k, b * K + r
            o["new_cand"][out] = PAD
            o["new_cand"][out, :c.width] = c.gen[cc, :c.width]
            o["new_cand"][out, c.width] = tok
            o["new_score"][out] = scores[b][r]
            o["parent"][out], o["parent_draft"][out], o["new_len"][out] = cc, 0, c.width + 1
            eos = bool(c.finished[cc]) or tok == c.eos
            o["new_finished"][out] = 1 if eos else 0
            o["summary"][0] += 1 if eos else 0
    return o


def step_exact_order(c):
    """Planted cases: the float64 order of every source's totals (ties: lower flat index), valid when the top K + 1 are either
    separated by >= GAP or bit-equal by construction (same logit in identical rows under identical scores) -- asserted."""
    tot, _ = step_totals(c)
    x = step_rows(c)
    picks = []
    for b in range(c.B):
        t = tot[b * c.beam:(b + 1) * c.beam].reshape(-1)
        order = sorted(range(len(t)), key=lambda i: (-t[i], i))[:c.K + 1]
        for u, w in zip(order[:-1], order[1:]):
            ku, vu, kw, vw = u // c.V, u % c.V, w // c.V, w % c.V
            cu, cw = b * c.beam + ku, b * c.beam + kw
            tied = (x[cu] == x[cw]).all() and c.score[cu] == c.score[cw] and x[cu, vu] == x[cw, vw]
            assert tied or t[u] - t[w] >= GAP, f"source {b}: totals {t[u]!r} and {t[w]!r} are neither planted ties nor {GAP} apart"
        picks.append([(i // c.V, i % c.V) for i in order[:c.K]])
    return picks


def check_step(got: dict, c, what: str, exact: bool) -> float:
    """k_beam_step against float64.  Always: every reported score within the bound of the fp64 total of the (parent, token) it
    names, and every other array exactly what that selection implies.  ``exact`` (planted gaps and ties): the selection is the
    float64 order.  Otherwise: scores non-increasing, (parent, token) pairs distinct, no unselected fp64 total above the smallest
    selected one by more than two bounds.  Returns the largest error / bound."""
    B, beam, K, V = c.B, c.beam, c.K, c.V
    tot, bnd = step_totals(c)
    parent, cand = got["parent"].reshape(B, K), got["new_cand"].reshape(B, K, c.ld)
    picks, worst = [], 0.0
    for b in range(B):
        assert ((parent[b] >= b * beam) & (parent[b] < (b + 1) * beam)).all(), f"{what}: source {b}: a parent outside the source's candidates"
        toks = cand[b, :, c.width]
        assert ((toks >= 0) & (toks < V)).all(), f"{what}: source {b}: a token outside [0, V)"
        picks.append([(int(p) - b * beam, int(t)) for p, t in zip(parent[b], toks)])
    if exact:
        want = step_exact_order(c)
        assert picks == want, f"{what}: selection {picks} differs from the float64 order {want}"
    sc = got["new_score"].reshape(B, K)
    for b in range(B):
        flat = [k * V + t for k, t in picks[b]]
        assert len(set(flat)) == K, f"{what}: source {b}: a (parent, token) pair was selected twice"
        t = tot[b * beam:(b + 1) * beam].reshape(-1)
        bd = bnd[b * beam:(b + 1) * beam].reshape(-1)
        ratio = np.abs(sc[b].astype(np.float64) - t[flat]) / bd[flat]
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, f"{what}: source {b}: score of rank {int(ratio.argmax())} off by {ratio.max():.2f} bounds"
        if not exact:
            assert (np.diff(sc[b]) <= 0).all(), f"{what}: source {b}: scores increase"
            rest = np.ones(len(t), bool)
            rest[flat] = False
            low = int(np.argmin(t[flat]))
            over = t[rest] - t[flat][low] - 2 * np.maximum(bd[rest], bd[flat][low])
            assert not (over > 0).any(), f"{what}: source {b}: an unselected total lies above the smallest selected one by more than two bounds"
    check_exact(got, step_outputs(c, picks, sc), what)
    return worst


def step_case(*, B, beam, K, V, kind="random", width=3, ld=0, seed=0):
    """Operands of one k_beam_step launch.  kind: random; gap (random, re-drawn until the top K + 1 totals of every source are GAP
    apart); tie_beams (two candidates of a source with identical rows and scores, two planted levels); tie_row (the row maximum
    in neighbouring lanes, 64 and 256 columns on: two lanes, two waves, two passes of one thread)."""
    for attempt in range(50):
        rng = np.random.default_rng(seed + 1000 * attempt)
        n_cand = B * beam
        c = NS(B=B, beam=beam, K=K, V=V, kind=kind, pad=PAD, eos=EOS, width=width, ld=ld or width + 2)
        c.finished = np.zeros(n_cand, U8)
        if beam >= 3 and kind in ("random", "gap"):
            c.finished[rng.integers(n_cand)] = 1
            c.finished[n_cand - 1] = 1
        run = np.flatnonzero(c.finished == 0)
        c.slot_of = np.full(n_cand, -1, I32)
        c.slot_of[run] = rng.permutation(len(run))
        c.logits = (rng.standard_normal((len(run), V)) * 4).astype(F32)
        c.score = (-rng.random(n_cand) * 9).astype(F32)
        c.gen = rng.integers(3, 90, size=(n_cand, c.ld)).astype(I32)
        c.summary = np.array([3, BIG, 0, 0, 0], I32)
        if kind == "tie_beams":
            assert beam >= 2 and K <= 4
            for b in range(B):
                a0, a1 = b * beam, b * beam + 1
                row = c.logits[c.slot_of[a0]]
                v1, v2 = rng.permutation(V)[:2]
                top = row.max()
                row[v1], row[v2] = top + 12.0, top + 6.0
                c.logits[c.slot_of[a1]] = row
                c.score[a1] = c.score[a0]
                c.score[b * beam + 2:(b + 1) * beam] -= 60.0
        elif kind == "tie_row":
            assert beam == 1
            for b in range(B):
                row = c.logits[c.slot_of[b]]
                v = int(rng.integers(0, max(V - 257, 1))) if V > 257 else 0
                at = [u for u in (v, v + 1, v + 64, v + 256) if u < V]
                assert len(at) >= K
                row[at] = row.max() + 12.0
        if kind == "random":
            return c
        try:
            step_exact_order(c)
            return c
        except AssertionError:
            if kind != "gap":
                raise
    raise AssertionError("no gap case found")


def step_arrays(c) -> dict:
    a = {k: getattr(c, k) for k in STEP_IN}
    B, K = c.B, c.K
    a.update(new_cand=sent((B * K, c.ld), I64), new_score=sent(B * K, F32), parent=sent(B * K, I32), new_len=sent(B * K, I32),
             new_finished=sent(B * K, U8), parent_draft=sent(B * K, I32), summary=c.summary.copy())
    return a


def step_fp32(c) -> dict:
    """What a correct fp32 evaluation in the kernel's order leaves behind (ties: lower flat index)."""
    tot = step_totals(c, fp32=True)
    picks, scores = [], []
    for b in range(c.B):
        t = tot[b * c.beam:(b + 1) * c.beam].reshape(-1)
        order = sorted(range(len(t)), key=lambda i: (-float(t[i]), i))[:c.K]
        picks.append([(i // c.V, i % c.V) for i in order])
        scores.append([t[i] for i in order])
    return step_outputs(c, picks, scores)


# ---------------------------------------------------------------------------------------------------------------------------
# k_tree_cache
def tree_case(*, d, layers, n_cand, prev_N, prev_D, slots=False, seed=0):
    """Operands of one k_tree_cache launch: candidates in turn fresh (parent -1), inactive, and children that keep 0, 1, .. 1 + prev_D
    new rows of parent drafts 0 .. prev_N - 1; one parent that was not running in the previous step (prev_slot_of -1).  ``slots``:
    one buffer and the pool's maps, with children that take over their parent's slot (append only) and children that move."""
    rng = np.random.default_rng(seed)
    Lc = 12 + prev_D
    c = NS(d=d, layers=layers, max_cand=n_cand, prev_N=prev_N, prev_D=prev_D, slots=slots, Lc=Lc)
    R = rps(prev_N, prev_D)
    c.prev_len = rng.integers(1, 9, size=n_cand).astype(I32)
    c.parent = rng.integers(0, n_cand, size=n_cand).astype(I32)
    c.active = np.ones(n_cand, U8)
    c.parent_draft = np.zeros(n_cand, I32)
    c.len = np.zeros(n_cand, I32)
    c.prev_slot_of = rng.permutation(n_cand).astype(I32)
    if n_cand > 4:
        c.prev_slot_of[c.parent[4]] = -1
    for cc in range(n_cand):
        if cc % 5 == 0:
            c.parent[cc] = -1
        if cc % 5 == 1:
            c.active[cc] = 0
        n_new = [0, 1, 1 + prev_D, min(2, 1 + prev_D)][cc % 4]
        c.parent_draft[cc] = [0, prev_N - 1][(cc // 2) % 2] if prev_N > 1 else 0
        c.len[cc] = (c.prev_len[c.parent[cc]] if c.parent[cc] >= 0 else 1) + n_new
    n_run = int((c.prev_slot_of >= 0).sum())
    c.qkv = rng.standard_normal((layers, n_cand * R, 3 * d)).astype(F32)
    n_slots = n_cand if not slots else 2 * n_cand
    c.k_old = rng.standard_normal((layers, n_slots, Lc, d)).astype(F32)
    c.v_old = rng.standard_normal((layers, n_slots, Lc, d)).astype(F32)
    c.slot_parent = c.slot_self = None
    if slots:                                                              # parents live in slots [0, n_cand); movers go to fresh ones
        c.slot_parent = np.where(c.parent >= 0, c.parent, 0).astype(I32)
        c.slot_self = (n_cand + np.arange(n_cand)).astype(I32)
        taken = set()
        for cc in range(n_cand):
            if c.active[cc] and c.parent[cc] >= 0 and cc % 2 == 0 and int(c.parent[cc]) not in taken:
                c.slot_self[cc] = c.slot_parent[cc]                        # takes over its parent's slot: append only
                taken.add(int(c.parent[cc]))
        c.taken = taken
    assert n_run >= 1
    return c


def tree_cache(c):
    """new_cache[c][0 .. len_c - 2] = parent's cache [0 .. len_p - 2] ++ parent's front row ++ the accepted rows of the parent's
    chosen draft (rows 1 + draft * prev_D + (j - 1) of the parent's slot in the previous step's packed Q/K/V), per layer, K and V.
    Returns (k_new, v_new) as the launch leaves them: two buffers -> sentinels elsewhere; slot maps -> the one buffer's content."""
    d, R = c.d, rps(c.prev_N, c.prev_D)
    if c.slots:
        kn, vn = c.k_old.copy(), c.v_old.copy()
    else:
        kn, vn = sent(c.k_old.shape, F32), sent(c.v_old.shape, F32)
    for cc in range(c.max_cand):
        p = int(c.parent[cc])
        if not c.active[cc] or p < 0:
            continue
        sp, sc = (int(c.slot_parent[cc]), int(c.slot_self[cc])) if c.slots else (p, cc)
        n_old, n_new, slot, dp = int(c.prev_len[p]) - 1, int(c.len[cc]) - int(c.prev_len[p]), int(c.prev_slot_of[p]), int(c.parent_draft[cc])
        for l in range(c.layers):
            for new, old, third in ((kn, c.k_old, 1), (vn, c.v_old, 2)):
                rows = [old[l, sp, :n_old]]
                if slot >= 0 and n_new > 0:
                    src = [slot * R] + [slot * R + 1 + dp * c.prev_D + (j - 1) for j in range(1, n_new)]
                    rows.append(c.qkv[l, src, third * d:(third + 1) * d])
                cat = np.concatenate(rows, axis=0)
                new[l, sc, :len(cat)] = cat
    return kn, vn


# ---------------------------------------------------------------------------------------------------------------------------
# the shared case tables: tests/test_beam_checks_host.py proves the bounds and caps on exactly the inputs the GPU test launches
def vpls_for(V: int):
    return [v for v in (4, 8, 16) if 64 * v >= V]


#                    V     K   N  dl  n_cand  smart  pool
LEAVES_CASES = [(30, 32, 3, 10, 15, False, False),       # K above V
                (64, 5, 1, 1, 16, False, False),         # one draft of one token
                (65, 10, 3, 11, 16, False, False),       # dl + 1 = 12: one wave per position, one pass
                (256, 1, 3, 12, 17, False, False),       # dl + 1 = 13: the position loop wraps
                (257, 10, 64, 2, 7, False, False),       # 64 drafts: topk(1)'s partial-sort branch
                (512, 5, 3, 0, 5, False, False),         # no draft
                (513, 10, 3, 10, 15, False, False),
                (1024, 24, 3, 40, 45, False, False),     # 984 segments per source at K = 24; accepted lengths 0 .. 40
                (1024, 32, 3, 10, 15, False, False),
                (65, 5, 6, 10, 15, True, False),         # smart: the table padded to the iteration's longest group
                (65, 5, 3, 10, 16, False, True),         # pool: dead slots, dl_of < dl
                (300, 10, 6, 4, 10, True, True)]          # pool + smart: grp_of wider than per_cand, a width-sensitive choice


def leaves_cases():
    for V, K, N, dl, n_cand, smart, pool in LEAVES_CASES:
        yield dict(V=V, K=K, N=N, dl=dl, n_cand=n_cand, max_cand=n_cand + 1, smart=smart, pool=pool, seed=V + K + dl)


def hits_cases():
    for V, K, N, dl, n_cand, smart, pool in LEAVES_CASES:
        # K above V ranks the whole row: the mass above the last ranks of a randn * 4 row creeps past the threshold in steps below
        # the margin, so more than the cap's share of such pairs is undecidable in fp32; k_bs_hits takes that case at K = 10
        yield dict(V=V, K=K if K <= V else 10, N=N, dl=dl, n_cand=n_cand, max_cand=n_cand + 1, pool=pool, seed=7 * V + K + dl)


#               B  beam  K    V   kind        width  ld
STEP_CASES = [(2, 3, 3, 30, "random", 3, 0), (2, 3, 3, 256, "random", 3, 0), (3, 1, 5, 65, "random", 1, 8), (1, 20, 20, 1024, "random", 3, 0),
              (2, 3, 3, 65, "gap", 3, 0), (2, 1, 4, 256, "gap", 1, 0), (1, 20, 20, 1024, "gap", 2, 0),
              (2, 3, 3, 30, "tie_beams", 3, 0), (2, 3, 3, 65, "tie_beams", 3, 0), (2, 3, 3, 256, "tie_beams", 3, 0),
              (2, 3, 3, 1024, "tie_beams", 3, 0),
              (2, 1, 2, 30, "tie_row", 1, 0), (2, 1, 3, 65, "tie_row", 1, 0), (2, 1, 3, 256, "tie_row", 1, 0), (2, 1, 4, 1024, "tie_row", 1, 0)]


def step_cases():
    for B, beam, K, V, kind, width, ld in STEP_CASES:
        yield dict(B=B, beam=beam, K=K, V=V, kind=kind, width=width, ld=ld, seed=V + beam)


def dev(buf):
    """The device tensor of a Buf; an empty operand (dl = 0) is handed over as one element of its allocation, since an empty
    tensor has no address."""
    return buf.v if buf.n else buf.buf[U.GUARD:U.GUARD + 1]
