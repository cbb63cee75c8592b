"""CPU checks of tests/util_sample_pool.py, the restatement the sampling slot pool is held to.

1  The restated pool (sources admitted in units of n under plan_admission's semantics, slots reused, a float64 sampler on a host
   model) returns the position-by-position sampler's rows for every capacity from n upward, for every list order, and for
   sub-chunked admissions, while draft tokens really are accepted.
2  A stand-in written as the kernels are (64-element passes and ballots per slot; the compacted rows of a draft pass) agrees with
   the restatement, and each single defect is flagged: a key or sample id left from a slot's previous occupant, sample = i / n,
   drafts or cross data of source i instead of i / n, row_of off by n, BOS missing from the caller row, the position taken from the
   compacted row instead of the mapped layout row, a draft straddling 64 elements credited to the wrong draft.
3  The binding: the new symbols and the argument struct.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import util_loop_checks as U
import util_sample_checks as S
import util_sample_pool as P
import util_sample_spec as X
from test_sample_spec_host import SEED, V, host_model, planted_drafts

PAD, BOS, EOS = X.PAD, X.BOS, X.EOS
N_D = (3, 4)
MAX_LEN = 14


def setting(S_total: int, n: int, seed: int = 1):
    """Sources of every kind of ending, their keys (high words too), the rows the plain sampler gives source s, sample j, and copy
    drafts per source planted from the source's first sample."""
    rng = np.random.default_rng(seed)
    kinds = (["eos", "pad", "long"] * S_total)[:S_total]
    model = host_model(kinds)
    keys = rng.integers(-2 ** 63, 2 ** 63, S_total, dtype=np.int64)
    params = S.Params(1.0)
    want = X.sequential(S_total * n, MAX_LEN, lambda r, prefix: model(r // n, prefix), np.repeat(keys, n), np.tile(np.arange(n), S_total),
                        SEED, params)
    drafts = planted_drafts(want[::n], N_D[0], N_D[1], rng)
    return model, keys, params, want, drafts


def reorder(x, order, n):
    """Rows of sources in list order ``order`` -> rows in the original order."""
    rows = np.concatenate([np.arange(s * n, (s + 1) * n) for s in order])
    out = np.empty_like(x)
    out[rows] = x
    return out


@pytest.mark.parametrize("n", [1, 2, 3])
def test_pool_returns_the_plain_samplers_rows_at_every_capacity(n):
    S_total = 5
    model, keys, params, want, drafts = setting(S_total, n)
    assert len({tuple(r) for r in want.tolist()}) > (S_total if n > 1 else S_total - 1), "the samples of a source do not differ"
    for C_ in range(n, S_total * n + 2):
        for sub in ((0, 1, 2) if C_ in (n, 2 * n) else (C_ % 3,)):     # sub-chunks of 1 and 2 sources at every third capacity
            out = P.run_pool(drafts, keys, n, C_, MAX_LEN, model, SEED, params, sub_chunk=sub)
            d = U.first_difference(out, want)
            assert d is None, f"n {n} capacity {C_} sub-chunk {sub}: {d}"


def test_pool_returns_the_plain_samplers_rows_in_every_list_order():
    S_total, n = 4, 2
    model, keys, params, want, drafts = setting(S_total, n, seed=2)
    for order in itertools.permutations(range(S_total)):
        o = list(order)
        km = lambda s, prefix: model(o[s], prefix)
        for C_ in (2, 5):
            out = P.run_pool(drafts[o], keys[o], n, C_, MAX_LEN, km, SEED, params)
            d = U.first_difference(reorder(out, o, n), want)
            assert d is None, f"order {o} capacity {C_}: {d}"


def test_draft_tokens_are_accepted():
    """The pool takes fewer steps than position-by-position sampling: planted drafts are accepted."""
    S_total, n = 3, 2
    model, keys, params, want, drafts = setting(S_total, n, seed=3)
    steps = []
    accept = lambda st, pred: (steps.append(1), X.sample_accept_step(st, pred))[1]
    out = P.run_pool(drafts, keys, n, S_total * n, MAX_LEN, model, SEED, params, accept_fn=accept)
    assert U.first_difference(out, want) is None and len(steps) < int(S.ends(want, PAD, EOS).max())


@pytest.mark.parametrize("defect", ["stale_key", "sample_div", "data_of_row", "row_of_off", "no_bos"])
def test_each_admission_defect_is_flagged(defect):
    S_total, n = 5, 2
    model, keys, params, want, drafts = setting(S_total, n, seed=4)
    ok = P.run_pool(drafts, keys, n, 4, MAX_LEN, model, SEED, params, sub_chunk=0)
    assert U.first_difference(ok, want) is None
    rows, bad_rows = {}, {}
    assert U.first_difference(P.run_pool(drafts, keys, n, 4, MAX_LEN, model, SEED, params, admitted=rows), want) is None
    bad = P.run_pool(drafts, keys, n, 4, MAX_LEN, model, SEED, params, sub_chunk=0, defect=defect, admitted=bad_rows)
    fresh = [BOS] + [PAD] * (MAX_LEN - 1)                 # a caller row between its admission and its end: the sampler's convention
    assert sorted(rows) == list(range(S_total * n)) and all(r.tolist() == fresh for r in rows.values())
    if defect == "no_bos":                                # an ended row is overwritten whole: the defect shows in the admitted rows
        assert any(r.tolist() != fresh for r in bad_rows.values()), f"{defect}: not flagged"
    else:
        assert U.first_difference(bad, want) is not None, f"{defect}: not flagged"


# -- stand-ins written as the kernels are -----------------------------------------------------------------------------------------
def wave_best_draft(drafts_b: np.ndarray, ps: np.ndarray, defect: str | None = None) -> tuple:
    """accept_best_draft_wave: lane e of a pass of 64 compares element e of the N x D draft tokens with its draw; the first mismatch
    of a draft comes out of the pass's ballot; a draft may straddle passes."""
    N, D = drafts_b.shape
    ND = N * D
    dr = drafts_b.reshape(-1)
    best, bacc, open_acc = 0, -1, D
    for base in range(0, ND, 64):
        m = 0
        for lane in range(64):
            e = base + lane
            if e < ND and dr[e] != ps[0 if e % D == 0 else e]:
                m |= 1 << lane
        n = base // D
        while n < N and n * D < base + 64:
            start, end = n * D, n * D + D
            lo, hi = max(start, base) - base, min(end, base + 64) - base
            bits = (m >> lo) & ((1 << (hi - lo)) - 1)
            if start >= base:
                open_acc = D
            if bits and open_acc == D:
                open_acc = base + lo - start + ((bits & -bits).bit_length() - 1)
            if end <= base + 64 and open_acc > bacc:
                bacc, best = open_acc, n
                if defect == "straddle" and start < base:
                    best = n + 1 if n + 1 < N else n - 1
            n += 1
    return best, bacc


@pytest.mark.parametrize("N,D", [(1, 1), (3, 4), (5, 13), (1, 70), (64, 1), (2, 64), (3, 50)])
def test_wave_standin_agrees_and_the_straddle_defect_is_flagged(N, D):
    rng = np.random.default_rng(N * 1000 + D)
    flagged = False
    for pats in U.tie_patterns(N, D) + [list(rng.integers(0, D + 1, size=N)) for _ in range(40)]:
        s = X.make_state(1, N, D, 200, 5, seed=int(rng.integers(1 << 30)))
        pred = U.new_pred(s)
        U.plant(s, pred, 0, pats, rng)
        want = X.sample_accept_step(s, pred)
        b = int(s.act_idx[0])
        got = wave_best_draft(s.drafts[b], pred[:U.rps(N, D)])
        assert got == (int(want.rec[0, 1]), int(want.rec[0, 2])), f"N {N} D {D} lengths {pats}: {got}"
        flagged |= wave_best_draft(s.drafts[b], pred[:U.rps(N, D)], "straddle") != got
    straddles = any((n * D) // 64 != (n * D + D - 1) // 64 for n in range(N))
    assert flagged == straddles, "the straddle defect must show exactly where a draft straddles a pass"


def select_rows_standin(act2, front, masks, N, D, defect=None) -> tuple:
    """(b, pos) of every compacted row of a draft pass, as k_sample_step forms them from the row map."""
    R = U.rps(N, D)
    row_map = P.select_row_map(masks, N, D)
    b, pos = [], []
    for row, lrow in enumerate(row_map):
        if defect == "pos_from_compacted_row":
            lrow = row
        slot, rs = divmod(int(lrow), R)
        br = int(act2[slot])
        b.append(br)
        pos.append(int(front[br]) + (1 if rs == 0 else 2 + (rs - 1) % D))
    return np.array(b), np.array(pos)


def test_select_rows_standin_agrees_and_the_mapping_defect_is_flagged():
    N, D = 3, 2
    rng = np.random.default_rng(5)
    act2 = np.array([4, 1, 6, 0], dtype=np.int32)
    front = rng.permutation(30)[:8].astype(np.int32)
    fb, fpos = X.step_rows(act2, front, len(act2), N, D)
    seen = False
    for masks in itertools.product(range(1, 1 << N), repeat=2):
        masks = list(masks) + [(1 << N) - 1, 1]
        rm = P.select_row_map(masks, N, D)
        assert len(rm) == sum(1 + D * bin(m).count("1") for m in masks) and len(set(rm.tolist())) == len(rm)
        b, pos = select_rows_standin(act2, front, masks, N, D)
        assert (b == fb[rm]).all() and (pos == fpos[rm]).all(), f"masks {masks}"
        bb, bp = select_rows_standin(act2, front, masks, N, D, "pos_from_compacted_row")
        seen |= bool((bb != fb[rm]).any() or (bp != fpos[rm]).any())
    assert seen, "taking the position from the compacted row is not flagged"
    full = [(1 << N) - 1] * len(act2)
    assert (P.select_row_map(full, N, D) == np.arange(len(act2) * U.rps(N, D))).all()


def test_accept_pool_step_is_the_sampling_step_with_the_pools_rows():
    s0, pred = X.retire_case(40, 13, 11)
    s = P.to_pool(s0)
    a, b = X.sample_accept_step(s0, pred), P.accept_pool_step(s, pred, exec_rows=77)
    n = s0.words["n_active"]
    fin = a.rec[:n, 4] == 1
    rows = s0.act_idx[:n]
    assert (b.rec == a.rec).all() and (b.gen == a.gen).all() and (b.act_idx == a.act_idx).all()
    assert (b.pool_out[s.row_of[rows[fin]]] == a.out[rows[fin]]).all()
    others = np.setdiff1d(np.arange(s.pool_rows), s.row_of[rows[fin]])
    assert (b.pool_out[others] == s.pool_out[others]).all()
    assert b.words["verified_positions"] == s0.words["verified_positions"] + 77
    assert {k: v for k, v in b.words.items() if k != "verified_positions"} == {k: v for k, v in a.words.items() if k != "verified_positions"}


def test_admit_restatement():
    rng = np.random.default_rng(1)
    pool = P.Pool(12, 3, 2, 9, 11, 8, out_rows=20, rng=rng)
    pool.act_idx[:3] = [7, 0, 4]
    pool.n_active = 3
    before = pool.clone()
    dn = rng.integers(3, 40, size=(3, 6), dtype=np.int32)
    vn = np.ones((3, 7), dtype=np.uint8)
    kn = rng.standard_normal((3, 7, 8)).astype(np.float32)
    res = P.admit(pool, dn, vn, kn, 3, 1, row_keys=np.arange(100, 110))
    new = pool.act_idx[3:12]
    assert res == dict(n_active=12, m_rows=12 * 7, error=0, host_n_active=12) and new.tolist() == [1, 2, 3, 5, 6, 8, 9, 10, 11]
    assert pool.key[new].tolist() == [101] * 3 + [102] * 3 + [103] * 3 and pool.sample[new].tolist() == [0, 1, 2] * 3
    assert pool.row_of[new].tolist() == list(range(3, 12)) and (pool.drafts[new[3:6]] == dn[1]).all()
    assert (pool.src_valid[new, 7:] == 0).all() and (pool.memkv[new[8], :7] == kn[2]).all()
    assert (pool.out[3:12, 0] == BOS).all() and (pool.out[3:12, 1:] == PAD).all() and (pool.out[:3] == -7).all()
    for b in (7, 0, 4):
        assert (pool.gen[b] == before.gen[b]).all() and pool.key[b] == before.key[b]
    assert P.admit(pool, dn, vn, kn, 1, 0)["error"] == 4


# -- the binding -----------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_new_symbols():
    from translation_transformer_amd import _native as NA
    assert len(NA.SYMBOLS["ttx_sample_speculative_generate_pool"][1]) == 12
    assert len(NA.SYMBOLS["ttx_debug_sample_step_select"][1]) == 17
    assert len(NA.SYMBOLS["ttx_debug_sample_accept_pool"][1]) == 6
    assert len(NA.SYMBOLS["ttx_debug_pool_fill_sample"][1]) == 4
    assert C.sizeof(NA.DebugPoolFillArgs) == 17 * 8 + 15 * 4 + 4
    import translation_transformer_amd as tta
    lib = tta.lib()
    for name in ("ttx_sample_speculative_generate_pool", "ttx_debug_sample_step_select", "ttx_debug_sample_accept_pool",
                 "ttx_debug_pool_fill_sample"):
        assert hasattr(lib, name), name
    assert hasattr(tta.TranslationInferenceSamplingSpeculative, "generate_many")
