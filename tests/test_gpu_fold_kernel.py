"""k_fold_hyps (csrc/ttx_fold.hip.h) through ttx_fold_hypotheses, one call at a time on arrays the test builds, against the NumPy
restatement of tests/util_fold.py (tests/test_fold_host.py shows that its checker can fail).  Every output must equal the
restatement EXACTLY; ``logmass`` must lie within one fp32 spacing of the float64 value rounded to fp32 (the double-side errors of
exp, log and the sum are about 1e-15 relative, so they can move the rounding by one ulp at most).

Shapes: every N of {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 1024} with two W, every W of {1, 2, 7, 63, 64, 65, 130, 200} with two N,
B of {1, 3, 70}: sizes around the wave width (64) of the candidate ballots and the column chunks, around the workgroup's 256
threads, one and many sources, and the largest N the entry point takes."""
import numpy as np
import pytest
import torch

import util_fold as U

pytestmark = pytest.mark.gpu
PAD, EOS = 0, 2
# (N, W, B)
SHAPES = [(1, 1, 3), (1, 7, 1), (2, 2, 70), (2, 200, 1), (3, 1, 1), (3, 63, 3), (4, 64, 3), (4, 2, 1), (5, 65, 70), (5, 130, 1),
          (63, 7, 3), (63, 64, 1), (64, 63, 3), (64, 200, 1), (65, 65, 3), (65, 130, 1), (255, 7, 1), (255, 130, 3), (256, 2, 1),
          (256, 200, 3), (1024, 64, 1), (1024, 200, 3)]
ORDERS = (U.FIRST, U.SCORE, U.COUNT)


@pytest.fixture(scope="module")
def lib():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    torch.zeros(1, device="cuda")
    return t.lib()


def check(lib, hyp, sc, order, flags, what, ld=None, want=U.OUTPUTS, session=None):
    rc, got = U.fold_call(lib, hyp, sc, order, flags, PAD, EOS, ld=ld, want=want, session=session)
    assert rc == 0, (what, rc, lib.ttx_last_error())
    ref = U.fold_reference(hyp, sc, order, flags & ~U.DEBUG_NO_FILTER, PAD, EOS)
    U.assert_fold_equal(got, ref, what=what)
    if got["perm"] is not None:                          # a permutation whatever the scores hold (NaN included)
        for b in range(hyp.shape[0]):
            u = int(ref["n_unique"][b])
            assert sorted(got["perm"][b, :u].tolist()) == sorted(set(ref["first"][b].tolist())), what
    return got


@pytest.mark.parametrize("N,W,B", SHAPES)
def test_layouts_orders_and_filter_flag(lib, N, W, B):
    """Every layout (the sources cycle through them; with B < 11 the seed rotates which ones), every order with and without
    UNFINISHED_LAST, ld_hyp > W with sentinels in the gap, and TTX_FOLD_DEBUG_NO_FILTER giving the same outputs."""
    for k, order in enumerate(ORDERS):
        for flags in (0, U.UNFINISHED_LAST):
            seed = 100 * N + 10 * k + flags
            kinds = U.LAYOUTS if N < 1024 else tuple(x for x in U.LAYOUTS if x != "distinct")     # all-distinct at 1024: below
            hyp, sc = U.make_case(B, N, W, seed, kinds)
            ld = W + (seed % 4)
            got = check(lib, hyp, sc, order, flags, f"N={N} W={W} B={B} order={order} flags={flags}", ld=ld)
            rc, plain = U.fold_call(lib, hyp, sc, order, flags | U.DEBUG_NO_FILTER, PAD, EOS, ld=ld)
            assert rc == 0
            for name in U.OUTPUTS:
                assert np.array_equal(plain[name].view(np.uint8), got[name].view(np.uint8)), (name, "DEBUG_NO_FILTER differs")


@pytest.mark.parametrize("kind", U.LAYOUTS)
@pytest.mark.parametrize("N,W", [(5, 7), (65, 65), (130, 2)])
def test_each_layout_alone(lib, kind, N, W):
    hyp, sc = U.make_case(3, N, W, 7, (kind,))
    for order in ORDERS:
        check(lib, hyp, sc, order, U.UNFINISHED_LAST if order == U.SCORE else 0, f"{kind} N={N} W={W} order={order}")
    check(lib, hyp, None, U.COUNT, 0, f"{kind} N={N} W={W} unscored", want=tuple(n for n in U.OUTPUTS if n != "logmass"))
    check(lib, hyp, sc, U.SCORE, U.DEBUG_NO_FILTER, f"{kind} N={N} W={W} no filter")


def test_all_distinct_and_all_equal_at_1024(lib):
    rng = np.random.default_rng(3)
    for kind in ("distinct", "equal"):
        hyp = U.layout_rows(kind, 1024, 200, rng, PAD, EOS)[None]
        sc = U.case_scores(1, 1024, rng)
        got = check(lib, hyp, sc, U.SCORE, U.UNFINISHED_LAST, f"{kind} at N=1024")
        assert got["n_unique"][0] == (1024 if kind == "distinct" else 1)
    check(lib, hyp, sc, U.COUNT, U.DEBUG_NO_FILTER, "equal at N=1024, no filter")


def test_scores_ties_zero_inf_denormal_nan(lib):
    """+-0.0 ties, equal scores, -inf, denormals, a NaN (read as -inf; perm stays a permutation), and repeats that carry other
    scores than their representative: the representative's own score is the one that ranks and the one handed out."""
    rng = np.random.default_rng(9)
    N, W = 12, 5
    hyp = U.layout_rows("distinct", N, W, rng, PAD, EOS)[None].repeat(2, 0)
    hyp[1, 6:] = hyp[1, :6]                                           # source 1: every hypothesis twice
    sc = np.array([[0.0, -0.0, -0.0, 0.0, -np.inf, np.nan, 1e-40, -1e-40, 1e-40, -2.0, -2.0, -np.inf],
                   [-1.0, -1.0, -5.0, -np.inf, np.nan, 0.0, 9.0, -9.0, 9.0, np.nan, 5.0, -0.0]], np.float32)
    for order in ORDERS:
        got = check(lib, hyp, sc, order, 0, f"score edge cases, order {order}")
    got = check(lib, hyp, sc, U.SCORE, 0, "score edge cases")
    assert got["perm"][0].tolist() == [6, 8, 0, 1, 2, 3, 7, 9, 10, 4, 5, 11]
    assert got["n_unique"][1] == 6 and got["score"][1, :6].tolist() == [0.0, -1.0, -1.0, -5.0, -np.inf, -np.inf]
    assert not np.isnan(got["score"]).any()
    allinf = np.full((2, N), -np.inf, np.float32)
    got = check(lib, hyp, allinf, U.SCORE, 0, "all -inf")
    assert np.isneginf(got["logmass"]).all()


def test_each_optional_output_null_in_turn(lib):
    hyp, sc = U.make_case(3, 9, 7, 21)
    for name in U.OUTPUTS:
        want = tuple(n for n in U.OUTPUTS if n != name)
        check(lib, hyp, sc, U.SCORE, U.UNFINISHED_LAST, f"without {name}", want=want, ld=9)
        check(lib, hyp, sc, U.COUNT, 0, f"only {name}", want=(name,))


def test_gather_paths_agree(lib):
    """The 16-byte row copies (W and ld_hyp even) and the 8-byte ones (either odd) hand out the same rows."""
    for W, ld in ((8, 8), (8, 9), (8, 10), (7, 7), (7, 8), (130, 132), (2, 2)):
        hyp, sc = U.make_case(3, 6, W, W + ld)
        check(lib, hyp, sc, U.SCORE, 0, f"W={W} ld={ld}", ld=ld)


def test_second_call_and_batching_are_bit_identical(lib):
    hyp, sc = U.make_case(70, 65, 65, 5)
    rc, a = U.fold_call(lib, hyp, sc, U.COUNT, U.UNFINISHED_LAST, PAD, EOS, ld=67)
    rc2, b = U.fold_call(lib, hyp, sc, U.COUNT, U.UNFINISHED_LAST, PAD, EOS, ld=67)
    assert rc == 0 and rc2 == 0
    for name in U.OUTPUTS:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name
    for src in (0, 33, 69):                                           # a source alone = the same source inside the batch
        rc, one = U.fold_call(lib, hyp[src:src + 1], sc[src:src + 1], U.COUNT, U.UNFINISHED_LAST, PAD, EOS)
        assert rc == 0
        for name in U.OUTPUTS:
            assert np.array_equal(one[name].view(np.uint8), a[name][src:src + 1].view(np.uint8)), (name, src)


def test_padded_width_changes_nothing(lib):
    """Rows that hold an EOS, and unfinished rows padded with PAD on both sides, fold the same at a wider W."""
    rng = np.random.default_rng(17)
    hyp = np.stack([U.layout_rows(k, 20, 9, rng, PAD, EOS) for k in ("mixed", "prefix", "after_eos")])
    sc = U.case_scores(3, 20, rng)
    wide = np.full((3, 20, 70), PAD, np.int64)
    wide[:, :, :9] = hyp
    _, a = U.fold_call(lib, hyp, sc, U.SCORE, U.UNFINISHED_LAST, PAD, EOS)
    _, b = U.fold_call(lib, wide, sc, U.SCORE, U.UNFINISHED_LAST, PAD, EOS)
    for name in ("first", "rank_of", "n_unique", "perm", "count", "score", "logmass"):
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name
    assert np.array_equal(a["out"], b["out"][:, :, :9]) and (b["out"][:, :, 9:] == PAD).all()


def test_with_a_session(lib):
    import translation_transformer_amd as t
    from util_models import tiny_state
    st, cfg = tiny_state()
    native = t.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    hyp, sc = U.make_case(3, 9, 7, 2)
    check(lib, hyp, sc, U.SCORE, 0, "with a session", session=native.session)


def test_refusals_launch_nothing(lib):
    from translation_transformer_amd import _native as N
    hyp, sc = U.make_case(2, 4, 6, 1)
    refused = [dict(B=0), dict(N=0), dict(N=1025), dict(W=0), dict(ld=5), dict(order=3), dict(order=-1), dict(flags=4),
               dict(flags=8 | U.UNFINISHED_LAST), dict(scores=None, order=U.SCORE), dict(scores=None, order=U.COUNT),
               dict(want=())]
    for kw in refused:
        a = dict(scores=sc, order=U.FIRST, flags=0, want=U.OUTPUTS, ld=None, B=None, N=None, W=None)
        a.update(kw)                                                   # (scores=None, COUNT) asks for logmass: refused too
        rc, out = U.fold_call(lib, hyp, a["scores"], a["order"], a["flags"], PAD, EOS, ld=a["ld"], want=a["want"], B=a["B"], N=a["N"],
                              W=a["W"])
        assert rc == N.TTX_ERR_INVALID, kw
        assert U.untouched(out), kw
