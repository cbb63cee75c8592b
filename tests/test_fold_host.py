"""CPU-side checks of the fold feature: the NumPy restatement of ttx_fold_hypotheses' rule (tests/util_fold.py) by hand and against
scoring.unique_samples, the checker against planted single defects of a stand-in, logmass by hand, and the Python argument
checks (which run before the library or a device is touched)."""
import math

import numpy as np
import pytest
import torch

import translation_transformer_amd as tta
from translation_transformer_amd import scoring
from translation_transformer_amd.model import fold_on_device

import util_fold as U

PAD, EOS = 0, 2


# ---- the restatement by hand ----
def hand_case():
    hyp = np.array([[[1, 5, 6, 2, 0, 0],      # 0  A, finished
                     [1, 5, 7, 2, 0, 0],      # 1  B, finished
                     [1, 5, 6, 2, 9, 9],      # 2  = A: differs only after the EOS
                     [1, 5, 6, 8, 0, 0],      # 3  C, no EOS: unfinished
                     [1, 5, 7, 2, 0, 0],      # 4  = B
                     [1, 5, 6, 2, 0, 0]]],    # 5  = A
                   np.int64)
    scores = np.array([[-2.0, -1.0, -0.5, -0.25, -9.0, -9.0]], np.float32)
    return hyp, scores


def test_restatement_by_hand_score_order():
    hyp, sc = hand_case()
    r = U.fold_reference(hyp, sc, U.SCORE, 0, PAD, EOS)
    assert r["first"].tolist() == [[0, 1, 0, 3, 1, 0]]
    assert r["n_unique"].tolist() == [3]
    assert r["perm"].tolist() == [[3, 1, 0, -1, -1, -1]]           # C (-0.25), B (-1.0), A (-2.0: its own score, not -0.5)
    assert r["count"].tolist() == [[1, 2, 3, 0, 0, 0]]
    assert r["score"].tolist() == [[-0.25, -1.0, -2.0, -math.inf, -math.inf, -math.inf]]
    assert r["rank_of"].tolist() == [[2, 1, 2, 0, 1, 2]]
    assert r["out"][0, 0].tolist() == [1, 5, 6, 8, 0, 0] and r["out"][0, 2].tolist() == [1, 5, 6, 2, 0, 0]
    assert (r["out"][0, 3:] == PAD).all()


def test_restatement_by_hand_other_orders():
    hyp, sc = hand_case()
    r = U.fold_reference(hyp, sc, U.SCORE, U.UNFINISHED_LAST, PAD, EOS)
    assert r["perm"].tolist() == [[1, 0, 3, -1, -1, -1]]
    r = U.fold_reference(hyp, sc, U.COUNT, 0, PAD, EOS)
    assert r["perm"].tolist() == [[0, 1, 3, -1, -1, -1]] and r["count"].tolist() == [[3, 2, 1, 0, 0, 0]]
    r = U.fold_reference(hyp, None, U.FIRST, 0, PAD, EOS)
    assert r["perm"].tolist() == [[0, 1, 3, -1, -1, -1]] and r["logmass"] is None
    assert np.isneginf(r["score"]).all()
    r = U.fold_reference(hyp, None, U.COUNT, U.UNFINISHED_LAST, PAD, EOS)
    assert r["perm"].tolist() == [[0, 1, 3, -1, -1, -1]]
    with pytest.raises(ValueError):
        U.fold_reference(hyp, None, U.SCORE, 0, PAD, EOS)


def test_restatement_ties_zero_nan_and_column0():
    hyp = np.array([[[2, 7, 7], [2, 8, 8], [4, 2, 1], [5, 2, 1], [4, 2, 3]]], np.int64)   # rows 0, 1: EOS in column 0
    sc = np.array([[np.nan, 3.0, -0.0, 0.0, 1.0]], np.float32)
    r = U.fold_reference(hyp, sc, U.SCORE, 0, PAD, EOS)
    assert r["first"].tolist() == [[0, 0, 2, 3, 2]]
    assert r["perm"].tolist() == [[2, 3, 0, -1, -1]]               # -0.0 ties 0.0: the lower index first; the NaN reads -inf
    assert r["score"][0, 2] == -np.inf and r["count"].tolist() == [[2, 1, 2, 0, 0]]
    big = np.array([[[7 + (1 << 40), 2], [7, 2]]], np.int64)        # ids are compared on all 64 bits
    assert U.fold_reference(big, None, U.FIRST, 0, PAD, EOS)["n_unique"].tolist() == [2]


def test_logmass_by_hand():
    hyp, sc = hand_case()
    r = U.fold_reference(hyp, sc, U.SCORE, 0, PAD, EOS)
    want = math.log(math.exp(-0.25) + math.exp(-1.0) + math.exp(-2.0))
    assert abs(r["logmass64"][0] - want) < 1e-14
    assert r["logmass"][0] == np.float32(want)
    assert U.logmass_ok(np.float32(want), want)
    assert U.logmass_ok(np.nextafter(np.float32(want), np.float32(0)), want)
    assert not U.logmass_ok(np.float32(want) + 4 * np.spacing(np.float32(want)), want)
    none = U.fold_reference(hyp, np.full((1, 6), -np.inf, np.float32), U.SCORE, 0, PAD, EOS)
    assert none["logmass"][0] == -np.inf and U.logmass_ok(np.float32(-np.inf), -math.inf)
    assert not U.logmass_ok(np.float32(np.nan), -math.inf)
    far = U.fold_reference(hyp, sc - 500, U.SCORE, 0, PAD, EOS)     # exp() of the raw scores would underflow: m keeps it exact
    assert abs(far["logmass64"][0] - (want - 500)) < 1e-12


# ---- the restatement against scoring.unique_samples ----
def test_restatement_matches_unique_samples():
    rng = np.random.default_rng(11)
    for trial in range(300):
        N, W = int(rng.integers(1, 9)), int(rng.integers(1, 7))
        pool = rng.integers(1, 5, size=(3, W))                      # a tiny vocabulary with the EOS in it: repeats are frequent
        hyp = pool[rng.integers(0, 3, size=N)][None].astype(np.int64)
        hyp[0, rng.random(N) < 0.3, -1] = rng.integers(1, 5)
        sc = rng.choice(np.array([-1.0, -1.0, -2.5, 0.0, -0.0, -np.inf], np.float32), size=(1, N))   # planted equal scores
        want = scoring.unique_samples(torch.from_numpy(hyp), torch.from_numpy(sc), eos=EOS)[0]
        r = U.fold_reference(hyp, sc, U.SCORE, 0, PAD, EOS)
        assert r["n_unique"][0] == len(want), trial
        for k, (tok, cnt, s) in enumerate(want):
            assert r["out"][0, k].tolist() == tok.tolist(), (trial, k)
            assert r["count"][0, k] == cnt and r["score"][0, k] == np.float32(s), (trial, k)
        assert (r["out"][0, len(want):] == PAD).all() and (r["perm"][0, len(want):] == -1).all()


# ---- the checker against planted single defects of a stand-in ----
def standin(hyp, scores, order, flags, pad, eos, defect=None):
    """A second statement of the rule with room for one planted defect."""
    hyp = np.asarray(hyp, np.int64)
    B, N, W = hyp.shape
    sc = np.asarray(scores, np.float32).copy()
    if defect != "nan_first":
        sc[np.isnan(sc)] = -np.inf
    res = U.fold_reference(hyp, scores, order, flags, pad, eos)
    res = {k: (None if v is None else v.copy()) for k, v in res.items()}
    for b in range(B):
        ext = [U.row_extent(hyp[b, j], eos) for j in range(N)]

        def same(i, j):
            ci, cj = ext[i][0], ext[j][0]
            if defect == "after_eos":
                return bool((hyp[b, i] == hyp[b, j]).all())
            if ci != cj:
                return False
            if defect == "filter_only":
                return True                                          # equal length taken for equality
            lo = 1 if defect == "skip_col0" else 0
            x, y = hyp[b, i, lo:ci], hyp[b, j, lo:ci]
            if defect == "narrow32":
                x, y = x.astype(np.int32), y.astype(np.int32)
            return bool((x == y).all())
        first = [next(i for i in range(j + 1) if same(i, j)) for j in range(N)]
        reps = [j for j in range(N) if first[j] == j]
        cnt = {a: first.count(a) for a in reps}
        val = dict((a, sc[b, a]) for a in reps)
        if defect == "repeat_score":
            val = {a: sc[b, max(j for j in range(N) if first[j] == a)] for a in reps}

        def key(a):
            s = float(val[a])
            if defect == "nan_first" and s != s:
                s = math.inf
            k = [0 if (ext[a][1] or not flags & U.UNFINISHED_LAST or defect == "ignore_unf_last") else 1]
            if order == U.COUNT:
                k.append(-cnt[a])
            if order != U.FIRST:
                k.append(-s)
            k.append(-a if defect == "tie_high" else a)
            return tuple(k)
        ranked = sorted(reps, key=key)
        res["first"][b] = first
        res["n_unique"][b] = len(ranked)
        res["perm"][b], res["count"][b], res["score"][b], res["out"][b] = -1, 0, -np.inf, pad
        for r, a in enumerate(ranked):
            res["perm"][b, r], res["count"][b, r], res["out"][b, r] = a, cnt[a], hyp[b, a]
            res["score"][b, r] = -np.inf if val[a] != val[a] else val[a]
        res["rank_of"][b] = [ranked.index(first[j]) for j in range(N)]
        if defect == "tail_not_pad" and len(ranked) < N:
            res["out"][b, N - 1, W - 1] = pad + 1
    return res


def defect_case():
    hyp = np.array([[[1, 5, 6, 2, 0, 0],
                     [1, 5, 6, 2, 7, 7],               # = row 0 (differs after the EOS)
                     [3, 5, 6, 2, 0, 0],               # differs from row 0 in column 0 only
                     [1, 5, 9, 2, 0, 0],               # same length as row 0, other tokens
                     [1 + (1 << 40), 5, 6, 2, 0, 0],   # differs from row 0 in bit 40 only
                     [1, 5, 6, 8, 8, 8],               # unfinished, the best score
                     [1, 5, 9, 2, 0, 0],               # = row 3
                     [4, 4, 2, 0, 0, 0]]],
                   np.int64)
    sc = np.array([[-1.0, -0.1, -1.0, -3.0, -2.0, -0.5, -0.2, np.nan]], np.float32)
    return hyp, sc


def test_standin_without_defect_passes_the_checker():
    hyp, sc = defect_case()
    for order in (U.FIRST, U.SCORE, U.COUNT):
        for flags in (0, U.UNFINISHED_LAST):
            want = U.fold_reference(hyp, sc, order, flags, PAD, EOS)
            assert U.first_difference(standin(hyp, sc, order, flags, PAD, EOS), want) is None


@pytest.mark.parametrize("defect", ["after_eos", "skip_col0", "filter_only", "narrow32", "tie_high", "repeat_score",
                                    "ignore_unf_last", "tail_not_pad", "nan_first"])
def test_checker_names_planted_defects(defect):
    hyp, sc = defect_case()
    want = U.fold_reference(hyp, sc, U.SCORE, U.UNFINISHED_LAST, PAD, EOS)
    got = standin(hyp, sc, U.SCORE, U.UNFINISHED_LAST, PAD, EOS, defect)
    d = U.first_difference(got, want)
    assert d is not None, defect
    name, b, i = d
    assert name in U.OUTPUTS and b == 0
    with pytest.raises(AssertionError, match=name):
        U.assert_fold_equal(got, want, what=defect)


def test_layouts_hold_what_they_claim():
    rng = np.random.default_rng(5)
    for N, W in ((1, 1), (5, 1), (4, 2), (9, 7), (65, 65)):
        for kind in U.LAYOUTS:
            rows = U.layout_rows(kind, N, W, rng, PAD, EOS)
            assert rows.shape == (N, W) and rows.dtype == np.int64
        r = U.fold_reference(U.layout_rows("equal", N, W, rng)[None], None, U.FIRST)
        assert r["n_unique"][0] == 1 and r["count"][0, 0] == N
        r = U.fold_reference(U.layout_rows("distinct", N, W, rng)[None], None, U.FIRST)
        assert r["n_unique"][0] == N
        r = U.fold_reference(U.layout_rows("after_eos", N, W, rng)[None], None, U.FIRST)
        assert r["n_unique"][0] == 1
    r = U.fold_reference(U.layout_rows("bit40", 4, 5, rng)[None], None, U.FIRST)
    assert r["n_unique"][0] == 2 and r["count"][0, :2].tolist() == [2, 2]
    r = U.fold_reference(U.layout_rows("col0", 9, 7, rng)[None], None, U.FIRST)
    assert r["n_unique"][0] == 3


# ---- the Python argument checks: all before the library or a device is touched ----
def test_argument_checks():
    hyp = torch.zeros((2, 3, 4), dtype=torch.int64)
    sc = torch.zeros((2, 3))
    with pytest.raises(ValueError, match="unique_samples"):
        scoring.fold_samples(hyp, sc)
    with pytest.raises(ValueError, match="no CPU fallback"):
        fold_on_device(None, None, hyp, sc)
    bad = [dict(hyp=hyp[0]), dict(hyp=hyp.float()), dict(hyp=torch.zeros((1, 1025, 2), dtype=torch.int64), scores=None, order="first"),
           dict(order="best"), dict(unfinished="first"), dict(scores=sc[:, :2]), dict(scores=torch.zeros((2, 3), dtype=torch.int64)),
           dict(scores=None, order="score"), dict(scores=None, order="count", with_logmass=True),
           dict(hyp=torch.zeros((2, 0, 4), dtype=torch.int64))]
    for kw in bad:
        args = dict(hyp=hyp, scores=sc)
        args.update(kw)
        with pytest.raises(ValueError):
            fold_on_device(None, None, args.pop("hyp"), args.pop("scores"), **args)
    assert hasattr(tta.NativeTransformer, "fold_hypotheses") and hasattr(tta.TranslationInferenceSampling, "fold")
    for cls in (tta.TranslationInferenceGreedy, tta.TranslationInferenceBeamSearch, tta.TranslationInferenceStochasticBeamSearch,
                tta.TranslationInferenceBeamSearchSpeculative, tta.TranslationInferenceGreedySpeculative):
        assert hasattr(cls, "fold")


def test_entry_point_refuses_before_any_device():
    lib = tta.lib()
    from translation_transformer_amd import _native as N
    one = 8                                               # a non-null address that is never read: every call below is refused
    calls = [dict(B=0), dict(N=0), dict(N=1025), dict(W=0), dict(ld=3), dict(order=3), dict(flags=4), dict(order=1, score=None),
             dict(logmass=one, score=None, first=one), dict(first=None)]
    for kw in calls:
        a = dict(B=1, N=2, W=4, ld=4, order=0, flags=0, score=one, first=one, logmass=None)
        a.update(kw)
        rc = lib.ttx_fold_hypotheses(None, one, a["B"], a["N"], a["W"], a["ld"], 0, 2, a["score"], a["order"], a["flags"], a["first"],
                                     None, None, None, None, None, None, a["logmass"], None)
        assert rc == N.TTX_ERR_INVALID, kw


def test_write_and_read_folds(tmp_path):
    count = torch.tensor([[3, 2, 1, 0], [4, 0, 0, 0]], dtype=torch.int32)
    n_unique = torch.tensor([3, 1], dtype=torch.int32)
    logmass = torch.tensor([-0.123456789, -float("inf")])
    f = tmp_path / "folds.csv"
    scoring.write_folds(str(f), (count, n_unique, logmass), append=False)
    scoring.write_folds(str(f), tta.FoldedHypotheses(None, None, count, n_unique, None, None, None, None))
    rows = scoring.read_folds(str(f))
    assert rows[0][0] == 3 and rows[0][2] == [3, 2, 1] and rows[1] == (1, -math.inf, [4])
    assert np.float32(rows[0][1]) == np.float32(-0.123456789)           # 9 significant digits: fp32 round-trips
    assert rows[2][0] == 3 and math.isnan(rows[2][1]) and rows[2][2] == [3, 2, 1]
