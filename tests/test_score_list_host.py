"""CPU-side checks of the length-bucketed scoring of a list of batches: the NumPy restatement of the three kernels
(tests/util_score_list.py) worked by hand on a three-batch list, the checker against planted single defects, the properties of
scheduling.score_plan on seeded random lengths, and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import translation_transformer_amd as tta
from translation_transformer_amd import _native as N
from translation_transformer_amd.scheduling import score_plan
from util_score_list import BOS, EOS, PAD, extents, first_difference, make_batch, pack, plan, row_n, unpack


def hand_list():
    """Three batches, shapes (B, Ls, N, W) = (2, 4, 1, 5), (1, 3, 2, 4), (1, 1, 1, 2); sources 0 .. 3, rows 0 .. 4."""
    a = {"src": np.array([[5, 0, 6, 0], [7, 8, 9, 4]], np.int64),                  # interior PAD, then a PAD tail: ls 3; full: ls 4
         "hyp": np.array([[[BOS, 5, EOS, 7, 0]], [[BOS, 5, 0, 6, 0]]], np.int64)}  # EOS at 2 (a token after it): n 2; unfinished, PAD inside: n 3
    b = {"src": np.array([[0, 0, 0]], np.int64),                                   # all PAD: ls 1
         "hyp": np.array([[[BOS, 0, 0, 0], [BOS, EOS, 4, 4]]], np.int64)}          # all PAD: n 0; EOS at column 1: n 1
    c = {"src": np.array([[9]], np.int64), "hyp": np.array([[[BOS, EOS]]], np.int64)}   # EOS in the last column: n 1
    return [a, b, c]


def test_restatement_by_hand():
    L = hand_list()
    e, ls, n = extents(L)
    assert n.tolist() == [2, 3, 0, 1, 1]
    assert e.tolist() == [3, 4, 2, 2]                     # max(2, 1 + n): source 2 has rows with n 0 and 1, source 3 n 1
    assert ls.tolist() == [3, 4, 1, 1]
    # a chunk of sources 3 and 0 (N = 1), wider than batch c and narrower than batch a
    src_c, hyp_c = pack(L, [3, 0], 1, 3, 3)
    assert src_c.tolist() == [[9, 0, 0], [5, 0, 6]]       # the interior PAD stays, the tail is cut
    assert hyp_c.tolist() == [[BOS, EOS, 0], [BOS, 5, EOS]]
    # the N = 2 source alone, at a width above its own
    src_c, hyp_c = pack(L, [2], 2, 6, 2)
    assert src_c.tolist() == [[0, 0]]
    assert hyp_c.tolist() == [[BOS, 0, 0, 0, 0, 0], [BOS, EOS, 4, 4, 0, 0]]
    # unpack of the first chunk into sentinel-filled outputs
    out = {"score": [np.full((2, 1), 9.0), np.full((1, 2), 9.0), np.full((1, 1), 9.0)],
           "length": [np.full((2, 1), -7), np.full((1, 2), -7), np.full((1, 1), -7)],
           "finished": [np.full((2, 1), 5), np.full((1, 2), 5), np.full((1, 1), 5)],
           "tok": [np.full((2, 1, 4), 9.0), np.full((1, 2, 3), 9.0), np.full((1, 1, 1), 9.0)]}
    unpack(L, [3, 0], 1, 3, np.array([-1.5, -2.5]), np.array([1, 2]), np.array([1, 1]), np.array([[-1.5, 0.0], [-1.0, -1.5]]), out)
    assert out["score"][2].tolist() == [[-1.5]] and out["score"][0].tolist() == [[-2.5], [9.0]] and out["score"][1].tolist() == [[9.0, 9.0]]
    assert out["length"][0].tolist() == [[2], [-7]] and out["finished"][2].tolist() == [[1]]
    assert out["tok"][2].tolist() == [[[-1.5]]]                                  # min(3, 2) - 1 = 1 value, no tail
    assert out["tok"][0][0].tolist() == [[-1.0, -1.5, 0.0, 0.0]]                 # 2 values, zeros up to W_i - 1 = 4
    assert out["tok"][0][1].tolist() == [[9.0] * 4]                              # a row of another chunk keeps its sentinel
    # the plan: sources by (N, e, ls, index) = 3 (1,2,1), 0 (1,3,3), 1 (1,4,4), 2 (2,2,1)
    p = plan([1, 1, 2, 1], e, ls, 6)
    # 3 sources x 1 x (4 - 1) = 9 > 6: the third source opens a chunk; 2 x 1 x 2 = 4, 1 x 3 = 3, 1 x 2 x 1 = 2: largest first
    assert p == [([3, 0], 1, 3, 3), ([1], 1, 4, 4), ([2], 2, 2, 1)]
    q = score_plan([1, 1, 2, 1], e, ls, 6)
    assert [(c.sources.tolist(), c.N, c.W, c.Ls) for c in q] == p


def _reference_outputs(L):
    """The restatement's outputs for a plan over the whole list, per-batch arrays; the chunk results are made-up numbers keyed by
    the global row, so that a misplaced row shows."""
    e, ls, n = extents(L)
    N_of = np.repeat([b["hyp"].shape[1] for b in L], [b["src"].shape[0] for b in L])
    out = {"score": [np.full(b["hyp"].shape[:2], 9.0) for b in L], "length": [np.full(b["hyp"].shape[:2], -7) for b in L],
           "finished": [np.full(b["hyp"].shape[:2], 5) for b in L],
           "tok": [np.full(b["hyp"].shape[:2] + (b["hyp"].shape[2] - 1,), 9.0) for b in L]}
    packed = []
    for sel, Nc, Wc, Lsc in plan(N_of, e, ls, 40):
        src_c, hyp_c = pack(L, sel, Nc, Wc, Lsc)
        length_c = np.array([row_n(h) for h in hyp_c])
        fin_c = np.array([int((h[1:] == EOS).any()) for h in hyp_c])
        tok_c = -(hyp_c[:, 1:].astype(np.float64) + 0.25) * (np.arange(Wc - 1)[None, :] < length_c[:, None])
        unpack(L, sel, Nc, Wc, tok_c.sum(1), length_c, fin_c, tok_c, out)
        packed.append((sel, src_c, hyp_c, Nc))
    return e, ls, n, packed, out


def test_checker_names_planted_defects():
    rng = np.random.default_rng(7)
    L = [make_batch(rng, 3, 6, 2, 7), make_batch(rng, 2, 4, 2, 5), make_batch(rng, 2, 5, 1, 6)]
    L[0]["hyp"][1, 0, 3], L[0]["hyp"][1, 0, 5:] = EOS, PAD          # finished at 3, a token at 4 after the EOS
    L[0]["hyp"][2, 1, 4:] = PAD                                     # unfinished, n = 3
    L[1]["hyp"][0, 1, 1:] = PAD                                     # all PAD
    L[1]["hyp"][0, 0, 1:] = PAD                                     # ... its whole source: e = max(2, 1) = 2
    L[2]["src"][1, 3:] = PAD
    e, ls, n, packed, out = _reference_outputs(L)
    assert first_difference([e], [e]) is None and first_difference(out["tok"], out["tok"]) is None
    # 1. a neighbouring source's row packed
    sel, src_c, hyp_c, Nc = next(p for p in packed if len(p[0]) >= 2)
    wrong = hyp_c.copy()
    wrong[1] = hyp_c[1 + Nc]                                        # row 1 of the chunk read from the next source
    msg = first_difference([wrong], [hyp_c], "hyp_c")
    assert msg is not None and msg.startswith("hyp_c: batch 0, row 1, column 1:"), msg
    # 2. the PAD fill missing: the restatement fills, a pack that leaves the buffer's old content (here 77) does not
    short = [p for p in packed if (p[2] == PAD).any()][0][2]
    unfilled = short.copy()
    unfilled[short == PAD] = 77
    r, c = np.argwhere(short == PAD)[0]
    assert first_difference([unfilled], [short], "hyp_c") == f"hyp_c: batch 0, row {r}, column {c}: got 77, expected 0"
    # 3. n at the last non-PAD column instead of the first EOS
    last_tok = np.array([max([c for c in range(1, len(h)) if h[c] != PAD] or [0]) for b in L for rows in b["hyp"] for h in rows])
    msg = first_difference([last_tok], [n], "n")
    assert msg == "n: batch 0, row 2: got 4, expected 3", msg            # global row 2 = batch 0, source 1, row 0
    # 4. e without the max(2, .)
    raw = np.array([1 + max(row_n(h) for h in rows) for b in L for rows in b["hyp"]])
    msg = first_difference([raw], [e], "e")
    assert msg == "e: batch 0, row 3: got 1, expected 2", msg            # source 3 = batch 1, source 0: all PAD
    # 5. the unpack's zero tail missing
    tail = [t.copy() for t in out["tok"]]
    i = next(i for i, t in enumerate(out["tok"]) if (t[..., -1] == 0).any())
    b, k = np.argwhere(out["tok"][i][..., -1] == 0)[0]
    first_zero = int(np.argmax(out["tok"][i][b, k] == 0))
    tail[i][b, k, first_zero:] = 9.0
    assert first_difference(tail, out["tok"], "tok_logp").startswith(f"tok_logp: batch {i}, row ({b}, {k}), column {first_zero}:")
    # 6. finished scattered by chunk order: the values land in the order the chunks ran, not in list order
    flat = np.concatenate([f.reshape(-1) for f in out["finished"]])
    rows_run = []
    for sel, _, hyp_c, _ in packed:
        rows_run += [int((h[1:] == EOS).any()) for h in hyp_c]
    assert sorted(rows_run) == sorted(flat.tolist()) and rows_run != flat.tolist()
    msg = first_difference([np.array(rows_run)], [flat], "finished")
    assert msg is not None and msg.startswith("finished: batch 0, row "), msg
    # shapes and batch counts are differences too
    assert "shape" in first_difference([np.zeros((2, 3))], [np.zeros((2, 4))]) and "batches" in first_difference([], [e])


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("max_rows", [1, 97, 1000, 32768])
def test_score_plan_properties(seed, max_rows):
    rng = np.random.default_rng(seed)
    S = int(rng.integers(1, 80))
    N_of = rng.choice([1, 3, 5, 8], S)
    e = rng.integers(2, 160, S)
    ls = rng.integers(1, 90, S)
    p = score_plan(N_of, e, ls, max_rows)
    allsrc = np.concatenate([c.sources for c in p])
    assert sorted(allsrc.tolist()) == list(range(S))                               # every source in exactly one chunk
    for c in p:
        assert c.sources.dtype == np.int32 and len(c.sources) >= 1
        assert (N_of[c.sources] == c.N).all()                                      # one N per chunk
        assert c.W == e[c.sources].max() and c.Ls == ls[c.sources].max()           # the chunk's maxima
        assert c.positions == len(c.sources) * c.N * (c.W - 1)
        assert c.positions <= max_rows or len(c.sources) == 1
    assert [c.positions for c in p] == sorted((c.positions for c in p), reverse=True)   # largest first
    q = score_plan(N_of.copy(), e.copy(), ls.copy(), max_rows)                     # the same plan twice
    assert len(p) == len(q) and all((a.sources == b.sources).all() and (a.N, a.W, a.Ls) == (b.N, b.W, b.Ls) for a, b in zip(p, q))
    if max_rows == 1:
        assert len(p) == S and all(len(c.sources) == 1 for c in p)
    # the restatement with plain loops cuts the same chunks
    assert [(c.sources.tolist(), c.N, c.W, c.Ls) for c in p] == [(list(s), n, w, l) for s, n, w, l in plan(N_of, e, ls, max_rows)]


def test_score_plan_is_greedy_and_keeps_the_sort_order():
    # equal lengths: the index decides, and a chunk takes as many sources as fit
    p = score_plan([2] * 7, [11] * 7, [4] * 7, 60)                                 # 3 sources x 2 x 10 = 60
    assert [c.sources.tolist() for c in p] == [[0, 1, 2], [3, 4, 5], [6]]
    p = score_plan([1, 1, 1, 1], [9, 3, 9, 3], [2, 7, 1, 7], 10 ** 6)
    assert [c.sources.tolist() for c in p] == [[1, 3, 2, 0]] and (p[0].W, p[0].Ls) == (9, 7)


def test_score_plan_rejects_bad_arguments():
    for bad in (([], [], []), ([1, 1], [2], [1, 1]), ([0], [2], [1]), ([1], [1], [1]), ([1], [2], [0])):
        with pytest.raises(ValueError):
            score_plan(*bad, 100)
    with pytest.raises(ValueError):
        score_plan([1], [2], [1], 0)


def test_binding_layout_and_symbols():
    assert C.sizeof(N.ScoreBatch) == 2 * 8 + 5 * 4 + 4                  # ttx_score_batch: 2 pointers, 5 int32, tail padding
    assert C.sizeof(N.ScoreChunk) == 5 * 4
    assert C.sizeof(N.DebugScoreListArgs) == 14 * 8 + 4 * 4
    assert N.DEBUG_SCORE_LIST_OPS == ("extents", "pack", "unpack")
    lib = tta.lib()
    for name in ("ttx_score_list_extents", "ttx_score_list_run", "ttx_debug_score_list"):
        assert name in N.SYMBOLS and hasattr(lib, name)
    assert hasattr(tta.NativeTransformer, "score_hypotheses_many")
    for cls in (tta.TranslationInferenceGreedy, tta.TranslationInferenceGreedySpeculative, tta.TranslationInferenceBeamSearch,
                tta.TranslationInferenceBeamSearchSpeculative, tta.TranslationInferenceSampling,
                tta.TranslationInferenceSamplingSpeculative, tta.TranslationInferenceStochasticBeamSearch):
        assert callable(getattr(cls, "score_many"))


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a machine without a GPU")
def test_entry_points_refuse_without_a_device():
    lib = tta.lib()
    tab = (N.ScoreBatch * 1)(N.ScoreBatch(None, None, 1, 1, 1, 2, 2))
    assert lib.ttx_score_list_extents(None, tab, 1, EOS, None, None, None, None, None) == N.TTX_ERR_NO_DEVICE
    assert lib.ttx_score_list_run(None, tab, 1, None, 0, None, 0, EOS, None, None, None, None, None, None) == N.TTX_ERR_NO_DEVICE
    assert lib.ttx_debug_score_list(None, 0, tab, 1, None, 0, None, None, None) == N.TTX_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.ttx_last_error()
