"""Hypothesis scores without a GPU: the length / masking / sum rule is pinned on the reference's fixture
(tests/golden/hyp_scores.npz, made by tests/golden/make_golden_scores.py) without a model; the two C entry points are declared,
bound and refuse to run without a device; scoring.rank_by_score and the scores side file."""
import ctypes as C
from typing import NamedTuple

import pytest
import torch

import translation_transformer_amd as tta
from translation_transformer_amd import _native as N
from translation_transformer_amd import scoring
from util_models import PAD, EOS
from util_score import golden_cases, length_rule, scores_from_token_logp

NEW = ("ttx_hypothesis_logprobs", "ttx_score_hypotheses")


# -- the rule itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["beam", "targets", "rule"])
def test_rule_reproduces_the_fixture(name):
    c = golden_cases()[name]
    # poison what lies past the length: the restatement must mask it, not rely on the fixture's zeros
    tok = c["tok_logp"].clone()
    n = c["length"].long()
    past = torch.arange(tok.shape[-1]).expand_as(tok) >= n.unsqueeze(-1)
    assert (tok[past] == 0).all()
    tok[past] = -123.0
    r = scores_from_token_logp(tok, c["hyp"], PAD, EOS)
    assert torch.equal(r["length"], n)
    assert torch.equal(r["finished"], c["finished"])
    assert torch.equal(r["tok_logp"], c["tok_logp"])
    assert torch.allclose(r["score"], c["score"], rtol=0, atol=1e-12)


def test_hand_made_rows_cover_every_case_of_the_rule():
    c = golden_cases()["rule"]
    hyp = c["hyp"].reshape(-1, c["hyp"].shape[-1])
    length, fin = length_rule(hyp, PAD, EOS)
    # EOS at column 1 | no EOS, trailing PAD | no EOS, full row | all-PAD | a PAD before the EOS | two EOS
    assert length.tolist() == [1, 4, 11, 0, 6, 3]
    assert fin.tolist() == [True, False, False, False, True, True]
    assert (hyp[3] == PAD).all() and float(c["score"].reshape(-1)[3]) == 0.0
    assert PAD in hyp[4, 1:6].tolist()                       # the PAD inside the sequence is scored like any token
    assert c["tok_logp"].reshape(-1, hyp.shape[1] - 1)[4, 2] < 0
    assert (hyp[5] == EOS).sum() == 2


def test_fixture_beam_scores_are_ordered_and_gaps_recorded():
    c = golden_cases()["beam"]
    sc = c["score"]
    assert c["finished"].all()
    assert (sc[:, :-1] > sc[:, 1:]).all()
    gaps = (sc[:, :-1] - sc[:, 1:]).amin(1)
    assert torch.allclose(gaps, c["min_gap"], rtol=0, atol=1e-12)
    assert float(gaps.min()) == pytest.approx(3.07e-3, abs=1e-5)      # source 6; every source stays above the 2e-3 cut
    assert int((gaps < 2e-3).sum()) == 0


# -- the C boundary ----------------------------------------------------------------------------------------------------
def test_entry_points_are_bound_and_abi_stays_4():
    lib = tta.lib()
    for name in NEW:
        assert name in N.SYMBOLS and hasattr(lib, name)
    assert lib.ttx_abi_version() == 4


def test_entry_points_without_a_session():
    """No device: TTX_ERR_NO_DEVICE like every other call (with one, a null session is a bad argument)."""
    lib = tta.lib()
    want = N.TTX_ERR_NO_DEVICE if lib.ttx_device_count() == 0 else N.TTX_ERR_INVALID
    assert lib.ttx_hypothesis_logprobs(None, None, None, 2, 5, 30, 0, 2, None, None, None, None, None) == want
    assert lib.ttx_score_hypotheses(None, None, 2, 7, None, 5, 1, 5, 2, None, None, None, None, None, None) == want
    if want == N.TTX_ERR_NO_DEVICE:
        assert b"no CPU fallback" in lib.ttx_last_error()


def test_python_surface_exists():
    assert tta.HypothesisScores._fields == ("score", "length", "finished", "token_logp")
    for cls in (tta.TranslationInferenceGreedy, tta.TranslationInferenceGreedySpeculative, tta.TranslationInferenceBeamSearch,
                tta.TranslationInferenceBeamSearchSpeculative):
        assert callable(cls.score)
    assert callable(tta.NativeTransformer.score_hypotheses) and callable(tta.NativeTransformer.hypothesis_logprobs)


# -- rank_by_score -----------------------------------------------------------------------------------------------------
class _Scores(NamedTuple):
    score: torch.Tensor
    length: torch.Tensor
    finished: torch.Tensor
    token_logp: torch.Tensor | None


def test_rank_by_score_order_ties_and_unfinished_last():
    score = torch.tensor([[-3.0, -1.0, -2.0, -1.0, -0.5],          # a tie (1 and 3) and an unfinished best score (4)
                          [-1.0, -2.0, -3.0, -4.0, -5.0],          # already ordered
                          [-5.0, -0.1, -5.0, -0.2, -5.0]])         # two unfinished (1, 3), a three-way tie
    fin = torch.tensor([[True, True, True, True, False],
                        [True, True, True, True, True],
                        [True, False, True, False, True]])
    length = torch.arange(15, dtype=torch.int32).reshape(3, 5)
    tok = torch.arange(3 * 5 * 4, dtype=torch.float32).reshape(3, 5, 4)
    pred = torch.arange(3 * 5 * 5).reshape(3, 5, 5)
    rp, rs, perm = scoring.rank_by_score(pred, _Scores(score, length, fin, tok))
    assert perm.tolist() == [[1, 3, 2, 0, 4], [0, 1, 2, 3, 4], [0, 2, 4, 1, 3]]
    for b in range(3):
        for k in range(5):
            j = perm[b, k]
            assert torch.equal(rp[b, k], pred[b, j]) and torch.equal(rs.token_logp[b, k], tok[b, j])
            assert rs.score[b, k] == score[b, j] and rs.length[b, k] == length[b, j] and rs.finished[b, k] == fin[b, j]
    assert isinstance(rs, _Scores)
    # without per-token values
    _, rs2, perm2 = scoring.rank_by_score(pred, _Scores(score, length, fin, None))
    assert rs2.token_logp is None and torch.equal(perm2, perm)


def test_scores_side_file_round_trip_leaves_the_csv_alone(tmp_path):
    csv = tmp_path / "pred.csv"
    csv.write_text("CCO,CC=O,CC=O,CCO\nCCN,CCN,CCC,CCN\n")
    before = scoring.score_csv(str(csv), canonicalize=None)
    score = torch.tensor([[-0.125, -2.7182817], [-1e-7, -33.5]])
    sc = _Scores(score, torch.tensor([[4, 3], [3, 3]], dtype=torch.int32), torch.tensor([[True, True], [True, False]]), None)
    side = tmp_path / "pred.scores.csv"
    scoring.write_scores(str(side), sc)
    scoring.write_scores(str(side), sc)                        # appends, like the prediction writer
    rows = scoring.read_scores(str(side))
    assert len(rows) == 4 and rows[:2] == rows[2:]
    for b in range(2):
        for k in range(2):
            s, n, f = rows[b][k]
            assert torch.tensor(s, dtype=torch.float32) == score[b, k]          # fp32 round-trips
            assert n == int(sc.length[b, k]) and f == bool(sc.finished[b, k])
    assert scoring.score_csv(str(csv), canonicalize=None) == before
    assert csv.read_text() == "CCO,CC=O,CC=O,CCO\nCCN,CCN,CCC,CCN\n"
