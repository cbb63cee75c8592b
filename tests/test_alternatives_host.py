"""Per-position alternatives without a GPU: the NumPy restatement (tests/util_alternatives.py) against the reference's fixture
(tests/golden/alternatives.npz, made by tests/golden/make_golden_alternatives.py) on the oracle's logits; the checkers of the GPU
test flag single defects of a stand-in result; the side file, near_ties, and the two C entry points are declared and bound."""
from typing import NamedTuple

import numpy as np
import pytest
import torch

import translation_transformer_amd as tta
from translation_transformer_amd import _native as N
from translation_transformer_amd import scoring
import util_alternatives as U
from util_models import PAD, BOS, EOS, tiny_state

NEW = ("ttx_hypothesis_alternatives", "ttx_score_alternatives")
K = 8


# -- the restatement against the reference ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    from oracle.model import OracleTransformer, config_from_state
    st, cfg = tiny_state()
    return OracleTransformer(config_from_state(st, cfg["num_heads"]), st)


@pytest.mark.parametrize("name", ["beam", "targets", "rule"])
def test_restatement_reproduces_the_fixture(oracle, name):
    """The oracle's logits are within 5e-5 of the reference's (test_oracle_model.py), so the comparison is the one the GPU test
    makes: sorted values within the bound, ids where the reference's value is clear of its neighbours, at most 1 % left out."""
    c = U.golden_cases()[name]
    B, n_hyp, W = c["hyp"].shape
    hyp = torch.from_numpy(c["hyp"]).reshape(B * n_hyp, W)
    with torch.inference_mode():
        logits = oracle(torch.from_numpy(c["src"]).repeat_interleave(n_hyp, 0), hyp[:, :-1]).float().numpy()
    got = U.restate(logits, hyp.numpy(), PAD, EOS, K)
    r = U.compare_with_golden(got, c, K)
    print(name, r)
    assert r["length_equal"]
    assert r["top_logp_err"] <= r["bound"] and r["entropy_err"] <= r["bound"]
    assert r["left_out"] <= 0.01 * r["pairs"]
    assert r["id_mismatches"] == 0 and r["rank_mismatches"] == 0
    # what is not live holds the not-live values, in the fixture and in the restatement
    dead = np.arange(W - 1) >= c["length"][..., None]
    assert (c["top_id"][dead] == -1).all() and (c["rank"][dead] == -1).all() and (c["entropy"][dead] == 0).all()
    assert (got["top_id"].reshape(B, n_hyp, W - 1, K)[dead] == -1).all() and (got["chosen_logp"].reshape(B, n_hyp, W - 1)[dead] == 0).all()


def test_fixture_is_small_and_holds_no_logits():
    from util_models import GOLDEN
    assert (GOLDEN / "alternatives.npz").stat().st_size < 1 << 20
    z = np.load(GOLDEN / "alternatives.npz")
    assert not any("logits" in k for k in z.files)
    assert all(z[f"{n}__top_logp"].shape[-1] == K + 1 for n in ("beam", "targets", "rule"))


# -- the checkers ------------------------------------------------------------------------------------------------------
def _stand_in():
    """Small-integer logits (most neighbours tie) with a few -inf and -0.0 entries, a result computed by the fp32 restatement."""
    rng = np.random.default_rng(7)
    R, W, V, k = 6, 9, 13, 5
    x = rng.integers(-2, 3, (R, W - 1, V)).astype(np.float32)
    x[1, :, 3] = -np.inf
    x.reshape(-1)[np.flatnonzero(x == 0)[::2]] = -0.0
    x[2] += rng.standard_normal((W - 1, V)).astype(np.float32)            # one row without ties
    hyp = rng.integers(3, V, (R, W)).astype(np.int64)
    hyp[:, 0] = BOS
    hyp[0, 5], hyp[1, 8], hyp[3, 1] = EOS, EOS, EOS
    hyp[4, 4:] = PAD
    hyp[5, :] = PAD
    got = {f: np.array(v) for f, v in U.restate(x, hyp, PAD, EOS, k, np.float32).items()}
    return x, hyp, got


def test_checker_accepts_the_fp32_restatement():
    x, hyp, got = _stand_in()
    assert got["length"].tolist() == [5, 8, 8, 1, 3, 0]
    assert U.check_result(got, x, hyp, PAD, EOS) == []


def _tie_towards_higher_id(x, hyp, got):
    xs = np.take_along_axis(x[0, 0], got["top_id"][0, 0], -1)
    j = int(np.nonzero(xs[1:] == xs[:-1])[0][0])
    got["top_id"][0, 0, [j, j + 1]] = got["top_id"][0, 0, [j + 1, j]]


def _rank_off_by_one(x, hyp, got):
    got["rank"][2, 3] += 1


def _unsorted(x, hyp, got):
    lp = got["top_logp"][2, 1]
    assert lp[0] > lp[1]
    got["top_logp"][2, 1, [0, 1]] = lp[[1, 0]]


def _entropy_term_dropped(x, hyp, got):
    xd = x[2, 2].astype(np.float64)
    logp = xd - xd.max() - np.log(np.exp(xd - xd.max()).sum())
    terms = np.exp(logp) * logp
    got["entropy"][2, 2] = -(terms.sum() - terms[np.argmin(logp)])       # the smallest probability's term
    assert abs(terms[np.argmin(logp)]) > 1e-3


def _value_past_the_length(x, hyp, got):
    got["entropy"][3, 1] = 1e-30


def _rank_points_elsewhere(x, hyp, got):
    assert got["rank"][2, 0] != 1
    got["rank"][2, 0] = 1


def _duplicated_id(x, hyp, got):
    got["top_id"][0, 1, 1] = got["top_id"][0, 1, 0]


@pytest.mark.parametrize("defect, flag", [
    (_tie_towards_higher_id, "a tie broken towards the higher id"), (_rank_off_by_one, "rank"), (_unsorted, "top_logp not sorted"),
    (_entropy_term_dropped, "entropy"), (_value_past_the_length, "a value past the length"),
    (_rank_points_elsewhere, "top_id[rank] != chosen"), (_duplicated_id, "duplicated id")])
def test_checker_flags_a_single_defect(defect, flag):
    x, hyp, got = _stand_in()
    defect(x, hyp, got)
    assert flag in U.check_result(got, x, hyp, PAD, EOS)


def test_checker_range_only_positions():
    x, hyp, got = _stand_in()
    x[0, 2] = -np.inf                                                    # outside the contract: only the ranges are checked
    mask = np.zeros(x.shape[:2], bool)
    mask[0, 2] = True
    got["top_logp"][0, 2], got["entropy"][0, 2] = np.nan, np.nan
    assert U.check_result(got, x, hyp, PAD, EOS, mask) == []
    got["top_id"][0, 2, 0] = x.shape[-1]
    assert U.check_result(got, x, hyp, PAD, EOS, mask) == ["id or rank outside [0, V)"]


# -- side file and near_ties -------------------------------------------------------------------------------------------
class _Alts(NamedTuple):
    top_id: torch.Tensor
    top_logp: torch.Tensor
    chosen_logp: torch.Tensor
    rank: torch.Tensor
    entropy: torch.Tensor
    length: torch.Tensor

    margin = tta.Alternatives.margin


def _torch_stand_in() -> _Alts:
    x, hyp, got = _stand_in()
    t = {f: torch.from_numpy(v) for f, v in got.items()}
    return _Alts(*(t[f].reshape((3, 2) + t[f].shape[1:]) for f in U.FIELDS))


def test_alternatives_side_file_round_trip(tmp_path):
    alts = _torch_stand_in()
    side = tmp_path / "pred.alternatives.csv"
    scoring.write_alternatives(str(side), alts)
    scoring.write_alternatives(str(side), alts)                          # appends, like the prediction writer
    rows = scoring.read_alternatives(str(side))
    assert len(rows) == 6 and rows[:3] == rows[3:]
    for b in range(3):
        assert len(rows[b]) == 2
        for h in range(2):
            n = int(alts.length[b, h])
            assert len(rows[b][h]) == n
            for p in range(n):
                pairs, rank, entropy = rows[b][h][p]
                assert [i for i, _ in pairs] == alts.top_id[b, h, p].tolist()
                assert torch.equal(torch.tensor([lp for _, lp in pairs], dtype=torch.float32), alts.top_logp[b, h, p])   # -inf too
                assert rank == int(alts.rank[b, h, p])
                assert torch.tensor(entropy, dtype=torch.float32) == alts.entropy[b, h, p]
    assert rows[2][1] == []                                               # the all-PAD hypothesis
    scoring.write_alternatives(str(side), alts, append=False)
    assert len(scoring.read_alternatives(str(side))) == 3


def test_margin_and_near_ties_on_hand_made_margins():
    lp = torch.tensor([[[-0.1, -2.5], [-0.7, -0.7], [-0.6931, -0.6932], [0.0, 0.0]],
                       [[-0.5, -0.5], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]])
    length = torch.tensor([3, 1], dtype=torch.int32)
    z = torch.zeros((2, 4))
    alts = tta.Alternatives(torch.zeros((2, 4, 2), dtype=torch.int32), lp, z, z.int(), z, length)
    assert torch.allclose(alts.margin, torch.tensor([[2.4, 0.0, 1e-4, 0.0], [0.0, 0.0, 0.0, 0.0]]), atol=1e-6)
    assert (alts.margin[0, 3] == 0) and (alts.margin[1, 1:] == 0).all()          # exactly 0 where not live
    assert scoring.near_ties(alts, 1e-3).tolist() == [[False, True, True, False], [True, False, False, False]]
    assert scoring.near_ties(alts, 5e-5).tolist() == [[False, True, False, False], [True, False, False, False]]
    with pytest.raises(ValueError):
        tta.Alternatives(alts.top_id[..., :1], lp[..., :1], z, z.int(), z, length).margin


# -- the C boundary and the Python surface -----------------------------------------------------------------------------
def test_entry_points_are_bound_and_abi_stays_4():
    lib = tta.lib()
    for name in NEW:
        assert name in N.SYMBOLS and hasattr(lib, name)
    assert lib.ttx_abi_version() == 4


def test_entry_points_without_a_session():
    lib = tta.lib()
    want = N.TTX_ERR_NO_DEVICE if lib.ttx_device_count() == 0 else N.TTX_ERR_INVALID
    assert lib.ttx_hypothesis_alternatives(None, None, None, 2, 5, 30, 0, 2, 5, None, None, None, None, None, None, None) == want
    assert lib.ttx_score_alternatives(None, None, 2, 7, None, 5, 1, 5, 2, 5, None, None, None, None, None, None, None, None) == want
    if want == N.TTX_ERR_NO_DEVICE:
        assert b"no CPU fallback" in lib.ttx_last_error()


def test_python_surface_exists():
    assert tta.Alternatives._fields == U.FIELDS
    for cls in (tta.TranslationInferenceGreedy, tta.TranslationInferenceGreedySpeculative, tta.TranslationInferenceBeamSearch,
                tta.TranslationInferenceBeamSearchSpeculative):
        assert callable(cls.alternatives)
    assert callable(tta.NativeTransformer.alternatives) and callable(tta.NativeTransformer.hypothesis_alternatives)
    for name in ("write_alternatives", "read_alternatives", "near_ties"):
        assert callable(getattr(scoring, name))
