"""Attention maps without a GPU: the float64 restatement of the definition (tests/util_attn_maps.py, on the oracle) is pinned on
the reference's fixture (tests/golden/attn_maps.npz, made by tests/golden/make_golden_attn.py); the length rule; the checkers of
the GPU tests flag a stand-in result with one deliberate defect at a time; the entry points are declared, bound and refuse to run
without a device; the alignment side file."""
import ctypes as C
from typing import NamedTuple

import numpy as np
import pytest
import torch

import translation_transformer_amd as tta
from translation_transformer_amd import _native as N
from translation_transformer_amd import scoring
from util_models import PAD, EOS, tiny_state, load_npz
from util_attn_maps import (golden_cases, oracle_maps, lengths_of, live_mask, np_attn_probs, check_result, head_mean, first_argmax,
                            align_agreement, EPS32)

NEW = ("ttx_attention_maps", "ttx_attn_probs_key_limit", "ttx_debug_attn_probs")


# -- the restatement against the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["targets", "rule"])
@pytest.mark.parametrize("layer", [0, 1])
def test_float64_restatement_reproduces_the_fixture(name, layer):
    c = golden_cases()[name]
    state, cfg = tiny_state()
    ref = oracle_maps(state, cfg["num_heads"], c["src"], c["hyp"], layer, PAD, EOS)
    gold = c[f"heads_l{layer}"]
    assert gold.dtype == np.float32 and gold.shape == ref.shape
    dist = np.abs(gold.astype(np.float64) - ref).max()
    recorded = float(c["f64_dist"][layer])
    print(f"{name} layer {layer}: |reference fp32 - float64 restatement| = {dist:.3e}, recorded {recorded:.3e}")
    # the file's distance is to the reference's own float64 copy; the oracle's float64 differs from that by float64 rounding only
    assert dist <= recorded + 1e-12
    src_rows = np.repeat(c["src"], c["hyp"].shape[1], axis=0)
    assert (ref[np.broadcast_to((src_rows == PAD)[:, None, None, :], ref.shape)] == 0).all()
    live = live_mask(c["length"], ref.shape[2])
    assert np.abs(ref.sum(-1)[np.broadcast_to(live[:, None, :], ref.shape[:3])] - 1).max() < 1e-12
    assert (ref[np.broadcast_to(~live[:, None, :, None], ref.shape)] == 0).all()


def test_fixture_holds_the_source_without_pad_and_the_rule_rows():
    g = golden_cases()
    assert 5 in g["targets"]["sources"].tolist()
    assert any((row != PAD).all() for row in g["targets"]["src"])
    hs = load_npz("hyp_scores.npz")
    assert np.array_equal(g["rule"]["hyp"], hs["rule__hyp"])
    for name in ("targets", "rule"):
        c = g[name]
        assert np.array_equal(lengths_of(c["hyp"], PAD, EOS), c["length"])
    assert np.array_equal(lengths_of(hs["rule__hyp"], PAD, EOS), hs["rule__length"])
    assert g["rule"]["length"].reshape(-1).tolist() == [1, 4, 11, 0, 6, 3]
    # the reference alone stays within the cap of the alignment comparison: few live positions have a near-tie
    for layer in (0, 1):
        c = g["targets"]
        R, _, T, _ = c["heads_l0"].shape
        _, compared, live = align_agreement(np.zeros((R, T), np.int32), c[f"heads_l{layer}"], c["length"],
                                            2 * 4 * float(c["f64_dist"][layer]))
        assert live - compared <= 0.02 * live


# -- the checkers flag one defect at a time -----------------------------------------------------------------------------
def _operands(H=3, dh=32, T=7, Ls=37, B=2, n_per_src=2, seed=5):
    rng = np.random.default_rng(seed)
    R = B * n_per_src
    q = rng.standard_normal((R * T, H * dh)).astype(np.float32)
    k = rng.standard_normal((B * Ls, H * dh)).astype(np.float32)
    key_pad = np.zeros((B, Ls), np.uint8)
    key_pad[0, 30:] = 1
    key_pad[1, 5] = 1
    mem_row = (np.arange(R) // n_per_src).astype(np.int32)
    length = np.array([T, 3, 0, 5], np.int32)
    return dict(q=q, k=k, key_pad=key_pad.reshape(-1), mem_row=mem_row, length=length, H=H, dh=dh, T=T, Ls=Ls,
                scale=1.0 / np.sqrt(dh), n_per_src=n_per_src)


def _check(defect, **over):
    o = {**_operands(), **over}
    ref = np_attn_probs(**o, dtype=np.float64)["heads"]
    clean = np_attn_probs(**o, dtype=np.float32)
    tol = 4 * np.abs(clean["heads"].astype(np.float64) - ref).max()
    got = np_attn_probs(**o, dtype=np.float32, defect=defect)
    pad_rows = (o["key_pad"].reshape(-1, o["Ls"]) != 0)[o["mem_row"]]
    return check_result(got, ref, pad_rows, o["length"], tol), got


def test_checkers_pass_the_clean_stand_in():
    assert _check(None)[0] == []


@pytest.mark.parametrize("defect,flag", [("no_scale", "tolerance"), ("pad_leak", "pad_zero"), ("unnormalised", "row_sum"),
                                         ("boundary", "nonlive_zero"), ("row_map", "tolerance"),
                                         ("nonlive_nonzero", "nonlive_zero"), ("align_zero", "align_nonlive")])
def test_checkers_flag_each_defect(defect, flag):
    assert flag in _check(defect)[0]


def test_checkers_flag_heads_summed_in_descending_order():
    """H = 3: (a + b) + c and (c + b) + a differ in the last bit somewhere."""
    bad, got = _check("descending_heads")
    assert bad == ["mean_bits"]
    assert np.abs(got["mean"].astype(np.float64) - head_mean(got["heads"]).astype(np.float64)).max() < 1e-6


def test_checkers_flag_the_last_maximum():
    """A tie is certain in a source that is all PAD: every mean is 0, so the first maximum is 0 and the last one Ls - 1."""
    key_pad = _operands()["key_pad"].copy().reshape(2, -1)
    key_pad[1, :] = 1                                       # rows 2, 3 read a source of PAD only: every mean is 0, first maximum 0
    bad, got = _check("last_max", key_pad=key_pad.reshape(-1))
    assert bad == ["align_first_max"]
    clean = _check(None, key_pad=key_pad.reshape(-1))
    assert clean[0] == [] and (clean[1]["align"][3, :5] == 0).all() and (clean[1]["heads"][3] == 0).all()


def test_row_sum_bound_and_first_argmax_helpers():
    assert EPS32 == np.finfo(np.float32).eps
    m = np.array([[[0.1, 0.4, 0.4, 0.0], [0.0, 0.0, 0.0, 0.0]]], np.float32)
    assert first_argmax(m, np.array([[True, False]])).tolist() == [[1, -1]]


# -- the boundary -------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound():
    lib = tta.lib()
    for name in NEW:
        assert name in N.SYMBOLS and hasattr(lib, name)
    assert lib.ttx_attn_probs_key_limit(32) >= 1024 and lib.ttx_attn_probs_key_limit(64) >= 1024
    assert lib.ttx_attn_probs_key_limit(48) == 0
    assert tta.NativeTransformer.attn_probs_key_limit(64) == lib.ttx_attn_probs_key_limit(64)
    assert lib.ttx_abi_version() == 4


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a machine without a GPU")
def test_entry_points_refuse_to_run_without_a_device():
    lib = tta.lib()
    assert lib.ttx_attention_maps(None, None, 1, 1, None, 2, 1, 2, 2, -1, None, None, None, None, None) == N.TTX_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.ttx_last_error()
    assert lib.ttx_debug_attn_probs(None, None, 32, None, 32, None, None, None, 1, 1, 1, 32, 1, 1, C.c_float(1.0), None, None, None,
                                    None) == N.TTX_ERR_NO_DEVICE


# -- the side file -------------------------------------------------------------------------------------------------------
class _Maps(NamedTuple):
    attn: object
    alignment: torch.Tensor
    length: torch.Tensor


def test_write_alignments_round_trip(tmp_path):
    al = torch.tensor([[[3, 1, 4, -1], [-1, -1, -1, -1]], [[0, 0, 2, 5], [7, -1, -1, -1]]], dtype=torch.int32)
    ln = torch.tensor([[3, 0], [4, 1]], dtype=torch.int32)
    path = tmp_path / "pred.align"
    scoring.write_alignments(str(path), _Maps(None, al[:1], ln[:1]))
    scoring.write_alignments(str(path), _Maps(None, al[1:], ln[1:]))
    assert path.read_text() == "3 1 4,\n0 0 2 5,7\n"
    assert scoring.read_alignments(str(path)) == [[[3, 1, 4], []], [[0, 0, 2, 5], [7]]]
