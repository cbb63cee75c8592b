"""The oracle at head dimension 64 against the reference's own outputs on the trained d = 128 / 2-head model (tests/golden/hd64_*):
test_oracle_model.py and test_oracle_decoding.py for that model.  No GPU."""
import numpy as np
import pytest
import torch

from oracle.model import OracleTransformer, config_from_state
from oracle.decoding import GreedyOracle, BeamSearchOracle, GreedySpeculativeOracle
from oracle.spec_beam import BeamSearchSpeculativeOracle
from util_models import load_npz, fixture_tokens, PAD, BOS, EOS
from util_hd64 import hd64_state, hd64_gen, BATCHES, NS, DS, BEAM

TOL = 5e-5  # absolute, as in test_oracle_model.py


@pytest.fixture(scope="module")
def model():
    st, cfg = hd64_state()
    ocfg = config_from_state(st, cfg["num_heads"])
    assert ocfg.embedding_dim // ocfg.num_heads == 64
    return OracleTransformer(ocfg, st)


def test_encode_decode_match_reference(model):
    io = load_npz("hd64_model_io.npz")
    src = torch.from_numpy(io["src"])
    mask = src == 0
    mem = model.encode_src(src, mask)
    ref_mem = torch.from_numpy(io["memory"])
    assert mem.shape[-1] == 128
    assert (mem - ref_mem)[~mask].abs().max() < TOL
    assert float(mem[mask].abs().max()) == 0.0
    lg = model.decode_tgt(torch.from_numpy(io["tgt_in"]), ref_mem, mask)
    assert (lg - torch.from_numpy(io["logits"])).abs().max() < TOL
    lg = model.decode_tgt(torch.from_numpy(io["tgt_ragged"]), ref_mem, mask)
    assert (lg - torch.from_numpy(io["logits_ragged"])).abs().max() < TOL
    fwd = model(src, torch.from_numpy(io["tgt_in"][:, :1]))
    assert (fwd - torch.from_numpy(io["fwd_bos"])).abs().max() < TOL


def test_float64_lead_along_the_target_paths():
    """What exact token identity of the greedy paths on the GPU rests on: the float64 oracle follows the ten targets with a lead
    of its best logit over the second best that is thousands of times the 1e-3 the logits are held to."""
    st, cfg = hd64_state()
    o64 = OracleTransformer(config_from_state(st, cfg["num_heads"]), st, dtype=torch.float64)
    src, tgt, _, _ = fixture_tokens()
    mask = src == PAD
    lg = o64.decode_tgt(tgt[:, :-1], o64.encode_src(src, mask), mask)
    real = tgt[:, 1:] != PAD
    assert torch.equal(lg.argmax(-1)[real], tgt[:, 1:][real])
    top2 = lg.topk(2, -1).values
    lead = float((top2[..., 0] - top2[..., 1])[real].min())
    assert abs(lead - float(load_npz("hd64_model_io.npz")["min_lead"])) < 1e-6 and lead > 3.0


def test_greedy_matches_reference(model):
    gold = hd64_gen("greedy")
    src, _, _, _ = fixture_tokens()
    for bsz in BATCHES:
        for max_len in (150, 40):
            g = GreedyOracle(model, max_len, PAD, BOS, EOS)
            for i in range(0, 10, bsz):
                out = g.generate(src[i:i + bsz]).numpy()
                ref = gold[f"b{bsz}_m{max_len}_tokens"][i:i + bsz]
                np.testing.assert_array_equal(out, ref[:, :, :out.shape[2]])
            assert g.model_calls_num == int(gold[f"b{bsz}_m{max_len}_calls"])


def test_beam_matches_reference(model):
    gold = hd64_gen("beam")
    src, _, _, _ = fixture_tokens()
    for bsz in BATCHES:
        g = BeamSearchOracle(model, BEAM, 150, PAD, BOS, EOS)
        for bi, i in enumerate(range(0, 10, bsz)):
            np.testing.assert_array_equal(g.generate(src[i:i + bsz]).numpy(), gold[f"b{bsz}_k{BEAM}_batch{bi}"])
        assert g.model_calls_num == int(gold[f"b{bsz}_k{BEAM}_calls"])


@pytest.mark.parametrize("bsz", BATCHES)
def test_greedy_speculative_matches_reference(model, bsz):
    gold = hd64_gen("spec_greedy")
    src, _, c, _ = fixture_tokens()
    for N in NS:
        for D in DS:
            g = GreedySpeculativeOracle(model, 150, D, N, PAD, BOS, EOS, c)
            out = np.concatenate([g.generate(src[i:i + bsz]).numpy() for i in range(0, 10, bsz)])
            np.testing.assert_array_equal(out, gold[f"b{bsz}_n{N}_d{D}_tokens"])
            assert g.model_calls_num == int(gold[f"b{bsz}_n{N}_d{D}_calls"])


def test_greedy_speculative_unfinished_rows_stay_pad(model):
    gold = hd64_gen("spec_greedy")
    src, _, c, _ = fixture_tokens()
    for max_len in (30, 45):
        g = GreedySpeculativeOracle(model, max_len, 10, 3, PAD, BOS, EOS, c)
        np.testing.assert_array_equal(g.generate(src).numpy(), gold[f"short_m{max_len}_tokens"])
        assert g.model_calls_num == int(gold[f"short_m{max_len}_calls"])


@pytest.mark.parametrize("smart", [False, True])
def test_beam_speculative_matches_reference(model, smart):
    """Every hypothesis of every source and the three counters, exactly: no rank needs a near-tie rule."""
    gold = hd64_gen("spec_beam")
    src, _, c, V = fixture_tokens()
    ci = total = 0
    while f"smart{int(smart)}_case{ci}_rows" in gold:
        key = f"smart{int(smart)}_case{ci}"
        rows = gold[key + "_rows"].tolist()
        bsz, nbest, N, D = gold[key + "_params"].tolist()
        g = BeamSearchSpeculativeOracle(model, 150, nbest, D, N, V, smart, PAD, BOS, EOS, c, max_steps=400)
        for bi, i in enumerate(range(0, len(rows), bsz)):
            sel = src[rows[i:i + bsz]]
            out = g.generate(sel[:, :int((sel != PAD).sum(1).max())]).numpy()
            np.testing.assert_array_equal(out, gold[f"{key}_batch{bi}"])
            total += out.shape[0] * out.shape[1]
        assert (g.model_calls_num, g.accepted_tokens_num, g.produced_non_pad_tokens) == \
            (int(gold[key + "_calls"]), int(gold[key + "_accepted"]), int(gold[key + "_produced"])), key
        ci += 1
    assert ci == 4 and total >= 40
