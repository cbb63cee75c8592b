"""Head dimension 64 (embedding_dim / num_heads = 64) end to end.

1. The model envelope of tests/test_gpu_envelope.py at head dimension 64, with that module's bars and helpers (logits within
   1e-3 of the float64 oracle, memory within 1e-4, the same argmax where the oracle's lead exceeds 2e-3, at most 1 % of the
   positions left out), on five seeded models:

       d / heads   F      V      layers  seed
       64 / 1      64     5      1       12     one head: the whole row is one head
       128 / 2     192    37     1       11
       256 / 4     2048   64     1       11     the bench model's width with 4 heads
       512 / 8     512    300    1       11     the base Transformer's d / heads
       1024 / 16   4096   1000   2       11

   test_fp32_oracle_meets_the_bars (no GPU) asserts that fp32 arithmetic meets the bars on these seeds (seed 11 does not for the
   first model: its logits leave more than 1 % of the positions undecided).

2. The reference's own model trained at d = 128 with 2 heads (tests/golden/hd64_*, tests/golden/make_golden_hd64.py): logits, the
   four generators, generate_many through the slot pool and the batch pool, score, teacher_forced and run_predict through the
   Lightning module, against the reference's outputs.  Tokens and counters of the greedy paths must be identical (the float64
   oracle's smallest lead along the target paths is 3.79).  Beam hypotheses: top-1 always identical; a lower rank may differ only
   where the oracle scores the two hypotheses within 2e-3 of each other (the rule of tests/test_gpu_beam_native.py).

3. embedding_dim / num_heads of 16 or 128, and an indivisible pair, are refused with a message that names 32 and 64.
"""
import functools
import json

import numpy as np
import pytest
import torch

import test_gpu_envelope as E
from util_models import seeded_weights, state_shapes, load_npz, fixture_tokens, upto_eos, PAD, BOS, EOS
from util_hd64 import hd64_state, hd64_gen, BATCHES, NS, DS, BEAM

#          name              d    heads  F     V     layers  seed
MODELS = [("d64-h1", 64, 1, 64, 5, 1, 12),
          ("d128-h2", 128, 2, 192, 37, 1, 11),
          ("d256-h4", 256, 4, 2048, 64, 1, 11),
          ("d512-h8", 512, 8, 512, 300, 1, 11),
          ("d1024-h16", 1024, 16, 4096, 1000, 2, 11)]
IDS = [m[0] for m in MODELS]


@functools.lru_cache(maxsize=None)
def state_of(name):
    _, d, heads, F, V, layers, seed = next(m for m in MODELS if m[0] == name)
    assert d // heads == 64
    return seeded_weights(state_shapes(V, d, F, layers, layers), seed), heads, V


@functools.lru_cache(maxsize=None)
def oracle_of(name, dtype):
    from oracle.model import OracleTransformer, config_from_state
    st, heads, _ = state_of(name)
    return OracleTransformer(config_from_state(st, heads), st, dtype=dtype)


@functools.lru_cache(maxsize=None)
def io_of(name):
    """test_gpu_envelope.io_of for the models of this module: its ragged inputs and the float64 oracle's outputs on them.  The
    token generator is seeded from the model's name as there, plus the first k = 0, 1, ... with which the float64 oracle itself
    leaves at most 1 % of the positions undecided (a property of the reference on the inputs, whatever is compared with it
    later): k = 0 for every model but d512-h8, where one of the 33 positions has a lead of 0.00199 and k = 1 is taken."""
    _, _, V = state_of(name)
    o64 = oracle_of(name, torch.float64)
    for k in range(8):
        gen = torch.Generator().manual_seed(sum(map(ord, name)) + k)
        src = E.ragged(gen, [9, 12, 6], V, 12, eos=True)
        tgt = E.ragged(gen, [11, 7, 9], V, 11, eos=False)
        mask = src == PAD
        memory = o64.encode_src(src, mask)
        lg64 = o64.decode_tgt(tgt, memory, mask)
        top2 = lg64.topk(2, -1).values
        if float(((top2[..., 0] - top2[..., 1]) <= E.GAP).float().mean()) <= 0.01:
            return src, tgt, mask, memory, lg64
    raise AssertionError(f"{name}: no input seed gives the float64 oracle decided positions")


@pytest.mark.parametrize("name", IDS)
def test_fp32_oracle_meets_the_bars(name):
    src, tgt, mask, mem64, lg64 = io_of(name)
    o32 = oracle_of(name, torch.float32)
    d_mem = float((o32.encode_src(src, mask).double() - mem64)[~mask].abs().max())
    err, left_out = E.compare_logits(o32.decode_tgt(tgt, mem64.float(), mask), lg64, f"{name} float32 oracle")
    print(f"{name}: float32 oracle against float64: memory {d_mem:.3e}, logits {err:.3e}, positions left out {left_out:.1%}")
    assert d_mem < E.MEMORY_TOL


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_envelope_at_head_dimension_64(tta, name):
    st, heads, _ = state_of(name)
    src, tgt, mask, mem64, lg64 = io_of(name)
    native = tta.NativeTransformer(st, heads, PAD, device=0)
    mem = native.encode_src(src.cuda(), mask.cuda()).cpu()
    d_mem = float((mem.double() - mem64)[~mask].abs().max())
    assert float(mem[mask].abs().max()) == 0.0
    lg = native.decode_tgt(tgt.cuda(), mem64.float().cuda(), memory_pad_mask=mask.cuda()).cpu()
    err, left_out = E.compare_logits(lg, lg64, name)
    print(f"{name}: memory error {d_mem:.3e}, logits error {err:.3e}, logits absmax {float(lg64.abs().max()):.2f}, "
          f"positions left out {left_out:.1%}")
    assert d_mem < E.MEMORY_TOL
    native.close()


# ---- the trained d = 128 / 2-head model against the reference ------------------------------------------------------------------
@pytest.fixture(scope="module")
def hd64(tta):
    st, cfg = hd64_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)


@pytest.fixture(scope="module")
def oracle():
    from oracle.model import OracleTransformer, config_from_state
    st, cfg = hd64_state()
    return OracleTransformer(config_from_state(st, cfg["num_heads"]), st)


@pytest.mark.gpu
def test_logits_match_reference(hd64):
    io = load_npz("hd64_model_io.npz")
    src = torch.from_numpy(io["src"]).cuda()
    mask = src == 0
    mem = hd64.encode_src(src, mask)
    ref_mem = torch.from_numpy(io["memory"]).cuda()
    assert (mem - ref_mem)[~mask].abs().max().item() < 1e-4 and float(mem[mask].abs().max()) == 0.0
    for tgt, ref in (("tgt_in", "logits"), ("tgt_ragged", "logits_ragged")):
        lg = hd64.decode_tgt(torch.from_numpy(io[tgt]).cuda(), ref_mem, memory_pad_mask=mask)
        ref = torch.from_numpy(io[ref]).cuda()
        assert (lg - ref).abs().max().item() < 1e-3
        assert torch.equal(lg.argmax(-1), ref.argmax(-1))
    fwd = hd64(src, torch.from_numpy(io["tgt_in"][:, :1]).cuda())
    assert (fwd - torch.from_numpy(io["fwd_bos"]).cuda()).abs().max().item() < 1e-3


@pytest.mark.gpu
def test_greedy_and_greedy_speculative_match_reference(tta, hd64, monkeypatch):
    src, _, c, _ = fixture_tokens()
    gold = hd64_gen("greedy")
    for bsz in BATCHES:
        for max_len in (150, 40):
            g = tta.TranslationInferenceGreedy(hd64, max_len, PAD, BOS, EOS)
            for i in range(0, 10, bsz):
                out = g.generate(src[i:i + bsz].cuda()).cpu().numpy()
                np.testing.assert_array_equal(out, gold[f"b{bsz}_m{max_len}_tokens"][i:i + bsz][:, :, :out.shape[2]])
            assert g.model_calls_num == int(gold[f"b{bsz}_m{max_len}_calls"])
    gold = hd64_gen("spec_greedy")
    for bsz in BATCHES:
        for N in NS:
            for D in DS:
                g = tta.TranslationInferenceGreedySpeculative(hd64, 150, D, N, PAD, BOS, EOS, c)
                out = np.concatenate([g.generate(src[i:i + bsz].cuda()).cpu().numpy() for i in range(0, 10, bsz)])
                np.testing.assert_array_equal(out, gold[f"b{bsz}_n{N}_d{D}_tokens"])
                assert g.model_calls_num == int(gold[f"b{bsz}_n{N}_d{D}_calls"])
    for max_len in (30, 45):
        g = tta.TranslationInferenceGreedySpeculative(hd64, max_len, 10, 3, PAD, BOS, EOS, c)
        np.testing.assert_array_equal(g.generate(src.cuda()).cpu().numpy(), gold[f"short_m{max_len}_tokens"])
        assert g.model_calls_num == int(gold[f"short_m{max_len}_calls"])
    # the streaming fallback k_attn for every attention launch: the same tokens
    monkeypatch.setenv("TTX_ATTN_FALLBACK", "1")
    st, cfg = hd64_state()
    slow = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    monkeypatch.delenv("TTX_ATTN_FALLBACK")
    g = tta.TranslationInferenceGreedySpeculative(slow, 150, 10, 3, PAD, BOS, EOS, c)
    np.testing.assert_array_equal(g.generate(src.cuda()).cpu().numpy(), gold["b10_n3_d10_tokens"])
    assert g.model_calls_num == int(gold["b10_n3_d10_calls"])
    slow.close()


def _hyp_logprob(oracle, src_row, hyp):
    """Cumulative log-probability of a hypothesis (tokens up to its first EOS) under the oracle model."""
    toks = upto_eos(hyp)
    t = torch.tensor([toks], dtype=torch.int64)
    s = src_row[None]
    mask = s == PAD
    lp = oracle.decode_tgt(t[:, :-1], oracle.encode_src(s, mask), mask)[0].log_softmax(-1)
    return float(lp[torch.arange(len(toks) - 1), t[0, 1:]].sum())


def _same_hypotheses(out, ref, sel, oracle, label):
    """Top-1 identical; a lower rank may differ only where the oracle scores the two hypotheses within 2e-3 of each other (two
    cumulative fp32 scores closer than that can rank either way).  Returns the number of such ranks."""
    assert out.shape[:2] == ref.shape[:2], label
    n_diff = 0
    for b in range(out.shape[0]):
        assert upto_eos(out[b, 0]) == upto_eos(ref[b, 0]), (label, b)
        for k in range(1, out.shape[1]):
            if upto_eos(out[b, k]) != upto_eos(ref[b, k]):
                sa, sb = _hyp_logprob(oracle, sel[b], out[b, k]), _hyp_logprob(oracle, sel[b], ref[b, k])
                print(f"{label} source {b} rank {k}: HIP {upto_eos(out[b, k])} ({sa:.6f}) vs reference {upto_eos(ref[b, k])} ({sb:.6f})")
                assert abs(sa - sb) < 2e-3, (label, b, k)
                n_diff += 1
    return n_diff


@pytest.mark.gpu
def test_beam_search_matches_reference(tta, hd64, oracle):
    src, _, _, _ = fixture_tokens()
    gold = hd64_gen("beam")
    for bsz in BATCHES:
        g = tta.TranslationInferenceBeamSearch(hd64, BEAM, 150, PAD, BOS, EOS)
        n_diff = 0
        for bi, i in enumerate(range(0, 10, bsz)):
            out = g.generate(src[i:i + bsz].cuda()).cpu().numpy()
            n_diff += _same_hypotheses(out, gold[f"b{bsz}_k{BEAM}_batch{bi}"], src[i:i + bsz], oracle, f"beam b{bsz} batch {bi}")
        if n_diff == 0:
            assert g.model_calls_num == int(gold[f"b{bsz}_k{BEAM}_calls"])


def _spec_beam_cases(gold, smart):
    src, _, _, _ = fixture_tokens()
    ci = 0
    while f"smart{int(smart)}_case{ci}_rows" in gold:
        key = f"smart{int(smart)}_case{ci}"
        rows = gold[key + "_rows"].tolist()
        bsz, nbest, N, D = gold[key + "_params"].tolist()
        batches = []
        for i in range(0, len(rows), bsz):
            sel = src[rows[i:i + bsz]]
            batches.append(sel[:, :int((sel != PAD).sum(1).max())])
        yield key, (nbest, N, D), batches
        ci += 1


@pytest.mark.gpu
@pytest.mark.parametrize("smart", [False, True])
def test_beam_speculative_matches_reference(tta, hd64, oracle, smart):
    """Per batch, through the sessions in flight and through the batch pool."""
    gold = hd64_gen("spec_beam")
    _, _, c, V = fixture_tokens()
    n_cases = 0
    for key, (nbest, N, D), batches in _spec_beam_cases(gold, smart):
        mk = lambda: tta.TranslationInferenceBeamSearchSpeculative(hd64, 150, nbest, D, N, V, smart, PAD, BOS, EOS, c, max_steps=400)
        g = mk()
        outs = [g.generate(b.cuda()) for b in batches]
        n_diff = sum(_same_hypotheses(o.cpu().numpy(), gold[f"{key}_batch{bi}"], batches[bi], oracle, f"{key} batch {bi}")
                     for bi, o in enumerate(outs))
        if n_diff == 0:
            assert (g.model_calls_num, g.accepted_tokens_num, g.produced_non_pad_tokens) == \
                (int(gold[key + "_calls"]), int(gold[key + "_accepted"]), int(gold[key + "_produced"])), key
        for kw in (dict(in_flight=3), dict(in_flight=3, pool=True)):
            m = mk()
            many = m.generate_many([b.cuda() for b in batches], **kw)
            for a, b in zip(many, outs):
                assert torch.equal(a, b), (key, kw)
            assert (m.model_calls_num, m.accepted_tokens_num, m.produced_non_pad_tokens) == \
                (g.model_calls_num, g.accepted_tokens_num, g.produced_non_pad_tokens), (key, kw)
            if kw.get("pool"):
                assert m.stats_total.get("pool_calls", 0) == 1
        n_cases += 1
    assert n_cases == 4


@pytest.mark.gpu
def test_generate_many_through_the_slot_pool(tta, hd64):
    """Greedy-speculative rows of many batches through the slot pool and through fixed row groups: every batch equals the
    reference's tokens for its rows (the b1 golden holds every fixture row decoded alone)."""
    fsrc, _, c, _ = fixture_tokens()
    gold = hd64_gen("spec_greedy")["b1_n3_d10_tokens"]
    order = torch.randperm(40, generator=torch.Generator().manual_seed(5)) % 10
    batches, rows = [], []
    for i in range(0, 40, 7):
        idx = order[i:i + 7]
        sel = fsrc[idx]
        batches.append(sel[:, :int((sel != PAD).sum(1).max())].cuda())
        rows.append(idx.tolist())
    for pool in (True, False):
        g = tta.TranslationInferenceGreedySpeculative(hd64, 150, 10, 3, PAD, BOS, EOS, c)
        out = g.generate_many(batches, in_flight=2, reorder=True, group_size=16, pool=pool)
        assert "device" in g.stats_total                     # the row schedule ran (no fallback to the batches as given)
        for o, idx in zip(out, rows):
            o = o.cpu().numpy()
            for j, r in enumerate(idx):
                assert upto_eos(o[j, 0]) == upto_eos(gold[r, 0]), (pool, r)


@pytest.mark.gpu
def test_score_and_teacher_forced_match_reference(tta, hd64):
    from util_score import reference_scores
    from util_eval import reference_metrics, same_float
    io = load_npz("hd64_model_io.npz")
    src, tgt, c, V = fixture_tokens()
    ref_logits = torch.from_numpy(io["logits"])                # the reference's forward(src, tgt[:, :-1])
    # score: the ten targets as N = 1 hypotheses, and what the beam search returns
    hyp = tgt[:, None, :]
    r = hd64.score_hypotheses(src.cuda(), hyp.cuda(), eos_token_idx=EOS, return_token_logp=True)
    ref = reference_scores(ref_logits[:, None], hyp, PAD, EOS)
    assert torch.equal(r.length.cpu().long(), ref["length"]) and torch.equal(r.finished.cpu().bool(), ref["finished"])
    assert (r.token_logp.cpu().double() - ref["tok_logp"]).abs().max().item() < 2e-4    # test_gpu_score.py's bar for a logp
    assert (r.score.cpu().double() - ref["score"]).abs().max().item() < 2e-4 * hyp.shape[-1]
    g = tta.TranslationInferenceBeamSearch(hd64, BEAM, 150, PAD, BOS, EOS)
    pred = g.generate(src[:4].cuda())
    sc = g.score(src[:4].cuda(), pred)
    assert sc.score.shape == pred.shape[:2] and bool((sc.score[:, :-1] >= sc.score[:, 1:] - 2e-3).all())
    # teacher_forced: loss and accuracies of the reference's metrics on the reference's logits
    t = hd64.teacher_forced(src.cuda(), tgt.cuda(), return_logits=True, eos_token_idx=EOS)
    want = reference_metrics(ref_logits, tgt, EOS)
    assert (t.logits.cpu() - ref_logits).abs().max().item() < 1e-3
    assert torch.equal(t.pred_tokens.cpu(), ref_logits.argmax(-1))       # the trained model's leads are far above 1e-3
    assert abs(float(t.loss) - want["loss"]) <= 1e-4
    assert same_float(float(t.token_acc), want["token_acc"]) and same_float(float(t.seq_acc), want["seq_acc"])


@pytest.mark.gpu
@pytest.mark.parametrize("generation", ["greedy_speculative", "beam_search_speculative"])
def test_run_predict_through_the_lightning_module(tta, tmp_path, generation):
    from test_gpu_lightning_surface import FixtureTokenizer, CsvWriter
    st, cfg = hd64_state()
    tkz = FixtureTokenizer()
    mod = tta.VanillaEncoderDecoderTransformerLightning(
        src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
        num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
        share_embeddings=True, generation=generation, beam_size=3, max_len=150, n_drafts=3, draft_len=10, smart_drafts_mode=False,
        report_prediction_file=str(tmp_path / "reports" / "r.txt"))
    missing, unexpected = mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    assert not missing and not unexpected
    src, tgt, _, _ = fixture_tokens()
    rows = hd64_gen("spec_beam")["smart0_case0_rows"].tolist() if "beam" in generation else list(range(10))
    batches = [{"src_tokens": src[rows[i:i + 5]].cuda(), "tgt_tokens": tgt[rows[i:i + 5]].cuda()} for i in range(0, len(rows), 5)]
    out_csv = tmp_path / "pred.csv"
    dm = type("DM", (), {"batch_size": 5, "tgt_test_path": "tests/product_prediction_tgt_test.txt"})()
    outs = tta.run_predict(mod, batches, writer=CsvWriter(out_csv), datamodule=dm)
    assert all(o.ndim == 3 and o.dtype == torch.int64 for o in outs)
    lines = out_csv.read_text().strip().split("\n")
    # the model is overfit on the fixtures: every top-1 string is the target
    assert len(lines) == len(rows) + 1 and all(l.split(",")[1] == l.split(",")[2] for l in lines[1:])
    rep = json.loads((tmp_path / "reports" / "r.txt").read_text().strip().split("\n")[-1])
    assert rep["algorithm"] == generation and rep["model_calls"] > 0


# ---- what stays refused ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d,heads", [(64, 4), (128, 1), (256, 16), (256, 2), (192, 5), (128, 3)], ids=lambda v: str(v))
def test_other_head_dimensions_are_refused(tta, d, heads):
    """16 and 128, and pairs in which num_heads does not divide embedding_dim (192 / 5 would truncate to 38, 128 / 3 to 42)."""
    from translation_transformer_amd import _native as N_
    st = seeded_weights(state_shapes(7, d, 64, 1, 1), 3)
    with pytest.raises(N_.TtxError) as e:
        tta.NativeTransformer(st, heads, PAD, device=0)
    assert e.value.code == N_.TTX_ERR_INVALID
    if d % 64 == 0:
        assert "32 or 64" in str(e.value)
