"""activation="gelu" end to end, on the reference's own GELU model (tests/golden/gelu_*, tests/golden/make_golden_gelu.py: 2+2
layers, d = 64, 2 heads, F = 128, trained on the ten fixture pairs).

encode_src / decode_tgt / forward and the ragged logits meet the bars tests/test_gpu_model.py applies to the tiny model; the four
generators return the reference's tokens and counters exactly (the float32 oracle reproduced every one of them when the fixtures
were made, and the float64 oracle's smallest lead along the target paths is 4.9); generate_many returns what the per-batch calls
return; teacher_forced and score_hypotheses agree with the float64 GELU oracle within the bars of tests/test_gpu_eval.py and
tests/test_gpu_score.py; the Lightning module with activation="gelu" predicts the golden tokens.  Negative control: the same
weights as a ReLU model are more than 100 bars away, so the flag demonstrably reaches the kernels; and a ReLU model built afterwards
still returns the ReLU goldens.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from util_models import load_npz, tiny_state, fixture_tokens, upto_eos, PAD, BOS, EOS
from util_gelu import GeluOracleTransformer, gelu_state, gelu_gen, BATCHES, NS, DS, BEAM, ACT_GELU, ACT_RELU

pytestmark = pytest.mark.gpu

LOGIT_TOL, MEMORY_TOL = 1e-3, 1e-4          # tests/test_gpu_model.py


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def gelu(tta):
    st, cfg = gelu_state()
    m = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0, activation=cfg["activation"])
    assert m.activation == "gelu" and m._lib.ttx_model_activation(m._model) == ACT_GELU
    return m


@pytest.fixture(scope="module")
def oracle64():
    from oracle.model import config_from_state
    st, cfg = gelu_state()
    return GeluOracleTransformer(config_from_state(st, cfg["num_heads"]), st, dtype=torch.float64)


def same_tokens(got, want, what=""):
    """Equal over the common width, nothing but PAD beyond it (the fixtures are stored without their all-PAD tail columns)."""
    got, want = np.asarray(got), np.asarray(want)
    w = min(got.shape[-1], want.shape[-1])
    assert got.shape[:-1] == want.shape[:-1], what
    np.testing.assert_array_equal(got[..., :w], want[..., :w], err_msg=what)
    assert not (got[..., w:] != PAD).any() and not (want[..., w:] != PAD).any(), what


def _logit_errors(model):
    """(memory error, [logits errors], argmax equal) of a model against the reference's GELU outputs."""
    io = load_npz("gelu_model_io.npz")
    src = torch.from_numpy(io["src"]).cuda()
    mask = src == 0
    mem = model.encode_src(src, mask)
    ref_mem = torch.from_numpy(io["memory"]).cuda()
    assert float(mem[mask].abs().max()) == 0.0
    errs, same = [], True
    for tgt, ref in (("tgt_in", "logits"), ("tgt_ragged", "logits_ragged")):
        lg = model.decode_tgt(torch.from_numpy(io[tgt]).cuda(), ref_mem, memory_pad_mask=mask)
        ref = torch.from_numpy(io[ref]).cuda()
        errs.append((lg - ref).abs().max().item())
        same = same and torch.equal(lg.argmax(-1), ref.argmax(-1))
    fwd = model(src, torch.from_numpy(io["tgt_in"][:, :1]).cuda())
    errs.append((fwd - torch.from_numpy(io["fwd_bos"]).cuda()).abs().max().item())
    return (mem - ref_mem)[~mask].abs().max().item(), errs, same


def test_logits_match_reference(gelu):
    d_mem, errs, same = _logit_errors(gelu)
    print(f"GELU model: memory error {d_mem:.3e}, logits / ragged logits / forward errors {errs}")
    assert d_mem < MEMORY_TOL and max(errs) < LOGIT_TOL and same
    assert float(load_npz("gelu_model_io.npz")["min_lead"]) > 1.0


def test_the_same_weights_as_a_relu_model_are_far_away(tta):
    """Negative control: the activation reaches the kernels."""
    st, cfg = gelu_state()
    relu = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    assert relu.activation == "relu" and relu._lib.ttx_model_activation(relu._model) == ACT_RELU
    d_mem, errs, _ = _logit_errors(relu)
    print(f"the GELU weights under ReLU: memory differs by {d_mem:.3e}, logits by {errs}")
    assert d_mem > 100 * MEMORY_TOL and min(errs) > 100 * LOGIT_TOL
    relu.close()


def test_activation_is_fixed_once_a_session_exists(tta, gelu):
    from translation_transformer_amd import _native as N_
    lib = gelu._lib
    for act in (ACT_RELU, ACT_GELU, 0, 3):
        assert lib.ttx_model_set_activation(gelu._model, act) == N_.TTX_ERR_INVALID
        assert lib.ttx_model_activation(gelu._model) == ACT_GELU
    assert lib.ttx_model_set_activation(None, ACT_GELU) == N_.TTX_ERR_INVALID
    # before the first session: both values are taken, everything else is refused and changes nothing
    cfg = gelu.cfg
    model = C.c_void_p()
    N_.check(lib.ttx_model_create_empty(C.byref(cfg), 0, C.byref(model)))
    assert lib.ttx_model_activation(model) == ACT_RELU
    assert lib.ttx_model_set_activation(model, ACT_GELU) == N_.TTX_OK and lib.ttx_model_activation(model) == ACT_GELU
    for act in (0, 3, -1):
        assert lib.ttx_model_set_activation(model, act) == N_.TTX_ERR_INVALID and lib.ttx_model_activation(model) == ACT_GELU
    assert lib.ttx_model_set_activation(model, ACT_RELU) == N_.TTX_OK and lib.ttx_model_activation(model) == ACT_RELU
    lib.ttx_model_destroy(model)
    with pytest.raises(ValueError, match="relu.*gelu"):
        tta.NativeTransformer(gelu_state()[0], 2, 0, device=0, activation="GELU")


def test_empty_model_filled_from_the_blob_is_the_gelu_model(tta, gelu):
    """The second construction path (state_dict=None, shape=...) takes the activation too: the blob does not hold it."""
    from translation_transformer_amd.model import shape_of_state
    st, cfg = gelu_state()
    b = tta.NativeTransformer(None, cfg["num_heads"], 0, device=0, shape=shape_of_state(st), activation="gelu")
    assert b.activation == "gelu"
    b.blob_tensor().copy_(gelu.blob_tensor())
    torch.cuda.synchronize()
    io = load_npz("gelu_model_io.npz")
    src, tgt = torch.from_numpy(io["src"]).cuda(), torch.from_numpy(io["tgt_in"]).cuda()
    assert torch.equal(b(src, tgt), gelu(src, tgt))
    meta = tta.dist.model_metadata(st, "gelu")
    assert meta == {"shape": shape_of_state(st), "activation": "gelu"}
    one = tta.dist.broadcast_model(st, cfg["num_heads"], 0, 0, None, activation="gelu")       # a single rank: built directly
    assert one.activation == "gelu" and torch.equal(one(src, tgt), gelu(src, tgt))
    one.close()
    b.close()


def test_greedy_and_greedy_speculative_match_reference(tta, gelu):
    src, _, c, _ = fixture_tokens()
    gold = gelu_gen("greedy")
    for bsz in BATCHES:
        for max_len in (150, 40):
            g = tta.TranslationInferenceGreedy(gelu, max_len, PAD, BOS, EOS)
            for i in range(0, 10, bsz):
                out = g.generate(src[i:i + bsz].cuda()).cpu().numpy()
                np.testing.assert_array_equal(out, gold[f"b{bsz}_m{max_len}_tokens"][i:i + bsz][:, :, :out.shape[2]])
            assert g.model_calls_num == int(gold[f"b{bsz}_m{max_len}_calls"])
    gold = gelu_gen("spec_greedy")
    for bsz in BATCHES:
        for N in NS:
            for D in DS:
                g = tta.TranslationInferenceGreedySpeculative(gelu, 150, D, N, PAD, BOS, EOS, c)
                out = np.concatenate([g.generate(src[i:i + bsz].cuda()).cpu().numpy() for i in range(0, 10, bsz)])
                np.testing.assert_array_equal(out, gold[f"b{bsz}_n{N}_d{D}_tokens"])
                assert g.model_calls_num == int(gold[f"b{bsz}_n{N}_d{D}_calls"])
    for max_len in (30, 45):
        g = tta.TranslationInferenceGreedySpeculative(gelu, max_len, 10, 3, PAD, BOS, EOS, c)
        np.testing.assert_array_equal(g.generate(src.cuda()).cpu().numpy(), gold[f"short_m{max_len}_tokens"])
        assert g.model_calls_num == int(gold[f"short_m{max_len}_calls"])


def test_beam_search_matches_reference(tta, gelu):
    src, _, _, _ = fixture_tokens()
    gold = gelu_gen("beam")
    for bsz in BATCHES:
        g = tta.TranslationInferenceBeamSearch(gelu, BEAM, 150, PAD, BOS, EOS)
        for bi, i in enumerate(range(0, 10, bsz)):
            out = g.generate(src[i:i + bsz].cuda()).cpu().numpy()
            same_tokens(out, gold[f"b{bsz}_k{BEAM}_batch{bi}"], f"beam b{bsz} batch {bi}")
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


@pytest.mark.parametrize("smart", [False, True], ids=["all-drafts", "smart"])
def test_beam_speculative_matches_reference(tta, gelu, smart):
    """Per batch against the reference; case 2 (two batches) also through the batch pool: the same tokens and counters."""
    gold = gelu_gen("spec_beam")
    _, _, c, V = fixture_tokens()
    n_cases = 0
    for key, (nbest, N, D), batches in _spec_beam_cases(gold, smart):
        mk = lambda: tta.TranslationInferenceBeamSearchSpeculative(gelu, 150, nbest, D, N, V, smart, PAD, BOS, EOS, c, max_steps=400)
        g = mk()
        outs = [g.generate(b.cuda()) for b in batches]
        for bi, o in enumerate(outs):
            same_tokens(o.cpu().numpy(), gold[f"{key}_batch{bi}"], f"{key} batch {bi}")
        assert (g.model_calls_num, g.accepted_tokens_num, g.produced_non_pad_tokens) == \
            (int(gold[key + "_calls"]), int(gold[key + "_accepted"]), int(gold[key + "_produced"])), key
        if key.endswith("case2"):
            assert len(batches) >= 2
            m = mk()
            many = m.generate_many([b.cuda() for b in batches], in_flight=3, pool=True)
            for a, b in zip(many, outs):
                assert torch.equal(a, b), key
            assert (m.model_calls_num, m.accepted_tokens_num, m.produced_non_pad_tokens) == \
                (g.model_calls_num, g.accepted_tokens_num, g.produced_non_pad_tokens), key
            assert m.stats_total.get("pool_calls", 0) == 1
        n_cases += 1
    assert n_cases == 4


def test_generate_many_through_the_slot_pool(tta, gelu):
    """Greedy-speculative rows of many batches through the slot pool: every batch equals the reference's tokens for its rows."""
    fsrc, _, c, _ = fixture_tokens()
    gold = gelu_gen("spec_greedy")["b1_n3_d10_tokens"]
    order = torch.randperm(40, generator=torch.Generator().manual_seed(5)) % 10
    batches, rows = [], []
    for i in range(0, 40, 7):
        idx = order[i:i + 7]
        sel = fsrc[idx]
        batches.append(sel[:, :int((sel != PAD).sum(1).max())].cuda())
        rows.append(idx.tolist())
    g = tta.TranslationInferenceGreedySpeculative(gelu, 150, 10, 3, PAD, BOS, EOS, c)
    out = g.generate_many(batches, in_flight=2, reorder=True, group_size=16, pool=True)
    assert "device" in g.stats_total                     # the row schedule ran (no fallback to the batches as given)
    per_batch = tta.TranslationInferenceGreedySpeculative(gelu, 150, 10, 3, PAD, BOS, EOS, c)
    for o, idx, b in zip(out, rows, batches):
        single = per_batch.generate(b).cpu().numpy()
        o = o.cpu().numpy()
        for j, r in enumerate(idx):
            assert upto_eos(o[j, 0]) == upto_eos(gold[r, 0]) == upto_eos(single[j, 0]), r


def test_score_and_teacher_forced_match_the_float64_oracle(tta, gelu, oracle64):
    from util_score import reference_scores
    from util_eval import reference_metrics, same_float
    src, tgt, c, V = fixture_tokens()
    mask = src == PAD
    with torch.inference_mode():
        lg64 = oracle64.decode_tgt(tgt[:, :-1], oracle64.encode_src(src, mask), mask)
    # teacher_forced: the bars of tests/test_gpu_eval.py (_check_teacher_forced)
    t = gelu.teacher_forced(src.cuda(), tgt.cuda(), return_logits=True, eos_token_idx=EOS)
    want = reference_metrics(lg64, tgt, EOS)
    d_lg = (t.logits.cpu().double() - lg64).abs().max().item()
    print(f"teacher_forced: logits error {d_lg:.3e}, loss {float(t.loss):.7g} against {want['loss']:.7g}")
    assert d_lg < 1e-3
    assert torch.equal(t.pred_tokens.cpu(), lg64.argmax(-1))            # the trained model's leads are far above 1e-3
    assert abs(float(t.loss) - want["loss"]) <= 1e-4
    assert same_float(float(t.token_acc), want["token_acc"]) and same_float(float(t.seq_acc), want["seq_acc"])
    assert torch.equal(t.logits, gelu(src.cuda(), tgt[:, :-1].contiguous().cuda()))
    # score_hypotheses: the ten targets as N = 1 hypotheses; tests/test_gpu_score.py's bar for a log-probability of a tiny model
    hyp = tgt[:, None, :]
    r = gelu.score_hypotheses(src.cuda(), hyp.cuda(), eos_token_idx=EOS, return_token_logp=True)
    ref = reference_scores(lg64[:, None], hyp, PAD, EOS)
    assert torch.equal(r.length.cpu().long(), ref["length"]) and torch.equal(r.finished.cpu().bool(), ref["finished"])
    tok_err = (r.token_logp.cpu().double() - ref["tok_logp"]).abs().max().item()
    print(f"score_hypotheses: largest token log-probability error {tok_err:.3e}")
    assert tok_err <= 2e-4
    assert ((r.score.cpu().double() - ref["score"]).abs() <= ref["length"].double() * 2e-4).all()


@pytest.mark.parametrize("generation", ["greedy_speculative", "beam_search_speculative"])
def test_lightning_module_with_gelu(tta, generation):
    from test_gpu_lightning_surface import FixtureTokenizer
    st, cfg = gelu_state()
    tkz = FixtureTokenizer()
    kw = dict(src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
              num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
              share_embeddings=True, generation=generation, beam_size=5, max_len=150, n_drafts=3, draft_len=10,
              smart_drafts_mode=False, report_prediction_time=False)
    mod = tta.VanillaEncoderDecoderTransformerLightning(activation="gelu", **kw)
    missing, unexpected = mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    assert not missing and not unexpected
    src, tgt, _, _ = fixture_tokens()
    if "beam" in generation:                 # case 1 of the fixtures: n_best 5, 3 drafts of 10, batches of 4
        gold = gelu_gen("spec_beam")
        rows = gold["smart0_case1_rows"].tolist()
        assert gold["smart0_case1_params"].tolist() == [4, 5, 3, 10]
        sel = [src[rows[i:i + 4]] for i in range(0, len(rows), 4)]
        batches = [{"src_tokens": s[:, :int((s != PAD).sum(1).max())].cuda()} for s in sel]
        want = [gold[f"smart0_case1_batch{bi}"] for bi in range(len(batches))]
    else:
        batches = [{"src_tokens": src.cuda()}]
        want = [gelu_gen("spec_greedy")["b10_n3_d10_tokens"]]
    # predict_step on its own, then the whole predict loop with its look-ahead (_PredictAhead)
    with torch.inference_mode():
        first = mod.predict_step(batches[0], 0)
    assert mod.native.activation == "gelu"
    same_tokens(first.cpu().numpy(), want[0], "predict_step")
    outs = tta.run_predict(mod, batches)
    for o, w in zip(outs, want):
        same_tokens(o.cpu().numpy(), w, "run_predict")


def test_a_relu_model_built_afterwards_returns_the_relu_goldens(tta, gelu):
    """No state leaks between models: the tiny ReLU model against tests/golden/tiny_model_io.npz, in the process that ran GELU."""
    st, cfg = tiny_state()
    relu = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    io = load_npz("tiny_model_io.npz")
    src = torch.from_numpy(io["src"]).cuda()
    mask = src == 0
    mem = relu.encode_src(src, mask)
    ref_mem = torch.from_numpy(io["memory"]).cuda()
    assert (mem - ref_mem)[~mask].abs().max().item() < MEMORY_TOL
    for tgt_key, out_key in (("tgt_in", "logits"), ("tgt_ragged", "logits_ragged")):
        lg = relu.decode_tgt(torch.from_numpy(io[tgt_key]).cuda(), ref_mem, memory_pad_mask=mask)
        ref = torch.from_numpy(io[out_key]).cuda()
        assert (lg - ref).abs().max().item() < LOGIT_TOL and torch.equal(lg.argmax(-1), ref.argmax(-1))
    d_mem, errs, _ = _logit_errors(gelu)                 # and the GELU model is still the GELU model
    assert d_mem < MEMORY_TOL and max(errs) < LOGIT_TOL
    relu.close()
