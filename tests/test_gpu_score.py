"""Log-likelihood scores of hypotheses on the MI355X (ttx_hypothesis_logprobs / ttx_score_hypotheses,
NativeTransformer.hypothesis_logprobs / score_hypotheses, the generators' score / return_scores, predict_with_scores) against a
float64 restatement of the definition (tests/util_score.py), the reference's own values (tests/golden/hyp_scores.npz, made by
tests/golden/make_golden_scores.py) and the oracle at full model size."""
import json

import pytest
import torch

from util_models import GOLDEN, PAD, BOS, EOS, fixture_tokens, tiny_state
from util_score import golden_cases, length_rule, reference_scores

pytestmark = pytest.mark.gpu

TOK_TOL = 1e-5          # per-token, relative to max(1, max|ref|): the bound test_gpu_eval.py holds token_nll to


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def tiny(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)


@pytest.fixture(scope="module")
def full_pair(tta, trained_full_state):
    from oracle.model import OracleTransformer, config_from_state
    st = trained_full_state(4)
    return tta.NativeTransformer(st, 8, 0, device=0), OracleTransformer(config_from_state(st, 8), st)


def _check_against(r, ref: dict, tok_tol: float, label: str) -> tuple:
    """length / finished exact, token_logp within tok_tol, exactly 0 past the length, score within length * tok_tol.
    Returns the observed maxima (token, score / max(1, length))."""
    length = ref["length"]
    assert r.length.dtype == torch.int32 and r.finished.dtype == torch.bool and r.score.dtype == torch.float32
    assert torch.equal(r.length.cpu().long(), length), label
    assert torch.equal(r.finished.cpu(), ref["finished"]), label
    tok = r.token_logp.cpu().double()
    assert tok.shape == ref["tok_logp"].shape, label
    past = torch.arange(tok.shape[-1]).expand_as(tok) >= length.unsqueeze(-1)
    assert (tok[past] == 0).all(), label
    assert torch.isfinite(tok).all() and torch.isfinite(r.score).all(), label
    tok_err = (tok - ref["tok_logp"]).abs().max().item()
    sc_err = (r.score.cpu().double() - ref["score"]).abs()
    print(f"{label}: max |token_logp - ref| {tok_err:.3g} (bound {tok_tol:.3g}), max |score - ref| {sc_err.max().item():.3g}, "
          f"max per scored token {(sc_err / length.clamp(min=1)).max().item():.3g}")
    assert tok_err <= tok_tol, label
    assert (sc_err <= length.double() * tok_tol).all(), label
    return tok_err, sc_err.max().item()


# -- 1. the stage alone ------------------------------------------------------------------------------------------------
def _rule_rows(V: int, W: int, gen: torch.Generator) -> torch.Tensor:
    """Hypothesis rows covering every case of the length rule, chunk boundaries of the 64-lane scan included."""
    def body(n):
        return torch.randint(3, V, (n,), generator=gen)

    rows = []

    def row(fill):                       # fill: list of (column, tensor or int)
        h = torch.full((W,), PAD, dtype=torch.int64)
        h[0] = BOS
        for c, v in fill:
            if isinstance(v, int):
                h[c] = v
            else:
                h[c:c + len(v)] = v
        rows.append(h)

    row([(1, EOS), (2, body(5))])                                     # EOS at column 1, tokens after it ignored
    for c in (64, 65, 128, 129, W - 1):                               # EOS at the scan's chunk boundaries and in the last column
        row([(1, body(c - 1)), (c, EOS)])
    row([(1, body(70))])                                              # no EOS, trailing PAD
    row([(1, body(W - 1))])                                           # no EOS, the row is full
    rows.append(torch.full((W,), PAD, dtype=torch.int64))             # all-PAD
    row([(1, body(9)), (4, PAD), (5, PAD), (10, EOS)])                # PADs before the EOS are targets
    row([(1, body(20)), (21, EOS), (22, body(8)), (30, EOS)])         # two EOS: the first counts
    row([(1, body(3)), (90, body(4))])                                # no EOS, PAD gap: the LAST non-PAD column counts
    row([(1, body(40)), (41, EOS)])                                   # its targets get the maximum logit (below)
    row([(1, body(100)), (101, EOS)])                                 # its logits get a 30-unit spread (below)
    return torch.stack(rows)


def _synthetic(V: int):
    gen = torch.Generator().manual_seed(1000 + V)
    W = 140
    hyp = _rule_rows(V, W, gen)
    R = hyp.shape[0]
    logits = torch.randn((R, W - 1, V), generator=gen) * 3.0
    r_max, r_spread = R - 2, R - 1
    peak = logits[r_max].amax(-1) + 5.0
    logits[r_max].scatter_(-1, hyp[r_max, 1:].unsqueeze(-1), peak.unsqueeze(-1))
    logits[r_spread] = torch.rand((W - 1, V), generator=gen) * 30.0 - 15.0
    logits[r_spread, :, 0], logits[r_spread, :, 1] = -15.0, 15.0
    return logits, hyp, r_max


@pytest.mark.parametrize("V", [12, 13, 64, 300, 1024])
def test_stage_alone_on_synthetic_logits(tiny, V):
    logits, hyp, r_max = _synthetic(V)
    ref = reference_scores(logits, hyp, PAD, EOS)
    assert sorted(set(ref["length"].tolist())) == sorted({1, 64, 65, 128, 129, 139, 70, 0, 10, 21, 93, 41, 101})
    x = logits.cuda()
    assert x.data_ptr() % 16 == 0
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")
    buf[1:] = x.reshape(-1)
    shifted = buf[1:].view(x.shape)
    assert shifted.data_ptr() % 16 != 0
    tol = TOK_TOL * max(1.0, ref["tok_logp"].abs().max().item())
    a = tiny.hypothesis_logprobs(x, hyp.cuda(), PAD, EOS)
    b = tiny.hypothesis_logprobs(shifted, hyp.cuda(), PAD, EOS)
    _check_against(a, ref, tol, f"V={V} aligned")
    _check_against(b, ref, tol, f"V={V} shifted")
    # the two load paths see the columns in another grouping: the sums may differ in the last bits
    assert torch.equal(a.length, b.length) and torch.equal(a.finished, b.finished)
    assert torch.allclose(a.token_logp, b.token_logp, rtol=1e-6, atol=1e-7)
    # every term is <= 0, so the per-token rule adds up to rtol * |score| + length * atol
    assert ((a.score - b.score).abs() <= 1e-6 * a.score.abs() + a.length * 1e-7 + 1e-12).all()
    # a target that is the maximum by 5 units: logp = -log1p(r) with r <= (V - 1) e^-5, resolved relative to itself
    want = ref["tok_logp"][r_max, :41]
    got = a.token_logp[r_max, :41].cpu().double()
    assert (want > -(V - 1) * 0.0068).all() and ((got - want).abs() <= 1e-5 * want.abs() + 1e-12).all()


# -- 2. against the reference (tiny weights) ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["beam", "targets", "rule"])
def test_scores_match_reference_fixture(tiny, name):
    """A logp is a logit minus a log-sum of logits, and test_gpu_model.py holds the tiny model's logits to 1e-4: 2e-4 per token."""
    c = golden_cases()[name]
    r = tiny.score_hypotheses(c["src"].cuda(), c["hyp"].cuda(), eos_token_idx=EOS, return_token_logp=True)
    assert r.score.shape == c["score"].shape and r.token_logp.shape == c["tok_logp"].shape
    _check_against(r, c | {"length": c["length"].long()}, 2e-4, f"tiny/{name}")
    r2 = tiny.score_hypotheses(c["src"].cuda(), c["hyp"].cuda(), eos_token_idx=EOS)
    assert r2.token_logp is None and torch.equal(r2.score, r.score) and torch.equal(r2.length, r.length)


# -- 3. against the oracle at full size --------------------------------------------------------------------------------
def test_scores_match_oracle_at_full_size(tta, full_pair):
    """Hypotheses = what the native speculative generators return for the fixture sources; expected values from the oracle's
    logits in float64.  Per token 2e-3: twice the 1e-3 test_gpu_eval.py holds the full-size logits to."""
    native, oracle = full_pair
    src, _, c, V = fixture_tokens()
    gens = {"greedy_speculative": tta.TranslationInferenceGreedySpeculative(native, 200, 10, 3, PAD, BOS, EOS, c),
            "beam_speculative": tta.TranslationInferenceBeamSearchSpeculative(native, 200, 5, 10, 3, V, False, PAD, BOS, EOS, c,
                                                                              max_steps=400)}
    for label, g in gens.items():
        pred = g.generate(src.cuda())
        calls = g.model_calls_num
        r = g.score(src.cuda(), pred, return_token_logp=True)
        assert g.model_calls_num == calls                      # scoring is no model call of the reference's loop
        hyp = pred.cpu()
        B, N, W = hyp.shape
        ext = int(length_rule(hyp, PAD, EOS)[0].max()) + 1     # the oracle (CPU) need not pay for the PAD columns either
        with torch.inference_mode():
            logits = oracle(src.repeat_interleave(N, 0), hyp.reshape(B * N, W)[:, :ext - 1]).float()
        ref = reference_scores(logits.reshape(B, N, ext - 1, -1), hyp[:, :, :ext], PAD, EOS)
        assert (r.token_logp[:, :, ext - 1:] == 0).all()
        got = tta.HypothesisScores(r.score, r.length, r.finished, r.token_logp[:, :, :ext - 1])
        _check_against(got, ref, 2e-3, f"full 4+4 {label} [{B},{N},{W}]")
        print(f"{label}: {int(ref['finished'].sum())} of {B * N} hypotheses finished, longest {ext - 1} tokens")


# -- 4. it is the forward pass -----------------------------------------------------------------------------------------
def test_logits_are_decode_tgt_and_scores_are_the_stage(tiny):
    c = golden_cases()["beam"]
    src, hyp = c["src"].cuda(), c["hyp"].cuda()
    B, N, W = hyp.shape
    V = tiny.tgt_vocab_size
    logits = torch.full((B * N, W - 1, V), float("nan"), device="cuda")
    r = tiny.score_hypotheses(src, hyp, eos_token_idx=EOS, return_token_logp=True, trim=False, logits_out=logits)
    rows = torch.arange(B * N, device="cuda", dtype=torch.int32) // N
    fwd = tiny.decode_tgt(hyp.reshape(B * N, W)[:, :-1].contiguous(), tiny.encode_src(src), src == PAD, memory_row=rows)
    assert torch.isfinite(fwd).all()
    assert torch.equal(logits, fwd)
    s = tiny.hypothesis_logprobs(logits, hyp.reshape(B * N, W), PAD, EOS)
    assert torch.equal(s.score, r.score.reshape(-1)) and torch.equal(s.token_logp, r.token_logp.reshape(B * N, W - 1))
    assert torch.equal(s.length, r.length.reshape(-1)) and torch.equal(s.finished, r.finished.reshape(-1))


# -- 5. independence of batching, chunking, trimming and PAD columns ---------------------------------------------------
def _check_independence(native, src, hyp, label):
    """One call against: source by source, chunks through max_rows, trim on / off, 7 more PAD columns.  length / finished equal;
    scores and per-token values bit-identical (measured so on the tiny and the full-size model: the GEMM family adds in one
    canonical order whatever the row count, and a row of the full-prefix attention reads its own keys in the same order whatever
    the width) — which is stronger than the stage's own tolerance."""
    B, N, W = hyp.shape
    kw = dict(eos_token_idx=EOS, return_token_logp=True)
    base = native.score_hypotheses(src, hyp, **kw)
    wide = torch.cat([hyp, torch.full((B, N, 7), PAD, dtype=torch.int64, device="cuda")], dim=2)
    one_by_one = [native.score_hypotheses(src[b:b + 1], hyp[b:b + 1], **kw) for b in range(B)]
    variants = {
        "source by source": tuple(torch.cat([getattr(r, f) for r in one_by_one]) for f in ("score", "length", "finished", "token_logp")),
        "chunks of 3 sources": native.score_hypotheses(src, hyp, max_rows=3 * N * (W - 1), trim=False, **kw),
        "chunks of 1 source": native.score_hypotheses(src, hyp, max_rows=1, **kw),
        "trim off": native.score_hypotheses(src, hyp, trim=False, **kw),
        "7 PAD columns, trim on": native.score_hypotheses(src, wide, **kw),
        "7 PAD columns, trim off": native.score_hypotheses(src, wide, trim=False, **kw),
    }
    tol = TOK_TOL * max(1.0, base.token_logp.abs().max().item())
    for name, (score, length, fin, tok) in variants.items():
        assert torch.equal(length, base.length) and torch.equal(fin, base.finished), (label, name)
        d_tok = (tok[:, :, :W - 1] - base.token_logp).abs().max().item()
        d_sc = (score - base.score).abs()
        print(f"{label} / {name}: max token diff {d_tok:.3g}, max score diff {d_sc.max().item():.3g}")
        assert d_tok <= tol and (d_sc <= base.length * tol).all(), (label, name)        # the bound of the stage itself
        assert torch.equal(tok[:, :, :W - 1], base.token_logp) and torch.equal(score, base.score), (label, name)
    assert (variants["7 PAD columns, trim off"][3][:, :, W - 1:] == 0).all()


@pytest.mark.parametrize("name", ["beam", "rule"])
def test_scores_do_not_depend_on_how_the_rows_are_batched(tiny, name):
    c = golden_cases()[name]
    _check_independence(tiny, c["src"].cuda(), c["hyp"].cuda(), f"tiny/{name}")


def test_scores_do_not_depend_on_how_the_rows_are_batched_at_full_size(tta, full_pair):
    native, _ = full_pair
    src, _, c, V = fixture_tokens()
    g = tta.TranslationInferenceBeamSearchSpeculative(native, 200, 5, 10, 3, V, False, PAD, BOS, EOS, c, max_steps=400)
    _check_independence(native, src.cuda(), g.generate(src.cuda()), "full 4+4 beam_speculative")


# -- 6. determinism ----------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical(tiny):
    c = golden_cases()["beam"]
    src, hyp = c["src"].cuda(), c["hyp"].cuda()
    a = tiny.score_hypotheses(src, hyp, eos_token_idx=EOS, return_token_logp=True)
    tiny.score_hypotheses(src[:3], hyp[:3, :2], eos_token_idx=EOS)          # another shape in between
    b = tiny.score_hypotheses(src, hyp, eos_token_idx=EOS, return_token_logp=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# -- 7. ordering -------------------------------------------------------------------------------------------------------
def test_beam_search_scores_are_ordered(tta, tiny):
    """Standard beam search returns its hypotheses best first by the same cumulative log-probability: the native scores are
    non-increasing along the hypothesis axis up to 1e-3.  A source is left out only if the reference's own smallest gap
    (recorded in the fixture) is below 2e-3, and at most 2 of the 10 may be."""
    c = golden_cases()["beam"]
    src = c["src"].cuda()
    g = tta.TranslationInferenceBeamSearch(tiny, 5, 150, PAD, BOS, EOS)
    pred, sc = g.generate(src, return_scores=True)
    assert pred.shape[:2] == (10, 5) and sc.score.shape == (10, 5)
    keep = c["min_gap"] >= 2e-3
    assert int((~keep).sum()) <= 2
    score = sc.score.cpu()
    step = score[:, 1:] - score[:, :-1]
    print("sources left out:", (~keep).nonzero().flatten().tolist(), " largest increase along the axis:", step[keep].max().item())
    assert (step[keep] <= 1e-3).all()
    assert sc.finished.all()


# -- 8. generators and Lightning ---------------------------------------------------------------------------------------
def _generators(tta, native):
    _, _, c, V = fixture_tokens()
    return {
        "greedy": lambda: tta.TranslationInferenceGreedy(native, 150, PAD, BOS, EOS),
        "beam_search": lambda: tta.TranslationInferenceBeamSearch(native, 3, 150, PAD, BOS, EOS),
        "greedy_speculative": lambda: tta.TranslationInferenceGreedySpeculative(native, 150, 10, 3, PAD, BOS, EOS, c),
        "beam_search_speculative": lambda: tta.TranslationInferenceBeamSearchSpeculative(native, 150, 3, 10, 3, V, False, PAD, BOS,
                                                                                         EOS, c, max_steps=400),
    }


def _same_scores(a, b) -> bool:
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["greedy", "beam_search", "greedy_speculative", "beam_search_speculative"])
def test_generate_with_scores(tta, tiny, kind):
    make = _generators(tta, tiny)[kind]
    src = fixture_tokens()[0].cuda()
    plain = make()
    ref = plain.generate(src)
    g = make()
    pred, sc = g.generate(src, return_scores=True)
    assert torch.equal(pred, ref)
    assert g.model_calls_num == plain.model_calls_num            # scoring does not touch the counters
    assert isinstance(sc, tta.HypothesisScores) and sc.score.shape == pred.shape[:2] and sc.token_logp is None
    assert _same_scores(sc, g.score(src, pred))
    assert (sc.score <= 0).all() and (sc.length > 0).all()
    if hasattr(g, "generate_many"):
        batches = [src[0:3], src[3:4], src[4:10]]
        batches = [b[:, :int((b != PAD).sum(1).max())].contiguous() for b in batches]
        one = make()
        per_batch = [one.generate(b, return_scores=True) for b in batches]
        many = make()
        pairs = many.generate_many(batches, in_flight=2, return_scores=True)
        assert many.model_calls_num == one.model_calls_num
        assert len(pairs) == len(batches)
        for (p, s), (q, t) in zip(pairs, per_batch):
            assert torch.equal(p, q) and _same_scores(s, t)
        assert all(torch.equal(p, q) for (p, _), q in zip(pairs, make().generate_many(batches, in_flight=2)))


class FixtureTokenizer:
    """Shape of the reference's GenericTokenizer that the module uses (tokenizer_base.py:16-94)."""
    pad_token_idx, bos_token_idx, eos_token_idx, unk_token_idx = 0, 1, 2, 3

    def __init__(self):
        self.decoder_dict = {int(k): v for k, v in json.loads((GOLDEN / "fixture_vocab.json").read_text()).items()}
        self.encoder_dict = {v: k for k, v in self.decoder_dict.items()}

    @property
    def n_tokens(self):
        return len(self.encoder_dict)


def _module(tta, generation, report_file, **kw):
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    mod = tta.VanillaEncoderDecoderTransformerLightning(
        src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
        num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"],
        num_heads=cfg["num_heads"], share_embeddings=True, generation=generation, max_len=150, n_drafts=3,
        draft_len=10, report_prediction_file=str(report_file), **kw)
    mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    return mod


@pytest.mark.parametrize("generation", ["greedy_speculative", "beam_search_speculative", "beam_search"])
def test_predict_with_scores(tta, tmp_path, generation, monkeypatch):
    monkeypatch.delenv("TTX_PREDICT_SCORES", raising=False)
    src, tgt, _, _ = fixture_tokens()
    batches = []
    for i, j in ((0, 3), (3, 4), (4, 8), (8, 10)):
        s_ = src[i:j]
        batches.append({"src_tokens": s_[:, :int((s_ != PAD).sum(1).max())].cuda(), "tgt_tokens": tgt[i:j].cuda()})
    kw = dict(beam_size=3, smart_drafts_mode=False) if generation != "greedy_speculative" else {}
    today = {"algorithm", "batch_size", "tgt_test_path", "max_len", "total_seconds", "model_calls", "seconds_per_model_call"}
    if "speculative" in generation:
        today |= {"n_drafts", "draft_len"}
    if generation == "beam_search_speculative":
        today |= {"accepted_tokens", "acceptance_rate"}
    res = {}
    for schedule in ("rows", "batches"):
        for on in (False, True):
            rf = tmp_path / f"r_{schedule}_{on}.txt"
            mod = _module(tta, generation, rf, **kw)
            mod.predict_with_scores = on
            outs = tta.run_predict(mod, batches, schedule=schedule, window=3, in_flight=2)
            rep = json.loads(rf.read_text().strip().split("\n")[-1])
            res[schedule, on] = (outs, rep, mod)
            if not on:
                assert set(rep) == today and mod.predict_scores == {}
        (off_outs, off_rep, _), (on_outs, on_rep, mod) = res[schedule, False], res[schedule, True]
        assert all(torch.equal(a, b) for a, b in zip(off_outs, on_outs))
        assert on_rep["model_calls"] == off_rep["model_calls"]
        assert set(on_rep) == today | {"scoring_seconds", "mean_top1_logprob", "unfinished_hypotheses"}
        assert sorted(mod.predict_scores) == list(range(len(batches)))
        for i, (b, p) in enumerate(zip(batches, on_outs)):
            sc = mod.predict_scores[i]
            assert sc.score.shape == p.shape[:2] and sc.length.shape == p.shape[:2] and sc.finished.shape == p.shape[:2]
            assert _same_scores(sc, mod.generator.score(b["src_tokens"], p))
        top1 = torch.cat([mod.predict_scores[i].score[:, 0] for i in range(len(batches))]).double().mean().item()
        assert on_rep["mean_top1_logprob"] == pytest.approx(top1, abs=1e-6)
        assert on_rep["unfinished_hypotheses"] == sum(int((~mod.predict_scores[i].finished).sum()) for i in range(len(batches)))
        assert on_rep["scoring_seconds"] > 0
        if schedule == "rows" and generation != "beam_search":
            assert mod._ahead is not None and mod._ahead.served == len(batches)
    # the environment switch does what the attribute does
    monkeypatch.setenv("TTX_PREDICT_SCORES", "1")
    mod = _module(tta, generation, tmp_path / "r_env.txt", **kw)
    outs = tta.run_predict(mod, batches, schedule="batches")
    assert sorted(mod.predict_scores) == list(range(len(batches)))
    assert all(_same_scores(mod.predict_scores[i], res["batches", True][2].predict_scores[i]) for i in range(len(batches)))


# -- 9. bad input ------------------------------------------------------------------------------------------------------
def test_rejects_bad_inputs(tta, tiny):
    N = tta._native
    c = golden_cases()["beam"]
    src, hyp = c["src"].cuda(), c["hyp"].cuda()
    V = tiny.tgt_vocab_size
    with pytest.raises(ValueError):
        tiny.score_hypotheses(src, hyp[:, :, :1])                                   # W = 1
    with pytest.raises(ValueError):
        tiny.score_hypotheses(src[:4], hyp)                                         # batch mismatch
    with pytest.raises(ValueError):
        tiny.score_hypotheses(src, hyp[:, 0])                                       # not [B, N, W]
    bad = hyp.clone()
    bad[2, 1, 5] = V
    with pytest.raises(IndexError):
        tiny.score_hypotheses(src, bad)
    with pytest.raises(IndexError):
        tiny.hypothesis_logprobs(torch.zeros((10, 5, hyp.shape[2] - 1, V), device="cuda"), bad, PAD, EOS)
    with pytest.raises(ValueError):
        tiny.hypothesis_logprobs(torch.zeros((10, 5, hyp.shape[2], V), device="cuda"), hyp, PAD, EOS)
    with pytest.raises(ValueError):
        tiny.score_hypotheses(src, hyp, trim=False, logits_out=torch.zeros((49, hyp.shape[2] - 1, V), device="cuda"))
    with pytest.raises(ValueError):                                                 # one chunk only
        tiny.score_hypotheses(src, hyp, trim=False, max_rows=1, logits_out=torch.zeros((50, hyp.shape[2] - 1, V), device="cuda"))
    # the C boundary refuses before any launch: the outputs keep their poison
    B, K, W = hyp.shape
    lib, sess, stream = tiny._lib, tiny._scoring_session(), tiny._stream()
    score = torch.full((B * K,), 7.0, device="cuda")
    length = torch.full((B * K,), 7, dtype=torch.int32, device="cuda")
    s, h = src.data_ptr(), hyp.data_ptr()

    def sh(B_=B, Ls=src.shape[1], ld=W, N_=K, W_=W):
        return lib.ttx_score_hypotheses(sess, s, B_, Ls, h, ld, N_, W_, EOS, None, None, score.data_ptr(), length.data_ptr(), None, stream)

    assert sh(W_=1) == N.TTX_ERR_INVALID
    assert sh(ld=W - 1) == N.TTX_ERR_INVALID and b"ld_hyp" in lib.ttx_last_error()
    assert sh(W_=5002, ld=5002) == N.TTX_ERR_INVALID
    assert sh(Ls=5001) == N.TTX_ERR_INVALID
    assert sh(B_=0) == N.TTX_ERR_INVALID and sh(N_=0) == N.TTX_ERR_INVALID
    assert sh(B_=1 << 12, N_=1 << 6, W_=65, ld=65) == N.TTX_ERR_INVALID           # 2^24 positions
    big = torch.zeros((2, 3, 1025), device="cuda")
    assert lib.ttx_hypothesis_logprobs(sess, big.data_ptr(), h, 2, 4, 1025, PAD, EOS, None, score.data_ptr(), length.data_ptr(),
                                       None, stream) == N.TTX_ERR_INVALID
    assert lib.ttx_hypothesis_logprobs(sess, big.data_ptr(), h, 2, 1, 30, PAD, EOS, None, score.data_ptr(), length.data_ptr(),
                                       None, stream) == N.TTX_ERR_INVALID
    assert lib.ttx_hypothesis_logprobs(sess, big.data_ptr(), h, 2, 4, 30, PAD, EOS, None, None, length.data_ptr(),
                                       None, stream) == N.TTX_ERR_INVALID
    torch.cuda.synchronize()
    assert (score == 7.0).all() and (length == 7).all()
    # the session is still usable
    r = tiny.score_hypotheses(src, hyp)
    assert torch.equal(r.length.cpu().long(), c["length"].long())
