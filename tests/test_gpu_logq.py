"""NativeTransformer.proposal_scores / the generators' logq (ttx_score_proposal) end to end on the ten fixture sources, with the
tiny golden model and the four-head model of tests/golden/h4_*: invariance under batching, the single pass with scores, sampled
rows against the float64 oracle, stochastic beam search's own logp as an independent witness, the pooled and Lightning paths,
and refused arguments.

Tolerances.  Support: a sampled token must lie in one of the admissible kept sets of the oracle's logits with the nucleus boundary
moved by tol = 2 LOGIT_TOL / T + 1e-4, the replay tolerance of tests/test_gpu_sampling.py.  Values: where the kernel's kept set
is the oracle's nominal one, token_logq agrees with the oracle's value within TOK_TOL * max(1, max |ref|) * max(1, 1 / T):
the bound tests/test_gpu_score.py holds token_logp to, and the temperature scales the logit error.  Stochastic beam search:
|logq - logp| within that per-token bound times the scored tokens, for every finite row; a row that ended on a sampled PAD is
compared with its PAD draw included (see the test), since the search's logp holds that draw and the length rule leaves it out.
Measured on an MI355X: 8 557 sampled tokens, none outside its admissible kept sets, none with a kept-set size other than the
oracle's, largest |token_logq - ref| 9.3e-6 (bound 6.9e-5); 200 beam rows, 27 PAD-ended, largest |logq - logp| 9.5e-6.
"""
import json

import numpy as np
import pytest
import torch

import util_logq_checks as Q
import util_sample_checks as S
from test_gpu_model import LOGIT_TOL
from test_gpu_score import TOK_TOL
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
SEED = 20260103
MAX_LEN = 32
FIELDS = ("logq", "length", "finished", "first_outside", "token_logq", "rank", "n_kept")


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


def states(name):
    if name == "tiny":
        return tiny_state()
    from util_draft_select import h4_state
    return h4_state()


@pytest.fixture(scope="module")
def models(tta):
    """name -> (NativeTransformer, float64 oracle), built once."""
    from oracle.model import OracleTransformer, config_from_state
    out = {}
    for name in ("tiny", "h4"):
        st, cfg = states(name)
        out[name] = (tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0),
                     OracleTransformer(config_from_state(st, cfg["num_heads"]), st, dtype=torch.float64))
    return out


@pytest.fixture(scope="module")
def src():
    s = fixture_tokens()[0]
    return s[:, :int((s != PAD).sum(1).max())]


@pytest.fixture(scope="module")
def samples(tta, models, src):
    """(name, T, filtered) -> sampled rows Long[10, 4, MAX_LEN] on the device, drawn once."""
    out = {}
    for name in ("tiny", "h4"):
        for T in (0.5, 2.0):
            for f in (dict(), dict(top_k=8, top_p=0.9)):
                g = tta.TranslationInferenceSampling(models[name][0], MAX_LEN, PAD, BOS, EOS, temperature=T, num_samples=4, seed=SEED, **f)
                out[name, T, bool(f)] = (g, g.generate(src.cuda()))
    return out


def same(a, b, fields=FIELDS) -> bool:
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        if (x is None) != (y is None):
            return False
        if x is not None and not torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y):
            return False
    return True


# -- invariance --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
@pytest.mark.parametrize("dist", [dict(temperature=0.5), dict(temperature=2.0, top_k=8, top_p=0.9), dict(temperature=0.0)], ids=str)
def test_does_not_depend_on_how_the_rows_are_batched(models, samples, src, name, dist):
    native = models[name][0]
    s, hyp = src.cuda(), samples[name, 2.0, True][1]
    B, N, W = hyp.shape
    kw = dict(return_token_logq=True, return_rank=True, eos_token_idx=EOS, **dist)
    base = native.proposal_scores(s, hyp, **kw)
    assert base.logq.shape == (B, N) and base.token_logq.shape == (B, N, W - 1) and base.scores is None
    assert base.logq.dtype == torch.float32 and base.first_outside.dtype == torch.int32 and base.rank.dtype == torch.int32
    one = [native.proposal_scores(s[b:b + 1], hyp[b:b + 1], **kw) for b in range(B)]
    wide = torch.cat([hyp, torch.full((B, N, 7), PAD, dtype=torch.int64, device="cuda")], dim=2)
    variants = {
        "source by source": type(base)(*(torch.cat([getattr(r, f) for r in one]) for f in FIELDS), None),
        "chunks of 3 sources": native.proposal_scores(s, hyp, max_rows=3 * N * (W - 1), trim=False, **kw),
        "chunks of 1 source": native.proposal_scores(s, hyp, max_rows=1, **kw),
        "trim off": native.proposal_scores(s, hyp, trim=False, **kw),
    }
    for label, r in variants.items():
        assert same(base, r), (name, dist, label)
    w = native.proposal_scores(s, wide, **kw)
    assert same(base, w, FIELDS[:4]) and torch.equal(w.token_logq[:, :, :W - 1], base.token_logq)
    assert (w.token_logq[:, :, W - 1:] == 0).all() and (w.rank[:, :, W - 1:] == -1).all() and (w.n_kept[:, :, W - 1:] == 0).all()
    again = native.proposal_scores(s, hyp, **kw)
    assert same(base, again)
    # the row sums and the marker follow from the per-token values
    tok = base.token_logq.cpu().numpy()
    for b in range(B):
        for j in range(N):
            n = int(base.length[b, j])
            neg = np.nonzero(tok[b, j, :n] == -np.inf)[0]
            assert int(base.first_outside[b, j]) == (int(neg[0]) if len(neg) else -1)
            assert (base.logq[b, j].item() == -np.inf) == bool(len(neg))


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_single_pass_with_scores(models, samples, src, name):
    native = models[name][0]
    s, hyp = src.cuda(), samples[name, 0.5, False][1]
    sc = native.score_hypotheses(s, hyp, eos_token_idx=EOS, return_token_logp=True)
    for dist in (dict(temperature=0.5), dict(temperature=2.0, top_k=8, top_p=0.9), dict()):
        q = native.proposal_scores(s, hyp, with_scores=True, return_token_logq=True, eos_token_idx=EOS, **dist)
        alone = native.proposal_scores(s, hyp, return_token_logq=True, eos_token_idx=EOS, **dist)
        assert all(torch.equal(a, b) for a, b in zip(q.scores, sc)), (name, dist)
        assert same(q, alone, FIELDS[:5])
        assert torch.equal(q.length, sc.length) and torch.equal(q.finished, sc.finished)
        if not dist:                      # q is the model's distribution: score_hypotheses' outputs on the bits
            assert torch.equal(q.logq, sc.score) and torch.equal(q.token_logq, sc.token_logp)
            assert (q.first_outside == -1).all()
    chunked = native.proposal_scores(s, hyp, with_scores=True, max_rows=1, eos_token_idx=EOS)
    assert torch.equal(chunked.logq, sc.score) and torch.equal(chunked.scores.score, sc.score)


def test_first_outside_under_the_model_distribution(tta, src):
    """T = 1 without a filter runs k_hyp_score for the values and k_logq_first_outside for the marker.  A model whose classifier
    bias is -inf at one token puts that token outside the support; V = 32, the token away from the lane-head columns, so that
    k_hyp_score gives numbers.  The stage alone (k_hyp_logq) on the same logits must say the same, on the bits."""
    from util_models import seeded_weights, state_shapes
    V, OUT = 32, 7
    w = seeded_weights(state_shapes(V, 64, 64, 1, 1), 9)
    w["tgt_token_featurizer.embedding.weight"] = w["src_token_featurizer.embedding.weight"]
    w["next_token_classifier.bias"][OUT] = -np.inf
    native = tta.NativeTransformer(w, 2, PAD, device=0)
    s = src[:3].cuda()
    gen = torch.Generator().manual_seed(5)
    W = 70                                                                    # more than one 64-position ballot
    hyp = torch.randint(8, V, (3, 2, W), generator=gen)
    hyp[:, :, 0] = BOS
    hyp[:, :, W - 1] = EOS
    hyp[0, 1, 4] = OUT
    hyp[2, 0, 67], hyp[2, 0, 68] = OUT, OUT
    hyp[1, 1, 30:] = PAD
    hyp[1, 1, 30] = EOS
    hyp[1, 1, 40] = OUT                                                       # behind the EOS: not scored
    hyp = hyp.cuda()
    want = torch.tensor([[-1, 3], [-1, -1], [66, -1]], dtype=torch.int32, device="cuda")
    sc = native.score_hypotheses(s, hyp, eos_token_idx=EOS, return_token_logp=True)
    assert not torch.isnan(sc.token_logp).any()
    for with_scores in (False, True):
        q = native.proposal_scores(s, hyp, with_scores=with_scores, return_token_logq=True, return_rank=True, eos_token_idx=EOS)
        assert torch.equal(q.first_outside, want)
        assert torch.equal(q.logq.view(torch.int32), sc.score.view(torch.int32)) and torch.equal(torch.isinf(q.logq), want >= 0)
        assert torch.equal(q.token_logq.view(torch.int32), sc.token_logp.view(torch.int32))
        assert (q.n_kept[q.rank >= 0] == V).all() and int(q.rank[0, 1, 3]) == V - 1
        if with_scores:
            assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                       for a, b in zip(q.scores, sc))
    lg = torch.empty((6, W - 1, V), dtype=torch.float32, device="cuda")
    native.score_hypotheses(s, hyp, eos_token_idx=EOS, trim=False, logits_out=lg)
    stage = native.hypothesis_logq(lg.view(3, 2, W - 1, V), hyp, PAD, EOS)
    assert same(stage, q)


# -- samples against the float64 oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("T", [0.5, 2.0])
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_samples_against_float64_oracle(models, samples, src, name, T, filtered):
    native, o64 = models[name]
    g, hyp = samples[name, T, filtered]
    q = g.logq(src.cuda(), hyp, return_token_logq=True, return_rank=True)
    B, N, W = hyp.shape
    rows = hyp.cpu().numpy().reshape(B * N, W)
    with torch.no_grad():
        lg = o64(src.repeat_interleave(N, 0), torch.from_numpy(rows[:, :-1])).numpy()
    p = S.Params(T, pad=PAD, eos=EOS, **(dict(top_k=8, top_p=0.9) if filtered else {}))
    tol = 2 * LOGIT_TOL / T + 1e-4
    tok = q.token_logq.cpu().numpy().reshape(B * N, W - 1).astype(np.float64)
    nk = q.n_kept.cpu().numpy().reshape(B * N, W - 1)
    length = q.length.cpu().numpy().reshape(-1)
    compared, worst, boundary, ref_max = 0, 0.0, 0, 0.0
    errs = []
    for r in range(B * N):
        for pos in range(length[r]):
            y = S.scaled(lg[r, pos], T)
            t = int(rows[r, pos + 1])
            sets = S.cdf_orders(y, p, tol)
            assert any(t in ids.tolist() for ids in sets), f"{name} T {T} row {r} position {pos}: token {t} is in no admissible kept set"
            nominal = len(sets[0]) if filtered else len(y)
            if nk[r, pos] != nominal:
                boundary += 1
                continue
            ref = Q.token_logq(lg[r, pos], t, p)[0]
            assert ref > -np.inf and tok[r, pos] > -np.inf, (name, T, r, pos)
            errs.append(abs(tok[r, pos] - ref))
            ref_max = max(ref_max, abs(ref))
            compared += 1
    bound = TOK_TOL * max(1.0, ref_max) * max(1.0, 1.0 / T)
    print(f"{name} T {T} filtered {filtered}: {compared} tokens compared, {boundary} on a nucleus boundary, max |token_logq - ref| "
          f"{max(errs):.3g} (bound {bound:.3g}); rows with logq = -inf: {int((q.logq == -np.inf).sum())} of {B * N}")
    assert compared > 100 and max(errs) <= bound
    if not filtered:
        assert (q.first_outside == -1).all() and torch.isfinite(q.logq).all()


# -- stochastic beam search as an independent witness --------------------------------------------------------------------------------
@pytest.mark.parametrize("prefixed", [False, True])
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_stochastic_beam_search_logp(tta, models, src, name, prefixed):
    native = models[name][0]
    s = src.cuda()
    g = tta.TranslationInferenceStochasticBeamSearch(native, 5, MAX_LEN, PAD, BOS, EOS, temperature=2.0, seed=SEED, top_k=8, top_p=0.9)
    prefix = None
    if prefixed:
        greedy = tta.TranslationInferenceGreedy(native, MAX_LEN, PAD, BOS, EOS).generate(s)[:, 0]
        prefix = greedy[:, 1:4].cpu()
        prefix = torch.where((prefix == EOS) | (prefix == PAD), torch.full_like(prefix, 5), prefix)
    rows, det = g.generate(s, return_details=True, prefix=prefix)
    q = g.logq(s, rows, prefix=prefix, return_token_logq=True)
    logp, lq = det.logp.cpu().double(), q.logq.cpu().double()
    tok = q.token_logq.cpu().double()
    scored = q.length.cpu().double()
    # A row that ended on a SAMPLED PAD: the search paid for that draw, the scoring length rule stops before a trailing PAD (the row
    # is not finished), so logq leaves the draw out by definition.  Such a row is compared all the same: the stage alone, told that
    # no token is PAD, evaluates the row cut behind its PAD on the same teacher-forced logits, and that value must equal logp.
    B, K, W = rows.shape
    n_pad = 0
    for b in range(B):
        for j in range(K):
            n = int(q.length[b, j])
            if bool(q.finished[b, j]) or n + 1 >= W or not np.isfinite(logp[b, j].item()):
                continue
            assert int(rows[b, j, n + 1]) == PAD
            lg = torch.empty((1, W - 1, native.tgt_vocab_size), dtype=torch.float32, device="cuda")
            native.score_hypotheses(s[b:b + 1], rows[b:b + 1, j:j + 1], eos_token_idx=EOS, trim=False, logits_out=lg)
            forced = None if prefix is None else torch.tensor([int((prefix[b] != PAD).sum())], dtype=torch.int32)
            ext = native.hypothesis_logq(lg[:, :n + 1].contiguous(), rows[b, j:j + 1, :n + 2], -1, EOS, temperature=2.0, top_k=8, top_p=0.9,
                                         forced_len=forced)
            assert int(ext.length[0]) == n + 1 and torch.equal(ext.token_logq[0, :n], q.token_logq[b, j, :n])
            lq[b, j], scored[b, j] = ext.logq[0].item(), n + 1
            n_pad += 1
    per_tok = TOK_TOL * max(1.0, tok[torch.isfinite(tok)].abs().max().item())          # temperature 2: max(1, 1 / T) = 1
    use = torch.isfinite(logp) & (q.first_outside.cpu() == -1) & torch.isfinite(lq)
    err = (lq - logp).abs()[use]
    bound = (scored * per_tok)[use]
    print(f"{name} prefixed {prefixed}: {int(use.sum())} of {logp.numel()} rows compared ({n_pad} ended on a sampled PAD), max |logq - logp| "
          f"{err.max().item():.3g}, largest share of its bound {(err / bound).max().item():.3g}; rows outside: {int((q.first_outside >= 0).sum())}")
    assert int(use.sum()) >= logp.numel() // 2
    assert (err <= bound).all()
    if prefixed:
        assert (tok[:, :, :3] == 0).all()
    g1 = tta.TranslationInferenceStochasticBeamSearch(native, 2, MAX_LEN, PAD, BOS, EOS, temperature=2.0, seed=SEED, top_k=1)
    rows1, det1 = g1.generate(s, return_details=True)
    q1 = g1.logq(s, rows1)
    finite = torch.isfinite(det1.logp)
    assert finite[:, 0].all() and (q1.logq[finite] == 0.0).all() and (q1.first_outside[finite] == -1).all()


# -- pooled and Lightning paths ------------------------------------------------------------------------------------------------------
def test_generate_and_generate_many_return_logq(tta, models, src):
    native = models["tiny"][0]
    c = fixture_tokens()[2]
    s = src.cuda()
    kw = dict(temperature=2.0, top_k=8, top_p=0.9, num_samples=3, seed=SEED)
    plain = tta.TranslationInferenceSampling(native, MAX_LEN, PAD, BOS, EOS, **kw)
    spec = tta.TranslationInferenceSamplingSpeculative(native, MAX_LEN, 4, 2, PAD, BOS, EOS, c, **kw)
    for g in (plain, spec):
        pred, q = g.generate(s[:4], return_logq=True)
        assert isinstance(q, tta.ProposalScores) and torch.equal(pred, g.generate(s[:4])) and q.scores is None
        assert same(q, g.logq(s[:4], pred))
        pred2, sc, q2 = g.generate(s[:4], return_scores=True, return_logq=True)
        assert torch.equal(pred2, pred) and same(q2, q) and q2.scores is sc
        assert all(torch.equal(a, b) for a, b in zip(sc[:3], g.score(s[:4], pred)[:3]))
        prefix = torch.tensor([[5, 6], [7, PAD], [PAD, PAD], [8, 9]])
        pp, qp = g.generate(s[:4], return_logq=True, prefix=prefix)
        assert same(qp, g.logq(s[:4], pp, prefix=prefix))
        full = g.logq(s[:4], pp, prefix=prefix, return_token_logq=True).token_logq
        assert (full[0, :, :2] == 0).all() and (full[1, :, :1] == 0).all() and (full[3, :, :2] == 0).all()
    batches = [s[0:4], s[4:8], s[8:10]]
    calls = spec.model_calls_num
    pairs = spec.generate_many(batches, in_flight=2, return_logq=True)
    assert len(pairs) == 3 and spec.model_calls_num > calls
    for b, (p, q) in zip(batches, pairs):
        assert same(q, spec.logq(b, p)) and q.logq.shape == p.shape[:2]
    triples = spec.generate_many(batches, in_flight=2, return_scores=True, return_logq=True)
    for (p, q), (p3, sc3, q3) in zip(pairs, triples):
        assert torch.equal(p, p3) and same(q, q3) and torch.equal(sc3.score, q3.scores.score)
    # the deterministic generators default to the model's own distribution
    greedy = tta.TranslationInferenceGreedy(native, MAX_LEN, PAD, BOS, EOS)
    gp, gs = greedy.generate(s[:4], return_scores=True)
    assert torch.equal(greedy.logq(s[:4], gp).logq, gs.score)
    assert (greedy.logq(s[:4], gp, temperature=0.0).logq == 0.0).all()


@pytest.mark.parametrize("generation", ["sampling", "sampling_speculative", "stochastic_beam_search"])
def test_lightning_keeps_logq(tta, tmp_path, generation, monkeypatch):
    from test_gpu_lightning_surface import FixtureTokenizer
    monkeypatch.delenv("TTX_PREDICT_LOGQ", raising=False)
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    s, tgt, _, _ = fixture_tokens()
    batches = [{"src_tokens": s[i:j, :int((s[i:j] != PAD).sum(1).max())].cuda(), "tgt_tokens": tgt[i:j].cuda()} for i, j in ((0, 4), (4, 8), (8, 10))]

    def module(report):
        mod = tta.VanillaEncoderDecoderTransformerLightning(
            src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
            num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
            share_embeddings=True, generation=generation, beam_size=3, max_len=MAX_LEN, n_drafts=2, draft_len=4, sampling_temperature=2.0,
            sampling_top_k=8, sampling_top_p=0.9, sampling_seed=11, report_prediction_file=str(report))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        return mod

    off = module(tmp_path / "off.txt")
    outs_off = tta.run_predict(off, batches)
    rep_off = json.loads((tmp_path / "off.txt").read_text().strip().split("\n")[-1])
    assert off.predict_logq == {} and "logq_seconds" not in rep_off and "hypotheses_outside_support" not in rep_off
    on = module(tmp_path / "on.txt")
    on.predict_with_logq = True
    outs_on = tta.run_predict(on, batches)
    rep_on = json.loads((tmp_path / "on.txt").read_text().strip().split("\n")[-1])
    assert all(torch.equal(a, b) for a, b in zip(outs_off, outs_on)) and rep_on["model_calls"] == rep_off["model_calls"]
    assert set(rep_on) == set(rep_off) | {"logq_seconds", "hypotheses_outside_support"}
    assert sorted(on.predict_logq) == [0, 1, 2]
    for i, (b, p) in enumerate(zip(batches, outs_on)):
        q = on.predict_logq[i]
        assert isinstance(q, tta.ProposalScores) and q.logq.shape == p.shape[:2]
        assert same(q, on.generator.logq(b["src_tokens"], p))
    assert rep_on["hypotheses_outside_support"] == sum(int((on.predict_logq[i].first_outside >= 0).sum()) for i in range(3))
    # both switches: the scores and log q of a batch come from one decoder pass and are what the two switches give alone
    both = module(tmp_path / "both.txt")
    both.predict_with_logq = both.predict_with_scores = True
    calls = []
    real = tta.NativeTransformer.score_hypotheses
    with monkeypatch.context() as mp:
        mp.setattr(tta.NativeTransformer, "score_hypotheses", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
        outs_both = tta.run_predict(both, batches)
    assert calls == [], "score_hypotheses ran beside proposal_scores: two decoder passes per batch"
    rep_both = json.loads((tmp_path / "both.txt").read_text().strip().split("\n")[-1])
    assert set(rep_both) == set(rep_on) | {"scoring_seconds", "mean_top1_logprob", "unfinished_hypotheses"}
    for i, (b, p) in enumerate(zip(batches, outs_both)):
        assert torch.equal(p, outs_on[i]) and same(both.predict_logq[i], on.predict_logq[i]) and both.predict_logq[i].scores is None
        sc, ref = both.predict_scores[i], both.generator.score(b["src_tokens"], p)
        assert torch.equal(sc.score, ref.score) and torch.equal(sc.length, ref.length) and torch.equal(sc.finished, ref.finished)
    # prefix_tokens of a batch become forced positions
    pre = [{**b, "prefix_tokens": torch.tensor([[5, 6, 7], [8, 9, PAD], [PAD, PAD, PAD], [4, PAD, PAD]])[:b["src_tokens"].shape[0]]}
           for b in batches]
    pm = module(tmp_path / "pre.txt")
    pm.predict_with_logq = True
    outs_pre = tta.run_predict(pm, pre)
    for i, (b, p) in enumerate(zip(pre, outs_pre)):
        q = pm.predict_logq[i]
        assert same(q, pm.generator.logq(b["src_tokens"], p, prefix=b["prefix_tokens"]))
        full = pm.generator.logq(b["src_tokens"], p, prefix=b["prefix_tokens"], return_token_logq=True).token_logq
        assert (p[0, :, 1:4].cpu() == torch.tensor([5, 6, 7])).all() and (full[0, :, :3] == 0).all()
        free = pm.generator.logq(b["src_tokens"], p, return_token_logq=True).token_logq
        assert (free[0, :, :3] != 0).any()                                  # unforced, those positions cost something
    monkeypatch.setenv("TTX_PREDICT_LOGQ", "1")
    env = module(tmp_path / "env.txt")
    tta.run_predict(env, batches)
    assert all(same(env.predict_logq[i], on.predict_logq[i]) for i in range(3))
    monkeypatch.delenv("TTX_PREDICT_LOGQ")
    bad = tta.VanillaEncoderDecoderTransformerLightning(
        src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
        num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
        share_embeddings=True, generation="greedy", max_len=MAX_LEN)
    bad.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    bad.predict_with_logq = True
    with pytest.raises(ValueError, match="predict_with_logq"):
        tta.run_predict(bad, batches)


# -- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(tta, models, samples, src):
    from translation_transformer_amd._native import TtxError
    from util_models import seeded_weights, state_shapes
    import ctypes as C
    N = tta._native
    native = models["tiny"][0]
    s, hyp = src.cuda(), samples["tiny", 2.0, True][1]
    B, K, W = hyp.shape
    for kw in (dict(top_k=33), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(temperature=-0.5), dict(temperature=float("nan")),
               dict(temperature=float("inf")), dict(forced_len=torch.zeros(B + 1, dtype=torch.int32)),
               dict(forced_len=torch.zeros((B, K + 1), dtype=torch.int32)), dict(forced_len=torch.zeros(B)),
               dict(forced_len=torch.full((B,), -1, dtype=torch.int32))):
        with pytest.raises(ValueError):
            native.proposal_scores(s, hyp, **kw)
    with pytest.raises(ValueError):
        native.proposal_scores(s[:4], hyp)
    bad = hyp.clone()
    bad[1, 1, 3] = native.tgt_vocab_size
    with pytest.raises(IndexError):
        native.proposal_scores(s, bad)
    # the C boundary refuses before any launch: the outputs keep their poison
    lib, sess, stream = native._lib, native._scoring_session(), native._stream()
    logq = torch.full((B * K,), 7.0, device="cuda")
    length = torch.full((B * K,), 7, dtype=torch.int32, device="cuda")

    def call(dist, B_=B, W_=W, ld=W, lq=logq):
        d = N.Dist(*dist) if dist is not None else None
        return lib.ttx_score_proposal(sess, s.data_ptr(), B_, s.shape[1], hyp.data_ptr(), ld, K, W_, EOS, C.byref(d) if d else None, None,
                                      None, None, None, None, lq.data_ptr() if lq is not None else None, None, None, None,
                                      length.data_ptr(), None, stream)

    for dist in ((1.0, 33, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.5), (-1.0, 0, 1.0), (float("nan"), 0, 1.0), (1e-45, 0, 1.0), None):
        assert call(dist) == N.TTX_ERR_INVALID, dist
    assert call((1.0, 0, 1.0), W_=1) == N.TTX_ERR_INVALID and call((1.0, 0, 1.0), ld=W - 1) == N.TTX_ERR_INVALID
    assert call((1.0, 0, 1.0), B_=0) == N.TTX_ERR_INVALID and call((1.0, 0, 1.0), lq=None) == N.TTX_ERR_INVALID
    x = torch.zeros((2, 3, 1025), device="cuda")
    d = N.Dist(1.0, 0, 1.0)
    assert lib.ttx_hypothesis_logq(sess, x.data_ptr(), hyp.data_ptr(), 2, 4, 1025, PAD, EOS, C.byref(d), None, None, logq.data_ptr(), None,
                                   None, None, length.data_ptr(), None, stream) == N.TTX_ERR_INVALID
    torch.cuda.synchronize()
    assert (logq == 7.0).all() and (length == 7).all()
    # V > 1 024: refused from the model's config
    V = 1030
    w = seeded_weights(state_shapes(V, 64, 64, 1, 1), 7)
    w["tgt_token_featurizer.embedding.weight"] = w["src_token_featurizer.embedding.weight"]
    big = tta.NativeTransformer(w, 2, PAD, device=0)
    with pytest.raises(TtxError, match="1024"):
        big.proposal_scores(s[:2], hyp[:2], temperature=0.5)
    # and the session is still usable
    assert torch.isfinite(native.proposal_scores(s, hyp, temperature=2.0).logq).any()
