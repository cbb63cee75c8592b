"""Folding sampled hypotheses end to end (NativeTransformer.fold_hypotheses, the generators' ``fold``, scoring.fold_samples and the
Lightning switch) on the ten fixture sources with the tiny golden model and the four-head model of tests/golden/h4_*, max_len 32,
against scoring.unique_samples (the host yardstick) and the NumPy restatement of tests/util_fold.py.

The case.  TranslationInferenceSampling at num_samples 16, seed 20260203, keys 0..9, temperature 1.5.  The temperature was chosen
beforehand with the float64 oracle sampling by the same rule on the CPU (tests/util_sample_checks.py: uniform, sample64), which
gives per source these numbers of distinct hypotheses among the 16 rows:
  tiny  T 0.7: 1 everywhere;  T 1.0: 4 2 3 2 1 1 1 1 1 1;  T 1.5: 14 11 14 13 13 14 10 15 10 9
  h4    T 0.7: 1 everywhere;  T 1.0: 2 4 3 2 2 1 2 1 1 2;  T 1.5: 14 12 14 12 10 12 10 15 10 11
so at 1.5 every source holds both repeats and distinct rows on either model; the test asserts 1 < n_unique < 16 for some source.

``logmass`` is held to one fp32 spacing of the float64 log-sum-exp of the distinct scores rounded to fp32 (the bound of
tests/test_gpu_fold_kernel.py); everything else is compared exactly."""
import json
import math

import numpy as np
import pytest
import torch

import util_fold as U
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
SEED = 20260203
MAX_LEN = 32
N_SAMPLES = 16
TEMPERATURE = 1.5
FIELDS = ("pred", "perm", "count", "n_unique", "first", "rank_of", "score", "logmass")


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
def src():
    s = fixture_tokens()[0]
    return s[:, :int((s != PAD).sum(1).max())].cuda()


@pytest.fixture(scope="module")
def cases(tta, src):
    """name -> (native, sampler, rows Long[10, 16, 32], their HypothesisScores), drawn and scored once."""
    out = {}
    for name in ("tiny", "h4"):
        st, cfg = states(name)
        native = tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0)
        g = tta.TranslationInferenceSampling(native, MAX_LEN, PAD, BOS, EOS, temperature=TEMPERATURE, num_samples=N_SAMPLES, seed=SEED)
        pred = g.generate(src)
        out[name] = (native, g, pred, g.score(src, pred))
    return out


def same_bits(a, b, fields=FIELDS) -> bool:
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        if (x is None) != (y is None):
            return False
        if x is not None and not torch.equal(x.view(torch.uint8) if x.dtype == torch.float32 else x,
                                             y.view(torch.uint8) if y.dtype == torch.float32 else y):
            return False
    return True


def as_numpy(f) -> dict:
    d = {k: (None if getattr(f, k) is None else getattr(f, k).cpu().numpy()) for k in FIELDS}
    d["out"] = d.pop("pred")
    return d


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_fold_equals_unique_samples(tta, cases, src, name):
    native, g, pred, sc = cases[name]
    want = tta.scoring.unique_samples(pred, sc, eos=EOS)
    f = g.fold(src, pred, scores=sc, order="score", unfinished="keep")
    nu = f.n_unique.cpu().tolist()
    print(name, "n_unique", nu)
    assert any(1 < u < N_SAMPLES for u in nu), "the case holds no source with both repeats and distinct rows"
    p, cnt, s = f.pred.cpu(), f.count.cpu(), f.score.cpu()
    for b, rows in enumerate(want):
        assert nu[b] == len(rows), b
        for r, (tok, c, v) in enumerate(rows):
            assert torch.equal(p[b, r], tok) and int(cnt[b, r]) == c and float(s[b, r]) == v, (b, r)
        assert (p[b, len(rows):] == PAD).all() and (cnt[b, len(rows):] == 0).all() and torch.isneginf(s[b, len(rows):]).all()
    # the same call with no model at hand, and the whole result against the restatement
    assert same_bits(tta.scoring.fold_samples(pred, sc, pad=PAD, eos=EOS), f)
    hyp, val = pred.cpu().numpy(), sc.score.cpu().numpy()
    U.assert_fold_equal(as_numpy(f), U.fold_reference(hyp, val, U.SCORE, 0, PAD, EOS), what=f"{name} keep")
    # the generator's default: it scores the rows itself and puts the unfinished hypotheses last
    d = g.fold(src, pred)
    U.assert_fold_equal(as_numpy(d), U.fold_reference(hyp, val, U.SCORE, U.UNFINISHED_LAST, PAD, EOS), what=f"{name} default")
    fin = (d.pred == EOS).any(-1).int()
    live = d.perm >= 0
    assert bool((fin[:, 1:] <= fin[:, :-1])[live[:, 1:]].all())                        # finished rows first among the live ones
    assert bool((d.pred[~live] == PAD).all())
    for order, code in (("count", U.COUNT), ("first", U.FIRST)):
        o = g.fold(src, pred, scores=sc, order=order, unfinished="keep")
        U.assert_fold_equal(as_numpy(o), U.fold_reference(hyp, val, code, 0, PAD, EOS), what=f"{name} {order}")
    # a view is folded in place through its row stride; gather=False hands out no rows
    wide = torch.full((10, N_SAMPLES, MAX_LEN + 5), 7, dtype=torch.int64, device="cuda")
    wide[:, :, :MAX_LEN] = pred
    v = native.fold_hypotheses(wide[:, :, :MAX_LEN], sc, eos=EOS)
    assert same_bits(v, f)
    ng = native.fold_hypotheses(pred, sc, gather=False, eos=EOS)
    assert ng.pred is None and same_bits(ng, f, FIELDS[1:])


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_ranks_and_mass_are_consistent(tta, cases, src, name):
    native, g, pred, sc = cases[name]
    f = g.fold(src, pred, scores=sc)
    perm, first, rank_of, count, nu = (t.cpu().long() for t in (f.perm, f.first, f.rank_of, f.count, f.n_unique))
    assert torch.equal(perm.gather(1, rank_of), first)                                  # a sample's rank names its first occurrence
    assert torch.equal(first.gather(1, first), first) and bool((first <= torch.arange(N_SAMPLES)).all())
    assert torch.equal(count.sum(1), torch.full((10,), N_SAMPLES)) and torch.equal((perm >= 0).sum(1), nu)
    for b in range(10):
        assert torch.equal(torch.bincount(rank_of[b], minlength=N_SAMPLES), count[b])
        u = int(nu[b])
        vals = f.score[b, :u].cpu().double().tolist()
        m = max(vals)
        want = m + math.log(sum(math.exp(v - m) for v in vals))
        assert U.logmass_ok(f.logmass[b].cpu().numpy(), want), (b, float(f.logmass[b]), want)
        if bool((f.pred[b, :u] == EOS).any(-1).all()):          # finished hypotheses exclude each other: a probability mass
            assert want <= 1e-4                                  # (an unfinished row's score is its prefix's, which overlaps)


def test_speculative_and_pooled_samplers_fold_alike(tta, cases, src):
    native, g, pred, sc = cases["tiny"]
    c = fixture_tokens()[2]
    make = lambda: tta.TranslationInferenceSamplingSpeculative(native, MAX_LEN, 4, 2, PAD, BOS, EOS, c, temperature=TEMPERATURE,
                                                               num_samples=N_SAMPLES, seed=SEED)
    spec = make()
    rows = [spec.generate(src), make().generate_many([src[:4], src[4:]]), make().generate_many([src[:4], src[4:]], capacity=3)]
    rows = [r if isinstance(r, torch.Tensor) else torch.cat(r, 0) for r in rows]
    folds = [spec.fold(src, r) for r in rows]
    assert same_bits(folds[0], folds[1]) and same_bits(folds[0], folds[2])
    assert any(1 < u < N_SAMPLES for u in folds[0].n_unique.cpu().tolist())


def test_merging_generators_sums_the_counts(tta, cases, src):
    native, g, pred, sc = cases["tiny"]
    beam = tta.TranslationInferenceBeamSearch(native, 4, MAX_LEN, PAD, BOS, EOS)
    bp = beam.generate(src)
    assert bp.shape[2] <= MAX_LEN
    wide = torch.full((10, bp.shape[1], MAX_LEN), PAD, dtype=torch.int64, device="cuda")
    wide[:, :, :bp.shape[2]] = bp
    both = torch.cat([wide, pred], dim=1)
    f = g.fold(src, both, order="count")
    alone_b, alone_s = g.fold(src, wide, order="first"), g.fold(src, pred, order="first")
    assert bool((alone_b.n_unique == bp.shape[1]).all())                                # a beam's hypotheses are distinct
    hyp = both.cpu().numpy()
    ref = U.fold_reference(hyp, g.score(src, both).score.cpu().numpy(), U.COUNT, U.UNFINISHED_LAST, PAD, EOS)
    U.assert_fold_equal(as_numpy(f), ref, what="beam + samples")
    shared = 0
    for b in range(10):
        keys_b = {tuple(r[:U.row_extent(r, EOS)[0]]) for r in wide[b].cpu().numpy()}
        cnt_s = {}
        for r in pred[b].cpu().numpy():
            k = tuple(r[:U.row_extent(r, EOS)[0]])
            cnt_s[k] = cnt_s.get(k, 0) + 1
        u = int(f.n_unique[b])
        assert u == len(keys_b | set(cnt_s))
        for r in range(u):
            row = f.pred[b, r].cpu().numpy()
            k = tuple(row[:U.row_extent(row, EOS)[0]])
            assert int(f.count[b, r]) == (k in keys_b) + cnt_s.get(k, 0)
            shared += (k in keys_b) and (k in cnt_s)
    assert shared > 0, "no hypothesis common to the beam and the samples: the case shows nothing"


def test_stochastic_beam_search_rows_are_distinct(tta, cases, src):
    native = cases["tiny"][0]
    K = 6
    sbs = tta.TranslationInferenceStochasticBeamSearch(native, K, MAX_LEN, PAD, BOS, EOS, temperature=TEMPERATURE, seed=SEED)
    rows = sbs.generate(src)
    f = sbs.fold(src, rows, unfinished="keep")
    assert bool((f.n_unique == K).all()) and bool((f.count == 1).all())


# -- Lightning ---------------------------------------------------------------------------------------------------------------------
def make_module(tta, generation, report, beam_size=N_SAMPLES, **kw):
    from test_gpu_lightning_surface import FixtureTokenizer
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    mod = tta.VanillaEncoderDecoderTransformerLightning(
        src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
        num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
        share_embeddings=True, generation=generation, beam_size=beam_size, max_len=MAX_LEN, n_drafts=2, draft_len=4,
        sampling_temperature=TEMPERATURE, sampling_seed=11, report_prediction_file=str(report), **kw)
    mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    return mod


def lightning_batches():
    s, tgt, _, _ = fixture_tokens()
    return [{"src_tokens": s[i:j, :int((s[i:j] != PAD).sum(1).max())].cuda(), "tgt_tokens": tgt[i:j].cuda()}
            for i, j in ((0, 4), (4, 8), (8, 10))]


@pytest.mark.parametrize("generation,pool", [("sampling", False), ("sampling_speculative", False), ("sampling_speculative", True)])
def test_lightning_returns_folded_rows(tta, tmp_path, monkeypatch, generation, pool):
    """The ways rows reach predict_step: decoded on the spot by either sampler, and ahead of it by the look-ahead window over the
    sample pool."""
    from test_gpu_lightning_surface import CsvWriter
    for var in ("TTX_PREDICT_FOLD", "TTX_PREDICT_SCORES", "TTX_PREDICT_SAMPLE_POOL"):
        monkeypatch.delenv(var, raising=False)
    batches = lightning_batches()
    off = make_module(tta, generation, tmp_path / "off.txt")
    off.predict_sample_pool = pool
    outs_off = tta.run_predict(off, batches)
    rep_off = json.loads((tmp_path / "off.txt").read_text().strip().split("\n")[-1])
    assert off.predict_folds == {} and "fold_seconds" not in rep_off
    on = make_module(tta, generation, tmp_path / "on.txt")
    on.predict_sample_pool = pool
    on.predict_fold_samples = on.predict_with_scores = True
    csv = tmp_path / "pred.csv"
    outs_on = tta.run_predict(on, batches, writer=CsvWriter(csv))
    rep_on = json.loads((tmp_path / "on.txt").read_text().strip().split("\n")[-1])
    assert set(rep_on) == set(rep_off) | {"fold_seconds", "distinct_hypotheses", "scoring_seconds", "mean_top1_logprob",
                                          "unfinished_hypotheses"}
    assert rep_on["model_calls"] == rep_off["model_calls"] and sorted(on.predict_folds) == [0, 1, 2]
    total, repeats = 0, 0
    for i, (b, raw, folded) in enumerate(zip(batches, outs_off, outs_on)):
        want = on.generator.fold(b["src_tokens"], raw, order="score", unfinished="last")
        count, n_unique, logmass = on.predict_folds[i]
        assert torch.equal(folded, want.pred) and torch.equal(count, want.count) and torch.equal(n_unique, want.n_unique)
        assert torch.equal(logmass, want.logmass)
        total += int(n_unique.sum())
        repeats += int((n_unique < raw.shape[1]).sum())
        # the kept scores are those of the folded rows; beyond n_unique what the scoring rule gives an all-PAD row
        sc, ref = on.predict_scores[i], on.generator.score(b["src_tokens"], folded)
        assert torch.equal(sc.score, ref.score) and torch.equal(sc.length, ref.length) and torch.equal(sc.finished, ref.finished)
        dead = want.perm < 0
        assert bool((sc.score[dead] == 0).all()) and bool((sc.length[dead] == 0).all()) and not bool(sc.finished[dead].any())
    assert rep_on["distinct_hypotheses"] == total and repeats > 0
    lines = csv.read_text().strip().split("\n")[1:]
    assert len(lines) == 10
    for line in lines:                                                                 # no duplicate inside a row of the CSV
        preds = [p for p in line.split(",")[2:] if p != ""]
        assert len(preds) == len(set(preds)), line
    # the switch alone (by the environment): the same rows, no scores kept
    monkeypatch.setenv("TTX_PREDICT_FOLD", "1")
    env = make_module(tta, generation, tmp_path / "env.txt")
    env.predict_sample_pool = pool
    outs_env = tta.run_predict(env, batches)
    assert all(torch.equal(a, b) for a, b in zip(outs_env, outs_on)) and env.predict_scores == {} and sorted(env.predict_folds) == [0, 1, 2]


def test_lightning_refusals(tta, tmp_path, monkeypatch):
    for var in ("TTX_PREDICT_FOLD", "TTX_PREDICT_LOGQ", "TTX_PREDICT_ATTENTION", "TTX_PREDICT_ALTERNATIVES"):
        monkeypatch.delenv(var, raising=False)
    batches = lightning_batches()
    for generation in ("greedy", "beam_search", "greedy_speculative", "beam_search_speculative", "stochastic_beam_search"):
        bad = make_module(tta, generation, tmp_path / "bad.txt", beam_size=3)
        bad.predict_fold_samples = True
        with pytest.raises(ValueError, match="predict_fold_samples"):
            tta.run_predict(bad, batches)
    for attr, value in (("predict_with_attention", True), ("predict_with_alternatives", 3), ("predict_with_logq", True)):
        bad = make_module(tta, "sampling", tmp_path / "bad.txt", beam_size=3)
        bad.predict_fold_samples = True
        setattr(bad, attr, value)
        with pytest.raises(ValueError, match="predict_fold_samples"):
            tta.run_predict(bad, batches)
