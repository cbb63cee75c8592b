"""TranslationInferenceStochasticBeamSearch (ttx_sbs_generate) end to end on the tiny golden model: the exact consequences of the
rule (distinct rows, gumbel non-increasing from 0, run to run, a source alone / in a batch / at another padded width, nesting in
K, order="logp"), refusals, the Lightning surface, a level-by-level replay against the float64 oracle, and logp against score().

The replay.  The trace gives every level's beam; the float64 oracle is run on those prefixes and the restatement's float64 step
(tests/util_sbs_checks.py) on its logits, from the device's own phi and G of the level before; check_step compares the level the
device recorded, with the kernel test's margin rule and cap.  The margin is measured on the CPU, independent of the device: the
same levels through the fp32 oracle and the restatement in float32 against the float64 oracle and the restatement in float64,
max |G'_fp32 - G'_float64| over the selected well-conditioned children of a source's levels, times ten (the GPU model's logits
differ from the float64 oracle's as an fp32 model's do).  Measured on an MI355X run of this file: the fp32 gap of the four
sources is 5.5e-7, 1.6e-6, 8.9e-7 and 3.0e-6, the margins ten times that, and 1 of the 460 ranks is excused.

logp against score, measured: |logp - float64| is at most 4.1e-7 per token (9.4e-6 per row of 15 .. 23 tokens), score() the same,
under the bound of 1.15e-4 per token that TOK_TOL gives on these rows.

logp against score.  At temperature 1, logp is the sum of the step's log-probabilities and score() the teacher-forced sum: both
are held to the float64 oracle's sequence log-probability within length * TOK_TOL * max(1, max |token logp|), TOK_TOL = 1e-5 per
token being the bound tests/test_gpu_score.py holds score() to (DESIGN.md §10 measures 6.2e-6).
"""
import json

import numpy as np
import pytest
import torch

import util_sbs_checks as S
from test_gpu_score import TOK_TOL
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
SEED = 20190611
MAX_LEN = 24


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def model(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0)


@pytest.fixture(scope="module")
def oracles():
    from oracle.model import OracleTransformer, config_from_state
    st, cfg = tiny_state()
    c = config_from_state(st, cfg["num_heads"])
    return OracleTransformer(c, st, dtype=torch.float64), OracleTransformer(c, st)


@pytest.fixture(scope="module")
def src():
    s = fixture_tokens()[0][:4]
    return s[:, :int((s != PAD).sum(1).max())]


KEYS = [5, 1 << 40, 7, -3]


def sbs(tta, model, K, **kw):
    kw.setdefault("temperature", 2.0)
    return tta.TranslationInferenceStochasticBeamSearch(model, K, MAX_LEN, PAD, BOS, EOS, seed=SEED, **kw)


@pytest.fixture(scope="module")
def run5(tta, model, src):
    """generate(K = 5) of the four sources with details and trace: computed once, shared, never modified."""
    out, d = sbs(tta, model, 5).generate(src.cuda(), row_keys=KEYS, return_details=True, trace=True)
    return out.cpu().numpy(), d


def ends(rows):
    stop = (rows[:, 1:] == EOS) | (rows[:, 1:] == PAD)
    return np.where(stop.any(1), stop.argmax(1) + 1, rows.shape[1] - 1)


def test_shape_distinct_rows_and_gumbel_order(run5):
    out, d = run5
    assert out.shape == (4, 5, MAX_LEN) and (out[:, :, 0] == BOS).all()
    for b in range(4):
        e = ends(out[b])
        for r, n in zip(out[b], e):
            assert (r[n + 1:] == PAD).all() and not np.isin(r[1:n], (PAD, EOS)).any(), r.tolist()
        assert len({tuple(r) for r in out[b].tolist()}) == 5, f"source {b}: hypotheses repeat"
    g, lp = d.gumbel.cpu().numpy(), d.logp.cpu().numpy()
    assert g.dtype == np.float32 and (g[:, 0] == 0).all() and (np.diff(g, axis=1) <= 0).all()
    assert (lp <= 0).all() and np.isfinite(lp).all()
    stop = ((out[:, :, 1:] == EOS) | (out[:, :, 1:] == PAD)).any(-1)
    assert (d.finished.cpu().numpy() == stop).all()


def test_run_to_run(tta, model, src, run5):
    out, d = sbs(tta, model, 5).generate(src.cuda(), row_keys=KEYS, return_details=True)
    assert (out.cpu().numpy() == run5[0]).all()
    assert torch.equal(d.logp, run5[1].logp) and torch.equal(d.gumbel, run5[1].gumbel) and d.trace is None


def test_a_source_alone_in_a_batch_and_at_another_width(tta, model, src, run5):
    for b in (1, 3):
        n = int((src[b] != PAD).sum())
        for s in (src[b:b + 1, :n], torch.nn.functional.pad(src[b:b + 1], (0, 3), value=PAD)):
            out, d = sbs(tta, model, 5).generate(s.cuda(), row_keys=[KEYS[b]], return_details=True)
            assert (out.cpu().numpy()[0] == run5[0][b]).all(), f"source {b} at width {s.shape[1]}"
            assert torch.equal(d.logp[0], run5[1].logp[b]) and torch.equal(d.gumbel[0], run5[1].gumbel[b])


def test_k3_is_the_first_three_rows_of_k5(tta, model, src, run5):
    out, d = sbs(tta, model, 3).generate(src.cuda(), row_keys=KEYS, return_details=True)
    assert (out.cpu().numpy() == run5[0][:, :3]).all()
    assert torch.equal(d.logp, run5[1].logp[:, :3]) and torch.equal(d.gumbel, run5[1].gumbel[:, :3])
    assert torch.equal(d.finished, run5[1].finished[:, :3])


def test_default_keys_and_the_seed(tta, model, src, run5):
    a = sbs(tta, model, 5).generate(src.cuda())
    b = sbs(tta, model, 5).generate(src.cuda(), row_keys=[0, 1, 2, 3])
    assert torch.equal(a, b) and not (a.cpu().numpy() == run5[0]).all()
    c = tta.TranslationInferenceStochasticBeamSearch(model, 5, MAX_LEN, PAD, BOS, EOS, temperature=2.0, seed=SEED + 1)
    assert not torch.equal(c.generate(src.cuda()), a)


def test_order_logp_is_a_sorted_permutation(tta, model, src, run5):
    out, d = sbs(tta, model, 5).generate(src.cuda(), row_keys=KEYS, return_details=True, order="logp")
    out, lp, g = out.cpu().numpy(), d.logp.cpu().numpy(), d.gumbel.cpu().numpy()
    ref_lp, ref_g = run5[1].logp.cpu().numpy(), run5[1].gumbel.cpu().numpy()
    assert (np.diff(lp, axis=1) <= 0).all()
    moved = False
    for b in range(4):
        perm = [next(j for j in range(5) if (run5[0][b, j] == out[b, i]).all()) for i in range(5)]
        assert sorted(perm) == list(range(5))
        assert (lp[b] == ref_lp[b, perm]).all() and (g[b] == ref_g[b, perm]).all()
        moved |= perm != list(range(5))
    assert moved, "sampling order and logp order agree for every source: the case shows nothing"
    with pytest.raises(ValueError):
        sbs(tta, model, 5).generate(src.cuda(), order="score")


def test_scores_and_counters(tta, model, src, run5):
    g = sbs(tta, model, 5)
    out, sc, d = g.generate(src.cuda(), row_keys=KEYS, return_scores=True, return_details=True)
    assert (out.cpu().numpy() == run5[0]).all() and sc.score.shape == (4, 5)
    assert g.model_calls_num == run5[1].trace.token.shape[0] and g.given_tokens == int((src != PAD).sum()) and g.b_sz > 0
    assert hasattr(g, "attention") and hasattr(g, "alternatives")


def test_refusals(tta, model, src):
    s = src.cuda()
    for kw, K, max_len in ((dict(temperature=0.0), 3, MAX_LEN), (dict(temperature=-1.0), 3, MAX_LEN),
                           (dict(temperature=float("inf")), 3, MAX_LEN), (dict(temperature=float("nan")), 3, MAX_LEN),
                           (dict(), 33, MAX_LEN), (dict(), 0, MAX_LEN), (dict(), 3, 1), (dict(), 3, 10 ** 6)):
        g = tta.TranslationInferenceStochasticBeamSearch(model, K, max_len, PAD, BOS, EOS, seed=1, **kw)
        with pytest.raises(tta.TtxError) as e:
            g.generate(s)
        assert e.value.code == -1, (kw, K, max_len)
    with pytest.raises(tta.TtxError):
        tta.TranslationInferenceStochasticBeamSearch(model, 3, MAX_LEN, PAD + 1, BOS, EOS).generate(s)
    with pytest.raises(ValueError):
        sbs(tta, model, 3).generate(s, row_keys=[1, 2])
    with pytest.raises(TypeError):
        tta.TranslationInferenceStochasticBeamSearch(object(), 3, MAX_LEN, PAD, BOS, EOS)


# -- float64 replay ---------------------------------------------------------------------------------------------------------------
def replay(run5, src, oracles, b: int):
    """Source b level by level.  Returns (problems, excused, ranks, fp32 gap) with the margin rule of the module docstring: the
    gap is measured first, over every level, then the levels are checked with ten times it."""
    out, d = run5
    o64, o32 = oracles
    tr = [t.cpu().numpy()[:, b] for t in d.trace]                      # [levels, K] each
    levels, K = tr[0].shape
    s = src[b:b + 1]
    rows = np.array([[BOS]], dtype=np.int64)
    phi, G, fin = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, bool)
    steps, gap = [], 0.0
    for lv in range(levels):
        live = np.nonzero(~fin)[0]
        lg64 = np.zeros((len(rows), 1), np.float64)
        lg32 = np.zeros((len(rows), 1), np.float32)
        if len(live):
            with torch.no_grad():
                a = o64(s.expand(len(live), -1), torch.from_numpy(rows[live]))[:, -1].numpy()
                c = o32(s.expand(len(live), -1), torch.from_numpy(rows[live]))[:, -1].numpy()
            lg64 = np.zeros((len(rows), a.shape[1]), np.float64)
            lg32 = np.zeros((len(rows), a.shape[1]), np.float32)
            lg64[live], lg32[live] = a, c
        args = (phi, G, fin, KEYS[b], lv + 1, SEED, 2.0, K, PAD, EOS)
        r64, r32 = S.step(lg64, *args), S.step(lg32, *args, dtype=np.float32)
        sel = r64.order[:K]
        sel = sel[~r64.ill.reshape(-1)[sel]]
        x, y = r64.img_g.reshape(-1)[sel], r32.img_g.reshape(-1)[sel].astype(np.float64)
        ok = np.isfinite(x) & np.isfinite(y)
        gap = max(gap, float(np.abs(x[ok] - y[ok]).max()) if ok.any() else 0.0)
        par, tok = tr[0][lv], tr[1][lv]
        dev_fin = fin[par] | (tok == EOS) | (tok == PAD) | np.isneginf(tr[3][lv])
        steps.append((dict(parent=par, token=tok, phi=tr[2][lv], g=tr[3][lv], finished=dev_fin), r64, G, phi, fin))
        rows = np.concatenate([rows[par], tok[:, None].astype(np.int64)], axis=1)
        phi, G, fin = tr[2][lv], tr[3][lv], dev_fin
    assert (rows == out[b][:, :rows.shape[1]]).all() and (out[b][:, rows.shape[1]:] == PAD).all(), "the trace does not rebuild the output"
    assert (phi == d.logp.cpu().numpy()[b]).all() and (G == d.gumbel.cpu().numpy()[b]).all()
    assert (fin == d.finished.cpu().numpy()[b]).all()
    from types import SimpleNamespace
    bad, excused = [], 0
    for lv, (dev, r64, pG, pphi, pfin) in enumerate(steps):
        p, ex = S.check_step(SimpleNamespace(**dev), r64, pG, pphi, pfin, K, PAD, EOS, 10 * gap)
        bad += [f"level {lv}: {m}" for m in p]
        excused += ex
    return bad, excused, levels * K, gap


def test_replay_level_by_level_against_the_float64_oracle(run5, src, oracles):
    total = excused = 0
    worst = 0.0
    for b in range(4):
        bad, ex, n, gap = replay(run5, src, oracles, b)
        print(f"source {b}: {n} ranks, {ex} excused, fp32 gap {gap:.3g}, margin {10 * gap:.3g}")
        assert not bad, f"source {b}: " + "; ".join(bad[:4])
        total, excused, worst = total + n, excused + ex, max(worst, gap)
    print(f"replay: {excused} of {total} ranks excused, largest fp32 gap {worst:.3g}")
    assert excused <= S.EXCUSED_CAP * total


def test_logp_agrees_with_score_at_temperature_one(tta, model, src, oracles):
    g = sbs(tta, model, 6, temperature=1.0)
    out, sc, d = g.generate(src.cuda(), row_keys=KEYS, return_scores=True, return_details=True)
    rows = out.cpu().numpy().reshape(24, MAX_LEN)
    with torch.no_grad():
        lp = torch.log_softmax(oracles[0](src.repeat_interleave(6, 0), torch.from_numpy(rows[:, :-1])), -1).numpy()
    tok = np.take_along_axis(lp, rows[:, 1:, None], 2)[:, :, 0]
    n = ends(rows)
    ref = np.array([tok[r, :n[r]].sum() for r in range(24)])
    tol = TOK_TOL * max(1.0, float(np.abs(np.concatenate([tok[r, :n[r]] for r in range(24)])).max()))
    logp, score = d.logp.cpu().numpy().reshape(24).astype(np.float64), sc.score.cpu().numpy().reshape(24).astype(np.float64)
    scored = np.array([rows[r, n[r]] != PAD for r in range(24)])       # score() stops before a sampled PAD; logp includes it
    assert scored.sum() >= 12
    print(f"max |logp - float64| / length {np.abs(logp - ref).max() / 1:.3g} over lengths {n.min()}..{n.max()}; per token "
          f"{(np.abs(logp - ref) / n).max():.3g}; score: {(np.abs(score - ref)[scored] / n[scored]).max():.3g}; bound {tol:.3g}")
    assert (np.abs(logp - ref) <= n * tol).all()
    assert (np.abs(score - ref)[scored] <= n[scored] * tol).all()
    assert (np.abs(logp - score)[scored] <= 2 * n[scored] * tol).all()


# -- Lightning -------------------------------------------------------------------------------------------------------------------
def test_lightning_stochastic_beam_search_does_not_depend_on_the_batch_size(tta, tmp_path):
    from test_gpu_lightning_surface import FixtureTokenizer, CsvWriter
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    s, tgt, _, _ = fixture_tokens()
    preds = {}
    for bs in (1, 4):
        report = tmp_path / f"r{bs}.txt"
        mod = tta.VanillaEncoderDecoderTransformerLightning(
            src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
            num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
            share_embeddings=True, generation="stochastic_beam_search", beam_size=3, max_len=MAX_LEN, sampling_temperature=2.0,
            sampling_seed=11, report_prediction_file=str(report))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        batches = [{"src_tokens": s[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda()} for i in range(0, 4, bs)]
        preds[bs] = torch.cat(tta.run_predict(mod, batches, writer=CsvWriter(tmp_path / f"pred{bs}.csv")), 0)
        rep = json.loads(report.read_text().strip().split("\n")[-1])
        assert rep["algorithm"] == "stochastic_beam_search" and rep["model_calls"] > 0
        assert sorted(rep) == sorted(["algorithm", "batch_size", "tgt_test_path", "max_len", "total_seconds", "model_calls",
                                      "seconds_per_model_call"])
    assert preds[1].shape == (4, 3, MAX_LEN) and torch.equal(preds[1], preds[4])
    for b in range(4):
        assert len({tuple(r) for r in preds[4][b].tolist()}) == 3
