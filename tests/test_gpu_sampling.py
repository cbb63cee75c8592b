"""TranslationInferenceSampling (ttx_sample_generate) end to end, on the tiny golden model (2 heads: the step's attention runs on
k_attn2) and on the four-head model of tests/golden/h4_* (k_attn1 / k_attn3): greedy settings against TranslationInferenceGreedy,
a replay of every sampled token against the float64 oracle, exact invariance under batching, the shape of the output, score(),
refused arguments and the Lightning surface.

The replay.  Every sampled row is teacher-forced through the float64 oracle and every token must be ``consistent``
(tests/util_sample_checks.py) with the oracle's logits at its position and the uniform the rule gives that position.  The GPU's
logits are held to LOGIT_TOL = 1e-3 of the float64 oracle by tests/test_gpu_model.py and tests/test_gpu_envelope.py; call that
delta.  Two rows of logits that differ by at most delta in every entry, scaled by 1 / T, give probabilities whose ratio lies in
exp(+-2 delta / T) for every token, so the two CDFs differ by at most 2 delta / T at every point (first order); the kernel's own
fp32 CDF adds the 1e-4 of tests/test_gpu_sample_kernel.py.  tol = 2 delta / T + 1e-4.
"""
import json

import numpy as np
import pytest
import torch

import util_sample_checks as S
from test_gpu_model import LOGIT_TOL
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
SEED = 20260102


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
    return s[:, :int((s != PAD).sum(1).max())]                  # the ten fixture sources at the width of the longest


def sampler(tta, native, max_len=32, **kw):
    return tta.TranslationInferenceSampling(native, max_len, PAD, BOS, EOS, **kw)


def check_shape(out: np.ndarray, B, n, max_len):
    assert out.shape == (B, n, max_len) and (out[:, :, 0] == BOS).all()
    rows = out.reshape(B * n, max_len)
    end = S.ends(rows, PAD, EOS)
    for r, e in zip(rows, end):
        assert (r[e + 1:] == PAD).all(), f"tokens after the row's end: {r.tolist()}"
        assert not np.isin(r[1:e], (PAD, EOS)).any()
    return end


# -- greedy settings -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_greedy_settings_equal_greedy(tta, models, src, name):
    native = models[name][0]
    B, n, max_len = 3, 2, 24
    s = src[:B].cuda()
    ref = tta.TranslationInferenceGreedy(native, max_len, PAD, BOS, EOS).generate(s).cpu().numpy()[:, 0]
    ref_end = S.ends(ref, PAD, EOS)
    for kw in (dict(top_k=1), dict(temperature=0.0), dict(temperature=0.0, top_k=4, top_p=0.5), dict(temperature=0.5, top_k=1)):
        g = sampler(tta, native, max_len, num_samples=n, seed=SEED, **kw)
        out = g.generate(s).cpu().numpy()
        end = check_shape(out, B, n, max_len).reshape(B, n)
        for b in range(B):
            for j in range(n):
                e = ref_end[b]
                assert end[b, j] == e and (out[b, j, :e + 1] == ref[b, :e + 1]).all(), \
                    f"{name} {kw} source {b} sample {j}: {out[b, j].tolist()} against greedy {ref[b].tolist()}"
        assert g.model_calls_num == int(ref_end.max())


# -- replay against the float64 oracle -------------------------------------------------------------------------------------------
def oracle_logits(o64, s: torch.Tensor, rows: np.ndarray, n: int) -> np.ndarray:
    """float64 logits [R, W-1, V] of the rows, teacher-forced (causal: a position sees its own prefix alone)."""
    with torch.no_grad():
        return o64(s.repeat_interleave(n, 0), torch.from_numpy(rows[:, :-1])).numpy()


def oracle_mean_prob(o64, s, keys, n, T, max_len) -> float:
    """Mean probability of the emitted token when the float64 oracle itself samples by the rule: the oracle alone decides T."""
    R = s.shape[0] * n
    rows = np.full((R, max_len), PAD, dtype=np.int64)
    rows[:, 0] = BOS
    alive = np.ones(R, dtype=bool)
    p = S.Params(T, pad=PAD, eos=EOS)
    probs = []
    for pos in range(1, max_len):
        if not alive.any():
            break
        with torch.no_grad():
            lg = o64(s.repeat_interleave(n, 0), torch.from_numpy(rows[:, :pos]))[:, -1].numpy()
        u = S.uniform(SEED, np.repeat(keys, n), np.tile(np.arange(n), len(keys)), pos)
        for r in np.nonzero(alive)[0]:
            t = S.sample64(lg[r], u[r], p)
            y = S.scaled(lg[r], T)
            probs.append(float(np.exp(y[t] - y.max()) / np.exp(y - y.max()).sum()))
            rows[r, pos] = t
            alive[r] = t not in (PAD, EOS)
    return float(np.mean(probs))


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_replay_against_float64_oracle(tta, models, src, name):
    native, o64 = models[name]
    B, n, max_len = 4, 8, 32
    s = src[:B]
    keys = np.array([5, 1 << 40, 7, -3], dtype=np.int64)
    T = next((t for t in (1.0, 2.0, 4.0, 8.0) if oracle_mean_prob(o64, s, keys, n, t, max_len) < 0.4), None)
    assert T is not None, "the oracle's samples stay confident up to T = 8"
    out = sampler(tta, native, max_len, temperature=T, num_samples=n, seed=SEED).generate(s.cuda(), row_keys=keys).cpu().numpy()
    end = check_shape(out, B, n, max_len)
    rows = out.reshape(B * n, max_len)
    lg = oracle_logits(o64, s, rows, n)
    p, tol = S.Params(T, pad=PAD, eos=EOS), 2 * LOGIT_TOL / T + 1e-4
    probs, worst = [], 0.0
    for r in range(B * n):
        for pos in range(1, end[r] + 1):
            u = float(S.uniform(SEED, keys[r // n], r % n, pos))
            ex = S.excess(int(rows[r, pos]), lg[r, pos - 1], u, p)
            worst = max(worst, ex)
            assert ex <= tol, f"{name} row {r} position {pos}: token {rows[r, pos]} lies {ex:.3e} outside its interval (tol {tol:.3e})"
            y = S.scaled(lg[r, pos - 1], T)
            probs.append(float(np.exp(y[rows[r, pos]] - y.max()) / np.exp(y - y.max()).sum()))
    print(f"{name}: T {T}, {len(probs)} tokens, mean probability of the emitted token {np.mean(probs):.3f}, "
          f"distinct rows {len({tuple(r) for r in rows.tolist()})} of {B * n}, largest excess over the exact interval {worst:.3e}")
    assert np.mean(probs) < 0.5, "the check went soft: the sampled tokens are the confident ones"


# -- invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_invariance_is_exact(tta, models, src, name):
    native = models[name][0]
    max_len, T = 32, 2.0
    s = src[:4].cuda()
    make = lambda n, seed=SEED, **kw: sampler(tta, native, max_len, temperature=T, num_samples=n, seed=seed, **kw)
    full = make(8).generate(s, row_keys=[0, 1, 2, 3])
    assert torch.equal(make(8).generate(s), full)                                     # the default keys are 0..B-1
    assert torch.equal(make(8).generate(s, row_keys=[0, 1, 2, 3]), full)              # two calls
    g = make(8)
    assert torch.equal(g.generate(s, row_keys=[0, 1, 2, 3]), full) and torch.equal(g.generate(s, row_keys=[0, 1, 2, 3]), full)
    assert torch.equal(make(8).generate(s[1:3], row_keys=[1, 2]), full[1:3])          # a sub-batch under its own keys
    assert torch.equal(make(8).generate(s[3:4], row_keys=torch.tensor([3])), full[3:4])
    assert torch.equal(make(2).generate(s, row_keys=[0, 1, 2, 3]), full[:, :2])       # sample j does not depend on n
    wide = torch.cat([s, torch.full((4, 7), PAD, dtype=s.dtype, device=s.device)], 1)
    assert torch.equal(make(8).generate(wide, row_keys=[0, 1, 2, 3]), full)           # right-padded by 7 columns
    assert not torch.equal(make(8, seed=SEED + 1).generate(s, row_keys=[0, 1, 2, 3]), full)
    assert not torch.equal(make(8).generate(s, row_keys=[4, 5, 6, 7]), full)
    assert len({tuple(r) for r in full.reshape(32, max_len).tolist()}) > 8            # it does sample
    # the filtered path too
    f8 = make(8, top_k=32, top_p=0.9975).generate(s)
    assert torch.equal(make(2, top_k=32, top_p=0.9975).generate(s[1:3], row_keys=[1, 2]), f8[1:3, :2])
    assert torch.equal(make(8, top_p=0.9975).generate(s), f8)                         # top_p alone runs with top_k = 32


# -- shape of the output ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_output_shape_and_model_calls(tta, models, src, name):
    native = models[name][0]
    s = src[:3].cuda()
    for max_len in (2, 3, 16, 150):
        for kw in (dict(temperature=1.0), dict(temperature=4.0), dict(temperature=1.5, top_k=5, top_p=0.9)):
            g = sampler(tta, native, max_len, num_samples=4, seed=SEED + max_len, **kw)
            out = g.generate(s).cpu().numpy()
            end = check_shape(out, 3, 4, max_len)
            assert g.model_calls_num == int(end.max()), f"max_len {max_len} {kw}: {g.model_calls_num} steps, longest row {end.max()}"
    g = sampler(tta, native, 1, num_samples=2)
    assert g.generate(s).cpu().tolist() == [[[BOS]] * 2] * 3 and g.model_calls_num == 0
    assert "temperature" in str(g)


def test_score_runs_on_samples(tta, models, src):
    native = models["tiny"][0]
    s = src[:4].cuda()
    g = sampler(tta, native, 32, temperature=3.0, num_samples=8, seed=SEED)
    out, sc = g.generate(s, return_scores=True)
    assert sc.score.shape == (4, 8) and bool(torch.isfinite(sc.score).all())
    rows = out.cpu().numpy().reshape(32, 32)
    end = S.ends(rows, PAD, EOS)
    by_pad = rows[np.arange(32), end] == PAD                   # a row a sampled PAD ended: score() counts its tokens before the PAD
    assert sc.length.cpu().numpy().reshape(32).tolist() == (end - by_pad).tolist()
    assert sc.finished.cpu().numpy().reshape(32).tolist() == (rows[np.arange(32), end] == EOS).tolist()
    from translation_transformer_amd.scoring import unique_samples
    uniq = unique_samples(out, sc)
    assert len(uniq) == 4 and all(sum(c for _, c, _ in per) == 8 for per in uniq)
    assert all(per == sorted(per, key=lambda e: -e[2]) for per in uniq)
    assert g.alternatives(s, out, k=3).top_id.shape[:2] == (4, 8) and g.attention(s, out).attn.shape[:2] == (4, 8)


# -- refused arguments -----------------------------------------------------------------------------------------------------------
def test_refused_arguments(tta, models, src):
    from translation_transformer_amd._native import TtxError
    from util_models import seeded_weights, state_shapes
    native = models["tiny"][0]
    s = src[:2].cuda()
    bad = [dict(num_samples=0), dict(num_samples=-1), dict(temperature=-0.5), dict(temperature=float("nan")),
           dict(temperature=float("inf")), dict(top_k=-1), dict(top_k=33), dict(top_p=0.0), dict(top_p=-1.0), dict(top_p=1.01),
           dict(top_p=float("nan")), dict(max_len=0), dict(max_len=4999), dict(pad_token=3)]
    for kw in bad:
        a = dict(max_len=16, pad_token=PAD, bos_token=BOS, eos_token=EOS)
        a.update(kw)
        with pytest.raises(TtxError):
            tta.TranslationInferenceSampling(native, **a).generate(s)
    with pytest.raises(ValueError):
        sampler(tta, native).generate(s, row_keys=[1, 2, 3])
    with pytest.raises(TypeError):
        tta.TranslationInferenceSampling(object(), 16, PAD, BOS, EOS)
    V = 1030
    w = seeded_weights(state_shapes(V, 64, 64, 1, 1), 7)
    w["tgt_token_featurizer.embedding.weight"] = w["src_token_featurizer.embedding.weight"]
    big = tta.NativeTransformer(w, 2, PAD, device=0)
    with pytest.raises(TtxError, match="1024"):
        sampler(tta, big, 8).generate(s)
    assert tta.TranslationInferenceGreedy(big, 8, PAD, BOS, EOS).generate(s).shape == (2, 1, 8)      # greedy has no such limit
    assert sampler(tta, native, 8).generate(s).shape == (2, 1, 8)                                    # and the session still works


# -- Lightning -------------------------------------------------------------------------------------------------------------------
def test_lightning_sampling_does_not_depend_on_the_batch_size(tta, tmp_path):
    from test_gpu_lightning_surface import FixtureTokenizer, CsvWriter
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    src, tgt, _, _ = fixture_tokens()
    texts, preds = {}, {}
    for bs in (1, 4):
        report = tmp_path / f"r{bs}.txt"
        mod = tta.VanillaEncoderDecoderTransformerLightning(
            src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
            num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
            share_embeddings=True, generation="sampling", beam_size=3, max_len=40, sampling_temperature=2.0, sampling_top_k=8,
            sampling_top_p=0.95, sampling_seed=11, report_prediction_file=str(report))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        batches = [{"src_tokens": src[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda()} for i in range(0, 4, bs)]
        csv = tmp_path / f"pred{bs}.csv"
        outs = tta.run_predict(mod, batches, writer=CsvWriter(csv))
        preds[bs] = torch.cat(outs, 0)
        texts[bs] = csv.read_text()
        rep = json.loads(report.read_text().strip().split("\n")[-1])
        assert rep["algorithm"] == "sampling" and rep["model_calls"] > 0
    assert preds[1].shape == (4, 3, 40) and torch.equal(preds[1], preds[4]) and texts[1] == texts[4]
    assert len({tuple(r) for r in preds[4].reshape(12, 40).tolist()}) > 4
    with pytest.raises(ValueError):
        tta.VanillaEncoderDecoderTransformerLightning(src_tokenizer=tkz, tgt_tokenizer=tkz, generation="nucleus")
