"""TranslationInferenceSamplingSpeculative (ttx_sample_speculative_generate) end to end, on the tiny golden model and on the
four-head model of tests/golden/h4_*: greedy settings against TranslationInferenceGreedySpeculative (tokens and accepted tokens), a
replay of every token against the float64 oracle at two temperatures, the plain sampler under the same seed and keys, exact
invariance under batching at a fixed (n_drafts, draft_len), the shape of the output, score(), refused arguments and Lightning.

The replay is tests/test_gpu_sampling.py's, with its tolerance tol = 2 delta / T + 1e-4 (delta = LOGIT_TOL, the bound the GPU's
logits are held to against the float64 oracle; the verify step's logits are held to it by tests/test_gpu_spec_greedy.py).  The
temperatures are chosen by the float64 oracle alone: the first is the one at which its own samples stop being confident; the second
is the largest of 1, 0.5, 0.25 at which its own keyed samples, walked on the CPU against the copy drafts of oracle/drafting.py,
accept at least one draft token, so that the accept path runs with real acceptance there.
"""
import json

import numpy as np
import pytest
import torch

import util_sample_checks as S
from oracle.drafting import make_drafts
from test_gpu_model import LOGIT_TOL
from test_gpu_sampling import SEED, check_shape, oracle_logits, oracle_mean_prob, states
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
N_DRAFTS, DRAFT_LEN = 3, 4
KEYS = np.array([5, 1 << 40, 7, -3], dtype=np.int64)


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


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
def c_token():
    return fixture_tokens()[2]


def spec(tta, native, c, max_len=32, n_drafts=N_DRAFTS, draft_len=DRAFT_LEN, **kw):
    return tta.TranslationInferenceSamplingSpeculative(native, max_len, draft_len, n_drafts, PAD, BOS, EOS, c, **kw)


# -- greedy settings -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_greedy_settings_equal_greedy_speculative(tta, models, src, c_token, name):
    native = models[name][0]
    B, n, max_len = 4, 8, 150
    s = src[:B].cuda()
    gs = tta.TranslationInferenceGreedySpeculative(native, max_len, DRAFT_LEN, N_DRAFTS, PAD, BOS, EOS, c_token)
    ref = gs.generate(s.repeat_interleave(n, 0)).cpu().numpy()[:, 0]            # the same rows repeated
    ref_end = S.ends(ref, PAD, EOS)
    assert (ref[np.arange(B * n), ref_end] == EOS).all(), "a fixture row does not end by EOS: the comparison needs a larger max_len"
    assert gs.stats_total["accepted_tokens"] > 0
    for kw in (dict(top_k=1), dict(temperature=0.0), dict(temperature=0.5, top_k=1, top_p=0.5)):
        g = spec(tta, native, c_token, max_len, num_samples=n, seed=SEED, **kw)
        out = g.generate(s).cpu().numpy()
        end = check_shape(out, B, n, max_len)
        rows = out.reshape(B * n, max_len)
        for r in range(B * n):
            e = ref_end[r]
            assert end[r] == e and (rows[r, :e + 1] == ref[r, :e + 1]).all(), \
                f"{name} {kw} row {r}: {rows[r].tolist()} against greedy speculative {ref[r].tolist()}"
        assert g.accepted_tokens_num == gs.stats_total["accepted_tokens"], f"{name} {kw}: accepted tokens"
        assert g.stats_total["produced_tokens"] == int(ref_end.sum()) and g.model_calls_num == gs.model_calls_num


# -- replay against the float64 oracle -------------------------------------------------------------------------------------------
def oracle_rows(o64, s, keys, n, T, max_len) -> np.ndarray:
    """[R, max_len]: the float64 oracle sampling by the rule, position by position."""
    R = s.shape[0] * n
    rows = np.full((R, max_len), PAD, dtype=np.int64)
    rows[:, 0] = BOS
    alive = np.ones(R, dtype=bool)
    p = S.Params(T, pad=PAD, eos=EOS)
    for pos in range(1, max_len):
        if not alive.any():
            break
        with torch.no_grad():
            lg = o64(s.repeat_interleave(n, 0), torch.from_numpy(rows[:, :pos]))[:, -1].numpy()
        u = S.uniform(SEED, np.repeat(keys, n), np.tile(np.arange(n), len(keys)), pos)
        for r in np.nonzero(alive)[0]:
            rows[r, pos] = S.sample64(lg[r], u[r], p)
            alive[r] = rows[r, pos] not in (PAD, EOS)
    return rows


def oracle_accepted(rows: np.ndarray, drafts: np.ndarray, n: int) -> int:
    """Draft tokens the speculative loop accepts when its draws are ``rows``: per row, from front f, the longest leading run of a
    draft equal to rows[f + 1 ..]; the front moves by that run plus one."""
    total = 0
    end = S.ends(rows, PAD, EOS)
    for r, row in enumerate(rows):
        f = 0
        while f < end[r]:
            best = 0
            for d in drafts[r // n]:
                a = 0
                while a < len(d) and f + 1 + a <= end[r] and row[f + 1 + a] == d[a]:
                    a += 1
                best = max(best, a)
            total += best
            f += best + 1
    return total


def replay(name, o64, s, out, T, n, max_len):
    rows = out.reshape(-1, max_len)
    end = S.ends(rows, PAD, EOS)
    lg = oracle_logits(o64, s, rows, n)
    p, tol = S.Params(T, pad=PAD, eos=EOS), 2 * LOGIT_TOL / T + 1e-4
    worst, probs = 0.0, []
    for r in range(len(rows)):
        for pos in range(1, end[r] + 1):
            u = float(S.uniform(SEED, KEYS[r // n], r % n, pos))
            ex = S.excess(int(rows[r, pos]), lg[r, pos - 1], u, p)
            worst = max(worst, ex)
            assert ex <= tol, f"{name} T {T} row {r} position {pos}: token {rows[r, pos]} lies {ex:.3e} outside its interval (tol {tol:.3e})"
            y = S.scaled(lg[r, pos - 1], T)
            probs.append(float(np.exp(y[rows[r, pos]] - y.max()) / np.exp(y - y.max()).sum()))
    return worst, float(np.mean(probs)), lg, end


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_replay_against_float64_oracle_and_the_plain_sampler(tta, models, src, c_token, name):
    native, o64 = models[name]
    B, n, max_len = 4, 8, 32
    s = src[:B]
    drafts = make_drafts(s[:, 1:].numpy(), DRAFT_LEN, N_DRAFTS, 1, max_len, EOS, PAD, c_token)
    T_hot = next((t for t in (1.0, 2.0, 4.0, 8.0) if oracle_mean_prob(o64, s, KEYS, n, t, max_len) < 0.4), None)
    assert T_hot is not None, "the oracle's samples stay confident up to T = 8"
    T_acc = next((t for t in (1.0, 0.5, 0.25) if oracle_accepted(oracle_rows(o64, s, KEYS, n, t, max_len), drafts, n) > 0), None)
    assert T_acc is not None, "the oracle's own samples accept no draft token down to T = 0.25"
    for T in (T_hot, T_acc):
        g = spec(tta, native, c_token, max_len, temperature=T, num_samples=n, seed=SEED)
        out = g.generate(s.cuda(), row_keys=KEYS).cpu().numpy()
        check_shape(out, B, n, max_len)
        worst, mean_p, lg, end = replay(name, o64, s, out, T, n, max_len)
        print(f"{name}: T {T}: mean probability of the emitted token {mean_p:.3f}, largest excess {worst:.3e}, accepted "
              f"{g.accepted_tokens_num} of {g.stats_total['produced_tokens']} produced tokens in {g.model_calls_num} steps "
              f"(longest row {int(end.max())})")
        if T == T_hot:
            assert mean_p < 0.5, "the check went soft: the sampled tokens are the confident ones"
        if T == T_acc:
            assert g.accepted_tokens_num > 0, "no draft token was accepted where the oracle's own samples accept some"
        # against the plain sampler under the same seed and keys: equal rows, or a near-boundary draw at the first difference
        plain = tta.TranslationInferenceSampling(native, max_len, PAD, BOS, EOS, temperature=T, num_samples=n, seed=SEED) \
            .generate(s.cuda(), row_keys=KEYS).cpu().numpy().reshape(B * n, max_len)
        rows = out.reshape(B * n, max_len)
        p, tol = S.Params(T, pad=PAD, eos=EOS), 2 * LOGIT_TOL / T + 1e-4
        near = 0
        for r in range(B * n):
            diff = np.nonzero(rows[r] != plain[r])[0]
            if len(diff) == 0:
                continue
            pos = int(diff[0])
            assert 1 <= pos <= end[r], f"{name} T {T} row {r}: the rows differ behind the row's end"
            u = float(S.uniform(SEED, KEYS[r // n], r % n, pos))
            for tok in (rows[r, pos], plain[r, pos]):
                assert S.consistent(int(tok), lg[r, pos - 1], u, p, tol), \
                    f"{name} T {T} row {r} position {pos}: {rows[r, pos]} against the plain sampler's {plain[r, pos]}: not a near-boundary draw"
            near += 1
        print(f"{name}: T {T}: {near} of {B * n} rows differ from the plain sampler's by a near-boundary draw")


# -- invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_invariance_is_exact(tta, models, src, c_token, name):
    """At the temperature of tests/test_gpu_sampling.py's invariance test, with its bar of more than 8 distinct rows among the 32
    (at lower temperatures these models are so confident that another seed gives the same rows)."""
    native = models[name][0]
    max_len, T = 32, 2.0
    s = src[:4].cuda()
    make = lambda n, seed=SEED, **kw: spec(tta, native, c_token, max_len, temperature=T, num_samples=n, seed=seed, **kw)
    full = make(8).generate(s, row_keys=[0, 1, 2, 3])
    assert torch.equal(make(8).generate(s), full)                                     # the default keys are 0..B-1
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
    f8 = make(8, top_k=32, top_p=0.9975).generate(s)                                  # the filtered path too
    assert torch.equal(make(2, top_k=32, top_p=0.9975).generate(s[1:3], row_keys=[1, 2]), f8[1:3, :2])
    assert torch.equal(make(8, top_p=0.9975).generate(s), f8)


# -- shape of the output ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_output_shape_and_counters(tta, models, src, c_token, name):
    native = models[name][0]
    s = src[:3].cuda()
    for N, D in ((N_DRAFTS, DRAFT_LEN), (1, 1), (5, 10)):
        for max_len in (1, 2, 3, D + 1, 16):
            if D > max_len:
                continue
            for kw in (dict(temperature=1.0), dict(temperature=4.0), dict(temperature=0.5, top_k=5, top_p=0.9)):
                g = spec(tta, native, c_token, max_len, N, D, num_samples=4, seed=SEED + max_len, **kw)
                out = g.generate(s).cpu().numpy()
                if max_len == 1:                                          # BOS alone, as the plain sampler writes it; no decoder pass
                    assert out.tolist() == [[[BOS]] * 4] * 3 and g.model_calls_num == 0 and g.last_stats.produced_tokens == 0
                    continue
                end = check_shape(out, 3, 4, max_len)
                st = g.last_stats
                what = f"{name} N {N} D {D} max_len {max_len} {kw}"
                assert g.model_calls_num <= int(end.max()), f"{what}: {g.model_calls_num} steps, longest row {end.max()}"
                assert g.model_calls_num >= 1 and st.produced_tokens - st.accepted_tokens >= 12 and st.src_tokens_padded == 3 * s.shape[1], what
                assert st.produced_tokens >= int(end.sum()), what           # tokens of dropped columns are counted too
    assert spec(tta, native, c_token, 1, 1, 1, num_samples=2).generate(s).cpu().tolist() == [[[BOS]] * 2] * 3
    assert "draft_len" in str(g) and "temperature" in str(g)


def test_score_runs_on_samples(tta, models, src, c_token):
    native = models["tiny"][0]
    s = src[:4].cuda()
    g = spec(tta, native, c_token, 32, temperature=2.0, num_samples=8, seed=SEED)
    out, sc = g.generate(s, return_scores=True)
    assert sc.score.shape == (4, 8) and bool(torch.isfinite(sc.score).all())
    rows = out.cpu().numpy().reshape(32, 32)
    end = S.ends(rows, PAD, EOS)
    by_pad = rows[np.arange(32), end] == PAD
    assert sc.length.cpu().numpy().reshape(32).tolist() == (end - by_pad).tolist()
    assert g.alternatives(s, out, k=3).top_id.shape[:2] == (4, 8) and g.attention(s, out).attn.shape[:2] == (4, 8)


# -- refused arguments -----------------------------------------------------------------------------------------------------------
def test_refused_arguments(tta, models, src, c_token):
    from translation_transformer_amd._native import TtxError
    native = models["tiny"][0]
    s = src[:2].cuda()
    bad = [dict(num_samples=0), dict(num_samples=-1), dict(temperature=-0.5), dict(temperature=float("nan")),
           dict(temperature=float("inf")), dict(top_k=-1), dict(top_k=33), dict(top_p=0.0), dict(top_p=-1.0), dict(top_p=1.01),
           dict(top_p=float("nan")), dict(max_len=0), dict(max_len=4999), dict(pad_token=3),
           dict(n_drafts=0), dict(n_drafts=-2), dict(draft_len=0), dict(draft_len=17), dict(replace_token=PAD), dict(replace_token=EOS),
           dict(eos_token=PAD), dict(max_len=4990, draft_len=10)]
    for kw in bad:
        a = dict(max_len=16, draft_len=4, n_drafts=3, pad_token=PAD, bos_token=BOS, eos_token=EOS, replace_token=c_token)
        a.update(kw)
        with pytest.raises(TtxError) as e:
            tta.TranslationInferenceSamplingSpeculative(native, **a).generate(s)
        assert e.value.code == -1, f"{kw}: code {e.value.code}"
    with pytest.raises(ValueError):
        spec(tta, native, c_token).generate(s, row_keys=[1, 2, 3])
    with pytest.raises(TtxError):
        spec(tta, native, c_token).generate(s[:, :1])
    assert spec(tta, native, c_token, 8).generate(s).shape == (2, 1, 8)                  # and the session still works


# -- Lightning -------------------------------------------------------------------------------------------------------------------
def test_lightning_does_not_depend_on_the_batch_size(tta, tmp_path):
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
            share_embeddings=True, generation="sampling_speculative", beam_size=3, max_len=40, draft_len=4, n_drafts=3,
            sampling_temperature=2.0, sampling_top_k=8, sampling_top_p=0.95, sampling_seed=11, report_prediction_file=str(report))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        batches = [{"src_tokens": src[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda()} for i in range(0, 4, bs)]
        csv = tmp_path / f"pred{bs}.csv"
        outs = tta.run_predict(mod, batches, writer=CsvWriter(csv))
        preds[bs] = torch.cat(outs, 0)
        texts[bs] = csv.read_text()
        rep = json.loads(report.read_text().strip().split("\n")[-1])
        assert rep["algorithm"] == "sampling_speculative" and rep["model_calls"] > 0 and rep["draft_len"] == 4
    assert preds[1].shape == (4, 3, 40) and torch.equal(preds[1], preds[4]) and texts[1] == texts[4]
    assert len({tuple(r) for r in preds[4].reshape(12, 40).tolist()}) > 4
