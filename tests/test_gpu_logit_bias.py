"""Per-source logit bias and token allow-lists end to end (include/ttx.h "Per-source logit bias"): the plain and the speculative
sampler, the sampling pool, stochastic beam search and log q, on the tiny golden model (2 heads) and the four-head model of
tests/golden/h4_* (whose pool steps run the probe and the compacted draft pass under draft select), the ten fixture sources,
max_len 32.

The bias of the tests (``make_bias``, chosen on the CPU): every source may emit the tokens that occur in it plus a few structure
tokens and EOS, never BOS or PAD (``scoring.allowlist_from_source``), and the allowed tokens carry nudges from {+-0.0, +-0.5,
+-2, +-8, 1.25}, drawn per source, so the ten bias rows differ.  |bias| <= 8, so the one extra fp32 rounding of the biased logit
(at most 2^-24 * 16 ~ 1e-6 for logits of this size) stays three orders below LOGIT_TOL.

Tolerances are those of the tests this file extends.  Replay of sampled tokens: tests/test_gpu_sampling.py's interval test on the
float64 oracle's logits PLUS THE BIAS, tol = 2 * LOGIT_TOL / T + 1e-4.  Temperature 0: the token is the first maximum of the biased
float64 logits wherever the top two are at least 2 * LOGIT_TOL apart; at most a tenth of the positions may be closer (an
assertion on the oracle alone).  token_logq: tests/test_gpu_logq.py's TOK_TOL * max(1, max |ref|) * max(1, 1 / T).  Stochastic
beam search: tests/test_gpu_sbs_mask.py's level-by-level replay with both oracles returning biased logits.  Everything else is
equality on the bits.
"""
import numpy as np
import pytest
import torch

import test_gpu_sbs_mask as TM
import util_logq_checks as Q
import util_sample_checks as S
from test_gpu_model import LOGIT_TOL
from test_gpu_sampling import check_shape, oracle_logits, states
from test_gpu_score import TOK_TOL
from util_models import fixture_tokens, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
SEED = 20261020
MAX_LEN = 32
T = 2.0
ALWAYS = [EOS, 4, 6, 7, 8]                    # frequent structure tokens of the fixture vocabulary
NUDGES = np.array([0.0, 0.0, 0.0, -0.0, 0.5, -0.5, 2.0, -2.0, 8.0, -8.0, 1.25], dtype=np.float32)
NAMES = ["tiny", "h4"]


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def models(tta):
    """name -> (NativeTransformer, float64 oracle, fp32 oracle), built once."""
    from oracle.model import OracleTransformer, config_from_state
    out = {}
    for name in NAMES:
        st, cfg = states(name)
        c = config_from_state(st, cfg["num_heads"])
        out[name] = (tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0), OracleTransformer(c, st, dtype=torch.float64),
                     OracleTransformer(c, st))
    return out


@pytest.fixture(scope="module")
def src():
    s = fixture_tokens()[0]
    return s[:, :int((s != PAD).sum(1).max())]


@pytest.fixture(scope="module")
def c_token():
    return fixture_tokens()[2]


def make_allowed(src: torch.Tensor, V: int) -> torch.Tensor:
    from translation_transformer_amd.scoring import allowlist_from_source
    allowed = allowlist_from_source(src, ALWAYS, V, PAD)
    allowed[:, BOS] = False                   # every source row begins with BOS; no target holds one after column 0
    return allowed


def make_bias(src: torch.Tensor, V: int, seed: int = 3) -> torch.Tensor:
    allowed = make_allowed(src, V)
    rng = np.random.default_rng(seed)
    nudge = torch.from_numpy(NUDGES[rng.integers(0, len(NUDGES), size=tuple(allowed.shape))])
    return torch.where(allowed, nudge, torch.full_like(nudge, float("-inf")))


@pytest.fixture(scope="module")
def bias(src):
    V = int(fixture_tokens()[3])
    b = make_bias(src, V)
    assert bool(torch.isinf(b).any(1).all()) and len({tuple(r) for r in b.tolist()}) == 10 and float(b[torch.isfinite(b)].abs().max()) == 8.0
    return b


def plain(tta, native, **kw):
    kw.setdefault("temperature", T)
    kw.setdefault("seed", SEED)
    return tta.TranslationInferenceSampling(native, MAX_LEN, PAD, BOS, EOS, **kw)


def spec(tta, native, c, **kw):
    kw.setdefault("temperature", T)
    kw.setdefault("seed", SEED)
    return tta.TranslationInferenceSamplingSpeculative(native, MAX_LEN, 4, 3, PAD, BOS, EOS, c, **kw)


def sbs(tta, native, K, **kw):
    kw.setdefault("temperature", TM.T)
    return tta.TranslationInferenceStochasticBeamSearch(native, K, MAX_LEN, PAD, BOS, EOS, seed=TM.SEED, **kw)


def forbidden_used(out: torch.Tensor, b: torch.Tensor) -> list:
    """(source, sample, position, token) of every emitted token (columns 1 .. the row's end) whose bias is -inf."""
    rows = out.cpu().numpy()
    B, n, L = rows.shape
    end = S.ends(rows.reshape(B * n, L), PAD, EOS).reshape(B, n)
    bad = []
    for s in range(B):
        for j in range(n):
            for pos in range(1, end[s, j] + 1):
                if b[s, rows[s, j, pos]] == float("-inf"):
                    bad.append((s, j, pos, int(rows[s, j, pos])))
    return bad


def signed_zeros(B: int, V: int) -> torch.Tensor:
    z = torch.zeros(B, V)
    z[:, ::3] = -0.0
    return z


# -- exactness -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_no_bias_and_a_zero_bias_are_the_unbiased_call(tta, models, src, c_token, name):
    native = models[name][0]
    s, V = src[:4].cuda(), native.tgt_vocab_size
    zero = signed_zeros(4, V)
    everything = torch.ones(4, V, dtype=torch.bool)
    for make in (lambda: plain(tta, native, num_samples=3), lambda: spec(tta, native, c_token, num_samples=3),
                 lambda: plain(tta, native, num_samples=2, top_k=8, top_p=0.9), lambda: plain(tta, native, temperature=0.0)):
        base = make().generate(s)
        assert torch.equal(make().generate(s, logit_bias=None, allowed=None), base)
        assert torch.equal(make().generate(s, logit_bias=zero), base), f"{name}: an all-zero bias changed a token"
        assert torch.equal(make().generate(s, allowed=everything), base) and torch.equal(make().generate(s, logit_bias=zero.cuda(), allowed=everything), base)
    batches = [s[:2], s[2:]]
    pool = spec(tta, native, c_token, num_samples=3).generate_many(batches)
    for kw in (dict(logit_biases=None), dict(logit_biases=[None, None]), dict(logit_biases=[zero[:2], None]), dict(allowed=[None, everything[2:]])):
        got = spec(tta, native, c_token, num_samples=3).generate_many(batches, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, pool)), f"{name}: generate_many with {list(kw)}"
    ob, db = sbs(tta, native, 5).generate(s, row_keys=TM.KEYS, return_details=True)
    for kw in (dict(logit_bias=None), dict(logit_bias=zero), dict(allowed=everything)):
        o, d = sbs(tta, native, 5).generate(s, row_keys=TM.KEYS, return_details=True, **kw)
        assert torch.equal(o, ob) and torch.equal(d.logp, db.logp) and torch.equal(d.gumbel, db.gumbel), f"{name}: stochastic beam search with {list(kw)}"


def test_an_unbiased_call_launches_no_bias_kernel(tta, src, bias, c_token):
    st, cfg = states("tiny")
    fresh = tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0)       # sessions that have served no call yet
    s = src[:4].cuda()
    for _ in range(3):                                                        # eager, captured, replayed
        plain(tta, fresh).generate(s)
        spec(tta, fresh, c_token).generate(s)
    spec(tta, fresh, c_token).generate_many([s[:2], s[2:]])
    sbs(tta, fresh, 3).generate(s)
    assert fresh.kernel_profile()["logit_bias_launches"] == 0, "an unbiased call launched k_logit_bias"
    unbiased = plain(tta, fresh).generate(s)
    biased = plain(tta, fresh).generate(s, logit_bias=bias[:4])
    n = fresh.kernel_profile()["logit_bias_launches"]
    assert n > 0 and not torch.equal(biased, unbiased)
    # and a biased step is never replayed for an unbiased call, nor the other way round: alternate them on one session
    for _ in range(3):
        assert torch.equal(plain(tta, fresh).generate(s), unbiased) and torch.equal(plain(tta, fresh).generate(s, logit_bias=bias[:4]), biased)


# -- support -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_no_forbidden_token_is_emitted(tta, models, src, bias, c_token, name):
    native = models[name][0]
    s = src.cuda()
    allowed = torch.isfinite(bias)
    for what, g, kw in (("plain", plain(tta, native, num_samples=4), dict(logit_bias=bias)),
                        ("plain, allow-list", plain(tta, native, num_samples=4, temperature=4.0), dict(allowed=allowed)),
                        ("plain, filtered", plain(tta, native, num_samples=4, top_k=8, top_p=0.9), dict(logit_bias=bias)),
                        ("speculative", spec(tta, native, c_token, num_samples=4), dict(logit_bias=bias)),
                        ("greedy", plain(tta, native, temperature=0.0), dict(allowed=allowed))):
        out = g.generate(s, **kw)
        check_shape(out.cpu().numpy(), 10, g.num_samples, MAX_LEN)           # BOS, tokens, the first EOS or PAD, PAD after
        assert forbidden_used(out, bias) == [], f"{name} {what}"
    free = plain(tta, native, num_samples=4, temperature=4.0).generate(s)
    assert forbidden_used(free, bias), "the unconstrained sampler never leaves the allow-list: the check shows nothing"


@pytest.mark.parametrize("name", NAMES)
def test_with_eos_forbidden_every_row_runs_to_max_len(tta, models, src, bias, c_token, name):
    native = models[name][0]
    b = bias[:4].clone()
    b[:, EOS] = float("-inf")                                                # PAD is forbidden already
    for g in (plain(tta, native, num_samples=3), spec(tta, native, c_token, num_samples=3), plain(tta, native, temperature=0.0)):
        out = g.generate(src[:4].cuda(), logit_bias=b).cpu().numpy()
        assert (out[:, :, 0] == BOS).all() and not np.isin(out[:, :, 1:], (PAD, EOS, BOS)).any(), f"{name}: a row ended before max_len"
        assert forbidden_used(torch.from_numpy(out), b) == []


# -- the float64 oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_replay_of_sampled_tokens_against_the_biased_oracle(tta, models, src, bias, name):
    native, o64, _ = models[name]
    B, n = 4, 8
    s, b64 = src[:B], bias[:B].numpy().astype(np.float64)
    keys = np.array([5, 1 << 40, 7, -3], dtype=np.int64)
    out = plain(tta, native, num_samples=n).generate(s.cuda(), row_keys=keys, logit_bias=bias[:B]).cpu().numpy()
    end = check_shape(out, B, n, MAX_LEN)
    rows = out.reshape(B * n, MAX_LEN)
    lg = oracle_logits(o64, s, rows, n) + np.repeat(b64, n, axis=0)[:, None, :]
    p, tol = S.Params(T, pad=PAD, eos=EOS), 2 * LOGIT_TOL / T + 1e-4
    worst, probs = 0.0, []
    for r in range(B * n):
        for pos in range(1, end[r] + 1):
            u = float(S.uniform(SEED, keys[r // n], r % n, pos))
            ex = S.excess(int(rows[r, pos]), lg[r, pos - 1], u, p)
            worst = max(worst, ex)
            assert ex <= tol, f"{name} row {r} position {pos}: token {rows[r, pos]} lies {ex:.3e} outside its interval (tol {tol:.3e})"
            y = S.scaled(lg[r, pos - 1], T)
            probs.append(float(np.exp(y[rows[r, pos]] - y.max()) / np.exp(y - y.max()).sum()))
    print(f"{name}: {len(probs)} tokens, mean probability of the emitted token {np.mean(probs):.3f}, distinct rows "
          f"{len({tuple(r) for r in rows.tolist()})} of {B * n}, largest excess over the exact interval {worst:.3e}")
    assert np.mean(probs) < 0.6 and len({tuple(r) for r in rows.tolist()}) > B, "the check went soft: the sampler hardly samples"


@pytest.mark.parametrize("name", NAMES)
def test_temperature_0_is_the_argmax_over_the_allowed_set(tta, models, src, bias, c_token, name):
    native, o64, _ = models[name]
    allowed = torch.isfinite(bias)
    out = plain(tta, native, temperature=0.0).generate(src.cuda(), allowed=allowed)
    assert torch.equal(spec(tta, native, c_token, temperature=0.0).generate(src.cuda(), allowed=allowed), out)
    rows = out.cpu().numpy()[:, 0]
    end = S.ends(rows, PAD, EOS)
    lg = oracle_logits(o64, src, rows, 1)
    lg = np.where(allowed.numpy()[:, None, :], lg, -np.inf)
    total = close = 0
    for r in range(10):
        for pos in range(1, end[r] + 1):
            x = lg[r, pos - 1]
            top = np.sort(x)[-2:]
            total += 1
            if top[1] - top[0] < 2 * LOGIT_TOL:
                close += 1
                continue
            assert rows[r, pos] == S.argmax_first(x), f"{name} source {r} position {pos}: {rows[r, pos]}, the allowed argmax is {S.argmax_first(x)}"
    print(f"{name}: {total} positions, {close} with the top two allowed logits closer than 2 * LOGIT_TOL")
    assert total > 100 and close <= total / 10
    free = plain(tta, native, temperature=0.0).generate(src.cuda())
    assert not torch.equal(free, out), "the allow-list changes no greedy token: the check shows nothing"


# -- invariance, bit for bit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_invariance_is_exact(tta, models, src, bias, c_token, name):
    native = models[name][0]
    s = src.cuda()
    keys = list(range(10))
    g = plain(tta, native, num_samples=4)
    full = g.generate(s, row_keys=keys, logit_bias=bias)
    assert torch.equal(g.generate(s, row_keys=keys, logit_bias=bias), full) and torch.equal(g.generate(s, row_keys=keys, logit_bias=bias), full)
    for b in (0, 3, 9):                      # a source alone against the same source among nine that carry other bias rows
        n = int((src[b] != PAD).sum())
        alone = plain(tta, native, num_samples=4).generate(s[b:b + 1, :n], row_keys=[b], logit_bias=bias[b:b + 1])
        assert torch.equal(alone, full[b:b + 1]), f"{name}: source {b} alone"
    assert torch.equal(plain(tta, native, num_samples=1).generate(s, row_keys=keys, logit_bias=bias), full[:, :1])
    wide = torch.nn.functional.pad(s, (0, 7), value=PAD)
    assert torch.equal(plain(tta, native, num_samples=4).generate(wide, row_keys=keys, logit_bias=bias.cuda()), full)
    strided = torch.zeros(10, bias.shape[1] + 3)                              # a bias that arrives as a view: it is made contiguous
    strided[:, :bias.shape[1]] = bias
    assert torch.equal(plain(tta, native, num_samples=4).generate(s, row_keys=keys, logit_bias=strided[:, :bias.shape[1]]), full)
    other = bias.roll(1, 0)
    assert not torch.equal(plain(tta, native, num_samples=4).generate(s, row_keys=keys, logit_bias=other), full)
    # the speculative sampler: the plain one's rows under the same bias, run to run, with a prefix, with a proposal of forbidden tokens
    sp = spec(tta, native, c_token, num_samples=4)
    assert torch.equal(sp.generate(s, row_keys=keys, logit_bias=bias), full), f"{name}: speculative against plain"
    assert torch.equal(sp.generate(s, row_keys=keys, logit_bias=bias), full) and torch.equal(sp.generate(s, row_keys=keys, logit_bias=bias), full)
    assert torch.equal(spec(tta, native, c_token, num_samples=1).generate(s[2:5], row_keys=keys[2:5], logit_bias=bias[2:5]), full[2:5, :1])
    junk = torch.full((10, 12), BOS, dtype=torch.int64)                       # BOS is forbidden for every source
    junk[:, 1::2] = full[:, 0, 2:13:2].cpu()
    junk[junk == PAD] = BOS
    assert torch.equal(spec(tta, native, c_token, num_samples=4).generate(s, row_keys=keys, logit_bias=bias, proposal=junk), full)
    good = full[:, 0, 1:].cpu()                                               # the first sample of every source as its proposal
    assert torch.equal(spec(tta, native, c_token, num_samples=4).generate(s, row_keys=keys, logit_bias=bias, proposal=good), full)
    pre = full[:, 1, 1:4].cpu().clone()                                       # three tokens of another sample, then a forbidden one
    pre[pre == EOS] = 5
    pre[pre == PAD] = 5
    pre = torch.cat([pre, torch.full((10, 1), BOS)], 1)
    a = plain(tta, native, num_samples=4).generate(s, row_keys=keys, logit_bias=bias, prefix=pre)
    assert torch.equal(a[:, :, 1:5].cpu(), pre[:, None, :].expand(10, 4, 4)), "a forced prefix position obeys the prefix, not the bias"
    assert torch.equal(spec(tta, native, c_token, num_samples=4).generate(s, row_keys=keys, logit_bias=bias, prefix=pre), a)
    rows = a.cpu().numpy().reshape(40, MAX_LEN)
    for r, e in enumerate(S.ends(rows, PAD, EOS)):
        assert bool(torch.isfinite(bias[r // 4, rows[r, 5:e + 1]]).all()), f"{name}: row {r}: the completion left the allow-list"


@pytest.mark.parametrize("name", NAMES)
def test_generate_many_equals_the_per_batch_calls(tta, models, src, bias, c_token, name, monkeypatch):
    native = models[name][0]
    sizes, offs = [4, 4, 2], [0, 4, 8]
    batches = [src[o:o + n, :max(2, int((src[o:o + n] != PAD).sum(1).max()))].cuda() for o, n in zip(offs, sizes)]
    biases = [bias[o:o + n] for o, n in zip(offs, sizes)]

    def per_batch(bs, n_samples=1):
        return [spec(tta, native, c_token, num_samples=n_samples).generate(x, row_keys=torch.arange(o, o + n), logit_bias=b)
                for x, o, n, b in zip(batches, offs, sizes, bs)]

    def same(what, got, want):
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), f"{name}: {what}"

    want = per_batch(biases)
    many = lambda **kw: spec(tta, native, c_token, num_samples=1).generate_many(batches, logit_biases=biases, **kw)
    same("default capacity", many(), want)
    for cap in (1, 3):
        for fl in (1, 2):
            same(f"capacity {cap}, in_flight {fl}", many(capacity=cap, in_flight=fl), want)
    g = spec(tta, native, c_token, num_samples=1)
    rev = g.generate_many(batches[::-1], row_keys=[torch.arange(o, o + n) for o, n in zip(offs, sizes)][::-1], logit_biases=biases[::-1], capacity=3)
    same("the list reversed", rev[::-1], want)
    for env in (dict(TTX_TWO_PHASE="0"), dict(TTX_DRAFT_SELECT="0"), dict(TTX_TWO_PHASE_MIN_ROWS="0"),
                dict(TTX_TWO_PHASE_MIN_ROWS="0", TTX_DRAFT_SELECT="0")):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            same(str(env), many(capacity=8), want)
            same(f"{env}, four samples", spec(tta, native, c_token, num_samples=4).generate_many(batches, logit_biases=biases, capacity=16),
                 per_batch(biases, 4))
    holes = [biases[0], None, biases[2]]
    same("a None entry among the biases", spec(tta, native, c_token, num_samples=1).generate_many(batches, logit_biases=holes, capacity=3),
         per_batch(holes))
    allowed = [torch.isfinite(b) for b in biases]
    both = spec(tta, native, c_token, num_samples=1).generate_many(batches, logit_biases=[None, biases[1], None], allowed=allowed)
    assert all(forbidden_used(o, b) == [] for o, b in zip(both, biases))
    same("temperature 0 in the pool", spec(tta, native, c_token, temperature=0.0).generate_many(batches, allowed=allowed),
         [plain(tta, native, temperature=0.0).generate(x, allowed=a) for x, a in zip(batches, allowed)])


# -- stochastic beam search ------------------------------------------------------------------------------------------------------------------
class Biased:
    """An oracle whose logits carry one source's bias row: what the step kernel reads after k_logit_bias."""

    def __init__(self, oracle, row: torch.Tensor):
        self.oracle, self.row = oracle, row

    def __call__(self, s, y):
        out = self.oracle(s, y)
        return out + self.row.to(out.dtype)


@pytest.fixture(scope="module")
def sbs_runs(tta, models, src, bias):
    """K = 5 under the bias, without and with the filter, on the four sources of tests/test_gpu_sbs_mask.py: computed once."""
    native = models["tiny"][0]
    run = lambda K, **kw: sbs(tta, native, K, **kw).generate(src[:4].cuda(), row_keys=TM.KEYS, return_details=True, trace=True, logit_bias=bias[:4])
    out = {}
    for which, kw in (("unfiltered", {}), ("filtered", dict(top_k=TM.TOP_K, top_p=TM.TOP_P))):
        for K in (5, 7):
            o, d = run(K, **kw)
            out[which, K] = (o.cpu().numpy(), d)
    return out


@pytest.mark.parametrize("which", ["unfiltered", "filtered"])
def test_sbs_rows_are_distinct_allowed_and_nested(sbs_runs, bias, which):
    out, d = sbs_runs[which, 5]
    g = d.gumbel.cpu().numpy()
    assert out.shape == (4, 5, MAX_LEN) and (g[:, 0] == 0).all() and (np.diff(g, axis=1) <= 0).all()
    for b in range(4):
        fin = np.isfinite(g[b])
        assert fin.sum() >= 2 and len({tuple(r) for r in out[b][fin].tolist()}) == int(fin.sum()), f"source {b}: hypotheses repeat"
    assert forbidden_used(torch.from_numpy(out[:, np.isfinite(g).all(0)]), bias[:4]) == []
    assert np.isfinite(g).all() or which == "filtered"
    TM.same_run(sbs_runs[which, 5], sbs_runs[which, 7], 5, "K = 5 against the first five of K = 7")


@pytest.mark.parametrize("which,top_k,top_p", [("unfiltered", 0, 1.0), ("filtered", TM.TOP_K, TM.TOP_P)])
def test_sbs_replay_against_the_biased_oracles(models, src, bias, sbs_runs, which, top_k, top_p):
    _, o64, o32 = models["tiny"]
    total = excused = 0
    for b in range(4):
        oracles = (Biased(o64, bias[b].double()), Biased(o32, bias[b]))
        bad, ex, n, gap, outside = TM.replay(sbs_runs[which, 5], src[:4], oracles, b, top_k, top_p, [])
        print(f"{which}, source {b}: {n} ranks, {ex} excused, fp32 gap {gap:.3g}, margin {10 * gap:.3g}")
        assert not bad, f"source {b}: " + "; ".join(bad[:4])
        assert not outside, f"source {b}: tokens outside their float64 kept set (level, rank, token): {outside[:4]}"
        total, excused = total + n, excused + ex
    assert excused <= TM.S.EXCUSED_CAP * total


def test_sbs_with_one_token_besides_eos(tta, models, src):
    native = models["tiny"][0]
    V = native.tgt_vocab_size
    allowed = torch.zeros(4, V, dtype=torch.bool)
    allowed[:, EOS] = True
    toks = [5, 9, 4, 12]
    for b, t in enumerate(toks):
        allowed[b, t] = True
    out, d = sbs(tta, native, 5).generate(src[:4].cuda(), row_keys=TM.KEYS, return_details=True, allowed=allowed)
    rows, g = out.cpu().numpy(), d.gumbel.cpu().numpy()
    assert np.isfinite(g).all(), "the rows t^k EOS, k = 0, 1, 2, .. are more than five"
    for b, t in enumerate(toks):
        end = S.ends(rows[b], PAD, EOS)
        for r, e in zip(rows[b], end):
            assert (r[1:e] == t).all() and r[e] in (t, EOS) and (r[e + 1:] == PAD).all(), f"source {b}: {r.tolist()}"
        assert len({tuple(r) for r in rows[b].tolist()}) == 5


# -- log q ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_logq_under_the_bias(tta, models, src, bias, name):
    native, o64, _ = models[name]
    B, n = 4, 4
    s = src[:B].cuda()
    g = plain(tta, native, num_samples=n)
    pred, sc, q = g.generate(s, logit_bias=bias[:B], return_scores=True, return_logq=True)
    assert bool(torch.isfinite(q.logq).all()) and bool((q.first_outside == -1).all()), f"{name}: a sampled row is outside its own distribution"
    ref = g.score(s, pred)
    assert torch.equal(sc.score, ref.score) and torch.equal(sc.length, ref.length), "with_scores must keep the RAW model's log p, on score()'s bits"
    assert not torch.equal(q.logq, sc.score)
    again = g.logq(s, pred, logit_bias=bias[:B], return_token_logq=True)
    assert torch.equal(again.logq, q.logq)
    by_allowed = g.logq(s, pred, allowed=torch.isfinite(bias[:B]))
    assert bool(torch.isfinite(by_allowed.logq).all())
    # a zero bias is the unbiased log q on the bits
    free, zero = g.logq(s, pred, return_token_logq=True, return_rank=True), g.logq(s, pred, logit_bias=signed_zeros(B, bias.shape[1]),
                                                                                   return_token_logq=True, return_rank=True)
    for f in ("logq", "length", "finished", "first_outside", "token_logq", "rank", "n_kept"):
        assert torch.equal(getattr(free, f), getattr(zero, f)), f"{name}: {f} under a zero bias"
    # a forbidden token: -inf, first_outside at its position
    hyp = pred.clone()
    length = q.length.cpu().numpy()
    where = {}
    for b in range(B):
        for j in range(0, n, 2):
            if length[b, j] >= 3:
                pos = int(length[b, j]) // 2                 # position pos predicts column pos + 1
                hyp[b, j, pos + 1] = BOS
                where[b, j] = pos
    assert len(where) >= 4
    bad = g.logq(s, hyp, logit_bias=bias[:B])
    lq, fo = bad.logq.cpu().numpy(), bad.first_outside.cpu().numpy()
    for b in range(B):
        for j in range(n):
            if (b, j) in where:
                assert lq[b, j] == -np.inf and fo[b, j] == where[b, j], f"{name} source {b} sample {j}: logq {lq[b, j]}, first_outside {fo[b, j]}"
            else:
                assert np.isfinite(lq[b, j]) and fo[b, j] == -1
    assert bool(torch.isfinite(g.logq(s, hyp).logq).all()), "without the bias the same rows are inside the support"
    # token_logq against the float64 restatement on biased logits
    rows = pred.cpu().numpy().reshape(B * n, MAX_LEN)
    lg = oracle_logits(o64, src[:B], rows, n) + np.repeat(bias[:B].numpy().astype(np.float64), n, axis=0)[:, None, :]
    tok = again.token_logq.cpu().numpy().reshape(B * n, MAX_LEN - 1).astype(np.float64)
    p = S.Params(T, pad=PAD, eos=EOS)
    errs, ref_max = [], 0.0
    for r in range(B * n):
        for pos in range(int(length.reshape(-1)[r])):
            want = Q.token_logq(lg[r, pos], int(rows[r, pos + 1]), p)[0]
            assert want > -np.inf
            errs.append(abs(tok[r, pos] - want))
            ref_max = max(ref_max, abs(want))
    bound = TOK_TOL * max(1.0, ref_max) * max(1.0, 1.0 / T)
    print(f"{name}: {len(errs)} tokens, max |token_logq - float64| {max(errs):.3g} (bound {bound:.3g})")
    assert len(errs) > 100 and max(errs) <= bound


def test_logq_of_the_speculative_sampler_the_pool_and_sbs(tta, models, src, bias, c_token):
    native = models["tiny"][0]
    s = src[:4].cuda()
    pred, q = spec(tta, native, c_token, num_samples=2).generate(s, logit_bias=bias[:4], return_logq=True)
    assert bool(torch.isfinite(q.logq).all())
    res = spec(tta, native, c_token, num_samples=2).generate_many([s[:2], s[2:]], logit_biases=[bias[:2], bias[2:4]], return_logq=True)
    assert torch.equal(torch.cat([r[0] for r in res]), pred) and torch.equal(torch.cat([r[1].logq for r in res]), q.logq)
    g = sbs(tta, native, 3, temperature=1.0)
    out, d = g.generate(s, row_keys=TM.KEYS, return_details=True, logit_bias=bias[:4])
    lq = g.logq(s, out, logit_bias=bias[:4], return_token_logq=True)
    # the search's own log-probability against log q under the same bias, as tests/test_gpu_logq.py compares the unbiased pair: rows
    # (PAD is forbidden, so no row ends on a sampled PAD: every row is scored over all the draws the search paid for, whether it
    # ended on EOS or ran to max_len), n * TOK_TOL * max(1, max |token log q|)
    use = torch.isfinite(d.logp)
    assert bool((lq.finished | (lq.length == MAX_LEN - 1)).all()), "a row ended on something other than EOS or max_len"
    tok = lq.token_logq[torch.isfinite(lq.token_logq)]
    bound = lq.length.double() * TOK_TOL * max(1.0, float(tok.abs().max()))
    err = (lq.logq.double() - d.logp.double()).abs()
    print(f"stochastic beam search: {int(use.sum())} rows, max |logq - logp| {float(err[use].max()):.3g}")
    assert int(use.sum()) >= 6 and bool((lq.first_outside[use] == -1).all()) and bool((err[use] <= bound[use]).all())


# -- surface ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(tta, models, src, bias, c_token):
    native = models["tiny"][0]
    s, V = src[:4].cuda(), native.tgt_vocab_size
    b = bias[:4]
    kw = dict(pad_token=PAD, bos_token=BOS, eos_token=EOS)
    others = [tta.TranslationInferenceGreedy(native, MAX_LEN, **kw),
              tta.TranslationInferenceGreedySpeculative(native, MAX_LEN, 4, 3, replace_token=c_token, **kw),
              tta.TranslationInferenceBeamSearch(native, 3, MAX_LEN, **kw),
              tta.TranslationInferenceBeamSearchSpeculative(native, MAX_LEN, 3, 4, 3, V, False, PAD, BOS, EOS, c_token)]
    for g in others:
        for k in (dict(logit_bias=b), dict(allowed=torch.isfinite(b))):
            with pytest.raises(ValueError, match="logit_bias"):
                g.generate(s, **k)
        assert g.generate(s).shape[0] == 4                                   # and the call without the keyword is what it was
        assert bool(torch.isfinite(g.logq(s, g.generate(s), allowed=torch.ones(4, V, dtype=torch.bool)).logq).all())
    for g in (others[1], others[3], sbs(tta, native, 3)):
        with pytest.raises(ValueError, match="logit_bias"):
            g.generate_many([s], logit_biases=[b])
        with pytest.raises(ValueError, match="logit_bias"):
            g.generate_many([s], allowed=[torch.isfinite(b)])
    for g in (plain(tta, native), spec(tta, native, c_token), sbs(tta, native, 3)):
        nan = b.clone()
        nan[1, 7] = float("nan")
        for bad in (b[:3], b[:, :V - 1], torch.zeros(4, V, dtype=torch.int64), nan, b.clamp(max=0).neg()):
            with pytest.raises(ValueError):
                g.generate(s, logit_bias=bad)
        with pytest.raises(ValueError):
            g.generate(s, allowed=torch.isfinite(b).float())
        with pytest.raises(ValueError):
            g.logq(s, g.generate(s), logit_bias=nan)
    with pytest.raises(ValueError, match="one entry per batch"):
        spec(tta, native, c_token).generate_many([s[:2], s[2:]], logit_biases=[b[:2]])
    # the entry point: a row stride below the vocabulary is refused before anything is launched
    import ctypes as C
    from translation_transformer_amd import _native as N
    out = torch.full((4, 1, MAX_LEN), -7, dtype=torch.int64, device="cuda")
    p = N.SampleParams(MAX_LEN, 1, T, 0, 1.0, PAD, BOS, EOS, 1)
    d_b = b.cuda().contiguous()
    opts = N.SampleOpts(None, 0, None, None, 0, None, d_b.data_ptr(), V - 1)
    rc = native._lib.ttx_sample_generate_ex(native.session, s.data_ptr(), 4, s.shape[1], None, C.byref(p), C.byref(opts), out.data_ptr(),
                                            C.byref(N.GenStats()), native._stream())
    torch.cuda.synchronize()
    assert rc == N.TTX_ERR_INVALID and bool((out == -7).all())


@pytest.mark.parametrize("generation", ["sampling", "sampling_speculative", "stochastic_beam_search"])
def test_lightning_passes_allowed_tokens_through(tta, models, src, bias, c_token, tmp_path, generation):
    from test_gpu_lightning_surface import FixtureTokenizer
    st, cfg = states("tiny")
    tkz = FixtureTokenizer()
    s, tgt = src[:4], fixture_tokens()[1][:4]
    allowed = torch.isfinite(bias[:4])
    preds = {}
    for bs in (1, 4):
        mod = tta.VanillaEncoderDecoderTransformerLightning(
            src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
            num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
            share_embeddings=True, generation=generation, beam_size=3, max_len=MAX_LEN, n_drafts=3, draft_len=4, sampling_temperature=4.0,
            sampling_seed=11, report_prediction_file=str(tmp_path / f"r{bs}.txt"))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        batches = [{"src_tokens": s[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda(), "allowed_tokens": allowed[i:i + bs]} for i in range(0, 4, bs)]
        preds[bs] = torch.cat(tta.run_predict(mod, batches), 0).cpu()
        also = [dict(b, logit_bias=bias[i:i + bs]) for i, b in zip(range(0, 4, bs), batches)]
        assert forbidden_used(torch.cat(tta.run_predict(mod, also), 0).cpu(), bias[:4]) == []
    assert preds[1].shape == (4, 3, MAX_LEN) and torch.equal(preds[1], preds[4])
    assert forbidden_used(preds[4], bias[:4]) == [], f"{generation}: the allow-list of the batch did not reach the generator"
    free = torch.cat(tta.run_predict(mod, [{"src_tokens": s.cuda(), "tgt_tokens": tgt.cuda()}]), 0).cpu()
    assert forbidden_used(free, bias[:4]), "the unconstrained module never leaves the allow-list: the check shows nothing"
    mod = tta.VanillaEncoderDecoderTransformerLightning(
        src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
        num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
        share_embeddings=True, generation="greedy", max_len=MAX_LEN)
    mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    with pytest.raises(ValueError, match="allowed_tokens"):
        tta.run_predict(mod, [{"src_tokens": s.cuda(), "tgt_tokens": tgt.cuda(), "allowed_tokens": allowed}])
