"""Forced target prefixes (prompted decoding) end to end: TranslationInferenceSampling.generate(prefix=),
TranslationInferenceSamplingSpeculative.generate(prefix=) and .generate_many(prefixes=), on the tiny golden model and the four-head
model of tests/golden/h4_*, the fixture sources, max_len 32, (n_drafts, draft_len) = (3, 4), the keys and seed of
tests/test_gpu_sampling_speculative.py.

1  Empty prefixes (None, zero width, all PAD) are today's call: the same tensors and counters from all three entry points.
2  The plain sampler prompted with the beginning of its own unprompted row returns that row on the bits.
3  Replay against the float64 oracle for the three calls: forced positions hold the prefix, every other token is consistent with
   the oracle's logits for the forced prefix and its keyed uniform, within the replay tolerance of the existing sampling tests,
   tol = 2 LOGIT_TOL / T + 1e-4.  At temperature 0 there is no uniform: the GPU's logits lie within LOGIT_TOL of the oracle's, so
   the emitted token's float64 logit is at most 2 LOGIT_TOL below the float64 maximum.
4  The same (source, prefix, key) gives the same bits alone and in a batch, at another padded prefix width, at another
   num_samples, through generate and generate_many, at two capacities and under the pool's switches.
5  Counters: a prefix of max_len - 1 tokens takes ceil((max_len - 1) / (draft_len + 1)) verify steps, max_len - 1 plain steps.
6  A forced EOS ends the row.  7  Refused arguments.  8  Lightning passes batch["prefix_tokens"] through on both predict paths.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import util_sample_checks as S
import test_gpu_sampling_speculative as TS
from oracle.drafting import make_drafts
from test_gpu_model import LOGIT_TOL
from test_gpu_sampling import SEED, check_shape, oracle_logits, oracle_mean_prob, states
from test_gpu_sampling_speculative import DRAFT_LEN, KEYS, N_DRAFTS, spec
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
MAX_LEN = 32
B = 4
COUNTERS = ("model_calls", "accepted_tokens", "produced_tokens", "verified_positions", "kv_prefix_positions", "src_positions")


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
    s = fixture_tokens()[0][:B]
    return s[:, :int((s != PAD).sum(1).max())]


@pytest.fixture(scope="module")
def c_token():
    return fixture_tokens()[2]


@pytest.fixture(scope="module")
def temperatures(models, src, c_token):
    """name -> (T_hot, T_acc), chosen by the float64 oracle alone as tests/test_gpu_sampling_speculative.py chooses them."""
    out = {}
    drafts = make_drafts(src[:, 1:].numpy(), DRAFT_LEN, N_DRAFTS, 1, MAX_LEN, EOS, PAD, c_token)
    for name, (_, o64) in models.items():
        hot = next(t for t in (1.0, 2.0, 4.0, 8.0) if oracle_mean_prob(o64, src, KEYS, 2, t, MAX_LEN) < 0.4)
        acc = next(t for t in (1.0, 0.5, 0.25) if TS.oracle_accepted(TS.oracle_rows(o64, src, KEYS, 2, t, MAX_LEN), drafts, 2) > 0)
        out[name] = (hot, acc)
    return out


def plain(tta, native, max_len=MAX_LEN, **kw):
    return tta.TranslationInferenceSampling(native, max_len, PAD, BOS, EOS, **kw)


def padded(rows, width=None) -> torch.Tensor:
    width = max([len(r) for r in rows] + [0]) if width is None else width
    out = torch.full((len(rows), width), PAD, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor([int(t) for t in r], dtype=torch.int64)
    return out


def pooled(g, s, prefix, keys=KEYS, sizes=(1, 2, 1), **kw):
    """generate_many over the sources split into batches of ``sizes``, each with its own rows of ``prefix`` (None: no prefixes)."""
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    parts = [slice(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    outs = g.generate_many([s[p].cuda() for p in parts], row_keys=[keys[p] for p in parts],
                           prefixes=None if prefix is None else [prefix[p] for p in parts], **kw)
    return torch.cat(outs, 0)


def counters(st) -> tuple:
    return tuple(int(getattr(st, k)) for k in COUNTERS)


def foreign_prefixes(tta, native, src, lengths=(0, 3, 7, 12)) -> list:
    """Per source a prefix taken from ANOTHER source's unprompted temperature-0 output (so that the completion is not the
    unprompted one), cut before that output's end; mixed lengths, one of them 0."""
    y = plain(tta, native, temperature=0.0).generate(src.cuda()).cpu().numpy()[:, 0]
    end = S.ends(y, PAD, EOS)
    rows = []
    for b, n in enumerate(lengths):
        o = (b + 1) % len(lengths)
        rows.append([int(t) for t in y[o, 1:1 + min(n, int(end[o]) - 1)]])
    assert [len(r) for r in rows][0] == 0 and max(len(r) for r in rows) > DRAFT_LEN + 1 and len({len(r) for r in rows}) > 2
    return rows


# -- 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_empty_prefixes_are_todays_call(tta, models, src, c_token, name):
    native = models[name][0]
    s = src.cuda()
    empties = [None, torch.zeros((B, 0), dtype=torch.int64), torch.full((B, 5), PAD, dtype=torch.int64)]
    for what, make, call in (
            ("plain", lambda: plain(tta, native, temperature=2.0, num_samples=2, seed=SEED), lambda g, p: g.generate(s, row_keys=KEYS, prefix=p)),
            ("speculative", lambda: spec(tta, native, c_token, MAX_LEN, temperature=2.0, num_samples=2, seed=SEED),
             lambda g, p: g.generate(s, row_keys=KEYS, prefix=p)),
            ("pool", lambda: spec(tta, native, c_token, MAX_LEN, temperature=2.0, num_samples=2, seed=SEED),
             lambda g, p: pooled(g, src, p, capacity=8))):
        g = make()
        base = (g.generate(s, row_keys=KEYS) if what != "pool" else
                torch.cat(g.generate_many([src[0:1].cuda(), src[1:3].cuda(), src[3:4].cuda()], row_keys=[KEYS[0:1], KEYS[1:3], KEYS[3:4]],
                                          capacity=8), 0))
        want = counters(g.last_stats)
        assert want[0] > 0
        for p in empties:
            g2 = make()
            out = call(g2, p)
            assert torch.equal(out, base), f"{name} {what}: an empty prefix changed the rows"
            assert counters(g2.last_stats) == want, f"{name} {what}: an empty prefix changed the counters"


# -- 2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_plain_sampler_completes_its_own_rows(tta, models, src, name):
    native = models[name][0]
    s = src.cuda()
    for T in (2.0, 0.0):
        y = plain(tta, native, temperature=T, seed=SEED).generate(s, row_keys=KEYS)
        rows = y.cpu().numpy()[:, 0]
        end = S.ends(rows, PAD, EOS)
        for shift in range(B):                                              # every row gets every P over the four calls
            P = []
            for r in range(B):
                L = int(end[r])
                want = [1, L // 2, L - 1, L][(r + shift) % 4]
                real = L if rows[r, L] not in (PAD,) else L - 1            # a row that ended by PAD: the PAD is padding in a prefix
                P.append(max(0, min(want, real)))
            pre = padded([rows[r, 1:1 + P[r]] for r in range(B)], width=max(P) + shift)
            out = plain(tta, native, temperature=T, seed=SEED).generate(s, row_keys=KEYS, prefix=pre)
            assert torch.equal(out, y), f"{name} T {T} P {P}: the prompted rows differ from the unprompted ones"


# -- 3 ----------------------------------------------------------------------------------------------------------------------------
def replay_prompted(what, o64, s, out, prefix_rows, T, n):
    rows = out.reshape(-1, MAX_LEN)
    end = S.ends(rows, PAD, EOS)
    lg = oracle_logits(o64, s, rows, n)                                   # teacher-forced on the rows: the logits for the forced prefix
    p = S.Params(T, pad=PAD, eos=EOS)
    worst = 0.0
    free = 0
    for r in range(len(rows)):
        pre = prefix_rows[r // n]
        for pos in range(1, int(end[r]) + 1):
            if pos <= len(pre):
                assert rows[r, pos] == pre[pos - 1], f"{what} row {r} position {pos}: {rows[r, pos]} where the prefix holds {pre[pos - 1]}"
                continue
            free += 1
            if T == 0:
                gap = float(lg[r, pos - 1].max() - lg[r, pos - 1][rows[r, pos]])
                worst = max(worst, gap)
                assert gap <= 2 * LOGIT_TOL, f"{what} row {r} position {pos}: token {rows[r, pos]} lies {gap:.3e} below the float64 maximum"
                continue
            tol = 2 * LOGIT_TOL / T + 1e-4
            u = float(S.uniform(SEED, KEYS[r // n], r % n, pos))
            ex = S.excess(int(rows[r, pos]), lg[r, pos - 1], u, p)
            worst = max(worst, ex)
            assert S.consistent(int(rows[r, pos]), lg[r, pos - 1], u, p, tol), \
                f"{what} row {r} position {pos}: token {rows[r, pos]} lies {ex:.3e} outside its interval (tol {tol:.3e})"
        assert end[r] >= min(len(pre), MAX_LEN - 1), f"{what} row {r} ended inside its prefix"
    assert free > len(rows), f"{what}: next to nothing was sampled behind the prefixes"
    return worst


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_replay_against_float64_oracle(tta, models, src, c_token, temperatures, name):
    native, o64 = models[name]
    n = 2
    pre_rows = foreign_prefixes(tta, native, src)
    pre = padded(pre_rows)
    free_rows = None
    for T in temperatures[name] + (0.0,):
        calls = {
            "plain": lambda: plain(tta, native, temperature=T, num_samples=n, seed=SEED).generate(src.cuda(), row_keys=KEYS, prefix=pre),
            "speculative": lambda: spec(tta, native, c_token, MAX_LEN, temperature=T, num_samples=n, seed=SEED)
            .generate(src.cuda(), row_keys=KEYS, prefix=pre),
            "pool": lambda: pooled(spec(tta, native, c_token, MAX_LEN, temperature=T, num_samples=n, seed=SEED), src, pre, capacity=4)}
        for what, call in calls.items():
            out = call().cpu().numpy()
            check_shape(out, B, n, MAX_LEN)
            worst = replay_prompted(f"{name} T {T} {what}", o64, src, out, pre_rows, T, n)
            print(f"{name}: T {T}: {what}: largest excess {worst:.3e}")
            if what == "plain" and T == 0.0:
                free_rows = plain(tta, native, temperature=0.0, num_samples=n, seed=SEED).generate(src.cuda(), row_keys=KEYS).cpu().numpy()
                assert np.array_equal(out[0], free_rows[0]) and not np.array_equal(out[2], free_rows[2]), \
                    "a foreign prefix did not change the completion (or an empty one did)"


# -- 4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_invariance_is_exact(tta, models, src, c_token, name, monkeypatch):
    native = models[name][0]
    T, n = 2.0, 8
    s = src.cuda()
    pre_rows = foreign_prefixes(tta, native, src)
    pre = padded(pre_rows)
    make = lambda n_=n, **kw: spec(tta, native, c_token, MAX_LEN, temperature=T, num_samples=n_, seed=SEED, **kw)
    full = make().generate(s, row_keys=KEYS, prefix=pre)
    assert len({tuple(r) for r in full.reshape(B * n, MAX_LEN).tolist()}) > 8                       # it does sample
    for b in range(B):
        assert (full[b, :, 1:1 + len(pre_rows[b])].cpu() == torch.tensor(pre_rows[b], dtype=torch.int64)).all()
    g = make()
    assert torch.equal(g.generate(s, row_keys=KEYS, prefix=pre), full) and torch.equal(g.generate(s, row_keys=KEYS, prefix=pre), full)
    for b in range(B):                                                    # alone, at the prefix's own width and at a wider one
        one = padded([pre_rows[b]], width=len(pre_rows[b]) + (3 if b % 2 else 0))
        assert torch.equal(make().generate(s[b:b + 1], row_keys=KEYS[b:b + 1], prefix=one), full[b:b + 1]), f"{name}: source {b} alone"
    assert torch.equal(make().generate(s, row_keys=KEYS, prefix=padded(pre_rows, width=MAX_LEN + 9)), full)
    assert torch.equal(make(1).generate(s, row_keys=KEYS, prefix=pre), full[:, :1])                 # sample j does not depend on n
    assert torch.equal(make(4).generate(s[1:3], row_keys=KEYS[1:3], prefix=pre[1:3]), full[1:3, :4])
    assert not torch.equal(make().generate(s, row_keys=KEYS), full)
    # the pool: its contract, two capacities, its switches
    assert torch.equal(pooled(make(), src, pre, capacity=64), full), f"{name}: generate_many against generate"
    assert torch.equal(pooled(make(), src, pre, capacity=8), full), f"{name}: capacity 8 (one source fills the pool)"
    assert torch.equal(pooled(make(), src, pre, capacity=64, sizes=(4,)), full)
    assert torch.equal(pooled(make(4), src, pre, capacity=16, sizes=(2, 2)), full[:, :4])
    for env in (dict(TTX_TWO_PHASE="0"), dict(TTX_DRAFT_SELECT="0", TTX_TWO_PHASE_MIN_ROWS="0"), dict(TTX_ACCEPT_SPREAD="0"),
                dict(TTX_TWO_PHASE_MIN_ROWS="0")):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            assert torch.equal(pooled(make(), src, pre, capacity=64), full), f"{name}: {env}"
            if env == dict(TTX_TWO_PHASE_MIN_ROWS="0"):
                pc = native.pool_last_counters()
                assert pc["split_steps"] > 0 and pc["split_steps"] == pc["steps"]
    # mixed: one batch with prefixes, one without
    mixed = make().generate_many([s[:2], s[2:]], row_keys=[KEYS[:2], KEYS[2:]], prefixes=[pre[:2], None], capacity=64)
    assert torch.equal(mixed[0], full[:2]) and torch.equal(mixed[1], make().generate(s[2:], row_keys=KEYS[2:]))
    # the plain sampler: alone and in a batch, at another width, at another num_samples
    pl = lambda n_=n: plain(tta, native, temperature=T, num_samples=n_, seed=SEED)
    pfull = pl().generate(s, row_keys=KEYS, prefix=pre)
    assert torch.equal(pl().generate(s[2:3], row_keys=KEYS[2:3], prefix=padded([pre_rows[2]], width=20)), pfull[2:3])
    assert torch.equal(pl(1).generate(s, row_keys=KEYS, prefix=pre), pfull[:, :1])


# -- 5 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_counters(tta, models, src, c_token, name):
    native = models[name][0]
    s = src.cuda()
    rng = np.random.default_rng(3)
    V = native.tgt_vocab_size
    body = [t for t in range(V) if t not in (PAD, BOS, EOS)]
    rows = [[int(t) for t in rng.choice(body, size=MAX_LEN - 1)] for _ in range(B)]
    pre = padded(rows)
    want = torch.cat([torch.full((B, 1), BOS, dtype=torch.int64), pre], 1)
    n = 2
    g = spec(tta, native, c_token, MAX_LEN, temperature=1.0, num_samples=n, seed=SEED)
    out = g.generate(s, row_keys=KEYS, prefix=pre)
    assert torch.equal(out.cpu(), want[:, None, :].expand(B, n, MAX_LEN))
    assert g.model_calls_num == -(-(MAX_LEN - 1) // (DRAFT_LEN + 1)), f"{name}: {g.model_calls_num} verify steps"
    g = plain(tta, native, temperature=1.0, num_samples=n, seed=SEED)
    assert torch.equal(g.generate(s, row_keys=KEYS, prefix=pre).cpu(), want[:, None, :].expand(B, n, MAX_LEN))
    assert g.model_calls_num == MAX_LEN - 1
    g = spec(tta, native, c_token, MAX_LEN, temperature=1.0, num_samples=n, seed=SEED)
    assert torch.equal(pooled(g, src, pre, capacity=8).cpu(), want[:, None, :].expand(B, n, MAX_LEN))
    P = 12
    short = padded([r[:P] for r in rows])
    for what, run in (("speculative", lambda g: g.generate(s, row_keys=KEYS, prefix=short)), ("pool", lambda g: pooled(g, src, short, capacity=8))):
        g = spec(tta, native, c_token, MAX_LEN, temperature=1.0, num_samples=n, seed=SEED)
        out = run(g)
        assert (out[:, :, 1:1 + P].cpu() == short[:, None, :]).all()
        assert g.accepted_tokens_num >= B * n * (P // (DRAFT_LEN + 1)) * DRAFT_LEN, f"{name} {what}: accepted {g.accepted_tokens_num}"


# -- 6 ----------------------------------------------------------------------------------------------------------------------------
def test_forced_eos_ends_the_row(tta, models, src, c_token):
    native = models["tiny"][0]
    s = src.cuda()
    rows = [[5, 6, EOS], [EOS], [7, 8, 9, 10, 11, 12, EOS, 4, 4], []]     # tokens behind a forced EOS are never reached
    pre = padded(rows)
    for what, call in (("plain", lambda: plain(tta, native, temperature=2.0, num_samples=2, seed=SEED).generate(s, row_keys=KEYS, prefix=pre)),
                       ("speculative", lambda: spec(tta, native, c_token, MAX_LEN, temperature=2.0, num_samples=2, seed=SEED)
                        .generate(s, row_keys=KEYS, prefix=pre)),
                       ("pool", lambda: pooled(spec(tta, native, c_token, MAX_LEN, temperature=2.0, num_samples=2, seed=SEED), src, pre, capacity=8))):
        out = call()
        o = out.cpu().numpy()
        check_shape(o, B, 2, MAX_LEN)
        for b in range(3):
            cut = rows[b].index(EOS) + 1
            assert (o[b, :, 1:1 + cut] == np.array(rows[b][:cut])).all() and (o[b, :, 1 + cut:] == PAD).all(), f"{what} source {b}: {o[b].tolist()}"
        g = spec(tta, native, c_token, MAX_LEN)
        length = g.score(s, out).length.cpu().numpy()
        assert length[:3].tolist() == [[3, 3], [1, 1], [7, 7]], f"{what}: score lengths {length.tolist()}"


# -- 7 ----------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(tta, models, src, c_token):
    from translation_transformer_amd import _native as NA
    native = models["tiny"][0]
    s = src.cuda().contiguous()
    width = s.shape[1]
    pre = torch.full((B, 6), 5, dtype=torch.int64, device="cuda")
    sp = NA.SampleParams(16, 2, 1.0, 0, 1.0, PAD, BOS, EOS, SEED)
    ssp = NA.SampleSpecParams(sp, 4, 3, c_token, 0)
    h_len = (C.c_int32 * B)(*[int(x) for x in (s != PAD).sum(1).tolist()])
    sess = (C.c_void_p * 1)(native.session.value)
    lib = native._lib

    def calls(d_prefix, ld, lens):
        out = torch.full((B, 2, 16), -7, dtype=torch.int64, device="cuda")
        h = None if lens is None else (C.c_int32 * B)(*lens)
        yield "plain", lib.ttx_sample_generate_prefix(native.session, s.data_ptr(), B, width, None, C.byref(sp), d_prefix, ld, h,
                                                      out.data_ptr(), None, native._stream()), out
        out = torch.full((B, 2, 16), -7, dtype=torch.int64, device="cuda")
        yield "speculative", lib.ttx_sample_speculative_generate_prefix(native.session, s.data_ptr(), B, width, None, C.byref(ssp), d_prefix,
                                                                        ld, h, out.data_ptr(), None, native._stream()), out
        out = torch.full((B, 2, 16), -7, dtype=torch.int64, device="cuda")
        yield "pool", lib.ttx_sample_speculative_generate_pool_prefix(sess, 1, s.data_ptr(), B, width, h_len, None, 8, C.byref(ssp),
                                                                      d_prefix, ld, h, out.data_ptr(), None, native._stream()), out

    bad = [(pre.data_ptr(), 6, [16, 0, 0, 0]),             # above max_len - 1 (and above ld_prefix)
           (pre.data_ptr(), 6, [0, 7, 0, 0]),              # above ld_prefix
           (pre.data_ptr(), 6, [0, 0, -1, 0]),             # negative
           (None, 6, [0, 0, 0, 1]),                        # a non-zero length without a prefix
           (pre.data_ptr(), -1, [0, 0, 0, 0])]             # a negative row length
    for d_prefix, ld, lens in bad:
        for what, rc, out in calls(d_prefix, ld, lens):
            torch.cuda.synchronize()
            assert rc == -1, f"{what} {lens} ld {ld}: code {rc}"
            assert bool((out == -7).all()), f"{what} {lens}: d_out was written"
    for d_prefix, ld, lens in [(pre.data_ptr(), 6, [6, 0, 3, 1]), (None, 0, [0, 0, 0, 0]), (None, 0, None)]:     # and these run
        for what, rc, out in calls(d_prefix, ld, lens):
            torch.cuda.synchronize()
            assert rc == 0 and bool((out[:, :, 0] == BOS).all()) and bool((out != -7).all()), f"{what} {lens}: code {rc}"
            if lens and lens[0] == 6:
                assert bool((out[0, :, 1:7] == 5).all()) and bool((out[3, :, 1] == 5).all())
    # the Python layer, at max_len 16: 16 forced tokens are one too many (max_len - 1 = 15), 15 fit
    g = spec(tta, native, c_token, 16, num_samples=2)
    for p in (torch.tensor([[5, PAD, 6]] * B), torch.full((B, 3), native.tgt_vocab_size), torch.full((B, 16), 5), torch.full((B - 1, 3), 5)):
        with pytest.raises(ValueError):
            g.generate(s, prefix=p)
        with pytest.raises(ValueError):
            plain(tta, native, 16).generate(s, prefix=p)
        with pytest.raises(ValueError):
            g.generate_many([s], prefixes=[p])
    with pytest.raises(ValueError):
        g.generate_many([s, s], prefixes=[None])
    assert g.generate(s, prefix=torch.full((B, 15), 5)).shape == (B, 2, 16)
    for other in (tta.TranslationInferenceGreedy(native, 16, PAD, BOS, EOS),
                  tta.TranslationInferenceGreedySpeculative(native, 16, 4, 3, PAD, BOS, EOS, c_token),
                  tta.TranslationInferenceBeamSearch(native, 2, 16, PAD, BOS, EOS)):
        with pytest.raises(TypeError):
            other.generate(s, prefix=pre)


# -- 8 ----------------------------------------------------------------------------------------------------------------------------
def test_lightning_passes_prefix_tokens_through(tta, tmp_path):
    from test_gpu_lightning_surface import FixtureTokenizer
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    src, tgt, _, _ = fixture_tokens()

    def module(generation, tag):
        mod = tta.VanillaEncoderDecoderTransformerLightning(
            src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
            num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
            share_embeddings=True, generation=generation, beam_size=3, max_len=40, draft_len=4, n_drafts=3, sampling_temperature=2.0,
            sampling_top_k=8, sampling_top_p=0.95, sampling_seed=11, report_prediction_file=str(tmp_path / f"{tag}.txt"))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        return mod

    rows = [[5, 6, 7, 8, 9, 10, 11], [], [12, 13], [9, 8, 7, 6, 5, 4, 9, 8, 7, 6]]
    pre = padded(rows)
    preds = {}
    for generation, pool, bs in (("sampling_speculative", False, 4), ("sampling_speculative", False, 1), ("sampling_speculative", True, 4),
                                 ("sampling_speculative", True, 1), ("sampling", False, 4), ("sampling", False, 1)):
        mod = module(generation, f"{generation}{pool}{bs}")
        mod.predict_sample_pool = pool
        batches = [{"src_tokens": src[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda(), "prefix_tokens": pre[i:i + bs]} for i in range(0, 4, bs)]
        out = torch.cat(tta.run_predict(mod, batches), 0).cpu()
        assert out.shape == (4, 3, 40)
        for b, r in enumerate(rows):
            assert (out[b, :, 1:1 + len(r)] == torch.tensor(r, dtype=torch.int64)).all(), f"{generation} pool {pool} bs {bs}: source {b}"
        if pool:
            assert mod._ahead is not None and mod._ahead.served == len(batches), "the look-ahead path did not serve the prompted batches"
        preds[(generation, pool, bs)] = out
    assert torch.equal(preds[("sampling_speculative", False, 4)], preds[("sampling_speculative", False, 1)])
    assert torch.equal(preds[("sampling_speculative", True, 4)], preds[("sampling_speculative", True, 1)])
    assert torch.equal(preds[("sampling_speculative", True, 4)], preds[("sampling_speculative", False, 4)])
    assert torch.equal(preds[("sampling", False, 4)], preds[("sampling", False, 1)])
    free = torch.cat(tta.run_predict(module("sampling_speculative", "free"), [{"src_tokens": src[:4].cuda(), "tgt_tokens": tgt[:4].cuda()}]), 0).cpu()
    assert torch.equal(free[1], preds[("sampling_speculative", False, 4)][1]) and not torch.equal(free[0], preds[("sampling_speculative", False, 4)][0])
    mod = module("greedy_speculative", "greedy")
    with pytest.raises(ValueError):
        tta.run_predict(mod, [{"src_tokens": src[:2].cuda(), "tgt_tokens": tgt[:2].cuda(), "prefix_tokens": pre[:2]}])
