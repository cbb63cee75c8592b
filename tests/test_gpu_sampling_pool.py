"""TranslationInferenceSamplingSpeculative.generate_many (ttx_sample_speculative_generate_pool) end to end, on the tiny golden model
and on the four-head model of tests/golden/h4_* (head dimension 32 and 4 heads, so draft select engages): the ten fixture sources
(lengths 28 .. 127; two of them share a length) in batches [4, 4, 2], num_samples = 4, (n_drafts, draft_len) = (3, 4).

  greedy settings   rows, accepted and produced tokens of TranslationInferenceGreedySpeculative on the same rows repeated: exact
  float64 replay    tests/test_gpu_sampling_speculative.py's replay and tolerance, at the two temperatures the oracle itself selects
  other samplers    the per-batch speculative sampler and the plain sampler under the same seed and keys: equal rows, except rows whose
                    first differing position holds two tokens consistent with the float64 oracle within the replay's tolerance; at
                    most MAX_EXCUSED of the 40 rows per comparison
  invariance        bit for bit across capacity, pools in flight, list order and batching, and every switch of the pool
  the rest          default keys, shapes, [], return_scores, refused arguments, no graph shared with the greedy pool, Lightning
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_sampling_speculative as TS
import util_sample_checks as S
from oracle.drafting import make_drafts
from test_gpu_model import LOGIT_TOL
from test_gpu_sampling import SEED, check_shape, oracle_mean_prob, states
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
N_DRAFTS, DRAFT_LEN, N_SAMPLES, MAX_LEN = 3, 4, 4, 32
SIZES = [4, 4, 2]
KEYS = np.array([5, 1 << 40, 7, -3, 11, (1 << 33) + 1, 0, 123456789, -(1 << 35), 42], dtype=np.int64)
MAX_EXCUSED = 1          # of 40 rows per comparison (DESIGN.md §18 measured 0 of 32 in its tests, at worst 1 of 768 in its bench)


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
    assert s.shape[0] == 10
    lengths = (s != PAD).sum(1)
    assert len(set(lengths.tolist())) >= 9                # 28 .. 127; two of the ten share a length
    return s[:, :int(lengths.max())]


@pytest.fixture(scope="module")
def c_token():
    return fixture_tokens()[2]


def split(x, sizes=SIZES):
    out, r0 = [], 0
    for b in sizes:
        out.append(x[r0:r0 + b])
        r0 += b
    return out


def trimmed(s):
    """A batch as a dataloader pads it: to its own longest source."""
    return s[:, :max(2, int((s != PAD).sum(1).max()))]


def batches_of(src, sizes=SIZES):
    return [trimmed(b).cuda() for b in split(src, sizes)]


def gen(tta, native, c, max_len=MAX_LEN, **kw):
    kw.setdefault("num_samples", N_SAMPLES)
    kw.setdefault("seed", SEED)
    return TS.spec(tta, native, c, max_len, **kw)


def pooled(g, src, sizes=SIZES, keys=KEYS, **kw) -> np.ndarray:
    outs = g.generate_many(batches_of(src, sizes), row_keys=None if keys is None else split(keys, sizes), **kw)
    assert [tuple(o.shape) for o in outs] == [(b, g.num_samples, g.max_len) for b in sizes]
    return torch.cat(outs, 0).cpu().numpy()


# -- greedy settings -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_greedy_settings_equal_greedy_speculative(tta, models, src, c_token, name):
    native = models[name][0]
    n, max_len = N_SAMPLES, 150
    gs = tta.TranslationInferenceGreedySpeculative(native, max_len, DRAFT_LEN, N_DRAFTS, PAD, BOS, EOS, c_token)
    ref = gs.generate(src.cuda().repeat_interleave(n, 0)).cpu().numpy()[:, 0]            # the same rows repeated
    ref_end = S.ends(ref, PAD, EOS)
    assert (ref[np.arange(10 * n), ref_end] == EOS).all(), "a fixture row does not end by EOS: the comparison needs a larger max_len"
    assert gs.stats_total["accepted_tokens"] > 0
    for kw in (dict(top_k=1), dict(temperature=0.0)):
        g = gen(tta, native, c_token, max_len, **kw)
        out = pooled(g, src)
        end = check_shape(out, 10, n, max_len)
        rows = out.reshape(10 * n, max_len)
        for r in range(10 * n):
            e = ref_end[r]
            assert end[r] == e and (rows[r, :e + 1] == ref[r, :e + 1]).all(), \
                f"{name} {kw} row {r}: {rows[r].tolist()} against greedy speculative {ref[r].tolist()}"
        assert g.accepted_tokens_num == gs.stats_total["accepted_tokens"], f"{name} {kw}: accepted tokens"
        assert g.stats_total["produced_tokens"] == int(ref_end.sum()), f"{name} {kw}: produced tokens"
        assert g.model_calls_num > 0 and g.last_stats.src_tokens_padded > 0


# -- float64 replay, the per-batch speculative sampler, the plain sampler ------------------------------------------------------------
def excused(name, what, rows, other, lg, end, T, n, keys=KEYS, seed=SEED, top_k=0, top_p=1.0) -> int:
    """Rows of ``rows`` that differ from ``other``: at the first differing position both tokens must be consistent with the float64
    logits ``lg`` within the replay's tolerance.  Returns their count."""
    p, tol = S.Params(T, top_k, top_p, pad=PAD, eos=EOS), 2 * LOGIT_TOL / T + 1e-4
    near = 0
    for r in range(len(rows)):
        diff = np.nonzero(rows[r] != other[r])[0]
        if len(diff) == 0:
            continue
        pos = int(diff[0])
        assert 1 <= pos <= end[r], f"{name} T {T} {what} row {r}: the rows differ behind the row's end"
        u = float(S.uniform(seed, keys[r // n], r % n, pos))
        for tok in (rows[r, pos], other[r, pos]):
            assert S.consistent(int(tok), lg[r, pos - 1], u, p, tol), \
                f"{name} T {T} {what} row {r} position {pos}: {rows[r, pos]} against {other[r, pos]}: not a near-boundary draw"
        near += 1
    print(f"{name}: T {T}: {near} of {len(rows)} rows differ from {what} by a near-boundary draw")
    assert near <= MAX_EXCUSED, f"{name} T {T} {what}: {near} rows excused, at most {MAX_EXCUSED} may be"
    return near


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_replay_against_float64_oracle_and_the_other_samplers(tta, models, src, c_token, name, monkeypatch):
    native, o64 = models[name]
    n, max_len = N_SAMPLES, MAX_LEN
    monkeypatch.setattr(TS, "KEYS", KEYS)                                 # the existing replay keys its rows by the module's KEYS
    drafts = make_drafts(src[:, 1:].numpy(), DRAFT_LEN, N_DRAFTS, 1, max_len, EOS, PAD, c_token)
    T_hot = next((t for t in (1.0, 2.0, 4.0, 8.0) if oracle_mean_prob(o64, src, KEYS, n, t, max_len) < 0.4), None)
    assert T_hot is not None, "the oracle's samples stay confident up to T = 8"
    T_acc = next((t for t in (1.0, 0.5, 0.25) if TS.oracle_accepted(TS.oracle_rows(o64, src, KEYS, n, t, max_len), drafts, n) > 0), None)
    assert T_acc is not None, "the oracle's own samples accept no draft token down to T = 0.25"
    for T in (T_hot, T_acc):
        g = gen(tta, native, c_token, temperature=T)
        out = pooled(g, src)
        check_shape(out, 10, n, max_len)
        worst, mean_p, lg, end = TS.replay(name, o64, src, out, T, n, max_len)
        print(f"{name}: T {T}: mean probability of the emitted token {mean_p:.3f}, largest excess {worst:.3e}, accepted "
              f"{g.accepted_tokens_num} of {g.stats_total['produced_tokens']} produced tokens in {g.model_calls_num} device steps")
        if T == T_hot:
            assert mean_p < 0.5, "the check went soft: the sampled tokens are the confident ones"
        if T == T_acc:
            assert g.accepted_tokens_num > 0, "no draft token was accepted where the oracle's own samples accept some"
        rows = out.reshape(10 * n, max_len)
        per = gen(tta, native, c_token, temperature=T)
        per_rows = torch.cat([per.generate(b, row_keys=k) for b, k in zip(batches_of(src), split(KEYS))], 0).cpu().numpy()
        excused(name, "the per-batch speculative sampler", rows, per_rows.reshape(10 * n, max_len), lg, end, T, n)
        plain = tta.TranslationInferenceSampling(native, max_len, PAD, BOS, EOS, temperature=T, num_samples=n, seed=SEED)
        plain_rows = torch.cat([plain.generate(b, row_keys=k) for b, k in zip(batches_of(src), split(KEYS))], 0).cpu().numpy()
        excused(name, "the plain sampler", rows, plain_rows.reshape(10 * n, max_len), lg, end, T, n)
        # the default keys are the running index over the concatenated batches
        dflt = pooled(gen(tta, native, c_token, temperature=T), src, keys=None).reshape(10 * n, max_len)
        per2 = gen(tta, native, c_token, temperature=T)
        offs = np.concatenate([[0], np.cumsum(SIZES)])
        want = torch.cat([per2.generate(b, row_keys=torch.arange(int(o), int(o) + b.shape[0]))
                          for b, o in zip(batches_of(src), offs)], 0).cpu().numpy().reshape(10 * n, max_len)
        monkeypatch.setattr(TS, "KEYS", np.arange(10, dtype=np.int64))
        _, _, lg_d, end_d = TS.replay(name, o64, src, dflt.reshape(10, n, max_len), T, n, max_len)
        monkeypatch.setattr(TS, "KEYS", KEYS)
        p, tol = S.Params(T, pad=PAD, eos=EOS), 2 * LOGIT_TOL / T + 1e-4
        near = 0
        for r in np.nonzero((dflt != want).any(1))[0]:
            pos = int(np.nonzero(dflt[r] != want[r])[0][0])
            assert 1 <= pos <= end_d[r]
            u = float(S.uniform(SEED, r // n, r % n, pos))
            assert all(S.consistent(int(t), lg_d[r, pos - 1], u, p, tol) for t in (dflt[r, pos], want[r, pos])), f"{name} T {T} default keys row {r}"
            near += 1
        print(f"{name}: T {T}: default keys: {near} of {10 * n} rows differ from per-batch generate by a near-boundary draw")
        assert near <= MAX_EXCUSED


# -- exact invariance --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_invariance_is_exact(tta, models, src, c_token, name, monkeypatch):
    """At the temperature of tests/test_gpu_sampling.py's invariance test.  Every variation must return the base rows bit for bit,
    with the same accepted and produced tokens."""
    native = models[name][0]
    T, n = 2.0, N_SAMPLES

    def run(sizes=SIZES, order=None, **kw):
        g = gen(tta, native, c_token, temperature=T)
        s, k = (src, KEYS) if order is None else (src[order], KEYS[order])
        out = pooled(g, s, sizes, k, **kw)
        if order is not None:
            out = out[np.argsort(order)]
        return out, (g.accepted_tokens_num, g.stats_total["produced_tokens"]), native.pool_last_counters()

    base, counts, pc = run(capacity=64)
    assert len({tuple(r) for r in base.reshape(10 * n, MAX_LEN).tolist()}) > 8                  # it does sample
    assert counts[1] > counts[0] >= 0 and pc["steps"] > 0

    def same(what, got):
        out, c, _ = got
        assert np.array_equal(out, base), f"{name}: {what}: rows differ from the base call"
        assert c == counts, f"{name}: {what}: accepted / produced tokens {c} against {counts}"

    for cap in (4, 8):                                   # one source fills the pool; slots are reused
        same(f"capacity {cap}", run(capacity=cap))
    for fl in (1, 2):
        same(f"in_flight {fl}", run(capacity=8, in_flight=fl))
    rev = np.arange(10)[::-1].copy()
    same("the batches reversed", run(order=rev, capacity=64))
    same("one batch of 10", run(sizes=[10], capacity=64))
    same("ten batches of 1", run(sizes=[1] * 10, capacity=64))
    same("default capacity", run())
    with monkeypatch.context() as mp:
        mp.setenv("TTX_TWO_PHASE", "0")
        got = run(capacity=64)
        same("TTX_TWO_PHASE=0", got)
        assert got[2]["split_steps"] == 0
    with monkeypatch.context() as mp:
        mp.setenv("TTX_TWO_PHASE_MIN_ROWS", "0")
        got = run(capacity=64)
        same("TTX_TWO_PHASE_MIN_ROWS=0", got)
        assert got[2]["split_steps"] > 0 and got[2]["split_steps"] == got[2]["steps"]
        assert got[2]["draft_select"] == (1 if name == "h4" else 0), "draft select runs on the four-head model alone"
        executed_select = got[2]["rows_executed"]
        mp.setenv("TTX_DRAFT_SELECT", "0")
        got = run(capacity=64)
        same("TTX_DRAFT_SELECT=0", got)
        assert got[2]["draft_select"] == 0 and got[2]["rows_executed"] >= executed_select
        mp.setenv("TTX_ADMIT_ROWS", "100")                # sub-chunks of one or two sources
        same("TTX_ADMIT_ROWS=100 with every step split", run(capacity=64))
    with monkeypatch.context() as mp:
        mp.setenv("TTX_ADMIT_ROWS", "100")
        same("TTX_ADMIT_ROWS=100", run(capacity=64))
    # more than 256 slots in one pool (the accept step in two launches): every source seven times, under its own key
    rep = np.tile(np.arange(10), 7)
    for spread in ("1", "0"):
        with monkeypatch.context() as mp:
            mp.setenv("TTX_ACCEPT_SPREAD", spread)
            mp.setenv("TTX_POOL_SESSIONS", "1")
            g = gen(tta, native, c_token, temperature=T)
            out = pooled(g, src[rep], [70], KEYS[rep], capacity=512)
            assert g.last_group_size == 512 and 70 * n > 256
            for i, r in enumerate(rep):
                assert np.array_equal(out[i], base[r]), f"{name}: 280 slots, TTX_ACCEPT_SPREAD={spread}: copy {i} of source {r}"
            assert (g.accepted_tokens_num, g.stats_total["produced_tokens"]) == (7 * counts[0], 7 * counts[1])


# -- shapes, scores, refused arguments ---------------------------------------------------------------------------------------------
def test_shapes_empty_list_and_scores(tta, models, src, c_token):
    native = models["tiny"][0]
    g = gen(tta, native, c_token, temperature=2.0)
    assert g.generate_many([]) == [] and g.model_calls_num == 0
    out = g.generate_many(batches_of(src), row_keys=split(KEYS))
    assert g.given_tokens == int((src != PAD).sum()) and g.stats_total["batches"] == 3
    scored = gen(tta, native, c_token, temperature=2.0).generate_many(batches_of(src), row_keys=split(KEYS), return_scores=True)
    for (pred, sc), o, b in zip(scored, out, SIZES):
        assert torch.equal(pred, o) and sc.score.shape == (b, N_SAMPLES) and bool(torch.isfinite(sc.score).all())
    for max_len in (1, 2, 5):
        g = gen(tta, native, c_token, max_len, draft_len=1, temperature=1.0)
        o = pooled(g, src, capacity=8)
        if max_len == 1:
            assert o.shape == (10, N_SAMPLES, 1) and (o == BOS).all()
        else:
            check_shape(o, 10, N_SAMPLES, max_len)
    with pytest.raises(ValueError):
        g.generate_many(batches_of(src), row_keys=split(KEYS)[:2])
    with pytest.raises(ValueError):
        g.generate_many(batches_of(src), row_keys=[[1, 2, 3]] * 3)


def pool_call(tta, native, src, c_token, **over):
    """ttx_sample_speculative_generate_pool on the first four sources: (rc, out with a sentinel)."""
    from translation_transformer_amd import _native as NA
    s = src[:4].cuda().contiguous()
    S_total, width = s.shape
    S_total = over.pop("S_total", S_total)
    a = dict(max_len=16, num_samples=2, temperature=1.0, top_k=0, top_p=1.0, pad=PAD, bos=BOS, eos=EOS, seed=SEED, draft_len=4, n_drafts=3,
             replace=c_token, capacity=8, Ls_all=width, h_len=[int(x) for x in (s != PAD).sum(1).tolist()], null=())
    a.update(over)
    p = NA.SampleSpecParams(NA.SampleParams(a["max_len"], a["num_samples"], a["temperature"], a["top_k"], a["top_p"], a["pad"], a["bos"],
                                            a["eos"], a["seed"]), a["draft_len"], a["n_drafts"], a["replace"], 0)
    out = torch.full((s.shape[0], max(a["num_samples"], 1), max(a["max_len"], 1)), -7, dtype=torch.int64, device="cuda")
    sess = (C.c_void_p * 1)(native.session.value)
    h_len = (C.c_int32 * len(a["h_len"]))(*a["h_len"])
    st = NA.GenStats()
    args = dict(sessions=sess, d_src=s.data_ptr(), h_len=h_len, p=C.byref(p), d_out=out.data_ptr())
    for k in a["null"]:
        args[k] = None
    rc = native._lib.ttx_sample_speculative_generate_pool(args["sessions"], 1, args["d_src"], S_total, a["Ls_all"], args["h_len"], None,
                                                          a["capacity"], args["p"], args["d_out"], C.byref(st), native._stream())
    torch.cuda.synchronize()
    return rc, out.cpu()


def test_refused_arguments(tta, models, src, c_token):
    native = models["tiny"][0]
    bad = [dict(num_samples=0), dict(temperature=-0.5), dict(temperature=float("nan")), dict(top_k=-1), dict(top_k=33), dict(top_p=0.0),
           dict(top_p=1.01), dict(max_len=0), dict(pad=3), dict(n_drafts=0), dict(draft_len=0), dict(draft_len=17), dict(replace=PAD),
           dict(replace=EOS), dict(eos=PAD), dict(max_len=4990, draft_len=10), dict(capacity=1), dict(capacity=0), dict(capacity=4097),
           dict(h_len=[200, 3, 3, 3], Ls_all=100), dict(null=("sessions",)), dict(null=("d_src",)), dict(null=("h_len",)),
           dict(null=("p",)), dict(null=("d_out",))]
    for kw in bad:
        rc, out = pool_call(tta, native, src, c_token, **kw)
        assert rc == -1, f"{kw}: code {rc}"
        assert (out == -7).all(), f"{kw}: d_out was written"
    rc, out = pool_call(tta, native, src, c_token)
    assert rc == 0 and (out[:, :, 0] == BOS).all() and (out != -7).all()      # and the session still works
    rc, out = pool_call(tta, native, src, c_token, S_total=0)                 # an empty list is no error and launches nothing
    assert rc == 0 and (out == -7).all()


def test_slot_width_beyond_the_positional_table_is_refused(tta, c_token):
    from translation_transformer_amd import _native as NA
    st, cfg = tiny_state()
    native = tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0, max_positions=256)
    width = 300                                           # a slot as wide as the longest source: beyond the 256 positions
    s = torch.full((1, width), 5, dtype=torch.int64, device="cuda")
    p = NA.SampleSpecParams(NA.SampleParams(16, 2, 1.0, 0, 1.0, PAD, BOS, EOS, SEED), 4, 3, c_token, 0)
    out = torch.full((1, 2, 16), -7, dtype=torch.int64, device="cuda")
    sess = (C.c_void_p * 1)(native.session.value)
    rc = native._lib.ttx_sample_speculative_generate_pool(sess, 1, s.data_ptr(), 1, width, (C.c_int32 * 1)(width), None, 8, C.byref(p),
                                                          out.data_ptr(), None, native._stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == -7).all())


# -- no graph shared with the greedy pool ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_greedy_pool_and_sampling_pool_share_no_graph(tta, models, src, c_token, name, monkeypatch):
    """The two pools at the same shape (capacity, slot width, N, D, max_len), alternating on one session so that every call replays
    what an earlier call captured: each returns what it returns alone."""
    native = models[name][0]
    monkeypatch.setenv("TTX_POOL_SESSIONS", "1")
    four = src[:4]                                        # 4 rows x 1 = 4 slots; 1 source x 4 samples = 4 slots
    rows = [four[i:i + 1].cuda() for i in range(4)]

    def greedy():
        g = tta.TranslationInferenceGreedySpeculative(native, MAX_LEN, DRAFT_LEN, N_DRAFTS, PAD, BOS, EOS, c_token)
        return torch.cat(g.generate_many(rows, reorder=True, group_size=4), 0)

    def sampling():
        return pooled(gen(tta, native, c_token, temperature=2.0), src[:1], [1], KEYS[:1], capacity=4)

    g0, s0 = greedy(), sampling()
    for _ in range(3):
        assert torch.equal(greedy(), g0), f"{name}: the greedy pool changed after a sampling pool call of its shape"
        assert np.array_equal(sampling(), s0), f"{name}: the sampling pool changed after a greedy pool call of its shape"
    alone = tta.TranslationInferenceGreedySpeculative(native, MAX_LEN, DRAFT_LEN, N_DRAFTS, PAD, BOS, EOS, c_token)
    assert torch.equal(torch.cat([alone.generate(r) for r in rows], 0), g0)


# -- Lightning ---------------------------------------------------------------------------------------------------------------------
def lightning_module(tta, tmp_path, tag):
    from test_gpu_lightning_surface import FixtureTokenizer
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    mod = tta.VanillaEncoderDecoderTransformerLightning(
        src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
        num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
        share_embeddings=True, generation="sampling_speculative", beam_size=3, max_len=40, draft_len=4, n_drafts=3,
        sampling_temperature=2.0, sampling_top_k=8, sampling_top_p=0.95, sampling_seed=11, report_prediction_file=str(tmp_path / f"{tag}.txt"))
    mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    return mod


def test_lightning_pools_on_request_only(tta, tmp_path, monkeypatch):
    from translation_transformer_amd import decoding as D
    src, tgt, _, _ = fixture_tokens()
    calls = []
    real = D.TranslationInferenceSamplingSpeculative.generate_many
    monkeypatch.setattr(D.TranslationInferenceSamplingSpeculative, "generate_many",
                        lambda self, *a, **kw: (calls.append(len(a[0])), real(self, *a, **kw))[1])
    preds = {}
    for tag, pool, bs in (("off", False, 4), ("on4", True, 4), ("on1", True, 1)):
        mod = lightning_module(tta, tmp_path, tag)
        mod.predict_sample_pool = pool
        batches = [{"src_tokens": src[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda()} for i in range(0, 8, bs)]
        before = len(calls)
        preds[tag] = torch.cat(tta.run_predict(mod, batches), 0)
        if pool:
            assert len(calls) > before, "the opt-in did not decode through generate_many"
            assert mod._ahead is not None and mod._ahead.served == len(batches) and mod._predict_rows == 8
        else:
            assert len(calls) == before, "the default predict path called generate_many"
    assert preds["off"].shape == (8, 3, 40)
    # the excuse rule of the other comparisons, under the module's settings: the reactions' running indices are the keys
    from oracle.model import OracleTransformer, config_from_state
    from test_gpu_sampling import oracle_logits
    st, cfg = tiny_state()
    o64 = OracleTransformer(config_from_state(st, cfg["num_heads"]), st, dtype=torch.float64)
    off = preds["off"].cpu().numpy().reshape(24, 40)
    lg = oracle_logits(o64, src[:8], off, 3)
    end = S.ends(off, PAD, EOS)
    for tag in ("on4", "on1"):
        excused("tiny", f"the per-batch rows (lightning {tag})", preds[tag].cpu().numpy().reshape(24, 40), off, lg, end, 2.0, 3,
                keys=np.arange(8), seed=11, top_k=8, top_p=0.95)
