"""TranslationInferenceStochasticBeamSearch.generate_many (ttx_sbs_generate_pool) end to end, on the tiny golden model and on the
four-head model of tests/golden/h4_*: the ten fixture sources (lengths 28 .. 127) in batches [4, 4, 2] with mixed 64-bit keys,
K = 5.  The per-batch call is the oracle and every comparison is on the bits: tokens, logp, gumbel, finished.

  max_len 24        every source hits the cap
  max_len 150       at the temperature of {0.5, 1.0} the test picks from the per-batch output: at least three sources have all K rows
                    ended by EOS at pairwise different levels and at least one has not, so retirement is staggered and slots are
                    reused beside running sources (both models, float64 oracle on the CPU: temperature 1.0 qualifies)
  invariance        capacity 1 / 3 / 10 / default, pools in flight 1 / 2, the list reversed, batching [10] against [1] x 10
  filter, prefixes  top_k = 8 with top_p = 0.9, top_k = 1, prefixes of lengths {3, 0, 5, 1, ...} with one that forces EOS
  nesting           pooled K = 3 is the first three rows of pooled K = 5
  counters          running_rows equals the sum over the per-batch calls exactly (both loops run unfinished candidates only)
  the rest          default keys, order="logp", return_scores, [], an empty batch in the list, refusals, run to run, no graph shared
                    with the beam-speculative pool, Lightning
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_sampling import states
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
SEED = 20190611
K = 5
SIZES = [4, 4, 2]
KEYS = np.array([5, 1 << 40, 7, -3, 11, (1 << 33) + 1, 0, 123456789, -(1 << 35), 42], dtype=np.int64)


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def models(tta):
    out = {}
    for name in ("tiny", "h4"):
        st, cfg = states(name)
        out[name] = tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0)
    return out


@pytest.fixture(scope="module")
def src():
    s = fixture_tokens()[0]
    assert s.shape[0] == 10
    return s[:, :int((s != PAD).sum(1).max())]


def split(x, sizes=SIZES):
    out, r0 = [], 0
    for b in sizes:
        out.append(x[r0:r0 + b])
        r0 += b
    return out


def trimmed(s):
    """A batch as a dataloader pads it: to its own longest source."""
    return s[:, :max(2, int((s != PAD).sum(1).max()))] if s.shape[0] else s[:, :2]


def batches_of(src, sizes=SIZES):
    return [trimmed(b).cuda() for b in split(src, sizes)]


def sbs(tta, native, max_len, k=K, temperature=1.0, **kw):
    return tta.TranslationInferenceStochasticBeamSearch(native, k, max_len, PAD, BOS, EOS, temperature=temperature, seed=SEED, **kw)


def cat(results):
    """[(out, details), ...] per batch -> (tokens, logp, gumbel, finished) as arrays over all sources."""
    return (torch.cat([r[0] for r in results], 0).cpu().numpy(), torch.cat([r[1].logp for r in results], 0).cpu().numpy(),
            torch.cat([r[1].gumbel for r in results], 0).cpu().numpy(), torch.cat([r[1].finished for r in results], 0).cpu().numpy())


def per_batch(g, src, sizes=SIZES, keys=KEYS, prefixes=None):
    res = []
    for i, (b, k) in enumerate(zip(batches_of(src, sizes), split(keys, sizes))):
        res.append(g.generate(b, row_keys=k, return_details=True, prefix=None if prefixes is None else prefixes[i]))
    return cat(res)


def pooled(g, src, sizes=SIZES, keys=KEYS, **kw):
    res = g.generate_many(batches_of(src, sizes), row_keys=None if keys is None else split(keys, sizes), return_details=True, **kw)
    assert all(r[1].trace is None for r in res)
    assert [tuple(r[0].shape) for r in res] == [(b, g.beam_size, g.max_len) for b in sizes]
    return cat(res)


def same(a, b, what):
    for x, y, part in zip(a, b, ("tokens", "logp", "gumbel", "finished")):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {part} differ"


_REF = {}


def reference(tta, models, src, name, max_len, temperature=1.0):
    """The per-batch rows of a setting, computed once and shared (never modified), with the per-batch counters."""
    key = (name, max_len, temperature)
    if key not in _REF:
        g = sbs(tta, models[name], max_len, temperature=temperature)
        _REF[key] = (per_batch(g, src), g.b_sz, g.model_calls_num)
    return _REF[key]


def staggered_temperature(tta, models, src, name):
    """The temperature of {0.5, 1.0} at which the per-batch output at max_len 150 exercises staggered retirement."""
    for T in (1.0, 0.5):
        tok = reference(tta, models, src, name, 150, T)[0][0]
        ended = (tok[:, :, 1:] == EOS).any(-1).all(-1)                                  # all K rows of the source ended by EOS
        level = (tok != PAD).sum(-1).max(-1) - 1                                         # the level its longest row ended at
        if len(set(level[ended].tolist())) >= 3 and (~ended).any():
            return T
    pytest.fail("fixture does not exercise staggered retirement")


# -- pooled equals per-batch, counters ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_len", [24, 150])
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_pooled_equals_per_batch(tta, models, src, name, max_len):
    T = staggered_temperature(tta, models, src, name) if max_len == 150 else 1.0
    ref, ref_rows, ref_calls = reference(tta, models, src, name, max_len, T)
    if max_len == 24:
        assert not ref[3].all(1).any(), "a source finished before max_len 24: the case is meant to hit the cap"
    g = sbs(tta, models[name], max_len, temperature=T)
    same(pooled(g, src), ref, f"{name} max_len {max_len} T {T}")
    st = g.last_stats
    print(f"{name} max_len {max_len} T {T}: pooled {st.model_calls} iterations, {st.running_rows} running rows; per batch "
          f"{ref_calls} iterations, {ref_rows} running rows")
    assert st.running_rows == ref_rows == g.b_sz, "running rows: the pool's sum differs from the per-batch calls'"
    assert st.model_calls > 0 and g.model_calls_num == st.model_calls and st.src_tokens_padded >= int((src != PAD).sum())
    assert g.given_tokens == int((src != PAD).sum())
    # the shares of the batches: exactly what generate(batch) counts in candidates and tokens, and decoder passes that sum to the call's
    shares = g.last_batch_counters
    one = sbs(tta, models[name], max_len, temperature=T)
    for sh, b, k in zip(shares, batches_of(src), split(KEYS)):
        before = (one.b_sz, one.given_tokens)
        one.generate(b, row_keys=k)
        assert sh["b_sz"] == one.b_sz - before[0] and sh["given_tokens"] == one.given_tokens - before[1]
    assert sum(sh["model_calls_num"] for sh in shares) == st.model_calls and sum(sh["b_sz"] for sh in shares) == st.running_rows


# -- invariance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_invariance(tta, models, src, name):
    T = staggered_temperature(tta, models, src, name)
    ref = reference(tta, models, src, name, 150, T)[0]
    g = sbs(tta, models[name], 150, temperature=T)
    for kw in (dict(capacity=1), dict(capacity=3), dict(capacity=10), dict(in_flight=1), dict(in_flight=2), dict(capacity=3, in_flight=2)):
        same(pooled(g, src, **kw), ref, f"{name} {kw}")
    # capacity 3: slots are reused at mixed levels, fresh sources beside running ones
    assert g.last_group_size == 3
    rev = g.generate_many(batches_of(src)[::-1], row_keys=split(KEYS)[::-1], return_details=True, capacity=3)
    same(cat(rev[::-1]), ref, f"{name} reversed list")
    same(pooled(g, src, [10]), ref, f"{name} one batch of ten")
    same(pooled(g, src, [1] * 10, capacity=4), ref, f"{name} ten batches of one")


def test_run_to_run(tta, models, src):
    g = sbs(tta, models["tiny"], 150)
    a = pooled(g, src, capacity=3)
    for _ in range(2):
        same(pooled(g, src, capacity=3), a, "run to run")


# -- filter and prefixes ------------------------------------------------------------------------------------------------------------
def make_prefixes(ref_tokens):
    """Per batch a Long[B, 5]: lengths {3, 0, 5, 1, ...} cut from the unprompted rank-1 rows (so that they are plausible tokens), and
    source 4's a forced EOS after two tokens."""
    lens = [3, 0, 5, 1, 2, 4, 0, 5, 1, 3]
    tab = torch.full((10, 5), PAD, dtype=torch.int64)
    for b, n in enumerate(lens):
        tab[b, :n] = torch.from_numpy(ref_tokens[b, 1, 1:1 + n])
    tab[4, 2] = EOS
    return split(tab)


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_filter_and_prefixes(tta, models, src, name):
    native = models[name]
    for kw in (dict(top_k=8, top_p=0.9), dict(top_k=1)):
        g = sbs(tta, native, 40, **kw)
        ref = per_batch(g, src)
        same(pooled(g, src, capacity=3), ref, f"{name} {kw}")
        same(pooled(g, src), ref, f"{name} {kw} default capacity")
        if kw.get("top_k") == 1:
            assert (ref[2][:, 0] == 0).all() and np.isneginf(ref[2][:, 1:]).all()
    prefixes = make_prefixes(reference(tta, models, src, name, 24)[0][0])
    for kw in (dict(), dict(top_k=8, top_p=0.9)):
        g = sbs(tta, native, 40, **kw)
        ref = per_batch(g, src, prefixes=prefixes)
        assert (ref[0][4, 0, 1:4] == np.array(prefixes[1][0, :3])).all() and np.isneginf(ref[2][4, 1:]).all(), "the forced EOS"
        same(pooled(g, src, prefixes=prefixes, capacity=3), ref, f"{name} prefixes {kw}")
        same(pooled(g, src, prefixes=prefixes), ref, f"{name} prefixes {kw} default capacity")
        mixed = [prefixes[0], None, prefixes[2]]
        ref_mixed = per_batch(g, src, prefixes=mixed)
        same(pooled(g, src, prefixes=mixed, capacity=4), ref_mixed, f"{name} prefixes on two of three batches {kw}")


# -- nesting --------------------------------------------------------------------------------------------------------------------------
def test_k3_is_the_first_three_rows_of_k5(tta, models, src):
    five = pooled(sbs(tta, models["tiny"], 150), src, capacity=3)
    three = pooled(sbs(tta, models["tiny"], 150, k=3), src, capacity=3)
    same(three, tuple(x[:, :3] for x in five), "K = 3 against the first three rows of K = 5")


# -- the rest -------------------------------------------------------------------------------------------------------------------------
def test_default_keys_order_scores_and_empty_lists(tta, models, src):
    native = models["tiny"]
    g = sbs(tta, native, 24)
    bs = batches_of(src)
    a = g.generate_many(bs)
    b = g.generate_many(bs, row_keys=split(np.arange(10)))
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "default keys are the running index"
    off = 0
    for x, s in zip(a, bs):
        assert torch.equal(x, g.generate(s, row_keys=np.arange(off, off + s.shape[0])))
        off += s.shape[0]
    by_logp = g.generate_many(bs, row_keys=split(KEYS), order="logp", return_details=True)
    for (out, d), s, k in zip(by_logp, bs, split(KEYS)):
        o2, d2 = g.generate(s, row_keys=k, order="logp", return_details=True)
        assert torch.equal(out, o2) and torch.equal(d.logp, d2.logp) and torch.equal(d.gumbel, d2.gumbel)
        assert bool((d.logp[:, :-1] >= d.logp[:, 1:]).all())
    scored = g.generate_many(bs, row_keys=split(KEYS), return_scores=True)
    for (out, sc), s, k in zip(scored, bs, split(KEYS)):
        o2, sc2 = g.generate(s, row_keys=k, return_scores=True)
        assert torch.equal(out, o2) and torch.equal(sc.score, sc2.score)
    assert g.generate_many([]) == []
    empty = src[:0, :2].cuda()
    with_empty = g.generate_many([bs[0], empty, bs[1]], row_keys=[KEYS[:4], [], KEYS[4:8]])
    assert tuple(with_empty[1].shape) == (0, K, 24)
    assert torch.equal(with_empty[0], g.generate(bs[0], row_keys=KEYS[:4])) and torch.equal(with_empty[2], g.generate(bs[1], row_keys=KEYS[4:8]))
    assert [tuple(x.shape) for x in g.generate_many([empty])] == [(0, K, 24)]


def test_refused_arguments(tta, models, src):
    native = models["tiny"]
    bs = batches_of(src)
    g = sbs(tta, native, 24)
    calls = g.model_calls_num
    with pytest.raises(ValueError):
        g.generate_many(bs, capacity=0)
    with pytest.raises(ValueError):
        g.generate_many(bs, capacity=1025)                   # as the entry point refuses it, not clamped
    with pytest.raises(ValueError):
        g.generate_many(bs, row_keys=split(KEYS)[:2])
    with pytest.raises(ValueError):
        g.generate_many(bs, row_keys=[KEYS[:4], KEYS[4:8], KEYS[:3]])
    with pytest.raises(ValueError):
        g.generate_many(bs, prefixes=[None])
    with pytest.raises(ValueError):
        g.generate_many(bs, order="score")
    with pytest.raises(ValueError):
        g.generate_many(bs, prefixes=[torch.full((4, 30), 5), None, None])          # a prefix longer than max_len - 1
    assert g.model_calls_num == calls
    for kw, k, max_len in ((dict(temperature=0.0), 3, 24), (dict(temperature=float("nan")), 3, 24), (dict(), 33, 24), (dict(), 0, 24),
                           (dict(), 3, 1), (dict(), 3, 10 ** 6), (dict(top_k=33), 3, 24), (dict(top_p=0.0), 3, 24)):
        bad = tta.TranslationInferenceStochasticBeamSearch(native, k, max_len, PAD, BOS, EOS, seed=1, **kw)
        with pytest.raises(tta.TtxError) as e:
            bad.generate_many(bs)
        assert e.value.code == -1, (kw, k, max_len)
    with pytest.raises(tta.TtxError):
        tta.TranslationInferenceStochasticBeamSearch(native, 3, 24, PAD + 1, BOS, EOS).generate_many(bs)
    same(pooled(g, src), reference(tta, models, src, "tiny", 24)[0], "after the refusals")


def pool_call(native, src, **over):
    """ttx_sbs_generate_pool on the first four sources: (rc, out with a sentinel)."""
    from translation_transformer_amd import _native as NA
    s = src[:4].cuda().contiguous()
    a = dict(S_total=4, Ls_all=s.shape[1], h_len=[int(x) for x in (s != PAD).sum(1).tolist()], capacity=4, null=())
    a.update(over)
    p = NA.SbsParams(16, 3, 1.0, PAD, BOS, EOS, SEED)
    out = torch.full((4, 3, 16), -7, dtype=torch.int64, device="cuda")
    logp = torch.full((4, 3), -7.0, dtype=torch.float32, device="cuda")
    gum = torch.full((4, 3), -7.0, dtype=torch.float32, device="cuda")
    st = NA.SbsPoolStats()
    args = dict(sessions=(C.c_void_p * 1)(native.session.value), d_src=s.data_ptr(), h_len=(C.c_int32 * 4)(*a["h_len"]), p=C.byref(p),
                d_out=out.data_ptr(), d_logp=logp.data_ptr(), d_gumbel=gum.data_ptr(), stats=C.byref(st))
    for k in a["null"]:
        args[k] = None
    rc = native._lib.ttx_sbs_generate_pool(args["sessions"], 1, args["d_src"], a["S_total"], a["Ls_all"], args["h_len"], None, a["capacity"],
                                           args["p"], None, None, 0, None, args["d_out"], args["d_logp"], args["d_gumbel"], args["stats"],
                                           native._stream())
    torch.cuda.synchronize()
    return rc, out.cpu(), logp.cpu()


def test_refused_arguments_of_the_entry_point(tta, models, src):
    native = models["tiny"]
    for kw in (dict(capacity=0), dict(capacity=1025), dict(h_len=[200, 30, 30, 30]), dict(h_len=[1, 30, 30, 30]), dict(null=("sessions",)),
               dict(null=("d_src",)), dict(null=("h_len",)), dict(null=("p",)), dict(null=("d_out",)), dict(null=("d_logp",)),
               dict(null=("d_gumbel",)), dict(null=("stats",))):
        rc, out, logp = pool_call(native, src, **kw)
        assert rc == -1, f"{kw}: code {rc}"
        assert (out == -7).all() and (logp == -7).all(), f"{kw}: an output was written"
    rc, out, logp = pool_call(native, src)
    assert rc == 0 and (out[:, :, 0] == BOS).all() and (out != -7).all() and (logp != -7).all()
    rc, out, logp = pool_call(native, src, S_total=0)
    assert rc == 0 and (out == -7).all()


# -- no graph shared with the beam-speculative pool ---------------------------------------------------------------------------------
def test_shares_no_graph_with_the_beam_speculative_pool(tta, models, src, monkeypatch):
    """The two pools at the same capacity, K and max_len, alternating on one session so that every call replays what an earlier call
    captured: each returns what it returns alone.  A proxy: the separation itself is by construction (the pool's iterations are keyed
    under a graph site of their own, GS_SBS_POOL_ITER), and two iterations that shared a key but happened to be compatible would pass
    here too; what this shows is that neither pool's results change when the other has captured graphs on the same session."""
    native = models["tiny"]
    monkeypatch.setenv("TTX_POOL_SESSIONS", "1")
    c = fixture_tokens()[2]
    bs = batches_of(src[:4], [4])

    def beam():
        g = tta.TranslationInferenceBeamSearchSpeculative(native, 24, K, 4, 3, native.tgt_vocab_size, False, PAD, BOS, EOS, c, max_steps=100)
        return torch.cat(g.generate_many(bs, in_flight=1), 0)

    def stochastic():
        return pooled(sbs(tta, native, 24), src[:4], [4], KEYS[:4], capacity=4, in_flight=1)

    b0, s0 = beam(), stochastic()
    for _ in range(3):
        assert torch.equal(beam(), b0), "the beam-speculative pool changed after a stochastic pool call of its shape"
        same(stochastic(), s0, "the stochastic pool after a beam-speculative pool call of its shape")
    same(s0, per_batch(sbs(tta, native, 24), src[:4], [4], KEYS[:4]), "against the per-batch call")


# -- Lightning ------------------------------------------------------------------------------------------------------------------------
def test_lightning_pools_on_request_only(tta, tmp_path, monkeypatch):
    from test_gpu_lightning_surface import FixtureTokenizer, CsvWriter
    from translation_transformer_amd import decoding as D
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    s, tgt, _, _ = fixture_tokens()
    calls = []
    real = D.TranslationInferenceStochasticBeamSearch.generate_many
    monkeypatch.setattr(D.TranslationInferenceStochasticBeamSearch, "generate_many",
                        lambda self, *a, **kw: (calls.append(len(a[0])), real(self, *a, **kw))[1])
    preds, csv = {}, {}
    for tag, pool, bs in (("off1", False, 1), ("off4", False, 4), ("on4", True, 4), ("on1", True, 1)):
        mod = tta.VanillaEncoderDecoderTransformerLightning(
            src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
            num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
            share_embeddings=True, generation="stochastic_beam_search", beam_size=3, max_len=24, sampling_temperature=2.0,
            sampling_seed=11, report_prediction_file=str(tmp_path / f"{tag}.txt"))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        mod.predict_sample_pool = pool
        batches = [{"src_tokens": s[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda()} for i in range(0, 8, bs)]
        before = len(calls)
        preds[tag] = torch.cat(tta.run_predict(mod, batches, writer=CsvWriter(tmp_path / f"{tag}.csv")), 0)
        csv[tag] = (tmp_path / f"{tag}.csv").read_text()
        if pool:
            assert len(calls) > before, "the opt-in did not decode through generate_many"
            assert mod._ahead is not None and mod._ahead.served == len(batches) and mod._predict_rows == 8
        else:
            assert len(calls) == before, "the default predict path called generate_many"
    assert preds["off4"].shape == (8, 3, 24)
    for tag in ("off1", "on4", "on1"):
        assert torch.equal(preds[tag], preds["off4"]), tag
    assert csv["on4"] == csv["off4"] and csv["on1"] == csv["off1"], "the CSV rows of the pooled run differ from the default run's"
