"""Proposal drafts end to end: TranslationInferenceSamplingSpeculative.generate(proposal=) and .generate_many(proposals=) on the tiny
golden model, the ten fixture sources, max_len 40.

1  Invariance.  A proposal is offered, never forced, so every call returns the rows of the call without proposals, bit for bit: with
   the call's own output as proposal, that output with one substitution, one insertion, one deletion per row, random tokens, and
   empty proposals; at temperature 0 and 1, num_samples 1 and 3, (n_drafts, draft_len) = (1, 4) and (3, 10); through generate and
   through generate_many on the slot pool as it runs by default, with TTX_TWO_PHASE=0, with every step split (the two-phase step and
   draft select really running) and with TTX_DRAFT_SELECT=0.  This follows from the rule that the speculative sampler returns the
   plain sampler's rows; there is no tolerance.
2  Step bound.  With its own output as proposal, every row ending in EOS with room to spare, a single-session call takes at most
   max_b ceil(L_b / (draft_len + 1)) verify steps (L_b: emitted tokens, EOS included), strictly fewer than without proposals.  The
   sources are chosen on the oracle: its greedy-speculative rows end in EOS before column 30 and need more steps than the bound.
3  Empty proposals: the same device steps and the same counters as the plain call.
4  Refusals.  5  Lightning passes batch["proposal_tokens"] through with the pool on and off, at batch sizes 4 and 1.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import util_proposal as Q
import util_sample_checks as S
from test_gpu_sampling import SEED
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
MAX_LEN = 40
KEYS = np.arange(10, dtype=np.int64) * 7 + 3
SIZES = (3, 4, 3)
COUNTERS = ("model_calls", "accepted_tokens", "produced_tokens", "verified_positions", "kv_prefix_positions", "src_positions")
KINDS = ("own", "sub", "ins", "del", "random", "empty")
ENDING = [4, 6, 9]                            # sources whose temperature-0 rows end in EOS well before max_len (checked on the oracle)


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def native(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0)


@pytest.fixture(scope="module")
def src():
    s = fixture_tokens()[0]
    assert s.shape[0] == 10
    return s[:, :int((s != PAD).sum(1).max())]


@pytest.fixture(scope="module")
def c_token():
    return fixture_tokens()[2]


def spec(tta, native, c, N_, D, **kw):
    return tta.TranslationInferenceSamplingSpeculative(native, MAX_LEN, D, N_, PAD, BOS, EOS, c, **kw)


def padded(rows, width=None) -> torch.Tensor:
    width = max([len(r) for r in rows] + [0]) if width is None else width
    out = torch.full((len(rows), width), PAD, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor([int(t) for t in r], dtype=torch.int64)
    return out


def proposals_of(base: torch.Tensor, kind: str, V: int, rng) -> torch.Tensor:
    """Long[B, Lq]: per source the proposal of ``kind`` made from sample 0's row of ``base`` [B, n, max_len]."""
    rows = []
    for b in range(base.shape[0]):
        t = Q.row_tokens(base[b, 0].tolist(), PAD, EOS)
        other = int(rng.integers(3, V))
        if kind in ("sub", "ins", "del"):
            t = Q.perturbed(t, kind, len(t) // 2, other)
        elif kind == "random":
            t = [int(x) for x in rng.integers(3, V, size=len(t))]
        elif kind == "empty":
            t = []
        rows.append(t[:MAX_LEN - 1])
    return padded(rows)


def pooled(g, s, proposal, **kw):
    cuts = np.concatenate([[0], np.cumsum(SIZES)])
    parts = [slice(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    outs = g.generate_many([s[p].cuda() for p in parts], row_keys=[KEYS[p] for p in parts],
                           proposals=None if proposal is None else [proposal[p] for p in parts], **kw)
    return torch.cat(outs, 0)


def counters(st) -> tuple:
    return tuple(int(getattr(st, k)) for k in COUNTERS)


# -- 1 ----------------------------------------------------------------------------------------------------------------------------
ENVS = [dict(), dict(TTX_TWO_PHASE="0"), dict(TTX_TWO_PHASE_MIN_ROWS="0"), dict(TTX_DRAFT_SELECT="0", TTX_TWO_PHASE_MIN_ROWS="0")]


@pytest.mark.parametrize("N_,D", [(1, 4), (3, 10)])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("T", [0.0, 1.0])
def test_no_proposal_changes_a_row(tta, native, src, c_token, monkeypatch, T, n, N_, D):
    rng = np.random.default_rng(int(T) * 100 + n * 10 + D)
    kw = dict(temperature=T, num_samples=n, seed=SEED)
    g0 = spec(tta, native, c_token, N_, D, **kw)
    base = g0.generate(src.cuda(), row_keys=KEYS)
    base_calls = int(g0.last_stats.model_calls)
    assert base.shape == (10, n, MAX_LEN)
    base_cpu = base.cpu()
    for kind in KINDS:
        prop = proposals_of(base_cpu, kind, native.tgt_vocab_size, rng)
        what = f"T {T} n {n} N {N_} D {D} {kind}"
        g = spec(tta, native, c_token, N_, D, **kw)
        out = g.generate(src.cuda(), row_keys=KEYS, proposal=prop)
        assert torch.equal(out, base), f"{what}: generate"
        if kind == "own":
            assert int(g.last_stats.model_calls) <= base_calls, f"{what}: the rows' own tokens as proposal cost steps"
        for env in ENVS:
            with monkeypatch.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)
                out = pooled(spec(tta, native, c_token, N_, D, **kw), src, prop, capacity=4 * n)
                assert torch.equal(out, base), f"{what}: generate_many under {env}"


# -- 2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_rows(src, c_token):
    """(N, D) -> (the oracle's greedy-speculative rows of the ENDING sources, its verify steps for them as one batch)."""
    from oracle.model import OracleTransformer, config_from_state
    from oracle.decoding import GreedySpeculativeOracle
    st, cfg = tiny_state()
    o = OracleTransformer(config_from_state(st, cfg["num_heads"]), st)
    out = {}
    for N_, D in ((1, 4), (3, 10)):
        g = GreedySpeculativeOracle(o, MAX_LEN, D, N_, PAD, BOS, EOS, c_token)
        out[(N_, D)] = (g.generate(src[ENDING]).reshape(len(ENDING), -1)[:, :MAX_LEN].numpy(), int(g.model_calls_num))
    return out


@pytest.mark.parametrize("N_,D", [(1, 4), (3, 10)])
def test_own_output_as_proposal_meets_the_step_bound(tta, native, src, c_token, oracle_rows, N_, D):
    rows, oracle_steps = oracle_rows[(N_, D)]
    emitted = S.ends(rows, PAD, EOS)
    assert (rows[np.arange(len(ENDING)), emitted] == EOS).all() and int(emitted.max()) < 30, "a source does not end with room to spare"
    bound = int(max(-(-int(L) // (D + 1)) for L in emitted))
    assert oracle_steps > bound, "the oracle's unproposed call already meets the bound: these sources show nothing"
    s = src[ENDING].cuda()
    g0 = spec(tta, native, c_token, N_, D, temperature=0.0, seed=SEED)
    base = g0.generate(s, row_keys=KEYS[ENDING])
    assert np.array_equal(base[:, 0].cpu().numpy(), rows), "the temperature-0 rows are not the oracle's greedy-speculative rows"
    plain_calls = int(g0.last_stats.model_calls)
    g = spec(tta, native, c_token, N_, D, temperature=0.0, seed=SEED)
    out = g.generate(s, row_keys=KEYS[ENDING], proposal=base[:, 0, 1:].cpu())
    calls = int(g.last_stats.model_calls)
    print(f"N {N_} D {D}: model_calls {calls} with the own output as proposal, {plain_calls} without, bound {bound}")
    assert torch.equal(out, base)
    assert calls <= bound, (calls, bound)
    assert calls < plain_calls, (calls, plain_calls)


# -- 3 ----------------------------------------------------------------------------------------------------------------------------
def test_empty_proposals_are_the_plain_call(tta, native, src, c_token):
    kw = dict(temperature=1.0, num_samples=2, seed=SEED)
    s = src.cuda()
    empties = [None, torch.zeros((10, 0), dtype=torch.int64), torch.full((10, 5), PAD, dtype=torch.int64)]
    g = spec(tta, native, c_token, 3, 4, **kw)
    base = g.generate(s, row_keys=KEYS)
    want = counters(g.last_stats)
    gp = spec(tta, native, c_token, 3, 4, **kw)
    base_pool = pooled(gp, src, None, capacity=8)
    want_pool = counters(gp.last_stats)
    assert want[0] > 0 and want_pool[0] > 0 and torch.equal(base_pool, base)
    for p in empties:
        g = spec(tta, native, c_token, 3, 4, **kw)
        assert torch.equal(g.generate(s, row_keys=KEYS, proposal=p), base)
        assert counters(g.last_stats) == want, "an empty proposal changed the counters"
        g = spec(tta, native, c_token, 3, 4, **kw)
        assert torch.equal(pooled(g, src, p, capacity=8), base)
        assert counters(g.last_stats) == want_pool, "an empty proposal changed the pool's counters"


# -- 4 ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(tta, native, src, c_token):
    from translation_transformer_amd import _native as N
    g = spec(tta, native, c_token, 3, 4, temperature=1.0, seed=SEED)
    s = src[:2].cuda()
    V = native.tgt_vocab_size
    ok = torch.full((2, MAX_LEN - 1), 5, dtype=torch.int64)
    g.generate(s, proposal=ok)                                             # max_len - 1 tokens fit
    for bad in (torch.full((2, MAX_LEN), 5, dtype=torch.int64),            # longer than max_len - 1
                torch.tensor([[5, 6]]),                                    # one row for two sources
                torch.tensor([5, 6]),                                      # not a matrix
                torch.tensor([[5, PAD, 6], [5, 6, 7]]),                    # a token after a PAD
                torch.tensor([[V, 5], [5, 5]]),                            # outside the vocabulary
                torch.tensor([[0.5, 1.0], [1.0, 2.0]])):
        with pytest.raises(ValueError):
            g.generate(s, proposal=bad)
        with pytest.raises(ValueError):
            g.generate_many([s], proposals=[bad])
    with pytest.raises(ValueError):
        g.generate(s, prefix=ok[:, :3], proposal=ok)
    with pytest.raises(ValueError):
        g.generate_many([s], prefixes=[ok[:, :3]], proposals=[ok])
    with pytest.raises(ValueError):
        g.generate_many([s], proposals=[ok, ok])                          # one entry per batch
    # the C side: both tables non-empty, a length beyond max_len - 1, a length beyond ld_proposal, a null table with a length
    p = N.SampleSpecParams(N.SampleParams(MAX_LEN, 1, 1.0, 0, 1.0, PAD, BOS, EOS, SEED), 4, 3, c_token, 0)
    out = torch.empty((2, 1, MAX_LEN), dtype=torch.int64, device="cuda")
    tab = ok.cuda()
    lens = lambda *v: (C.c_int32 * 2)(*v)

    def call(pre, ld_pre, plen, prop, ld_prop, qlen):
        st = N.GenStats()
        return native._lib.ttx_sample_speculative_generate_proposal(native.session, s.data_ptr(), 2, int(s.shape[1]), None, C.byref(p), pre,
                                                                    ld_pre, plen, prop, ld_prop, qlen, out.data_ptr(), C.byref(st),
                                                                    native._stream())
    assert call(None, 0, None, tab.data_ptr(), MAX_LEN - 1, lens(3, 0)) == N.TTX_OK
    assert call(tab.data_ptr(), MAX_LEN - 1, lens(2, 0), None, 0, None) == N.TTX_OK            # the prompted call
    assert call(tab.data_ptr(), MAX_LEN - 1, lens(2, 0), tab.data_ptr(), MAX_LEN - 1, lens(0, 0)) == N.TTX_OK
    assert call(tab.data_ptr(), MAX_LEN - 1, lens(2, 0), tab.data_ptr(), MAX_LEN - 1, lens(0, 3)) == N.TTX_ERR_INVALID
    assert call(None, 0, None, tab.data_ptr(), MAX_LEN - 1, lens(MAX_LEN, 0)) == N.TTX_ERR_INVALID
    assert call(None, 0, None, tab.data_ptr(), 2, lens(3, 0)) == N.TTX_ERR_INVALID
    assert call(None, 0, None, None, 4, lens(3, 0)) == N.TTX_ERR_INVALID
    assert call(None, 0, None, tab.data_ptr(), -1, lens(0, 0)) == N.TTX_ERR_INVALID
    torch.cuda.synchronize()
    # what stays as it is
    for cls_args in ((tta.TranslationInferenceGreedy, (native, MAX_LEN, PAD, BOS, EOS)),
                     (tta.TranslationInferenceGreedySpeculative, (native, MAX_LEN, 4, 3, PAD, BOS, EOS, c_token))):
        gen = cls_args[0](*cls_args[1])
        with pytest.raises(TypeError):
            gen.generate(s, prefix=ok[:, :3])
        with pytest.raises(TypeError):
            gen.generate(s, proposal=ok)
    with pytest.raises(TypeError):
        tta.TranslationInferenceSampling(native, MAX_LEN, PAD, BOS, EOS).generate(s, proposal=ok)


# -- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_lightning_passes_proposal_tokens_through(tta, tmp_path):
    from test_gpu_lightning_surface import FixtureTokenizer
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    src, tgt, _, _ = fixture_tokens()

    def module(generation, tag):
        mod = tta.VanillaEncoderDecoderTransformerLightning(
            src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
            num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
            share_embeddings=True, generation=generation, beam_size=3, max_len=MAX_LEN, draft_len=4, n_drafts=3, sampling_temperature=1.0,
            sampling_top_k=8, sampling_top_p=0.95, sampling_seed=11, report_prediction_file=str(tmp_path / f"{tag}.txt"))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        return mod

    free = torch.cat(tta.run_predict(module("sampling_speculative", "free"), [{"src_tokens": src[:4].cuda(), "tgt_tokens": tgt[:4].cuda()}]), 0).cpu()
    assert free.shape == (4, 3, MAX_LEN)
    prop = padded([Q.row_tokens(free[b, 0].tolist(), PAD, EOS)[:MAX_LEN - 1] for b in range(4)])
    calls = {}                                         # accepted draft tokens of each run
    for pool, bs in ((False, 4), (False, 1), (True, 4), (True, 1)):
        mod = module("sampling_speculative", f"prop{pool}{bs}")
        mod.predict_sample_pool = pool
        batches = [{"src_tokens": src[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda(), "proposal_tokens": prop[i:i + bs]} for i in range(0, 4, bs)]
        out = torch.cat(tta.run_predict(mod, batches), 0).cpu()
        assert torch.equal(out, free), f"pool {pool} bs {bs}: a proposal changed the rows"
        if pool:
            assert mod._ahead is not None and mod._ahead.served == len(batches), "the look-ahead path did not serve the proposed batches"
        calls[(pool, bs)] = int(mod.generator.accepted_tokens_num)
    plain = module("sampling_speculative", "plain4")
    tta.run_predict(plain, [{"src_tokens": src[:4].cuda(), "tgt_tokens": tgt[:4].cuda()}])
    # sample 0 of every source is its own proposal: nearly all of its tokens are accepted draft tokens
    assert min(calls.values()) > int(plain.generator.accepted_tokens_num), "the proposals did not reach the generator"
    for generation in ("sampling", "greedy_speculative"):
        with pytest.raises(ValueError):
            tta.run_predict(module(generation, generation), [{"src_tokens": src[:2].cuda(), "tgt_tokens": tgt[:2].cuda(), "proposal_tokens": prop[:2]}])
    with pytest.raises(ValueError):                    # stays as it is
        tta.run_predict(module("greedy_speculative", "gp"), [{"src_tokens": src[:2].cuda(), "tgt_tokens": tgt[:2].cuda(), "prefix_tokens": prop[:2, :3]}])
