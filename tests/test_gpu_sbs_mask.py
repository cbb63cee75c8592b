"""TranslationInferenceStochasticBeamSearch under top_k / top_p and a forced prefix (ttx_sbs_generate_ex, k_sbs_step_masked) end to
end on the tiny golden model (V = 30): the exact consequences of the rule (include/ttx.h), refusals, the Lightning surface, a
level-by-level replay against the float64 oracle, the rows' tokens against the float64 kept sets, and logp against score().

Exact: a kept set of every token (V = 30 <= 32, top_k = 32, top_p = 1) gives the unfiltered call's outputs bit for bit; top_k = 1
gives the greedy row with logp == gumbel == 0.0f and -inf, finished rows behind it; an empty prefix with the filter off is
ttx_sbs_generate (rows, logp, gumbel, trace, model_calls); a prompted call's finite rows are BOS, the prefix, a completion, rank 0
has gumbel 0.0f, rows are distinct, K is the first K of K + 2, a source alone is the source in a batch, a wider pad changes nothing.

The replay is tests/test_gpu_sbs.py's with the masked restatement (tests/util_sbs_mask_checks.py): every level's beam from the
trace, the float64 oracle on those prefixes, the float64 masked step from the device's own phi and G of the level before, the
checker with a margin of ten times the fp32 gap measured on the same levels on the CPU (fp32 oracle and float32 restatement against
float64, both on the float64 kept sets), and the kept-set excuse with the sampler kernel test's TOL.  At most 5 % of the ranks may be
excused.  Measured on an MI355X run of this file: fp32 gaps of the four sources 1.8e-6 .. 3.4e-6 (filtered), 1.2e-6 .. 2.1e-5
(prompted) and 2.3e-6 .. 1.1e-5 (both), the margins ten times that, and 0, 0 and 1 of the 460 ranks excused.

logp.  At temperature 1 with the filter off, logp of a prompted row is the sum of score()'s token_logp over the positions after
the prefix: both are held to the float64 oracle's sum within n * TOK_TOL * max(1, max |token logp|), n the completion's length
(tests/test_gpu_score.py's per-token bound).  With the filter on, logp is renormalised over the kept sets and is
>= that sum; the assertion allows the same n * tol below it, since both sides are fp32 sums within that of their exact values.
Measured: |logp - float64| is at most 3.8e-7 per completion token.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import util_sample_checks as P
import util_sbs_checks as S
import util_sbs_mask_checks as M
from test_gpu_sample_kernel import TOL
from test_gpu_score import TOK_TOL
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
SEED = 20190611
MAX_LEN = 24
T = 2.0
TOP_K, TOP_P = 8, 0.9
KEYS = [5, 1 << 40, 7, -3]
PREFIXES = [[5, 6, 7], [], [12, 13, 9, 4, 8], [9]]


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def model(tta):
    st, cfg = tiny_state()
    assert cfg["vocab_size"] <= 32                      # the full-mask consequence applies to this model
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


def padded(rows, width=None):
    w = max(len(r) for r in rows) if width is None else width
    out = torch.full((len(rows), w), PAD, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return out


def sbs(tta, model, K, **kw):
    kw.setdefault("temperature", T)
    return tta.TranslationInferenceStochasticBeamSearch(model, K, MAX_LEN, PAD, BOS, EOS, seed=SEED, **kw)


def run(tta, model, src, K, prefix=None, keys=KEYS, **kw):
    out, d = sbs(tta, model, K, **kw).generate(src.cuda(), row_keys=keys, return_details=True, trace=True,
                                               prefix=None if prefix is None else padded(prefix))
    return out.cpu().numpy(), d


@pytest.fixture(scope="module")
def plain5(tta, model, src):
    """The unfiltered, unprompted K = 5 call: computed once, shared, never modified."""
    return run(tta, model, src, 5)


@pytest.fixture(scope="module")
def runs(tta, model, src):
    """K = 5 under the filter, under the prefixes, and under both: computed once, shared, never modified."""
    return SimpleNamespace(filtered=run(tta, model, src, 5, top_k=TOP_K, top_p=TOP_P),
                           prompted=run(tta, model, src, 5, PREFIXES),
                           both=run(tta, model, src, 5, PREFIXES, top_k=TOP_K, top_p=TOP_P))


def ends(rows):
    stop = (rows[:, 1:] == EOS) | (rows[:, 1:] == PAD)
    return np.where(stop.any(1), stop.argmax(1) + 1, rows.shape[1] - 1)


def same_run(a, b, k=None, what=""):
    (oa, da), (ob, db) = a, b
    s = slice(None) if k is None else slice(0, k)
    assert (oa == ob[:, s]).all(), f"{what}: rows"
    assert torch.equal(da.logp, db.logp[:, s]) and torch.equal(da.gumbel, db.gumbel[:, s]), f"{what}: logp / gumbel"
    assert torch.equal(da.finished, db.finished[:, s]), f"{what}: finished"


# -- exact consequences -----------------------------------------------------------------------------------------------------------
def test_a_mask_of_all_tokens_is_the_unfiltered_search(tta, model, src, plain5):
    full = run(tta, model, src, 5, top_k=32, top_p=1.0)
    same_run(full, plain5, what="top_k 32 on V = 30")
    for a, b in zip(full[1].trace, plain5[1].trace):
        assert torch.equal(a, b)


def test_empty_prefix_and_filter_off_is_ttx_sbs_generate(tta, model, src, plain5):
    """The class (ttx_sbs_generate_ex with top_k 0, top_p 1) with no prefix, an all-PAD one and a zero-width one, against a direct
    ttx_sbs_generate call: rows, logp, gumbel, every level of the trace, model_calls."""
    from translation_transformer_amd import _native as N
    s = src.cuda().contiguous()
    B, K = s.shape[0], 5
    keys = torch.tensor(KEYS, dtype=torch.int64).cuda()
    out = torch.empty((B, K, MAX_LEN), dtype=torch.int64, device="cuda")
    logp, gum = torch.empty((B, K), device="cuda"), torch.empty((B, K), device="cuda")
    shape = (MAX_LEN - 1, B, K)
    tr = [torch.zeros(shape, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
    p = N.SbsParams(MAX_LEN, K, T, PAD, BOS, EOS, SEED)
    st = N.BeamSearchStats()
    N.check(model._lib.ttx_sbs_generate(model.session, s.data_ptr(), B, s.shape[1], keys.data_ptr(), C.byref(p), out.data_ptr(),
                                        logp.data_ptr(), gum.data_ptr(), C.byref(N.SbsTrace(*(t.data_ptr() for t in tr))), C.byref(st),
                                        model._stream()))
    torch.cuda.synchronize()
    levels = int(st.model_calls)
    for prefix in (None, [[], [], [], []], torch.zeros((4, 0), dtype=torch.int64)):
        g = sbs(tta, model, K)
        o, d = g.generate(s, row_keys=KEYS, return_details=True, trace=True, prefix=padded(prefix, 3) if isinstance(prefix, list) else prefix)
        assert torch.equal(o, out) and torch.equal(d.logp, logp) and torch.equal(d.gumbel, gum) and g.model_calls_num == levels
        for a, b in zip(d.trace, tr):
            assert torch.equal(a, b[:levels])
    assert (plain5[0] == out.cpu().numpy()).all()


def test_top_k_1_is_the_greedy_row_and_nothing_else(tta, model, src):
    out, d = run(tta, model, src, 3, top_k=1)
    greedy = tta.TranslationInferenceGreedy(model, MAX_LEN, PAD, BOS, EOS).generate(src.cuda()).cpu().numpy()[:, 0]
    lp, g = d.logp.cpu().numpy(), d.gumbel.cpu().numpy()
    for b in range(4):
        n = ends(greedy[b:b + 1])[0]
        assert (out[b, 0, :n + 1] == greedy[b, :n + 1]).all() and (out[b, 0, n + 1:] == PAD).all()
    assert (lp[:, 0].view(np.int32) == 0).all() and (g[:, 0].view(np.int32) == 0).all()        # +0.0f on the bits
    assert np.isneginf(lp[:, 1:]).all() and np.isneginf(g[:, 1:]).all() and d.finished.cpu().numpy()[:, 1:].all()


@pytest.mark.parametrize("which", ["prompted", "both"])
def test_prompted_rows_are_bos_prefix_completion(runs, which):
    out, d = getattr(runs, which)
    g, lp = d.gumbel.cpu().numpy(), d.logp.cpu().numpy()
    assert out.shape == (4, 5, MAX_LEN) and (out[:, :, 0] == BOS).all()
    assert (g[:, 0] == 0).all() and (np.diff(g, axis=1) <= 0).all() and (lp[np.isfinite(g)] <= 0).all()
    assert np.isfinite(g).sum() >= 16, "hardly any finite row: the case shows nothing"
    for b, pre in enumerate(PREFIXES):
        fin = np.isfinite(g[b])
        assert (out[b, fin, 1:1 + len(pre)] == np.array(pre, dtype=np.int64)).all(), f"source {b}"
        assert len({tuple(r) for r in out[b][fin].tolist()}) == int(fin.sum()), f"source {b}: hypotheses repeat"
        assert len({tuple(r) for r in out[b].tolist()}) == 5
        for r, n in zip(out[b][fin], ends(out[b][fin])):
            assert (r[n + 1:] == PAD).all() and not np.isin(r[1 + len(pre):n], (PAD, EOS)).any(), r.tolist()
    assert (d.finished.cpu().numpy()[~np.isfinite(g)]).all() and np.isneginf(lp[~np.isfinite(g)]).all()


@pytest.mark.parametrize("which,kw", [("filtered", dict(top_k=TOP_K, top_p=TOP_P)), ("prompted", {}), ("both", dict(top_k=TOP_K, top_p=TOP_P))])
def test_nesting_alone_and_padding(tta, model, src, runs, which, kw):
    ref = getattr(runs, which)
    pre = None if which == "filtered" else PREFIXES
    same_run(run(tta, model, src, 3, pre, **kw), ref, 3, "K = 3 against the first three of K = 5")
    same_run(ref, run(tta, model, src, 7, pre, **kw), 5, "K = 5 against the first five of K = 7")
    for b in (0, 2):
        n = int((src[b] != PAD).sum())
        for s in (src[b:b + 1, :n], torch.nn.functional.pad(src[b:b + 1], (0, 3), value=PAD)):
            for width in (None, 9):
                q = None if pre is None else padded([pre[b]], width)
                out, d = sbs(tta, model, 5, **kw).generate(s.cuda(), row_keys=[KEYS[b]], return_details=True, prefix=q)
                assert (out.cpu().numpy()[0] == ref[0][b]).all(), f"source {b} alone at width {s.shape[1]}, prefix width {width}"
                assert torch.equal(d.logp[0], ref[1].logp[b]) and torch.equal(d.gumbel[0], ref[1].gumbel[b])


def test_a_forced_eos_ends_the_row(tta, model, src):
    out, d = run(tta, model, src, 3, [[5, EOS], [EOS], [5, 6], []])
    g = d.gumbel.cpu().numpy()
    assert out[0, 0, :4].tolist() == [BOS, 5, EOS, PAD] and out[1, 0, :3].tolist() == [BOS, EOS, PAD]
    assert np.isneginf(g[0, 1:]).all() and np.isneginf(g[1, 1:]).all() and (g[:2, 0] == 0).all()
    assert (d.logp.cpu().numpy()[:2, 0] == 0).all()               # nothing but forced tokens: the conditional probability is 1
    assert np.isfinite(g[2:]).all()


def test_order_logp_scores_and_counters_keep_working(tta, model, src, runs):
    g = sbs(tta, model, 5, top_k=TOP_K, top_p=TOP_P)
    out, sc, d = g.generate(src.cuda(), row_keys=KEYS, return_scores=True, return_details=True, order="logp", prefix=padded(PREFIXES))
    lp = d.logp.cpu().numpy()
    assert (np.diff(lp, axis=1) <= 0).all() and sc.score.shape == (4, 5)
    for b in range(4):
        assert sorted(map(tuple, out[b].cpu().numpy().tolist())) == sorted(map(tuple, runs.both[0][b].tolist()))
    assert g.model_calls_num == runs.both[1].trace.token.shape[0] and g.b_sz > 0
    assert "top_k=8" in str(g) and "top_p=0.9" in str(g)


# -- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(tta, model, src):
    s = src.cuda()
    for kw in (dict(top_k=33), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.5), dict(top_p=float("nan"))):
        with pytest.raises(tta.TtxError) as e:
            sbs(tta, model, 3, **kw).generate(s)
        assert e.value.code == -1, kw
    g = sbs(tta, model, 3)
    for p in (torch.tensor([[5, PAD, 6]] * 4), torch.full((4, 3), model.tgt_vocab_size), torch.full((4, MAX_LEN), 5), torch.full((3, 3), 5)):
        with pytest.raises(ValueError):
            g.generate(s, prefix=p)
    assert g.generate(s, prefix=torch.full((4, MAX_LEN - 1), 5)).shape == (4, 3, MAX_LEN)
    # the entry point itself: lengths above max_len - 1 or ld_prefix, negative ones, a length without a table; nothing is written
    from translation_transformer_amd import _native as N
    pre = torch.full((4, 6), 5, dtype=torch.int64, device="cuda")
    p = N.SbsParams(16, 3, 1.0, PAD, BOS, EOS, 1)
    for d_prefix, ld, lens, filt in ((pre.data_ptr(), 6, [16, 0, 0, 0], None), (pre.data_ptr(), 6, [0, 7, 0, 0], None),
                                     (pre.data_ptr(), 6, [0, 0, -1, 0], None), (None, 6, [0, 0, 0, 1], None),
                                     (pre.data_ptr(), -1, [0, 0, 0, 0], None), (None, 0, None, N.SbsFilter(40, 1.0)),
                                     (None, 0, None, N.SbsFilter(0, 0.0))):
        out = torch.full((4, 3, 16), -7, dtype=torch.int64, device="cuda")
        lp, gm = torch.full((4, 3), -7.0, device="cuda"), torch.full((4, 3), -7.0, device="cuda")
        st = N.BeamSearchStats()
        rc = model._lib.ttx_sbs_generate_ex(model.session, s.data_ptr(), 4, s.shape[1], None, C.byref(p), None if filt is None else C.byref(filt),
                                            d_prefix, ld, None if lens is None else (C.c_int32 * 4)(*lens), out.data_ptr(), lp.data_ptr(),
                                            gm.data_ptr(), None, C.byref(st), model._stream())
        torch.cuda.synchronize()
        assert rc == -1, (ld, lens)
        assert bool((out == -7).all()) and bool((lp == -7).all()) and bool((gm == -7).all()), "a refused call wrote its outputs"


# -- float64 replay -----------------------------------------------------------------------------------------------------------------
def replay(result, src, oracles, b: int, top_k: int, top_p: float, prefix):
    """Source b level by level.  Returns (problems, excused, ranks, fp32 gap, tokens outside their float64 kept set)."""
    out, d = result
    o64, o32 = oracles
    tr = [t.cpu().numpy()[:, b] for t in d.trace]                      # [levels, K] each
    levels, K = tr[0].shape
    s = src[b:b + 1]
    rows = np.array([[BOS]], dtype=np.int64)
    phi, G, fin = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, bool)
    steps, gap, outside = [], 0.0, []
    prm = M.params(T, top_k, top_p)
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
        forced = prefix[lv] if lv < len(prefix) else None
        args = (phi, G, fin, KEYS[b], lv + 1, SEED, T, K, PAD, EOS, top_k, top_p, forced)
        r64, flip = M.step(lg64, *args, tol=TOL)
        r32 = r64                                                       # a forced level has no arithmetic
        if forced is None:                                              # fp32 arithmetic on the float64 kept sets: the gap is rounding alone
            lg32m = np.where(np.isneginf(M.masked_logits(lg64, fin, prm)[0]), -np.inf, lg32).astype(np.float32)
            r32 = S.step(lg32m, phi, G, fin, KEYS[b], lv + 1, SEED, T, K, PAD, EOS, np.float32)
        sel = r64.order[:K]
        sel = sel[~r64.ill.reshape(-1)[sel]]
        x, y = r64.img_g.reshape(-1)[sel], r32.img_g.reshape(-1)[sel].astype(np.float64)
        ok = np.isfinite(x) & np.isfinite(y)
        gap = max(gap, float(np.abs(x[ok] - y[ok]).max()) if ok.any() else 0.0)
        par, tok = tr[0][lv], tr[1][lv]
        dev_fin = fin[par] | (tok == EOS) | (tok == PAD) | np.isneginf(tr[3][lv])
        steps.append((dict(parent=par, token=tok, phi=tr[2][lv], g=tr[3][lv], finished=dev_fin), r64, flip, G, phi, fin))
        if forced is None and prm.filtered:                             # the emitted tokens against the float64 kept sets
            for r in range(K):
                if np.isfinite(tr[3][lv][r]) and not fin[par[r]]:
                    keep, fl = M.kept(P.scaled(lg64[par[r]], T), prm, TOL)
                    if not (keep[tok[r]] or fl[tok[r]]):
                        outside.append((lv, r, int(tok[r])))
        rows = np.concatenate([rows[par], tok[:, None].astype(np.int64)], axis=1)
        phi, G, fin = tr[2][lv], tr[3][lv], dev_fin
    assert (rows == out[b][:, :rows.shape[1]]).all() and (out[b][:, rows.shape[1]:] == PAD).all(), "the trace does not rebuild the output"
    assert (phi == d.logp.cpu().numpy()[b]).all() and (G == d.gumbel.cpu().numpy()[b]).all()
    assert (fin == d.finished.cpu().numpy()[b]).all()
    bad, excused = [], 0
    for lv, (dev, r64, flip, pG, pphi, pfin) in enumerate(steps):
        p, ex = M.check_step(SimpleNamespace(**dev), r64, flip, pG, pphi, pfin, K, PAD, EOS, 10 * gap)
        bad += [f"level {lv}: {m}" for m in p]
        excused += ex
    return bad, excused, levels * K, gap, outside


@pytest.mark.parametrize("which,top_k,top_p", [("filtered", TOP_K, TOP_P), ("prompted", 0, 1.0), ("both", TOP_K, TOP_P)])
def test_replay_level_by_level_against_the_float64_oracle(runs, src, oracles, which, top_k, top_p):
    total = excused = 0
    for b in range(4):
        prefix = [] if which == "filtered" else PREFIXES[b]
        bad, ex, n, gap, outside = replay(getattr(runs, which), src, oracles, b, top_k, top_p, prefix)
        print(f"{which}, source {b}: {n} ranks, {ex} excused, fp32 gap {gap:.3g}, margin {10 * gap:.3g}")
        assert not bad, f"source {b}: " + "; ".join(bad[:4])
        assert not outside, f"source {b}: tokens outside their float64 kept set (level, rank, token): {outside[:4]}"
        total, excused = total + n, excused + ex
    print(f"{which}: {excused} of {total} ranks excused")
    assert excused <= S.EXCUSED_CAP * total


# -- logp against score() -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, dict(top_k=TOP_K, top_p=TOP_P)], ids=["filter-off", "filter-on"])
def test_logp_is_the_completions_conditional_log_probability(tta, model, src, oracles, kw):
    g = sbs(tta, model, 5, temperature=1.0, **kw)
    out, d = g.generate(src.cuda(), row_keys=KEYS, return_details=True, prefix=padded(PREFIXES))
    sc = g.score(src.cuda(), out, return_token_logp=True)
    rows = out.cpu().numpy().reshape(20, MAX_LEN)
    tokp = sc.token_logp.cpu().numpy().reshape(20, -1).astype(np.float64)
    with torch.no_grad():
        lp64 = torch.log_softmax(oracles[0](src.repeat_interleave(5, 0), torch.from_numpy(rows[:, :-1])), -1).numpy()
    tok64 = np.take_along_axis(lp64, rows[:, 1:, None], 2)[:, :, 0]
    n, plen = ends(rows), np.repeat([len(p) for p in PREFIXES], 5)
    logp, gum = d.logp.cpu().numpy().reshape(20).astype(np.float64), d.gumbel.cpu().numpy().reshape(20)
    use = np.isfinite(gum) & np.array([rows[r, n[r]] != PAD for r in range(20)])       # score() stops before a sampled PAD
    assert use.sum() >= 10
    worst = 0.0
    for r in np.nonzero(use)[0]:
        after, ref = tokp[r, plen[r]:n[r]].sum(), tok64[r, plen[r]:n[r]].sum()
        m = n[r] - plen[r]
        tol = m * TOK_TOL * max(1.0, float(np.abs(tok64[r, plen[r]:n[r]]).max()))
        assert abs(after - ref) <= tol, f"row {r}: score() is {abs(after - ref):.3g} from float64"
        if kw:
            assert logp[r] >= after - tol, f"row {r}: filtered logp {logp[r]!r} below the unfiltered sum {after!r}"
        else:
            worst = max(worst, abs(logp[r] - ref) / max(m, 1))
            assert abs(logp[r] - ref) <= tol and abs(logp[r] - after) <= 2 * tol, f"row {r}: logp {logp[r]!r}, score {after!r}, float64 {ref!r}"
    print(f"max |logp - float64| per completion token {worst:.3g}")
    if kw:
        assert (logp[use] > np.array([tokp[r, plen[r]:n[r]].sum() for r in np.nonzero(use)[0]])).any(), "the filter cut nothing"


# -- Lightning ----------------------------------------------------------------------------------------------------------------------
def test_lightning_takes_the_filter_and_passes_prefix_tokens_through(tta, model, tmp_path):
    from test_gpu_lightning_surface import FixtureTokenizer
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    s, tgt, _, _ = fixture_tokens()
    pre = padded(PREFIXES)
    preds = {}
    for bs in (1, 4):
        mod = tta.VanillaEncoderDecoderTransformerLightning(
            src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
            num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
            share_embeddings=True, generation="stochastic_beam_search", beam_size=3, max_len=MAX_LEN, sampling_temperature=T,
            sampling_top_k=TOP_K, sampling_top_p=TOP_P, sampling_seed=11, report_prediction_file=str(tmp_path / f"r{bs}.txt"))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        batches = [{"src_tokens": s[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda(), "prefix_tokens": pre[i:i + bs]} for i in range(0, 4, bs)]
        preds[bs] = torch.cat(tta.run_predict(mod, batches), 0).cpu()
        assert mod.generator.top_k == TOP_K and mod.generator.top_p == TOP_P
    assert preds[1].shape == (4, 3, MAX_LEN) and torch.equal(preds[1], preds[4])
    direct = tta.TranslationInferenceStochasticBeamSearch(model, 3, MAX_LEN, PAD, BOS, EOS, temperature=T, seed=11, top_k=TOP_K,
                                                          top_p=TOP_P).generate(s[:4].cuda(), row_keys=[0, 1, 2, 3], prefix=pre)
    assert torch.equal(direct.cpu(), preds[4])
    for b, r in enumerate(PREFIXES):
        assert (preds[4][b, 0, 1:1 + len(r)] == torch.tensor(r, dtype=torch.int64)).all()
