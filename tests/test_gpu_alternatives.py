"""Per-position alternatives of hypotheses on the MI355X (k_alternatives through ttx_hypothesis_alternatives /
ttx_score_alternatives, NativeTransformer.hypothesis_alternatives / alternatives, the generators' alternatives,
predict_with_alternatives) against the NumPy restatement of the definition (tests/util_alternatives.py), the scoring stage's own
bits and the reference's values (tests/golden/alternatives.npz, made by tests/golden/make_golden_alternatives.py)."""
import json

import numpy as np
import pytest
import torch

import util_alternatives as U
from util_models import GOLDEN, PAD, BOS, EOS, fixture_tokens, tiny_state

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x7FC12345          # a NaN as fp32, no id or rank as int32
VOCABS = [4, 5, 30, 63, 64, 65, 255, 256, 257, 1023, 1024]     # the lane and 256-column sweep edges, with V % 4 != 0
WIDTHS = [2, 3, 66, 130]


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def tiny(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)


@pytest.fixture(scope="module")
def trained(tta, trained_full_state):
    return tta.NativeTransformer(trained_full_state(4), 8, 0, device=0)


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a: dict, b: dict) -> bool:
    return all(np.array_equal(_bits(a[f]), _bits(b[f])) for f in U.FIELDS)


# -- the stage alone through the C entry point, outputs in sentinel-filled buffers with guard margins -----------------------
def _stage(model, logits: torch.Tensor, hyp: torch.Tensor, k: int) -> dict:
    """ttx_hypothesis_alternatives on device logits [R, T, V] (read in place) and hyp [R, T+1] -> FIELDS as NumPy arrays."""
    R, T, V = logits.shape
    shapes = {"top_id": (R, T, k), "top_logp": (R, T, k), "chosen_logp": (R, T), "rank": (R, T), "entropy": (R, T), "length": (R,)}
    buf = {f: torch.full((GUARD + int(np.prod(s)) + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for f, s in shapes.items()}
    ptr = {f: buf[f].data_ptr() + 4 * GUARD for f in shapes}
    from translation_transformer_amd import _native as N
    N.check(model._lib.ttx_hypothesis_alternatives(model._scoring_session(), logits.data_ptr(), hyp.data_ptr(), R, T + 1, V, PAD, EOS, k,
                                                   *(ptr[f] for f in U.FIELDS), model._stream()))
    out = {}
    for f, s in shapes.items():
        raw = buf[f].cpu().numpy()
        n = int(np.prod(s))
        assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + n:] == SENTINEL).all(), f"{f}: guard overwritten"
        body = raw[GUARD:GUARD + n]
        assert not (body == SENTINEL).any(), f"{f}: elements left unwritten"
        out[f] = body.view(np.float32 if f in ("top_logp", "chosen_logp", "entropy") else np.int32).reshape(s)
    return out


def _rule_rows(V: int, W: int, rng) -> np.ndarray:
    """Hypothesis rows covering every case of the length rule at width W, chunk boundaries of the 64-lane scan included."""
    rows = []

    def row(fill):                       # fill: list of (column, count or token)
        h = np.full(W, PAD, np.int64)
        h[0] = BOS
        for c, v in fill:
            if isinstance(v, tuple):
                h[c:c + v[0]] = rng.integers(3, V, v[0])
            else:
                h[c] = v
        rows.append(h)

    row([(1, EOS)] + ([(2, (W - 2,))] if W > 2 else []))               # EOS at column 1, tokens after it ignored
    for c in sorted({64, 65, 128, 129, W - 1}):                         # EOS at the scan's chunk boundaries and in the last column
        if 1 < c < W:
            row([(1, (c - 1,)), (c, EOS)])
    row([(1, (W - 1,))])                                                # no EOS, the row is full
    rows.append(np.full(W, PAD, np.int64))                              # all-PAD
    if W > 2:
        row([(1, (max(1, (W - 1) // 2),))])                             # no EOS, trailing PAD
    if W >= 66:
        row([(1, (9,)), (4, PAD), (5, PAD), (10, EOS)])                 # PADs before the EOS are targets
        row([(1, (20,)), (21, EOS), (22, (8,)), (30, EOS)])             # two EOS: the first counts
        row([(1, (3,)), (60, (4,))])                                    # no EOS, PAD gap: the LAST non-PAD column counts
    return np.stack(rows)


PATTERNS = ("noise", "small integers", "constant", "one logit 30 above", "-inf entries")


def _synthetic(V: int, W: int):
    """hyp [R, W], logits [R, W-1, V] (row r carries pattern r % 5; the last row also one all -inf position) and the mask of the
    positions outside the contract."""
    rng = np.random.default_rng(1000 * V + W)
    base = _rule_rows(V, W, rng)
    full = np.full(W, PAD, np.int64)                                    # a full row for the all -inf position
    full[0], full[1:] = BOS, rng.integers(3, V, W - 1)
    hyp = np.concatenate([base] * -(-2 * len(PATTERNS) // len(base)) + [full[None]])   # every pattern on two rows at least
    R, T = hyp.shape[0], W - 1
    x = (rng.standard_normal((R, T, V)) * 3.0).astype(np.float32)
    for r in range(R - 1):
        kind = PATTERNS[r % len(PATTERNS)]
        if kind == "small integers":                                    # most neighbours tie; -0.0 and 0.0 are one value
            x[r] = rng.integers(-2, 3, (T, V)).astype(np.float32)
            x[r].reshape(-1)[np.flatnonzero(x[r] == 0)[::2]] = -0.0
        elif kind == "constant":
            x[r] = np.float32(0.37)
        elif kind == "one logit 30 above":
            hot = rng.integers(0, V, T)
            x[r, np.arange(T), hot] = x[r].max(-1) + np.float32(30.0)
        elif kind == "-inf entries":                                    # position p keeps 1 + p % 7 finite logits, or about half of V
            for p in range(T):
                keep = 1 + p % 7 if p % 2 == 0 else max(1, V // 2)
                gone = rng.permutation(V)[min(keep, V):]
                x[r, p, gone] = -np.inf
    outside = np.zeros((R, T), bool)
    x[R - 1, T // 2] = -np.inf
    outside[R - 1, T // 2] = True
    return hyp, x, outside


def _ks(V: int) -> list:
    return sorted({k for k in (1, 2, 5, 32, V) if k <= min(32, V)})


@pytest.mark.parametrize("V", VOCABS)
def test_stage_alone_is_exact_and_within_tolerance(tiny, V):
    """(a) ids, rank and length equal the restatement exactly at every position; (b) the values are within TOK_TOL * max(1, max|ref|)
    of the float64 restatement; the bits do not depend on the alignment of the logits, on the call or on how the rows are split."""
    worst = {"top_logp": 0.0, "chosen_logp": 0.0, "entropy": 0.0}
    worst32 = dict(worst)
    for W in WIDTHS:
        hyp, x, outside = _synthetic(V, W)
        R, T = hyp.shape[0], W - 1
        assert set(U.lengths(hyp, PAD, EOS).tolist()) >= {0, 1, W - 1}
        d_hyp = torch.from_numpy(hyp).cuda()
        d_x = torch.from_numpy(x).cuda()
        assert d_x.data_ptr() % 16 == 0
        shifted = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")[1:].view(x.shape)
        shifted.copy_(d_x)
        assert shifted.data_ptr() % 16 != 0
        ref = U.restate(x, hyp, PAD, EOS, min(32, V))
        ref32 = U.restate(x, hyp, PAD, EOS, min(32, V), np.float32)
        live = (np.arange(T)[None, :] < ref["length"][:, None]) & ~outside
        scores = tiny.hypothesis_logprobs(d_x, d_hyp, PAD, EOS)
        tok = scores.token_logp.cpu().numpy()
        for k in _ks(V):
            got = _stage(tiny, d_x, d_hyp, k)
            label = f"V={V} W={W} k={k}"
            assert U.check_result(got, x, hyp, PAD, EOS, outside, ref) == [], label
            for f, e in U.value_errors(got, U.first_k(ref, k), live).items():
                worst[f] = max(worst[f], e)
            for f, e in U.value_errors(U.first_k(ref32, k), U.first_k(ref, k), live).items():
                worst32[f] = max(worst32[f], e)
            # the same bits: a base off 16 bytes, a second call, the rows split over two calls
            assert _same_bits(got, _stage(tiny, shifted, d_hyp, k)), label
            assert _same_bits(got, _stage(tiny, d_x, d_hyp, k)), label
            cut = R // 2
            a, b = _stage(tiny, d_x[:cut], d_hyp[:cut], k), _stage(tiny, d_x[cut:], d_hyp[cut:], k)
            assert _same_bits(got, {f: np.concatenate([a[f], b[f]]) for f in U.FIELDS}), label
            # chosen_logp is tok_logp of the scoring stage on the same logits wherever that stage gives a number (it gives NaN
            # on rows with -inf entries and nowhere else), and the top list holds it at the token's rank
            number = ~np.isnan(tok)
            assert number[[r for r in range(R - 1) if r % len(PATTERNS) != 4]].all(), label
            assert np.array_equal(_bits(got["chosen_logp"][number & ~outside]), _bits(tok[number & ~outside])), label
            assert np.array_equal(got["length"], scores.length.cpu().numpy()), label
            inside = live & (got["rank"] < k)
            at_rank = np.take_along_axis(got["top_logp"], np.clip(got["rank"], 0, k - 1)[..., None], -1)[..., 0]
            assert np.array_equal(_bits(at_rank[inside]), _bits(got["chosen_logp"][inside])), label
            # constant rows: ids 0..k-1, every top_logp equal, entropy log V
            for r in range(2, R - 1, len(PATTERNS)):
                n = int(ref["length"][r])
                assert (got["top_id"][r, :n] == np.arange(k)).all() and (got["top_logp"][r, :n] == got["top_logp"][r, :n, :1]).all()
                assert np.allclose(got["entropy"][r, :n], np.log(V), rtol=0, atol=U.TOK_TOL * max(1.0, np.log(V)))
            # rows with -inf entries: distinct ids (check_result), a finite entropy, -inf values where the logit is -inf
            for r in range(4, R - 1, len(PATTERNS)):
                n = int(ref["length"][r])
                assert np.isfinite(got["entropy"][r, :n]).all()
                assert np.array_equal(np.isneginf(got["top_logp"][r, :n]), np.isneginf(ref["top_logp"][r, :n, :k]))
    print(f"V={V}: max |value - float64 restatement|", {f: f"{e:.3g}" for f, e in worst.items()},
          " NumPy fp32 restatement:", {f: f"{e:.3g}" for f, e in worst32.items()})


# -- end to end ----------------------------------------------------------------------------------------------------------
def _np(alts) -> dict:
    return {f: getattr(alts, f).cpu().numpy() for f in U.FIELDS}


def _flat(d: dict, R: int) -> dict:
    return {f: v.reshape((R,) + v.shape[2:]) for f, v in d.items()}


def _end_to_end(tta, native, src, hyp, label, k=5):
    B, n_hyp, W = hyp.shape
    V = native.tgt_vocab_size
    logits = torch.full((B * n_hyp, W - 1, V), float("nan"), device="cuda")
    ref_sc = native.score_hypotheses(src, hyp, eos_token_idx=EOS, return_token_logp=True, trim=False, logits_out=logits)
    base = native.alternatives(src, hyp, k=k, eos_token_idx=EOS, trim=False)
    got = _flat(_np(base), B * n_hyp)
    # ids, rank and length equal the restatement on the GPU's own logits exactly
    assert U.check_result(got, logits.cpu().numpy(), hyp.reshape(B * n_hyp, W).cpu().numpy(), PAD, EOS) == [], label
    assert torch.equal(base.chosen_logp, ref_sc.token_logp) and torch.equal(base.length, ref_sc.length), label
    alts, sc = native.alternatives(src, hyp, k=k, eos_token_idx=EOS, with_scores=True)
    plain = native.score_hypotheses(src, hyp, eos_token_idx=EOS, return_token_logp=True)
    for a, b in zip(sc, plain):
        assert torch.equal(a, b), label
    wide = torch.cat([hyp, torch.full((B, n_hyp, 7), PAD, dtype=torch.int64, device="cuda")], dim=2)
    one_by_one = [native.alternatives(src[b:b + 1], hyp[b:b + 1], k=k, eos_token_idx=EOS) for b in range(B)]
    variants = {
        "with_scores": alts,
        "trim on": native.alternatives(src, hyp, k=k, eos_token_idx=EOS),
        "chunks of 3 sources": native.alternatives(src, hyp, k=k, eos_token_idx=EOS, max_rows=3 * n_hyp * (W - 1), trim=False),
        "chunks of 1 source": native.alternatives(src, hyp, k=k, eos_token_idx=EOS, max_rows=1),
        "source by source": tta.Alternatives(*(torch.cat([getattr(r, f) for r in one_by_one]) for f in U.FIELDS)),
        "7 PAD columns, trim on": native.alternatives(src, wide, k=k, eos_token_idx=EOS),
        "7 PAD columns, trim off": native.alternatives(src, wide, k=k, eos_token_idx=EOS, trim=False),
    }
    want = _np(base)
    for name, v in variants.items():
        g = _np(v)
        assert g["top_id"].shape[2] in (W - 1, W + 6), (label, name)
        for f in U.FIELDS[:5]:
            assert np.array_equal(_bits(g[f][:, :, :W - 1]), _bits(want[f])), (label, name, f)
        assert np.array_equal(g["length"], want["length"]), (label, name)
    for name in ("7 PAD columns, trim on", "7 PAD columns, trim off"):
        g = _np(variants[name])
        assert (g["top_id"][:, :, W - 1:] == -1).all() and (g["rank"][:, :, W - 1:] == -1).all(), (label, name)
        assert all((g[f][:, :, W - 1:] == 0).all() for f in ("top_logp", "chosen_logp", "entropy")), (label, name)


@pytest.mark.parametrize("name", ["beam", "rule"])
def test_end_to_end_on_the_tiny_model(tta, tiny, name):
    c = U.golden_cases()[name]
    _end_to_end(tta, tiny, torch.from_numpy(c["src"]).cuda(), torch.from_numpy(c["hyp"]).cuda(), f"tiny/{name}")


def test_end_to_end_on_a_trained_model(tta, trained):
    src, _, c, V = fixture_tokens()
    g = tta.TranslationInferenceBeamSearchSpeculative(trained, 200, 5, 10, 3, V, False, PAD, BOS, EOS, c, max_steps=400)
    _end_to_end(tta, trained, src.cuda(), g.generate(src.cuda()), "trained 4+4 beam_speculative")


# -- against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["beam", "targets", "rule"])
def test_alternatives_match_reference_fixture(tiny, name):
    """k = 8 against the float64 values of the reference's own logits: length exact, the sorted top_logp values and the entropy
    within TOK_TOL * max(1, max|ref|); ids at the (position, rank) pairs whose reference value is more than 4 bounds away from
    both neighbours in rank (the stored 9th value serves rank 7), at most 1 % of the pairs left out; rank exact where the
    emitted token's own pair is compared."""
    c = U.golden_cases()[name]
    alts = tiny.alternatives(torch.from_numpy(c["src"]).cuda(), torch.from_numpy(c["hyp"]).cuda(), k=8, eos_token_idx=EOS)
    r = U.compare_with_golden(_np(alts), c, 8)
    print(f"tiny/{name}:", r)
    assert r["length_equal"]
    assert r["top_logp_err"] <= r["bound"]
    assert r["entropy_err"] <= r["bound"]
    assert r["left_out"] <= 0.01 * r["pairs"]
    assert r["id_mismatches"] == 0
    assert r["rank_mismatches"] == 0


# -- the surface -----------------------------------------------------------------------------------------------------------
def _generators(tta, native):
    _, _, c, V = fixture_tokens()
    return {
        "greedy": lambda: tta.TranslationInferenceGreedy(native, 150, PAD, BOS, EOS),
        "beam_search": lambda: tta.TranslationInferenceBeamSearch(native, 3, 150, PAD, BOS, EOS),
        "greedy_speculative": lambda: tta.TranslationInferenceGreedySpeculative(native, 150, 10, 3, PAD, BOS, EOS, c),
        "beam_search_speculative": lambda: tta.TranslationInferenceBeamSearchSpeculative(native, 150, 3, 10, 3, V, False, PAD, BOS,
                                                                                         EOS, c, max_steps=400),
    }


@pytest.mark.parametrize("kind", ["greedy", "beam_search", "greedy_speculative", "beam_search_speculative"])
def test_generator_alternatives(tta, tiny, kind):
    from translation_transformer_amd import scoring
    g = _generators(tta, tiny)[kind]()
    src = fixture_tokens()[0].cuda()
    pred = g.generate(src)
    calls = g.model_calls_num
    alts = g.alternatives(src, pred)
    assert g.model_calls_num == calls                          # no model call of the reference's loop
    B, n_hyp, W = pred.shape
    assert isinstance(alts, tta.Alternatives) and alts.top_id.shape == (B, n_hyp, W - 1, 5) and alts.rank.shape == (B, n_hyp, W - 1)
    sc = g.score(src, pred, return_token_logp=True)
    assert torch.equal(alts.chosen_logp, sc.token_logp) and torch.equal(alts.length, sc.length)
    live = torch.arange(W - 1, device="cuda") < alts.length.unsqueeze(-1)
    assert (alts.rank[live] >= 0).all() and (alts.rank[~live] == -1).all() and (alts.margin[~live] == 0).all()
    assert (alts.margin[live] >= 0).all() and (alts.entropy[live] >= 0).all()
    if kind.startswith("greedy"):
        # a greedy generator emits the first maximum of its own step logits: rank 0 except where an fp32 near-tie decided
        tol = 4 * U.TOK_TOL * max(1.0, float(alts.top_logp[live].abs().max()))
        near = scoring.near_ties(alts, tol)
        off = live & (alts.rank != 0)
        print(f"{kind}: {int(live.sum())} live positions, {int(off.sum())} with rank != 0, {int(near.sum())} near-ties below {tol:.3g}")
        assert not (off & ~near).any()
    a2, s2 = g.alternatives(src, pred, k=2, with_scores=True)
    assert torch.equal(a2.top_id, alts.top_id[..., :2]) and torch.equal(a2.top_logp, alts.top_logp[..., :2])
    assert torch.equal(s2.score, sc.score) and torch.equal(s2.finished, sc.finished)


class FixtureTokenizer:
    """Shape of the reference's GenericTokenizer that the module uses (tokenizer_base.py:16-94)."""
    pad_token_idx, bos_token_idx, eos_token_idx, unk_token_idx = 0, 1, 2, 3

    def __init__(self):
        self.decoder_dict = {int(k): v for k, v in json.loads((GOLDEN / "fixture_vocab.json").read_text()).items()}
        self.encoder_dict = {v: k for k, v in self.decoder_dict.items()}

    @property
    def n_tokens(self):
        return len(self.encoder_dict)


def _module(tta, generation, report_file, **kw):
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    mod = tta.VanillaEncoderDecoderTransformerLightning(
        src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
        num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"],
        num_heads=cfg["num_heads"], share_embeddings=True, generation=generation, max_len=150, n_drafts=3,
        draft_len=10, report_prediction_file=str(report_file), **kw)
    mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    return mod


@pytest.mark.parametrize("generation", ["greedy_speculative", "beam_search"])
def test_predict_with_alternatives(tta, tmp_path, generation, monkeypatch):
    monkeypatch.delenv("TTX_PREDICT_ALTERNATIVES", raising=False)
    monkeypatch.delenv("TTX_PREDICT_SCORES", raising=False)
    src, tgt, _, _ = fixture_tokens()
    batches = []
    for i, j in ((0, 3), (3, 4), (4, 10)):
        s_ = src[i:j]
        batches.append({"src_tokens": s_[:, :int((s_ != PAD).sum(1).max())].cuda(), "tgt_tokens": tgt[i:j].cuda()})
    kw = dict(beam_size=3, smart_drafts_mode=False) if generation == "beam_search" else {}

    def run(k, scores, tag):
        rf = tmp_path / f"r_{tag}.txt"
        mod = _module(tta, generation, rf, **kw)
        mod.predict_with_alternatives, mod.predict_with_scores = k, scores
        outs = tta.run_predict(mod, batches, schedule="batches")
        return outs, json.loads(rf.read_text().strip().split("\n")[-1]), mod

    off_outs, off_rep, off = run(0, False, "off")
    assert off.predict_alternatives == {} and off.predict_scores == {}
    on_outs, on_rep, on = run(4, False, "on")
    both_outs, both_rep, both = run(4, True, "both")
    sc_outs, sc_rep, sc = run(0, True, "scores")
    for outs in (on_outs, both_outs, sc_outs):
        assert all(torch.equal(a, b) for a, b in zip(off_outs, outs))
    assert set(on_rep) == set(off_rep) | {"alternatives_seconds"} and set(both_rep) == set(sc_rep) | {"alternatives_seconds"}
    assert on.predict_scores == {} and on_rep["alternatives_seconds"] > 0
    assert both_rep["model_calls"] == off_rep["model_calls"] and both_rep["mean_top1_logprob"] == sc_rep["mean_top1_logprob"]
    for mod in (on, both):
        assert sorted(mod.predict_alternatives) == list(range(len(batches)))
        for i, (b, p) in enumerate(zip(batches, off_outs)):
            want = mod.generator.alternatives(b["src_tokens"], p, k=4)
            assert all(torch.equal(x, y) for x, y in zip(mod.predict_alternatives[i], want))
    for i in range(len(batches)):
        for x, y in zip(both.predict_scores[i], sc.predict_scores[i]):
            assert (x is None and y is None) or torch.equal(x, y)
    monkeypatch.setenv("TTX_PREDICT_ALTERNATIVES", "five")
    with pytest.raises(ValueError, match="TTX_PREDICT_ALTERNATIVES"):
        run(0, False, "bad_env")
    monkeypatch.setenv("TTX_PREDICT_ALTERNATIVES", "4")
    env_outs, _, env = run(0, False, "env")
    assert all(torch.equal(x, y) for i in range(len(batches)) for x, y in zip(env.predict_alternatives[i], on.predict_alternatives[i]))


def test_c_boundary_refuses_bad_arguments(tta, tiny):
    N = tta._native
    c = U.golden_cases()["rule"]
    src, hyp = torch.from_numpy(c["src"]).cuda(), torch.from_numpy(c["hyp"]).cuda()
    B, n_hyp, W = hyp.shape
    V, R = tiny.tgt_vocab_size, B * n_hyp
    lib, sess, stream = tiny._lib, tiny._scoring_session(), tiny._stream()
    out = [torch.full((R * (W - 1) * 32,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(6)]
    ptrs = [t.data_ptr() for t in out]
    logits = torch.zeros((R, W - 1, V), device="cuda")

    def full(k=5, W_=W, ld=W, Ls=src.shape[1], B_=B, outputs=ptrs):
        return lib.ttx_score_alternatives(sess, src.data_ptr(), B_, Ls, hyp.data_ptr(), ld, n_hyp, W_, EOS, k, None, *outputs, stream)

    def stage(k=5, W_=W, V_=V, outputs=ptrs):
        return lib.ttx_hypothesis_alternatives(sess, logits.data_ptr(), hyp.data_ptr(), R, W_, V_, PAD, EOS, k, *outputs, stream)

    for call in (full, stage):
        assert call(k=0) == N.TTX_ERR_INVALID and b"k must be at least 1" in lib.ttx_last_error()
        assert call(k=33) == N.TTX_ERR_INVALID and b"larger than 32" in lib.ttx_last_error()
        assert call(W_=1) == N.TTX_ERR_INVALID
        assert call(outputs=[None] * 5 + ptrs[5:]) == N.TTX_ERR_INVALID and b"no output requested" in lib.ttx_last_error()
    assert stage(k=5, V_=4) == N.TTX_ERR_INVALID and b"larger than the vocabulary" in lib.ttx_last_error()
    if V < 32:
        assert full(k=V + 1) == N.TTX_ERR_INVALID and b"larger than the vocabulary" in lib.ttx_last_error()
    assert stage(V_=1025) == N.TTX_ERR_INVALID
    assert full(ld=W - 1) == N.TTX_ERR_INVALID and b"ld_hyp" in lib.ttx_last_error()
    assert full(Ls=5001) == N.TTX_ERR_INVALID and b"positional table" in lib.ttx_last_error()
    assert full(B_=0) == N.TTX_ERR_INVALID
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in out)
    with pytest.raises(ValueError):
        tiny.alternatives(src, hyp, k=0)
    with pytest.raises(ValueError):
        tiny.alternatives(src, hyp, k=33)
    with pytest.raises(ValueError):
        tiny.hypothesis_alternatives(logits, hyp.reshape(R, W)[:, :-1], PAD, EOS)
    # the session is still usable, with single outputs too
    only_rank = [None, None, None, ptrs[3], None, None]
    assert full(outputs=only_rank) == N.TTX_OK
    torch.cuda.synchronize()
    rank = out[3][:R * (W - 1)].reshape(B, n_hyp, W - 1)
    assert torch.equal(rank, tiny.alternatives(src, hyp, trim=False).rank)
    assert all((out[i] == SENTINEL).all() for i in (0, 1, 2, 4, 5))
