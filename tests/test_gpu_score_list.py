"""Length-bucketed scoring of a list of batches on the MI355X (NativeTransformer.score_hypotheses_many, the generators'
score_many and generate_many(return_scores=True), ttx_score_list_extents / ttx_score_list_run) against the per-batch
score_hypotheses: length and finished equal, score and token_logp equal on the bits.  max_len <= 200 keeps every source and
hypothesis window inside the range in which the full-prefix pass is bit-identical across widths."""
import ctypes as C

import numpy as np
import pytest
import torch

from util_draft_select import h4_state
from util_models import PAD, BOS, EOS, fixture_tokens, tiny_state
from util_score import golden_cases
from util_score_list import first_difference

pytestmark = pytest.mark.gpu

FIELDS = ("score", "length", "finished", "token_logp")


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def models(tta):
    st, cfg = tiny_state()
    h4, h4cfg = h4_state()
    return {"tiny": tta.NativeTransformer(st, cfg["num_heads"], 0, device=0), "h4": tta.NativeTransformer(h4, h4cfg["num_heads"], 0, device=0)}


def _trimmed(src: torch.Tensor, extra: int) -> torch.Tensor:
    """The rows cut to their longest non-PAD extent, then ``extra`` PAD columns appended."""
    s = src[:, :int((src != PAD).sum(1).max())]
    return torch.cat([s, torch.full((s.shape[0], extra), PAD, dtype=torch.int64)], dim=1).contiguous().cuda()


@pytest.fixture(scope="module")
def lists(tta, models):
    """Per model: (srcs, hyps, per-batch reference) of a list of five batches, B = 1, 3, 4, 10 and the golden "rule" rows (B = 3),
    padded source widths that differ, N = 3 (sampler), 1 (greedy-speculative), 5 (beam search), 1, 2.  The reference is computed once."""
    src, _, c, V = fixture_tokens()
    out = {}
    for name, m in models.items():
        srcs = [_trimmed(src[0:1], 9), _trimmed(src[1:4], 0), _trimmed(src[4:8], 3), _trimmed(src, 0), golden_cases()["rule"]["src"].cuda()]
        spec = tta.TranslationInferenceGreedySpeculative(m, 200, 10, 3, PAD, BOS, EOS, c)
        hyps = [tta.TranslationInferenceSampling(m, 120, PAD, BOS, EOS, temperature=1.0, num_samples=3, seed=5).generate(srcs[0]),
                spec.generate(srcs[1]),
                tta.TranslationInferenceBeamSearch(m, 5, 150, PAD, BOS, EOS).generate(srcs[2]),
                spec.generate(srcs[3]),
                golden_cases()["rule"]["hyp"].cuda()]
        assert [h.shape[1] for h in hyps] == [3, 1, 5, 1, 2] and len({h.shape[2] for h in hyps}) >= 3
        ref = [m.score_hypotheses(s, h, eos_token_idx=EOS, return_token_logp=True) for s, h in zip(srcs, hyps)]
        out[name] = (srcs, hyps, ref)
    return out


def _assert_same(got: list, want: list, label: str, fields=FIELDS) -> None:
    """Every batch, every field: equal on the bits (torch.equal); the message names the first differing batch, row and column."""
    assert len(got) == len(want), label
    for f in fields:
        g = [None if r is None else getattr(r, f) for r in got]
        w = [None if r is None else getattr(r, f) for r in want]
        assert [x is None for x in g] == [x is None for x in w], (label, f)
        g, w = [x for x in g if x is not None], [x for x in w if x is not None]
        if not all(torch.equal(a, b) for a, b in zip(g, w)):
            raise AssertionError(f"{label}: " + str(first_difference([x.cpu().numpy() for x in g], [x.cpu().numpy() for x in w], f)))
        assert all(a.dtype == b.dtype and a.shape == b.shape for a, b in zip(g, w)), (label, f)


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_list_equals_the_per_batch_calls(models, lists, name):
    m = models[name]
    srcs, hyps, ref = lists[name]
    got = m.score_hypotheses_many(srcs, hyps, eos_token_idx=EOS, return_token_logp=True)
    _assert_same(got, ref, name)
    plan = m.last_score_plan
    assert len({c.N for c in plan}) == 4 and sum(len(c.sources) for c in plan) == sum(s.shape[0] for s in srcs)
    plain = m.score_hypotheses_many(srcs, hyps, eos_token_idx=EOS)
    assert all(r.token_logp is None for r in plain)
    _assert_same(plain, ref, name + " without token_logp", FIELDS[:3])
    for r, h in zip(got, hyps):
        assert r.score.shape == h.shape[:2] and r.token_logp.shape == h.shape[:2] + (h.shape[2] - 1,)
        assert r.score.dtype == torch.float32 and r.length.dtype == torch.int32 and r.finished.dtype == torch.bool


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_source_padding_changes_no_bit(models, lists, name):
    """score_hypotheses itself: the same batch with 0 and with 9 more PAD source columns.  The bucketed pass cuts PAD tails of
    sources and relies on this."""
    m = models[name]
    srcs, hyps, ref = lists[name]
    for i in (1, 2, 3):
        wide = torch.cat([srcs[i], torch.full((srcs[i].shape[0], 9), PAD, dtype=torch.int64, device="cuda")], dim=1)
        r = m.score_hypotheses(wide, hyps[i], eos_token_idx=EOS, return_token_logp=True)
        d = (r.token_logp - ref[i].token_logp).abs().max().item()
        print(f"{name} batch {i}: source width {srcs[i].shape[1]} -> {wide.shape[1]}: max token diff {d:.3g}")
        _assert_same([r], [ref[i]], f"{name} batch {i} with 9 PAD source columns")


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_same_bits_however_the_list_is_cut(models, lists, name, monkeypatch):
    m = models[name]
    srcs, hyps, ref = lists[name]
    kw = dict(eos_token_idx=EOS, return_token_logp=True)
    S = sum(s.shape[0] for s in srcs)
    _assert_same(m.score_hypotheses_many(srcs, hyps, max_rows=1, **kw), ref, "max_rows=1")
    assert len(m.last_score_plan) == S
    _assert_same(m.score_hypotheses_many(srcs, hyps, max_rows=700, **kw), ref, "max_rows=700")
    assert 4 < len(m.last_score_plan) < S
    _assert_same(m.score_hypotheses_many(srcs, hyps, max_rows=None, **kw), ref, "default max_rows")
    assert len(m.last_score_plan) == 4
    _assert_same(m.score_hypotheses_many(srcs[::-1], hyps[::-1], **kw), ref[::-1], "reversed")
    rep = [0, 2, 2, 1, 2]
    _assert_same(m.score_hypotheses_many([srcs[i] for i in rep], [hyps[i] for i in rep], **kw), [ref[i] for i in rep], "a batch repeated")
    with_none = m.score_hypotheses_many(srcs, [hyps[0], None, hyps[2], None, hyps[4]], **kw)
    assert with_none[1] is None and with_none[3] is None
    _assert_same(with_none, [ref[0], None, ref[2], None, ref[4]], "None entries")
    assert m.score_hypotheses_many(srcs[:2], [None, None]) == [None, None] and m.score_hypotheses_many([], []) == []
    # host tensors and int32 tokens are converted as score_hypotheses converts them
    _assert_same(m.score_hypotheses_many([srcs[1].cpu()], [hyps[1].to(torch.int32)], **kw), [ref[1]], "converted inputs")
    # two calls
    a = m.score_hypotheses_many(srcs, hyps, **kw)
    m.score_hypotheses_many(srcs[:2], hyps[:2])
    _assert_same(m.score_hypotheses_many(srcs, hyps, **kw), a, "two calls")


@pytest.mark.parametrize("name", ["tiny", "h4"])
def test_generate_many_with_scores(tta, models, lists, name, monkeypatch):
    m = models[name]
    src, _, c, V = fixture_tokens()
    batches = [_trimmed(src[0:3], 0), _trimmed(src[3:4], 5), _trimmed(src[4:10], 2)]
    gens = {"greedy_speculative": lambda: tta.TranslationInferenceGreedySpeculative(m, 150, 10, 3, PAD, BOS, EOS, c),
            "sampling_speculative": lambda: tta.TranslationInferenceSamplingSpeculative(m, 120, 10, 3, PAD, BOS, EOS, c, temperature=1.0,
                                                                                       num_samples=3, seed=11)}
    for label, make in gens.items():
        monkeypatch.delenv("TTX_SCORE_LIST", raising=False)
        g = make()
        pairs = g.generate_many(batches, return_scores=True)
        assert len(pairs) == len(batches)
        per_batch = [g.score(b, p) for b, (p, _) in zip(batches, pairs)]
        _assert_same([s for _, s in pairs], per_batch, f"{name} {label}", FIELDS[:3])
        _assert_same(g.score_many(batches, [p for p, _ in pairs], return_token_logp=True),
                     [g.score(b, p, return_token_logp=True) for b, (p, _) in zip(batches, pairs)], f"{name} {label} score_many")
        monkeypatch.setenv("TTX_SCORE_LIST", "0")                     # the per-batch loop: the same rows, the same bits
        off = make().generate_many(batches, return_scores=True)
        assert all(torch.equal(p, q) for (p, _), (q, _) in zip(pairs, off))
        _assert_same([s for _, s in off], per_batch, f"{name} {label} TTX_SCORE_LIST=0", FIELDS[:3])


def test_switch_selects_the_path(tta, models, lists, monkeypatch):
    """generate_many(return_scores=True) goes through score_many unless TTX_SCORE_LIST=0; a call with return_logq never does."""
    m = models["tiny"]
    src, _, c, V = fixture_tokens()
    batches = [_trimmed(src[0:2], 0), _trimmed(src[2:4], 1)]
    calls = []
    real = type(m).score_hypotheses_many
    monkeypatch.setattr(type(m), "score_hypotheses_many", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    g = tta.TranslationInferenceSamplingSpeculative(m, 100, 10, 3, PAD, BOS, EOS, c, num_samples=2, seed=3)
    monkeypatch.delenv("TTX_SCORE_LIST", raising=False)
    g.generate_many(batches, return_scores=True)
    assert len(calls) == 1
    g.generate_many(batches, return_scores=True, return_logq=True)
    assert len(calls) == 1
    monkeypatch.setenv("TTX_SCORE_LIST", "0")
    g.generate_many(batches, return_scores=True)
    assert len(calls) == 1


def test_rejects_bad_inputs(tta, models, lists):
    N = tta._native
    m = models["tiny"]
    srcs, hyps, ref = lists["tiny"]
    V = m.tgt_vocab_size
    with pytest.raises(ValueError):
        m.score_hypotheses_many(srcs, hyps[:-1])                                       # one hyp per src
    with pytest.raises(ValueError):
        m.score_hypotheses_many(srcs, hyps[:1] + [hyps[1][:, :, :1]] + hyps[2:])       # W = 1
    with pytest.raises(ValueError):
        m.score_hypotheses_many([srcs[0], srcs[1][:2]], hyps[:2])                      # batch mismatch
    with pytest.raises(ValueError):
        m.score_hypotheses_many(srcs[:2], [hyps[0], hyps[1][:, 0]])                    # not [B, N, W]
    with pytest.raises(ValueError):
        m.score_hypotheses_many(srcs, hyps, max_rows=-3)
    bad = hyps[2].clone()
    bad[1, 4, bad.shape[2] - 1] = V                                                    # behind every EOS, in the last column
    with pytest.raises(IndexError):
        m.score_hypotheses_many(srcs, hyps[:2] + [bad] + hyps[3:])
    bad_src = srcs[3].clone()
    bad_src[9, 0] = -1
    with pytest.raises(IndexError):
        m.score_hypotheses_many(srcs[:3] + [bad_src] + srcs[4:], hyps)
    g = tta.TranslationInferenceGreedy(m, 100, 5, BOS, EOS)                            # a generator whose pad is not the model's
    with pytest.raises(ValueError):
        g.score_many(srcs, hyps)

    # the C boundary refuses before any launch: the outputs keep their poison
    lib, sess, stream = m._lib, m._scoring_session(), m._stream()
    two = [(srcs[1], hyps[1].reshape(-1, hyps[1].shape[2]), 1, hyps[1].shape[2]), (srcs[2], hyps[2].reshape(-1, hyps[2].shape[2]), 5, hyps[2].shape[2])]
    S, R = 3 + 4, 3 + 20
    score = torch.full((R,), 7.0, device="cuda")
    length = torch.full((R,), 7, dtype=torch.int32, device="cuda")
    e = torch.full((S,), 7, dtype=torch.int32, device="cuda")
    ls = torch.full((S,), 7, dtype=torch.int32, device="cuda")
    W1, W2, L1, L2 = hyps[1].shape[2], hyps[2].shape[2], srcs[1].shape[1], srcs[2].shape[1]

    def table(**edit):
        t = m.score_batch_table(two)
        for k, v in edit.items():
            setattr(t[1], k, v)
        return t

    def ext(t, nb=2, d_e=e.data_ptr(), d_ls=ls.data_ptr()):
        return lib.ttx_score_list_extents(sess, t, nb, EOS, d_e, d_ls, None, None, stream)

    def run(t=None, nb=2, order=(0, 1, 2, 3, 4, 5, 6), chunks=((0, 3, 1, W1, L1), (3, 4, 5, W2, L2)), d_score=score.data_ptr(),
            d_length=length.data_ptr(), tok=None, off=None, n_order=None, null_order=False, null_chunks=False):
        o = (C.c_int32 * len(order))(*order)
        ch = (N.ScoreChunk * max(1, len(chunks)))(*[N.ScoreChunk(*c) for c in chunks])
        return lib.ttx_score_list_run(sess, t if t is not None else table(), nb, None if null_order else o,
                                      len(order) if n_order is None else n_order, None if null_chunks else ch, len(chunks), EOS,
                                      d_score, d_length, None, tok, off, stream)

    INV = N.TTX_ERR_INVALID
    assert lib.ttx_score_list_extents(None, table(), 2, EOS, e.data_ptr(), ls.data_ptr(), None, None, stream) == INV
    assert ext(table(), d_e=None) == INV and ext(table(), d_ls=None) == INV and ext(None) == INV and ext(table(), nb=0) == INV
    for edit in (dict(ld_hyp=W2 - 1), dict(W=1), dict(B=0), dict(N=0), dict(Ls=0), dict(d_src=None), dict(d_hyp=None)):
        assert ext(table(**edit)) == INV and run(table(**edit)) == INV, edit
    assert b"ld_hyp" in (ext(table(ld_hyp=W2 - 1)), lib.ttx_last_error())[1]
    assert run(null_order=True) == INV and run(null_chunks=True) == INV and run(chunks=()) == INV and run(nb=0) == INV
    assert run(d_score=None) == INV and run(d_length=None) == INV
    assert run(order=(0, 1, 2, 3, 4, 5, 5)) == INV and b"twice" in lib.ttx_last_error()                # a source covered twice
    assert run(chunks=((0, 3, 1, W1, L1), (3, 3, 5, W2, L2))) == INV and b"left out" in lib.ttx_last_error()
    assert run(order=(0, 1, 2, 3, 4, 5), chunks=((0, 3, 1, W1, L1), (3, 3, 5, W2, L2))) == INV         # the order names 6 of 7 sources
    assert run(chunks=((0, 3, 1, W1, L1), (2, 5, 5, W2, L2))) == INV                                   # overlapping chunks
    assert run(chunks=((0, 3, 1, W1, L1), (3, 5, 5, W2, L2))) == INV                                   # beyond the order
    assert run(order=(0, 1, 2, 3, 4, 5, 7)) == INV and run(order=(0, 1, 2, 3, 4, 5, -1)) == INV        # outside the list
    assert run(chunks=((0, 4, 1, W1, L1), (4, 3, 5, W2, L2))) == INV and b"another N" in lib.ttx_last_error()
    assert run(chunks=((0, 3, 1, 1, L1), (3, 4, 5, W2, L2))) == INV                                    # W_c < 2
    assert run(chunks=((0, 3, 1, W1, 0), (3, 4, 5, W2, L2))) == INV                                    # Ls_c < 1
    assert run(chunks=((0, 3, 1, W1, L1), (3, 4, 5, 5002, L2))) == INV                                 # beyond the positional table
    assert run(chunks=((0, 3, 1, W1, 5001), (3, 4, 5, W2, L2))) == INV
    assert run(chunks=((0, 3, 1, W1, L1), (3, 4, 1 << 20, 5, L2))) == INV                              # N of no batch
    tok = torch.full((R * 200,), 7.0, device="cuda")
    assert run(tok=tok.data_ptr(), off=None) == INV                                                    # tok_logp without offsets
    # 2^24 positions in one chunk: 4 096 sources x 64 rows x 64 columns, described but never read
    big = (N.ScoreBatch * 1)(N.ScoreBatch(srcs[2].data_ptr(), hyps[2].data_ptr(), 1 << 12, L2, 1 << 6, 65, 65))
    assert lib.ttx_score_list_run(sess, big, 1, (C.c_int32 * 4096)(*range(4096)), 4096, (N.ScoreChunk * 1)(N.ScoreChunk(0, 4096, 64, 65, L2)),
                                  1, EOS, score.data_ptr(), length.data_ptr(), None, None, None, stream) == INV
    assert b"2^24" in lib.ttx_last_error()
    a = N.DebugScoreListArgs(N=1, W=W1, Ls=L1, eos=EOS)
    assert lib.ttx_debug_score_list(sess, 3, table(), 2, None, 0, None, C.byref(a), stream) == INV     # no such op
    assert lib.ttx_debug_score_list(sess, 0, table(), 2, None, 0, None, C.byref(a), stream) == INV     # op 0 without d_e
    assert lib.ttx_debug_score_list(sess, 1, table(), 2, (C.c_int32 * 1)(0), 1, None, C.byref(a), stream) == INV   # op 1 without outputs
    assert lib.ttx_debug_score_list(sess, 1, table(), 2, (C.c_int32 * 1)(3), 1, None, C.byref(a), stream) == INV   # a source of another N
    assert lib.ttx_debug_score_list(sess, 2, table(), 2, None, 0, None, C.byref(a), stream) == INV     # op 2 without sources
    torch.cuda.synchronize()
    assert (score == 7.0).all() and (length == 7).all() and (e == 7).all() and (ls == 7).all() and (tok == 7.0).all()
    # the accepted call, and the session is still usable
    assert ext(table()) == 0 and run() == 0
    torch.cuda.synchronize()
    assert torch.equal(score[:3], ref[1].score.reshape(-1)) and torch.equal(score[3:], ref[2].score.reshape(-1))
    _assert_same(m.score_hypotheses_many(srcs, hyps), ref, "after the refusals", FIELDS[:3])


def test_vocabulary_above_1024_is_refused(tta):
    N = tta._native
    from util_models import seeded_weights, state_shapes
    st = seeded_weights(state_shapes(1025, 64, 64, 1, 1), 3)
    m = tta.NativeTransformer(st, 2, 0, device=0)
    src = torch.ones((1, 3), dtype=torch.int64, device="cuda")
    hyp = torch.ones((1, 1, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(tta.TtxError) as err:
        m.score_hypotheses_many([src], [hyp])
    assert err.value.code == N.TTX_ERR_INVALID and "1024" in str(err.value)


# -- Lightning: the look-ahead scores its windows through score_many -----------------------------------------------------------
class FixtureTokenizer:
    """Shape of the reference's GenericTokenizer that the module uses (tokenizer_base.py:16-94)."""
    pad_token_idx, bos_token_idx, eos_token_idx, unk_token_idx = 0, 1, 2, 3

    def __init__(self):
        import json
        from util_models import GOLDEN
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


@pytest.mark.parametrize("generation,fold", [("greedy_speculative", False), ("beam_search_speculative", False),
                                             ("sampling_speculative", False), ("sampling_speculative", True)])
def test_look_ahead_serves_the_scores_of_the_per_batch_pass(tta, tmp_path, monkeypatch, generation, fold):
    import json
    monkeypatch.delenv("TTX_PREDICT_SCORES", raising=False)
    src, tgt, _, _ = fixture_tokens()
    batches = []
    for i, j in ((0, 3), (3, 4), (4, 8), (8, 10)):
        s_ = src[i:j]
        batches.append({"src_tokens": s_[:, :int((s_ != PAD).sum(1).max())].cuda(), "tgt_tokens": tgt[i:j].cuda()})
    kw = {"greedy_speculative": {}, "beam_search_speculative": dict(beam_size=3, smart_drafts_mode=False),
          "sampling_speculative": dict(beam_size=4, sampling_seed=9)}[generation]
    runs = {}
    for label, env in (("list", None), ("per_batch", "0")):
        if env is None:
            monkeypatch.delenv("TTX_SCORE_LIST", raising=False)
        else:
            monkeypatch.setenv("TTX_SCORE_LIST", env)
        mod = _module(tta, generation, tmp_path / f"{label}.txt", **kw)
        mod.predict_with_scores, mod.predict_fold_samples, mod.predict_sample_pool = True, fold, True
        outs = tta.run_predict(mod, batches, schedule="rows", window=3, in_flight=2)
        rep = json.loads((tmp_path / f"{label}.txt").read_text().strip().split("\n")[-1])
        runs[label] = (outs, rep, mod)
        assert mod._ahead is not None and mod._ahead.served == len(batches) and mod._ahead.score_ahead == (env is None)
        assert mod._ahead.scores == {} and rep["scoring_seconds"] > 0
    (a_outs, a_rep, a), (b_outs, b_rep, b) = runs["list"], runs["per_batch"]
    assert all(torch.equal(x, y) for x, y in zip(a_outs, b_outs))
    assert set(a_rep) == set(b_rep) and a_rep["model_calls"] == b_rep["model_calls"]
    assert a_rep["mean_top1_logprob"] == b_rep["mean_top1_logprob"] and a_rep["unfinished_hypotheses"] == b_rep["unfinished_hypotheses"]
    assert sorted(a.predict_scores) == sorted(b.predict_scores) == list(range(len(batches)))
    _assert_same([a.predict_scores[i] for i in range(len(batches))], [b.predict_scores[i] for i in range(len(batches))],
                 f"{generation} fold={fold}", FIELDS[:3])
    if fold:
        for i in range(len(batches)):
            assert all(torch.equal(x, y) for x, y in zip(a.predict_folds[i], b.predict_folds[i]))
    else:
        for i, (bt, p) in enumerate(zip(batches, a_outs)):
            _assert_same([a.predict_scores[i]], [a.generator.score(bt["src_tokens"], p)], f"{generation} batch {i}", FIELDS[:3])
    # a look-ahead that also owes log q keeps the per-batch passes
    if generation == "sampling_speculative" and not fold:
        monkeypatch.delenv("TTX_SCORE_LIST", raising=False)
        mod = _module(tta, generation, tmp_path / "logq.txt", **kw)
        mod.predict_with_scores, mod.predict_with_logq, mod.predict_sample_pool = True, True, True
        tta.run_predict(mod, batches, schedule="rows", window=3, in_flight=2)
        assert mod._ahead is not None and not mod._ahead.score_ahead
        _assert_same([mod.predict_scores[i] for i in range(len(batches))], [a.predict_scores[i] for i in range(len(batches))],
                     "with log q", FIELDS[:3])
