"""Constrained beam search end to end (include/ttx.h "Constrained beam search"; TranslationInferenceBeamSearchConstrained) on the tiny
golden model with the fixture vocabulary and the ten fixture sources.

The settings were chosen on the CPU with the float64 oracle alone (tests/util_beam_constrained.py), and the tests repeat that choice
as assertions: K = 3 and max_len = 8.  The tiny model's distributions are flat, so its totals lie close together: at these settings
at most two of the ten sources per setting have, at some level, two of the best K + 1 totals closer than 2 * LOGIT_TOL * level (none
to two, by setting), at K = 3 and max_len = 10 up to four have.  The model's rows are long, so under max_len = 8 the column budget
of the syntax rule binds on every row: no unconstrained row is finished, every constrained one is.

Tolerances.  The exhaustive case: LOGIT_TOL per token against the float64 oracle, the constant the sampling tests use.  logp against
logq: tests/test_gpu_logq.py's bound, TOK_TOL * max(1, max |token_logq|) per scored token.  Rows against the float64 search: equal
tokens; a source is left out only where the oracle's own margin is below 2 * LOGIT_TOL * level, at most 2 of 10 per setting, printed.
Everything else is equality on the bits.
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import util_beam_constrained as C
import util_syntax as Y
from test_gpu_model import LOGIT_TOL
from test_gpu_score import TOK_TOL
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
K, MAX_LEN = 3, 8
ATOM, OPEN_ID, CLOSE_ID = 5, 6, 7                          # "C", "(", ")" of tests/golden/fixture_vocab.json
V = 30
NEG = float("-inf")


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def model(tta):
    """(NativeTransformer, float64 oracle) of the tiny golden model, built once."""
    from oracle.model import OracleTransformer, config_from_state
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0), OracleTransformer(config_from_state(st, cfg["num_heads"]), st, dtype=torch.float64)


@pytest.fixture(scope="module")
def src():
    s = fixture_tokens()[0]
    return s[:, :int((s != PAD).sum(1).max())]


@pytest.fixture(scope="module")
def syn(tta):
    vocab = json.loads((Path(__file__).resolve().parent / "golden" / "fixture_vocab.json").read_text())
    return tta.SmilesSyntax.from_vocab(vocab)


@pytest.fixture(scope="module")
def allow(tta, src):
    """The "tokens of the source" allow-list with EOS and the structure tokens, Bool[10, V]."""
    a = tta.scoring.allowlist_from_source(src, [EOS, OPEN_ID, CLOSE_ID], V, PAD)
    assert a.shape == (10, V) and bool((~a).any(1).all())
    return a


@pytest.fixture(scope="module")
def prefixes():
    """Per-source prefixes of 0, 1, 2 and 3 tokens ("C(C"), right-padded."""
    p = torch.full((10, 3), PAD, dtype=torch.int64)
    for b in range(10):
        p[b, :b % 4] = torch.tensor([ATOM, OPEN_ID, ATOM])[:b % 4]
    return p


def plain(tta, native, k=K, max_len=MAX_LEN):
    return tta.TranslationInferenceBeamSearch(native, k, max_len, PAD, BOS, EOS)


def constrained(tta, native, k=K, max_len=MAX_LEN):
    return tta.TranslationInferenceBeamSearchConstrained(native, k, max_len, PAD, BOS, EOS)


def bad_rows(rows, cls) -> list:
    """Every row that is not finished, not balanced or holds a FORBID token."""
    rows = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows)
    return [r.tolist() for r in rows.reshape(-1, rows.shape[-1]) if Y.row_report(cls, r, EOS) != (True, True, False)]


def widened(a: torch.Tensor, width: int) -> torch.Tensor:
    out = torch.full(a.shape[:-1] + (width,), PAD, dtype=a.dtype, device=a.device)
    out[..., :a.shape[-1]] = a
    return out


def same_rows(a: torch.Tensor, b: torch.Tensor) -> bool:
    w = max(a.shape[-1], b.shape[-1])
    return torch.equal(widened(a, w), widened(b, w))


def launches(native) -> tuple:
    p = native.kernel_profile()
    return p["logit_bias_launches"], p["syntax_launches"], native.debug_beam_step_masked_launches()


# -- identity ------------------------------------------------------------------------------------------------------------------------
def test_unconstrained_calls_are_plain_beam_search(tta, src, syn):
    st, cfg = tiny_state()
    native = tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0)          # a session of its own: the counters start at zero
    s = src.cuda()
    want = plain(tta, native).generate(s)
    g = constrained(tta, native)
    out, det = g.generate(s, return_details=True)
    assert torch.equal(out, want) and launches(native) == (0, 0, 0), "the call without a keyword launched a constraint kernel"
    assert det.logp.shape == (10, K) and bool(det.alive.all()) and bool((det.logp[:, :-1] >= det.logp[:, 1:]).all())
    zero, lp0 = g.generate(s, logit_bias=torch.zeros(10, V), return_details=True)
    lb, sy, ms = launches(native)
    assert torch.equal(zero, want) and torch.equal(lp0.logp, det.logp) and lb > 0 and sy == 0 and ms == lb
    assert torch.equal(g.generate(s, allowed=torch.ones(10, V, dtype=torch.bool)), want)
    # an all-neutral table forbids nothing before the last column: the sources whose K rows end before max_len = 32
    sub = s[[4, 6, 9]]
    want32 = plain(tta, native, max_len=32).generate(sub)
    assert want32.shape[-1] < 32, "a row reaches the last column: the neutral table would bind there"
    neutral = torch.zeros(V, dtype=torch.int8)
    assert torch.equal(constrained(tta, native, max_len=32).generate(sub, syntax=neutral), want32)
    assert launches(native)[1] > 0
    # the counters are the plain generator's
    a, b = plain(tta, native), constrained(tta, native)
    a.generate(s), b.generate(s)
    assert (a.model_calls_num, a.b_sz, a.given_tokens) == (b.model_calls_num, b.b_sz, b.given_tokens)


# -- the exhaustive case ---------------------------------------------------------------------------------------------------------------
def test_two_token_allow_list_is_enumerated(tta, model, src):
    native, o64 = model
    s = src.cuda()
    two = torch.zeros(10, V, dtype=torch.bool)
    two[:, [ATOM, EOS]] = True
    out, det = constrained(tta, native, k=5, max_len=4).generate(s, allowed=two, return_details=True)
    out, logp, alive = out.cpu(), det.logp.cpu().double(), det.alive.cpu()
    assert out.shape == (10, 5, 4)
    X = ATOM
    every = {(BOS, EOS, PAD, PAD): 1, (BOS, X, EOS, PAD): 2, (BOS, X, X, EOS): 3, (BOS, X, X, X): 3}      # row -> scored tokens
    worst = 0.0
    for b in range(10):
        rows = [tuple(r) for r in out[b].tolist()]
        assert sorted(rows[:4]) == sorted(every) and alive[b].tolist() == [True] * 4 + [False], f"source {b}: {rows}"
        assert rows[4] == (BOS, PAD, PAD, PAD) and logp[b, 4].item() == NEG and bool(det.finished[b, 4])
        assert bool((logp[b, :3] >= logp[b, 1:4]).all())
        for r, row in enumerate(rows[:4]):
            n = every[row]
            with torch.no_grad():
                lg = o64(src[b:b + 1], torch.tensor([row[:n]]))[0].numpy()
            ref = sum(lg[t, row[t + 1]] - np.logaddexp(lg[t, X], lg[t, EOS]) for t in range(n))
            worst = max(worst, abs(logp[b, r].item() - ref) / n)
            assert abs(logp[b, r].item() - ref) <= LOGIT_TOL * n, f"source {b} row {row}: logp {logp[b, r].item()} against {ref}"
    print(f"exhaustive case: largest |logp - oracle| per token {worst:.3g} (bound {LOGIT_TOL})")


# -- properties --------------------------------------------------------------------------------------------------------------------------
def test_properties(tta, model, src, syn, allow, prefixes):
    native, _ = model
    s, cls = src.cuda(), syn.cls.numpy()
    g = constrained(tta, native)
    free = plain(tta, native).generate(s)
    out, det = g.generate(s, allowed=allow, return_details=True)
    for b in range(10):
        toks = out[b][det.alive[b]][:, 1:].cpu().numpy()
        assert toks.size and bool(allow[b].numpy()[toks[toks != PAD]].all()), f"source {b}: a forbidden id under its allow-list"
    assert any(not allow[b].numpy()[t] for b in range(10) for t in free[b, :, 1:].cpu().numpy().ravel() if t != PAD), \
        "the unconstrained beam stays inside the allow-lists: the check shows nothing"
    out, det = g.generate(s, syntax=syn, return_details=True)
    assert bool(det.alive.all()) and not bad_rows(out, cls), f"{bad_rows(out, cls)[:3]}"
    rep = syn.check(out, EOS)
    assert bool(rep.balanced.all()) and bool(rep.finished.all()) and bool((rep.first_offending == -1).all()) and bool(det.finished.all())
    assert len(bad_rows(free, cls)) >= 20, "the unconstrained beam ends most rows balanced inside max_len: the check shows nothing"
    out, det = g.generate(s, prefix=prefixes, return_details=True)
    assert bool(det.alive.all())
    for b in range(10):
        n = b % 4
        assert bool((out[b, :, 1:1 + n].cpu() == prefixes[b, :n]).all()), f"source {b}: a row leaves its prefix"
    for kw in (dict(allowed=allow), dict(syntax=syn), dict(prefix=prefixes), dict(allowed=allow, syntax=syn, prefix=prefixes)):
        out, det = g.generate(s, return_details=True, **kw)
        for b in range(10):
            rows = [tuple(r) for r, a in zip(out[b].tolist(), det.alive[b].tolist()) if a]
            assert len(set(rows)) == len(rows), f"{sorted(kw)}: source {b} returns a row twice"
            assert bool((det.logp[b, :-1] >= det.logp[b, 1:]).all())


# -- scores -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["allow", "syntax", "prefix", "all"])
def test_logp_is_logq(tta, model, src, syn, allow, prefixes, setting):
    native, _ = model
    s = src.cuda()
    kw = dict(allow=dict(allowed=allow), syntax=dict(syntax=syn), prefix=dict(prefix=prefixes),
              all=dict(allowed=allow, syntax=syn, prefix=prefixes))[setting]
    g = constrained(tta, native)
    out, det = g.generate(s, return_details=True, **kw)
    q = g.logq(s, out, return_token_logq=True, **kw)
    alive = det.alive.cpu()
    assert bool((q.first_outside.cpu()[alive] == -1).all()), "a returned row lies outside the constrained distribution"
    tok = q.token_logq.cpu().double()
    per_tok = TOK_TOL * max(1.0, tok[torch.isfinite(tok)].abs().max().item())
    err = (q.logq.cpu().double() - det.logp.cpu().double()).abs()[alive]
    bound = (q.length.cpu().double() * per_tok)[alive]
    print(f"{setting}: {int(alive.sum())} rows, max |logq - logp| {err.max().item():.3g}, largest share of its bound {(err / bound).max().item():.3g}")
    assert int(alive.sum()) >= 20 and bool((err <= bound).all())
    if "prefix" in kw:
        for b in range(10):
            assert bool((tok[b, :, :b % 4] == 0).all()), "a forced position costs something"


# -- against the float64 constrained beam search -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["free", "allow", "syntax", "prefix"])
def test_rows_are_the_float64_search(tta, model, src, syn, allow, prefixes, setting):
    native, o64 = model
    s = src.cuda()
    kw = dict(free={}, allow=dict(allowed=allow), syntax=dict(syntax=syn), prefix=dict(prefix=prefixes))[setting]
    out, det = constrained(tta, native).generate(s, return_details=True, **kw)
    out, logp = out.cpu().numpy(), det.logp.cpu().numpy()
    left_out, worst = [], 0.0
    for b in range(10):
        okw = {}
        if setting == "allow":
            okw["bias"] = np.where(allow[b].numpy(), 0.0, -np.inf)
        if setting == "syntax":
            okw["cls"] = syn.cls.numpy()
        if setting == "prefix":
            okw["prefix"] = prefixes[b, :b % 4].tolist()
        rows, tot, close = C.search(o64, src[b], K, MAX_LEN, PAD, BOS, EOS, LOGIT_TOL, levels=out.shape[-1] - 1, **okw)
        if close:
            left_out.append(b)
            continue
        assert rows.tolist() == out[b].tolist(), f"{setting}: source {b}: {out[b].tolist()} against the float64 search's {rows.tolist()}"
        n = np.maximum((rows[:, 1:] != PAD).sum(1), 1)
        assert (np.isneginf(logp[b]) == np.isneginf(tot)).all(), f"{setting}: source {b}: dead rows differ"
        err = np.where(np.isneginf(tot), 0.0, np.abs(np.where(np.isneginf(logp[b]), 0.0, logp[b]) - np.where(np.isneginf(tot), 0.0, tot)))
        worst = max(worst, float((err / n).max()))
        assert (err <= 2 * LOGIT_TOL * n).all()       # a log-softmax value moves by at most twice the logits' error
    print(f"{setting}: sources left out (an oracle margin below 2 * LOGIT_TOL * level): {left_out}; largest |logp - oracle| per token {worst:.3g}")
    assert len(left_out) <= 2, f"{setting}: the oracle alone leaves out {left_out}: choose other settings"


# -- invariance ---------------------------------------------------------------------------------------------------------------------------
def test_invariance(tta, model, src, syn, allow, prefixes):
    native, _ = model
    s = src.cuda()
    g = constrained(tta, native)
    kw = dict(allowed=allow, syntax=syn, prefix=prefixes)
    out, det = g.generate(s, return_details=True, **kw)
    again, det2 = g.generate(s, return_details=True, **kw)
    assert torch.equal(out, again) and torch.equal(det.logp, det2.logp), "run to run"
    wide = torch.cat([s, torch.full((10, 9), PAD, dtype=s.dtype, device=s.device)], 1)
    padded, det3 = g.generate(wide, return_details=True, **kw)
    assert torch.equal(out, padded) and torch.equal(det.logp, det3.logp), "a wider source pad"
    for b in (0, 3, 7):
        one, d1 = g.generate(s[b:b + 1], return_details=True, allowed=allow[b:b + 1], syntax=syn, prefix=prefixes[b:b + 1])
        assert same_rows(one, out[b:b + 1]) and torch.equal(d1.logp, det.logp[b:b + 1]), f"source {b} alone against the batch"


# -- refusals at the entry point -----------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_before_any_launch(tta, model, src, syn):
    import ctypes as Ct
    from translation_transformer_amd import _native as N
    native, _ = model
    s = src[:2].cuda().contiguous()
    out = torch.full((2, K, MAX_LEN), -7, dtype=torch.int64, device="cuda")
    p = N.BeamSearchParams(MAX_LEN, K, PAD, BOS, EOS)
    bias, d_cls = torch.zeros(2, V, device="cuda"), syn.cls.cuda()
    pre = torch.full((2, 3), ATOM, dtype=torch.int64, device="cuda")

    def call(bias_ptr=None, ld_bias=0, syntax=None, prefix_ptr=None, ld_prefix=0, lens=None):
        h = None if lens is None else (Ct.c_int32 * 2)(*lens)
        rc = native._lib.ttx_beam_generate_constrained(native.session, s.data_ptr(), 2, s.shape[1], Ct.byref(p), bias_ptr, ld_bias, syntax,
                                                       prefix_ptr, ld_prefix, h, out.data_ptr(), None, Ct.byref(N.BeamSearchStats()),
                                                       native._stream())
        torch.cuda.synchronize()
        return rc

    for bad in (dict(bias_ptr=bias.data_ptr(), ld_bias=V - 1), dict(syntax=Ct.byref(N.Syntax(d_cls.data_ptr(), MAX_LEN + 1))),
                dict(prefix_ptr=pre.data_ptr(), ld_prefix=3, lens=[MAX_LEN, 0]), dict(prefix_ptr=pre.data_ptr(), ld_prefix=2, lens=[3, 0]),
                dict(prefix_ptr=None, ld_prefix=3, lens=[1, 0]), dict(prefix_ptr=pre.data_ptr(), ld_prefix=3, lens=[-1, 0])):
        assert call(**bad) == N.TTX_ERR_INVALID and bool((out == -7).all()), f"{sorted(bad)}"
    assert call(bias_ptr=bias.data_ptr(), ld_bias=V, syntax=Ct.byref(N.Syntax(d_cls.data_ptr(), 0)), prefix_ptr=pre.data_ptr(), ld_prefix=3,
                lens=[3, 0]) == 0
    want = constrained(tta, native).generate(s, logit_bias=bias, syntax=syn, prefix=torch.tensor([[ATOM] * 3, [PAD] * 3]))
    assert torch.equal(out[:, :, :want.shape[-1]], want)


# -- Lightning ---------------------------------------------------------------------------------------------------------------------------
def test_lightning_passes_the_constraints_through(tta, src, syn, allow, tmp_path):
    from test_gpu_lightning_surface import FixtureTokenizer
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    cls = syn.cls.numpy()
    s, tgt = src[:4], fixture_tokens()[1][:4]

    def module(gen="beam_search_constrained"):
        mod = tta.VanillaEncoderDecoderTransformerLightning(
            src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
            num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
            share_embeddings=True, generation=gen, beam_size=K, max_len=MAX_LEN, n_drafts=3, draft_len=4,
            report_prediction_file=str(tmp_path / "r.txt"))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        return mod

    def batches(bs, **more):
        return [dict({"src_tokens": s[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda()}, **{k: v[i:i + bs].cuda() for k, v in more.items()})
                for i in range(0, 4, bs)]

    cat = lambda preds: torch.cat([widened(q, MAX_LEN) for q in preds], 0).cpu()
    free = cat(tta.run_predict(module("beam_search"), batches(4)))
    assert torch.equal(cat(tta.run_predict(module(), batches(4))), free)                        # no constraint: the plain rows
    pred = cat(tta.run_predict(module(), batches(2, allowed_tokens=allow[:4])))
    inside = lambda rows: all(bool(allow[b].numpy()[t]) for b in range(4) for t in rows[b, :, 1:].numpy().ravel() if t != PAD)
    assert pred.shape[:2] == (4, K) and inside(pred), "the allow-list did not reach the generator"
    assert not inside(free), "the unconstrained module stays inside the allow-lists: the check shows nothing"
    mod = module()
    mod.predict_syntax_constraint = True
    pred = cat(tta.run_predict(mod, batches(4)))
    assert not bad_rows(pred, cls), "the switch did not reach the generator"
    assert bad_rows(free, cls), "the unconstrained module balances every row: the check shows nothing"
    with pytest.raises(ValueError, match="allowed_tokens"):
        tta.run_predict(module("beam_search"), batches(4, allowed_tokens=allow[:4]))
