"""Syntax-constrained sampling end to end (include/ttx.h "Syntax-constrained sampling"): the plain and the speculative sampler, the
sampling pool and log q on the tiny golden model with the fixture vocabulary ("(" opens, ")" closes, "1" .. "4" are ring labels 0 .. 3;
PAD, BOS and "?" are forbidden), the ten fixture sources.

The settings (chosen on the CPU with the float64 oracle's own sampler, which the first test repeats): temperature 3 and max_len 24.
The tiny model's rows are long, so hardly any unconstrained row is finished and balanced inside 24 columns, and the budget part of the
rule acts on every constrained row: about one position in eleven leaves a single token (a closer, or EOS in the last column), which
the sampler emits with probability 1.  At temperature 3 the oracle's constrained sampler still gives its emitted tokens a mean
probability of 0.33 (0.64 at temperature 2, which would trip the replay test's own "the check went soft" guard).

Tolerances are those of the tests this file extends.  Replay of sampled tokens: tests/test_gpu_logit_bias.py's interval test on the
float64 oracle's logits UNDER THE RESTATEMENT'S MASK (tests/util_syntax.py), tol = 2 * LOGIT_TOL / T + 1e-4.  Temperature 0: the token
is the first maximum of the masked float64 logits wherever the top two are at least 2 * LOGIT_TOL apart; at most a tenth of the
positions may be closer (an assertion on the oracle alone).  token_logq: tests/test_gpu_logq.py's TOK_TOL * max(1, max |ref|) *
max(1, 1 / T).  Everything else is equality on the bits.
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import util_logq_checks as Q
import util_sample_checks as S
import util_syntax as Y
from test_gpu_model import LOGIT_TOL
from test_gpu_sampling import check_shape, oracle_logits
from test_gpu_score import TOK_TOL
from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
SEED = 20261021
MAX_LEN = 24
T = 3.0
OPEN_ID, CLOSE_ID, RING1_ID, ATOM = 6, 7, 8, 5          # "(", ")", "1", "C" of tests/golden/fixture_vocab.json


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
def c_token():
    return fixture_tokens()[2]


@pytest.fixture(scope="module")
def syn(tta):
    vocab = json.loads((Path(__file__).resolve().parent / "golden" / "fixture_vocab.json").read_text())
    s = tta.SmilesSyntax.from_vocab(vocab)
    cls = s.cls.numpy()
    assert cls[OPEN_ID] == 1 and cls[CLOSE_ID] == 2 and cls[RING1_ID] == 3 and cls[ATOM] == 0 and (cls[[PAD, BOS, 3]] == -1).all()
    return s


def plain(tta, native, max_len=MAX_LEN, **kw):
    kw.setdefault("temperature", T)
    kw.setdefault("seed", SEED)
    return tta.TranslationInferenceSampling(native, max_len, PAD, BOS, EOS, **kw)


def spec(tta, native, c, max_len=MAX_LEN, **kw):
    kw.setdefault("temperature", T)
    kw.setdefault("seed", SEED)
    return tta.TranslationInferenceSamplingSpeculative(native, max_len, 4, 3, PAD, BOS, EOS, c, **kw)


def bad_rows(out, cls) -> list:
    """(row index, row) of every row that is not finished, not balanced or holds a FORBID token."""
    rows = np.asarray(out.cpu() if isinstance(out, torch.Tensor) else out)
    rows = rows.reshape(-1, rows.shape[-1])
    return [(i, r.tolist()) for i, r in enumerate(rows) if Y.row_report(cls, r, EOS) != (True, True, False)]


def masked(lg_row: np.ndarray, cls, prefix, pos: int, max_len: int) -> np.ndarray:
    """The oracle's logits of one position as the constrained sampler's consumer reads them."""
    x = lg_row.copy()
    x[~Y.allowed(cls, *Y.state(cls, prefix), pos, max_len, EOS)] = -np.inf
    return x


def oracle_walk(o64, s: torch.Tensor, keys, n: int, cls=None) -> np.ndarray:
    """The float64 oracle's own sampler by the rule (S.sample64), unconstrained or under the restatement's mask."""
    R = s.shape[0] * n
    rows = np.full((R, MAX_LEN), PAD, dtype=np.int64)
    rows[:, 0] = BOS
    alive = np.ones(R, dtype=bool)
    p = S.Params(T, pad=PAD, eos=EOS)
    for pos in range(1, MAX_LEN):
        if not alive.any():
            break
        with torch.no_grad():
            lg = o64(s.repeat_interleave(n, 0), torch.from_numpy(rows[:, :pos]))[:, -1].numpy()
        u = S.uniform(SEED, np.repeat(keys, n), np.tile(np.arange(n), len(keys)), pos)
        for r in np.nonzero(alive)[0]:
            x = lg[r] if cls is None else masked(lg[r], cls, rows[r, 1:pos], pos, MAX_LEN)
            rows[r, pos] = S.sample64(x, u[r], p)
            alive[r] = rows[r, pos] not in (EOS, PAD)
    return rows


# -- 1: the rows ---------------------------------------------------------------------------------------------------------------------
def test_constrained_rows_end_in_eos_balanced_and_free_rows_do_not(tta, model, src, syn, c_token):
    native, o64 = model
    cls, s = syn.cls.numpy(), src.cuda()
    keys = list(range(10))
    # the float64 oracle's own sampler at these settings: unconstrained rows break the syntax, constrained ones cannot
    free64 = oracle_walk(o64, src[:3], np.arange(3), 2)
    assert bad_rows(free64, cls), "the oracle's unconstrained sampler happens to balance every row: choose other settings"
    assert not bad_rows(oracle_walk(o64, src[:3], np.arange(3), 2, cls), cls)
    batches = [s[:4], s[4:8], s[8:]]
    outs = {"plain": plain(tta, native, num_samples=4).generate(s, row_keys=keys, syntax=syn),
            "speculative": spec(tta, native, c_token, num_samples=4).generate(s, row_keys=keys, syntax=syn),
            "pooled": torch.cat(spec(tta, native, c_token, num_samples=4).generate_many(batches, syntax=syn)),
            "filtered": plain(tta, native, num_samples=4, top_k=8, top_p=0.9).generate(s, row_keys=keys, syntax=syn),
            "hot": plain(tta, native, num_samples=4, temperature=8.0).generate(s, row_keys=keys, syntax=syn)}
    used = set()
    for what, out in outs.items():
        check_shape(out.cpu().numpy(), 10, 4, MAX_LEN)
        assert not bad_rows(out, cls), f"{what}: {bad_rows(out, cls)[:3]}"
        rep = syn.check(out, EOS)
        assert rep.balanced.all() and rep.finished.all() and (rep.first_offending == -1).all(), f"{what}: SmilesSyntax.check disagrees"
        used |= set(out.cpu().numpy().reshape(-1).tolist())
    assert {OPEN_ID, CLOSE_ID, RING1_ID} <= used, "no row opens a branch or a ring: the check shows nothing"
    lens = S.ends(outs["plain"].cpu().numpy().reshape(40, MAX_LEN), PAD, EOS)
    assert (lens == MAX_LEN - 1).any(), "no row runs to the last column: the budget rule never acted"
    free = plain(tta, native, num_samples=4).generate(s, row_keys=keys)
    assert bad_rows(free, cls), "the unconstrained sampler balances every row: the check shows nothing"
    assert not (syn.check(free, EOS).first_offending == -1).all()


# -- 2: the float64 oracle -------------------------------------------------------------------------------------------------------------
def test_replay_of_sampled_tokens_against_the_masked_oracle(tta, model, src, syn):
    native, o64 = model
    cls = syn.cls.numpy()
    B, n = 4, 8
    s = src[:B]
    keys = np.array([5, 1 << 40, 7, -3], dtype=np.int64)
    out = plain(tta, native, num_samples=n).generate(s.cuda(), row_keys=keys, syntax=syn).cpu().numpy()
    end = check_shape(out, B, n, MAX_LEN)
    rows = out.reshape(B * n, MAX_LEN)
    lg = oracle_logits(o64, s, rows, n)
    p, tol = S.Params(T, pad=PAD, eos=EOS), 2 * LOGIT_TOL / T + 1e-4
    worst, probs, cut = 0.0, [], 0
    for r in range(B * n):
        for pos in range(1, end[r] + 1):
            x = masked(lg[r, pos - 1], cls, rows[r, 1:pos], pos, MAX_LEN)
            cut += int(np.isinf(x).sum())
            u = float(S.uniform(SEED, keys[r // n], r % n, pos))
            ex = S.excess(int(rows[r, pos]), x, u, p)
            worst = max(worst, ex)
            assert ex <= tol, f"row {r} position {pos}: token {rows[r, pos]} lies {ex:.3e} outside its interval (tol {tol:.3e})"
            y = S.scaled(x, T)
            probs.append(float(np.exp(y[rows[r, pos]] - y.max()) / np.exp(y - y.max()).sum()))
    print(f"{len(probs)} tokens, {cut} masked logits, mean probability of the emitted token {np.mean(probs):.3f}, distinct rows "
          f"{len({tuple(r) for r in rows.tolist()})} of {B * n}, largest excess over the exact interval {worst:.3e}")
    assert np.mean(probs) < 0.6 and len({tuple(r) for r in rows.tolist()}) > B, "the check went soft: the sampler hardly samples"


# -- 3: equality and invariance, bit for bit ---------------------------------------------------------------------------------------------
def test_speculative_and_pooled_rows_are_the_plain_samplers(tta, model, src, syn, c_token, monkeypatch):
    native = model[0]
    s = src.cuda()
    keys = list(range(10))
    g = plain(tta, native, num_samples=4)
    full = g.generate(s, row_keys=keys, syntax=syn)
    assert torch.equal(g.generate(s, row_keys=keys, syntax=syn), full) and torch.equal(g.generate(s, row_keys=keys, syntax=syn.cls), full)
    for b in (0, 3, 9):                      # a source alone, at its own width
        n = int((src[b] != PAD).sum())
        assert torch.equal(plain(tta, native, num_samples=4).generate(s[b:b + 1, :n], row_keys=[b], syntax=syn), full[b:b + 1]), f"source {b} alone"
    assert torch.equal(plain(tta, native, num_samples=1).generate(s, row_keys=keys, syntax=syn), full[:, :1])
    wide = torch.nn.functional.pad(s, (0, 7), value=PAD)
    assert torch.equal(plain(tta, native, num_samples=4).generate(wide, row_keys=keys, syntax=syn), full)
    sp = spec(tta, native, c_token, num_samples=4)
    assert torch.equal(sp.generate(s, row_keys=keys, syntax=syn), full), "speculative against plain"
    assert torch.equal(sp.generate(s, row_keys=keys, syntax=syn), full) and torch.equal(sp.generate(s, row_keys=keys, syntax=syn), full)
    assert torch.equal(spec(tta, native, c_token, num_samples=1).generate(s[2:5], row_keys=keys[2:5], syntax=syn), full[2:5, :1])
    good = full[:, 0, 1:].cpu()                                               # the first sample of every source as its proposal
    assert torch.equal(spec(tta, native, c_token, num_samples=4).generate(s, row_keys=keys, syntax=syn, proposal=good), full)
    junk = torch.full((10, 12), CLOSE_ID, dtype=torch.int64)                  # drafts the mask forbids at once: never accepted
    junk[:, 1::2] = 3
    assert torch.equal(spec(tta, native, c_token, num_samples=4).generate(s, row_keys=keys, syntax=syn, proposal=junk), full)
    # the pool
    sizes, offs = [4, 4, 2], [0, 4, 8]
    batches = [src[o:o + n, :max(2, int((src[o:o + n] != PAD).sum(1).max()))].cuda() for o, n in zip(offs, sizes)]
    want = [full[o:o + n] for o, n in zip(offs, sizes)]

    def same(what, got, ref=want):
        assert len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref)), what

    many = lambda **kw: spec(tta, native, c_token, num_samples=4).generate_many(batches, syntax=syn, **kw)
    same("default capacity", many())
    for cap in (4, 12):
        for fl in (1, 2):
            same(f"capacity {cap}, in_flight {fl}", many(capacity=cap, in_flight=fl))
    rev = spec(tta, native, c_token, num_samples=4).generate_many(batches[::-1], row_keys=[torch.arange(o, o + n) for o, n in zip(offs, sizes)][::-1],
                                                                  syntax=syn, capacity=12)
    same("the list reversed", rev[::-1])
    for env in (dict(TTX_TWO_PHASE="0"), dict(TTX_DRAFT_SELECT="0"), dict(TTX_TWO_PHASE_MIN_ROWS="0"),
                dict(TTX_TWO_PHASE_MIN_ROWS="0", TTX_DRAFT_SELECT="0")):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            same(str(env), many(capacity=16))
            same(f"{env}, one sample", spec(tta, native, c_token, num_samples=1).generate_many(batches, syntax=syn, capacity=3), [w[:, :1] for w in want])


# -- 4: no effect where it should have none ------------------------------------------------------------------------------------------------
def test_a_neutral_table_far_from_max_len_and_no_table_change_nothing(tta, src, syn, c_token):
    st, cfg = tiny_state()
    fresh = tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0)       # sessions that have served no call yet
    s = src[:4].cuda()
    long_len, V = 160, fresh.tgt_vocab_size
    neutral = tta.SmilesSyntax(torch.zeros(V, dtype=torch.int8))
    for _ in range(3):                                                        # eager, captured, replayed
        a = plain(tta, fresh, long_len, temperature=1.0, num_samples=3).generate(s)
        b = spec(tta, fresh, c_token, long_len, temperature=1.0, num_samples=3).generate(s)
    many = spec(tta, fresh, c_token, long_len, temperature=1.0, num_samples=3).generate_many([s[:2], s[2:]])
    plain(tta, fresh, long_len, temperature=1.0).generate(s, syntax=None)
    assert fresh.kernel_profile()["syntax_launches"] == 0, "a call without syntax launched k_syntax_mask"
    ends = S.ends(a.cpu().numpy().reshape(12, long_len), PAD, EOS)
    assert ends.max() < long_len - 1, "a row reaches max_len: choose a longer one"
    assert torch.equal(plain(tta, fresh, long_len, temperature=1.0, num_samples=3).generate(s, syntax=neutral), a), "plain"
    n = fresh.kernel_profile()["syntax_launches"]
    assert n > 0
    assert torch.equal(spec(tta, fresh, c_token, long_len, temperature=1.0, num_samples=3).generate(s, syntax=neutral), b), "speculative"
    got = spec(tta, fresh, c_token, long_len, temperature=1.0, num_samples=3).generate_many([s[:2], s[2:]], syntax=neutral)
    assert all(torch.equal(x, y) for x, y in zip(got, many)), "pooled"
    # a constrained step is never replayed for an unconstrained call, nor the other way round: alternate them on one session
    con = plain(tta, fresh, long_len, temperature=1.0, num_samples=3).generate(s, syntax=syn)
    assert not torch.equal(con, a)
    for _ in range(3):
        assert torch.equal(plain(tta, fresh, long_len, temperature=1.0, num_samples=3).generate(s), a)
        assert torch.equal(plain(tta, fresh, long_len, temperature=1.0, num_samples=3).generate(s, syntax=syn), con)


# -- 5: temperature 0 ------------------------------------------------------------------------------------------------------------------------
def test_temperature_0_is_the_argmax_over_the_allowed_set(tta, model, src, syn, c_token):
    native, o64 = model
    cls = syn.cls.numpy()
    out = plain(tta, native, temperature=0.0).generate(src.cuda(), syntax=syn)
    assert torch.equal(spec(tta, native, c_token, temperature=0.0).generate(src.cuda(), syntax=syn), out)
    assert torch.equal(torch.cat(spec(tta, native, c_token, temperature=0.0).generate_many([src[:5].cuda(), src[5:].cuda()], syntax=syn)), out)
    assert not bad_rows(out, cls)
    rows = out.cpu().numpy()[:, 0]
    end = S.ends(rows, PAD, EOS)
    lg = oracle_logits(o64, src, rows, 1)
    total = close = 0
    for r in range(10):
        for pos in range(1, end[r] + 1):
            x = masked(lg[r, pos - 1], cls, rows[r, 1:pos], pos, MAX_LEN)
            top = np.sort(x)[-2:]
            total += 1
            if top[1] - top[0] < 2 * LOGIT_TOL:
                close += 1
                continue
            assert rows[r, pos] == S.argmax_first(x), f"source {r} position {pos}: {rows[r, pos]}, the allowed argmax is {S.argmax_first(x)}"
    print(f"{total} positions, {close} with the top two allowed logits closer than 2 * LOGIT_TOL")
    assert total > 100 and close <= total / 10
    free = plain(tta, native, temperature=0.0).generate(src.cuda())
    assert not torch.equal(free, out) and bad_rows(free, cls), "the constraint changes no greedy token: the check shows nothing"


# -- 6: prefix and bias --------------------------------------------------------------------------------------------------------------------
def test_forced_tokens_count_in_the_state_and_a_bias_intersects(tta, model, src, syn, c_token):
    native = model[0]
    cls, s = syn.cls.numpy(), src[:4].cuda()
    # "C(1?" : a branch and a ring label the completion has to close, and a FORBID token the mask would never let through
    pre = torch.tensor([[ATOM, OPEN_ID, RING1_ID, 3]] * 4)
    out = plain(tta, native, num_samples=4).generate(s, prefix=pre, syntax=syn)
    assert torch.equal(out[:, :, 1:5].cpu(), pre[:, None, :].expand(4, 4, 4)), "a forced prefix position obeys the prefix, not the mask"
    assert torch.equal(spec(tta, native, c_token, num_samples=4).generate(s, prefix=pre, syntax=syn), out)
    rows = out.cpu().numpy().reshape(16, MAX_LEN)
    for r in rows:
        fin, bal, _ = Y.row_report(cls, r, EOS)
        assert fin and bal, f"the completion did not close what the prefix opened: {r.tolist()}"
        e = int(np.nonzero(r == EOS)[0][0])
        assert not (cls[r[5:e]] == -1).any() and (r[5:e] == CLOSE_ID).sum() >= 1 and (r[5:e] == RING1_ID).sum() % 2 == 1
    rep = syn.check(out, EOS)
    assert (rep.first_offending == 4).all(), "only the forced FORBID token offends"
    # a prefix that closes what was never opened is refused; one that needs more columns than remain is accepted and ends unfinished
    with pytest.raises(ValueError, match="depth goes negative"):
        plain(tta, native).generate(s, prefix=torch.tensor([[ATOM, CLOSE_ID]] * 4), syntax=syn)
    deep = torch.full((4, MAX_LEN - 4), OPEN_ID)
    got = plain(tta, native).generate(s, prefix=deep, syntax=syn).cpu().numpy()[:, 0]
    assert (got[:, 1:MAX_LEN - 3] == OPEN_ID).all() and (got[:, MAX_LEN - 3:] == CLOSE_ID).all(), "closers only once need exceeds the columns left"
    # a bias: the allowed set is the intersection (no ring label, no "c"; "(" and ")" stay)
    V = native.tgt_vocab_size
    allowed = torch.ones(4, V, dtype=torch.bool)
    allowed[:, [8, 10, 15, 19, 4]] = False
    for g in (plain(tta, native, num_samples=4), spec(tta, native, c_token, num_samples=4)):
        both = g.generate(s, allowed=allowed, syntax=syn)
        toks = set(both.cpu().numpy()[:, :, 1:].reshape(-1).tolist())
        assert not toks & {8, 10, 15, 19, 4} and not bad_rows(both, cls) and OPEN_ID in toks
    many = spec(tta, native, c_token, num_samples=4).generate_many([s[:2], s[2:]], allowed=[allowed[:2], allowed[2:]], syntax=syn)
    assert torch.equal(torch.cat(many), both)


# -- 7: log q --------------------------------------------------------------------------------------------------------------------------------
def test_logq_under_the_constraint(tta, model, src, syn, c_token):
    native, o64 = model
    cls = syn.cls.numpy()
    B, n = 4, 4
    s = src[:B].cuda()
    g = plain(tta, native, num_samples=n)
    pred, sc, q = g.generate(s, syntax=syn, return_scores=True, return_logq=True)
    assert bool(torch.isfinite(q.logq).all()) and bool((q.first_outside == -1).all()), "a sampled row is outside its own distribution"
    ref = g.score(s, pred)
    assert torch.equal(sc.score, ref.score) and torch.equal(sc.length, ref.length), "with_scores must keep the RAW model's log p, on score()'s bits"
    again = g.logq(s, pred, syntax=syn, return_token_logq=True)
    free = g.logq(s, pred, return_token_logq=True)
    assert torch.equal(again.logq, q.logq) and not torch.equal(free.logq, q.logq)
    assert bool((again.logq >= free.logq).all()), "masking can only raise the probability of a token that stays allowed"
    # the sum of the replayed constrained log-probabilities on the float64 oracle
    rows = pred.cpu().numpy().reshape(B * n, MAX_LEN)
    length = q.length.cpu().numpy().reshape(-1)
    lg = oracle_logits(o64, src[:B], rows, n)
    tok = again.token_logq.cpu().numpy().reshape(B * n, MAX_LEN - 1).astype(np.float64)
    p = S.Params(T, pad=PAD, eos=EOS)
    errs, ref_max, sums = [], 0.0, np.zeros(B * n)
    for r in range(B * n):
        for pos in range(int(length[r])):
            want = Q.token_logq(masked(lg[r, pos], cls, rows[r, 1:pos + 1], pos + 1, MAX_LEN), int(rows[r, pos + 1]), p)[0]
            assert want > -np.inf
            errs.append(abs(tok[r, pos] - want))
            ref_max = max(ref_max, abs(want))
            sums[r] += want
    bound = TOK_TOL * max(1.0, ref_max) * max(1.0, 1.0 / T)
    print(f"{len(errs)} tokens, max |token_logq - float64| {max(errs):.3g} (bound {bound:.3g})")
    assert len(errs) > 100 and max(errs) <= bound
    assert np.abs(again.logq.cpu().numpy().reshape(-1).astype(np.float64) - sums).max() <= bound * length.max()
    # an unmatched ")": -inf, first_outside at its position; a neighbouring row stays inside
    hyp = pred.clone()
    where = {}
    for b in range(B):
        col = 1 + b                                                   # ")" right after BOS, or after a few tokens at depth 0
        while Y.state(cls, rows[b * n, 1:col])[0] != 0:
            col += 1
        hyp[b, 0, col] = CLOSE_ID
        where[b] = col - 1                                            # position col - 1 predicts column col
    bad = g.logq(s, hyp, syntax=syn)
    lq, fo = bad.logq.cpu().numpy(), bad.first_outside.cpu().numpy()
    for b in range(B):
        assert lq[b, 0] == -np.inf and fo[b, 0] == where[b], f"source {b}: logq {lq[b, 0]}, first_outside {fo[b, 0]}, the unmatched ) is at {where[b]}"
        assert np.isfinite(lq[b, 1:]).all() and (fo[b, 1:] == -1).all()
    assert bool(torch.isfinite(g.logq(s, hyp).logq).all()), "without the constraint the same rows are inside the support"
    # the speculative sampler and the pool score under the call's table
    p2, q2 = spec(tta, native, c_token, num_samples=n).generate(s, syntax=syn, return_logq=True)
    assert torch.equal(p2, pred) and torch.equal(q2.logq, q.logq)
    res = spec(tta, native, c_token, num_samples=n).generate_many([s[:2], s[2:]], syntax=syn, return_logq=True)
    assert torch.equal(torch.cat([r[0] for r in res]), pred) and torch.equal(torch.cat([r[1].logq for r in res]), q.logq)
    # the stage alone on the caller's logits (the oracle's, rounded to fp32): the replayed sums again, the logits not written
    logits = torch.from_numpy(lg.astype(np.float32)).cuda().reshape(B, n, MAX_LEN - 1, -1).contiguous()
    keep = logits.clone()
    stage = native.hypothesis_logq(logits, pred, PAD, EOS, temperature=T, syntax=syn, syntax_max_len=MAX_LEN)
    assert torch.equal(logits, keep) and bool((stage.first_outside == -1).all())
    assert (np.abs(stage.logq.cpu().numpy().reshape(-1).astype(np.float64) - sums) <= bound * length).all()


# -- 8: surface ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(tta, model, src, syn, c_token):
    native = model[0]
    s, V = src[:4].cuda(), native.tgt_vocab_size
    kw = dict(pad_token=PAD, bos_token=BOS, eos_token=EOS)
    others = [tta.TranslationInferenceGreedy(native, MAX_LEN, **kw),
              tta.TranslationInferenceGreedySpeculative(native, MAX_LEN, 4, 3, replace_token=c_token, **kw),
              tta.TranslationInferenceBeamSearch(native, 3, MAX_LEN, **kw),
              tta.TranslationInferenceBeamSearchSpeculative(native, MAX_LEN, 3, 4, 3, V, False, PAD, BOS, EOS, c_token),
              tta.TranslationInferenceStochasticBeamSearch(native, 3, MAX_LEN, PAD, BOS, EOS, seed=1)]
    for g in others:
        with pytest.raises(ValueError, match="takes no syntax"):
            g.generate(s, syntax=syn)
        out = g.generate(s)
        assert out.shape[0] == 4                                             # and the call without the keyword is what it was
        q = g.logq(s, out, syntax=syn)                                       # log q under the constraint is every generator's
        assert q.logq.shape == out.shape[:2]
    for g in (others[1], others[3], others[4]):
        with pytest.raises(ValueError, match="takes no syntax"):
            g.generate_many([s], syntax=syn)
    for g in (plain(tta, native), spec(tta, native, c_token)):
        for bad in (syn.cls[:V - 1], syn.cls.long(), torch.zeros(2, V, dtype=torch.int8)):
            with pytest.raises(ValueError):
                g.generate(s, syntax=bad)
        with pytest.raises(ValueError):
            g.logq(s, g.generate(s), syntax=syn.cls[:V - 1])
    # the entry point: a max_len that is neither 0 nor the call's is refused before anything is launched
    import ctypes as C
    from translation_transformer_amd import _native as N
    out = torch.full((4, 1, MAX_LEN), -7, dtype=torch.int64, device="cuda")
    p = N.SampleParams(MAX_LEN, 1, T, 0, 1.0, PAD, BOS, EOS, 1)
    d_cls = syn.cls.cuda()
    for bad_len in (MAX_LEN - 1, MAX_LEN + 1):
        rc = native._lib.ttx_sample_generate_syntax(native.session, s.data_ptr(), 4, s.shape[1], None, C.byref(p), None,
                                                    C.byref(N.Syntax(d_cls.data_ptr(), bad_len)), out.data_ptr(), C.byref(N.GenStats()),
                                                    native._stream())
        torch.cuda.synchronize()
        assert rc == N.TTX_ERR_INVALID and bool((out == -7).all())
    # max_len 0 is the call's; a null table is the unconstrained call
    for syntax_arg, want in ((N.Syntax(d_cls.data_ptr(), 0), plain(tta, native, seed=1).generate(s, syntax=syn)),
                             (N.Syntax(None, 0), plain(tta, native, seed=1).generate(s))):
        rc = native._lib.ttx_sample_generate_syntax(native.session, s.data_ptr(), 4, s.shape[1], None, C.byref(p), None, C.byref(syntax_arg),
                                                    out.data_ptr(), C.byref(N.GenStats()), native._stream())
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(out, want)


@pytest.mark.parametrize("generation", ["sampling", "sampling_speculative"])
def test_lightning_passes_the_switch_through(tta, src, syn, tmp_path, generation, monkeypatch):
    from test_gpu_lightning_surface import FixtureTokenizer
    st, cfg = tiny_state()
    tkz = FixtureTokenizer()
    cls = syn.cls.numpy()
    s, tgt = src[:4], fixture_tokens()[1][:4]

    def module(gen=generation):
        mod = tta.VanillaEncoderDecoderTransformerLightning(
            src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
            num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"], num_heads=cfg["num_heads"],
            share_embeddings=True, generation=gen, beam_size=3, max_len=MAX_LEN, n_drafts=3, draft_len=4, sampling_temperature=T,
            sampling_seed=11, report_prediction_file=str(tmp_path / "r.txt"))
        mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
        return mod

    batches = lambda bs: [{"src_tokens": s[i:i + bs].cuda(), "tgt_tokens": tgt[i:i + bs].cuda()} for i in range(0, 4, bs)]
    preds = {}
    for bs in (1, 4):
        mod = module()
        mod.predict_syntax_constraint = True
        preds[bs] = torch.cat(tta.run_predict(mod, batches(bs)), 0).cpu()
    assert preds[1].shape == (4, 3, MAX_LEN) and torch.equal(preds[1], preds[4])
    assert not bad_rows(preds[4], cls), f"{generation}: the switch did not reach the generator"
    free = torch.cat(tta.run_predict(module(), batches(4)), 0).cpu()
    assert bad_rows(free, cls), "the unconstrained module balances every row: the check shows nothing"
    with monkeypatch.context() as mp:                                        # the environment switch, and log q under the table
        mp.setenv("TTX_PREDICT_SYNTAX", "1")
        mod = module()
        mod.predict_with_logq = True
        assert torch.equal(torch.cat(tta.run_predict(mod, batches(4)), 0).cpu(), preds[4])
        assert all(bool((q.first_outside == -1).all()) for q in mod.predict_logq.values())
    if generation == "sampling_speculative":                                 # decoded ahead from the slot pool: the same rows
        mod = module()
        mod.predict_syntax_constraint = mod.predict_sample_pool = True
        assert torch.equal(torch.cat(tta.run_predict(mod, batches(1)), 0).cpu(), preds[4])
    mod = module("greedy")
    mod.predict_syntax_constraint = True
    with pytest.raises(ValueError, match="predict_syntax_constraint"):
        tta.run_predict(mod, batches(4))
