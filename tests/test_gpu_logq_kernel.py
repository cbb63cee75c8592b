"""k_hyp_logq (csrc/ttx_logq.hip.h) through ttx_hypothesis_logq on logits the test builds, against the kernels it must agree with on
the bits (k_hyp_score, k_argmax's rule, k_nucleus, k_sample) and the float64 restatement of tests/util_logq_checks.py
(tests/test_logq_checks_host.py shows that its checker can fail).

The bound of the value check, derived from the arithmetic (eps = 2^-23, one fp32 ulp relative; a rounding is eps / 2; expf, logf
and log1pf within 1 ulp, the bound tests/util_beam_checks.py uses; the restatement forms the same fp32 product y = x * inv_T, so
the product itself contributes nothing):
  filter on    tok = (y_t - m) - logf(S), S the Hillis-Steele sum of <= 32 terms e_r = expf(y_r - m), D = max_r (m - y_r):
               y_t - m: d_t eps/2;  S relative: 6 additions 3 eps + expf 1 eps + its argument's rounding D eps/2;  logf: 1 ulp of
               |log S| <= log 32;  the last subtraction (d_t + log 32) eps/2.   Sum <= eps * (9.2 + 1.5 D).
  filter off   tok = -(log1pf(rs) + (m - y_t)); an element reaches lane 0's sum through at most 16 + 6 steps, each an addition
               (eps/2) or a rescaling by an expf factor (1 eps, the product eps/2): 44 eps relative on 1 + rs; the arguments'
               roundings weigh in by sum_v p_v d_v eps/2 <= log V eps/2;  log1pf 1 ulp of log(1 + rs) <= log V;  m - y_t:
               d_t eps/2;  the sum (log V + d_t) eps/2.   Sum <= eps * (44 + 2 log V + d_t).
"""
import math

import numpy as np
import pytest
import torch

import util_logq_checks as Q
import util_sample_checks as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD, BOS, EOS = 0, 1, 2
EPS = 2.0 ** -23
SHAPES = [(V, W) for V in (7, 64, 256, 1000) for W in (2, 65, 66)]


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def lane_heads(V: int) -> np.ndarray:
    """The columns that are the FIRST element of a lane in k_hyp_score's pass (V % 4 == 0: 4 * lane, else lane): met_push forms
    exp(-inf + inf) = NaN when one of them holds -inf, so the scoring stage gives a number only where all of them are finite."""
    heads = 4 * np.arange(64) if V % 4 == 0 else np.arange(64)
    return heads[heads < V]


def make_case(V: int, W: int, seed: int, holes: str = "random"):
    """(logits fp32 [6, W-1, V], hyp int64 [6, W]).  Rows: EOS at column 1; all PAD; no EOS; a PAD before the EOS; a token id
    outside [0, V); EOS in the last column.  ``holes``: "random": about a tenth of the logits -inf (never the whole row of a
    position); "off_heads": the same, but never in a lane-head column (``lane_heads``); "none": no -inf.  At every third position
    two equal values straddle rank k - 1 | k for k = min(8, V - 1), and the rows' tokens come from the first ranks."""
    rng = np.random.default_rng(seed)
    T = W - 1
    x = (2.0 * rng.standard_normal((6, T, V))).astype(np.float32)
    hole = rng.random(x.shape) < 0.1
    hole[np.arange(6)[:, None], np.arange(T)[None, :], rng.integers(0, V, (6, T))] = False
    if holes == "off_heads":
        hole[:, :, lane_heads(V)] = False
    elif holes == "none":
        hole[:] = False
    else:
        assert holes == "random"
    x[hole] = -np.inf
    k = min(8, V - 1)
    h = np.full((6, W), PAD, dtype=np.int64)
    h[:, 0] = BOS
    for r in range(6):
        for p in range(T):
            order = S.rank_order(x[r, p].astype(np.float64))
            if p % 3 == 0 and np.isfinite(x[r, p, order[k]]):
                x[r, p, order[k]] = x[r, p, order[k - 1]]              # exact tie across the top_k edge
                order = S.rank_order(x[r, p].astype(np.float64))
            t = int(order[(p * 5 + r - 2) % min(V, 11)])                   # ranks 0..10: inside and outside every filter of the tests
            h[r, p + 1] = t if t not in (PAD, EOS) else int(order[0]) if int(order[0]) not in (PAD, EOS) else 3
    h[0, 1:] = PAD
    h[0, 1] = EOS
    h[1, 1:] = PAD
    if W > 4:
        h[3, W // 2] = PAD
        h[3, W - 2] = EOS
        h[3, W - 1] = PAD
        h[4, 2] = V + 3
        h[4, 3] = -1
    else:
        h[4, 1] = V + 3
    h[5, W - 1] = EOS
    return x, h


def run(native, x, h, forced=None, **dist):
    """One ttx_hypothesis_logq call on device copies; ``x`` may be a device tensor (read in place)."""
    xd = x if torch.is_tensor(x) else torch.from_numpy(x).to(DEV)
    out = native.hypothesis_logq(xd, torch.from_numpy(h).to(DEV), PAD, EOS, forced_len=forced, check_ids=False, **dist)
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b) -> bool:
    return all(torch.equal(bits(u), bits(v)) for u, v in zip(a[:7], b[:7]))


def logprobs_raw(native, x, h):
    """ttx_hypothesis_logprobs at the C boundary (the Python wrapper refuses the row with ids outside [0, V))."""
    xd, hd = torch.from_numpy(x).to(DEV), torch.from_numpy(h).to(DEV)
    R, W = h.shape
    tok = torch.empty((R, W - 1), dtype=torch.float32, device=DEV)
    score = torch.empty(R, dtype=torch.float32, device=DEV)
    length = torch.empty(R, dtype=torch.int32, device=DEV)
    fin = torch.empty(R, dtype=torch.bool, device=DEV)
    N = __import__("translation_transformer_amd")._native
    N.check(native._lib.ttx_hypothesis_logprobs(native._scoring_session(), xd.data_ptr(), hd.data_ptr(), R, W, x.shape[-1], PAD, EOS,
                                                tok.data_ptr(), score.data_ptr(), length.data_ptr(), fin.data_ptr(), native._stream()))
    torch.cuda.synchronize()
    return tok, score, length, fin


def token_at(h, r, p, V):
    t = int(h[r, p + 1])
    return t if 0 <= t < V else 0


def seq_sum(vals) -> float:
    acc = 0.0
    for v in vals:
        acc += float(v)
    return acc


def check_row_sums(out, h):
    """logq is the position-order double sum rounded once, first_outside the first -inf, positions >= n hold 0 / -1 / 0."""
    tok = out.token_logq.cpu().numpy()
    for r in range(h.shape[0]):
        n, fin = Q.length_rule(h[r], PAD, EOS)
        assert int(out.length[r]) == n and bool(out.finished[r]) == fin
        want = np.float32(seq_sum(tok[r, :n]))
        got = out.logq[r].cpu().numpy()
        assert got == want or (np.isnan(got) and np.isnan(want)), (r, got, want)
        neg = [p for p in range(n) if tok[r, p] == -np.inf]
        assert int(out.first_outside[r]) == (neg[0] if neg else -1)
        assert (tok[r, n:] == 0).all() and (np.signbit(tok[r, n:]) == 0).all()
        assert (out.rank[r, n:] == -1).all() and (out.n_kept[r, n:] == 0).all()


@pytest.mark.parametrize("holes", ["none", "off_heads", "random"])
@pytest.mark.parametrize("V,W", SHAPES)
def test_model_distribution_is_the_scoring_stage(native, V, W, holes):
    """T = 1 without a filter: tok_logq, logq, length and finished are ttx_hypothesis_logprobs' on the bits.  Without -inf logits
    and with -inf away from the lane-head columns k_hyp_score gives a number at EVERY live position, and every one is compared;
    with -inf anywhere it gives NaN at most positions of the wide vocabularies (met_push on a lane that starts with -inf), and
    the bits match wherever it gives a number."""
    x, h = make_case(V, W, 100 * V + W, holes)
    out = run(native, x, h)
    tok, score, length, fin = logprobs_raw(native, x, h)
    assert torch.equal(out.length, length) and torch.equal(out.finished, fin)
    n_live = sum(Q.length_rule(h[r], PAD, EOS)[0] for r in range(6))
    live = (torch.arange(W - 1, device=DEV)[None, :] < length[:, None])
    assert int(live.sum()) == n_live and n_live >= 5
    assert not torch.isnan(out.token_logq).any() and not torch.isnan(out.logq).any()
    num = ~torch.isnan(tok)
    if holes != "random":
        assert num.all() and not torch.isnan(score).any()                   # every live position of every row is compared
        assert torch.equal(bits(out.token_logq), bits(tok)) and torch.equal(bits(out.logq), bits(score))
        if holes == "off_heads" and V > 64:
            assert np.isinf(x).sum() > 100                                   # the -inf logits are there, away from the lane heads
    else:
        compared = int((num & live).sum())
        print(f"V {V} W {W}: the scoring stage gives a number at {compared} of {n_live} live positions")
        assert torch.equal(bits(out.token_logq)[num], bits(tok)[num])
        rows = ~torch.isnan(score)
        assert torch.equal(bits(out.logq)[rows], bits(score)[rows])
    assert (out.n_kept[out.rank >= 0] == V).all()
    check_row_sums(out, h)


@pytest.mark.parametrize("V,W", SHAPES)
def test_greedy_and_top_k_1_are_the_first_maximum(native, V, W):
    x, h = make_case(V, W, 200 * V + W)
    for dist, T in ((dict(temperature=0.0), 1.0), (dict(temperature=0.7, top_k=1), 0.7), (dict(temperature=0.0, top_k=5, top_p=0.5), 1.0)):
        out = run(native, x, h, **dist)
        tok = out.token_logq.cpu().numpy()
        hit = 0
        for r in range(6):
            n, _ = Q.length_rule(h[r], PAD, EOS)
            for p in range(n):
                first = S.argmax_first(S.scaled(x[r, p], T) if T != 1.0 else x[r, p].astype(np.float64))
                want = 0.0 if token_at(h, r, p, V) == first else -np.inf
                assert tok[r, p] == want and (want != 0.0 or not np.signbit(tok[r, p])), (dist, r, p)
                hit += want == 0.0
                assert int(out.n_kept[r, p]) == 1 and (int(out.rank[r, p]) == 0) == (want == 0.0)
        assert hit > 0
        lq = out.logq.cpu().numpy()
        assert np.isin(lq, [0.0, -np.inf]).all()
        check_row_sums(out, h)


@pytest.mark.parametrize("top_k", [1, 8, 32])
@pytest.mark.parametrize("top_p", [0.5, 0.9, 1.0])
@pytest.mark.parametrize("V,W", [(7, 66), (64, 65), (256, 66), (1000, 65)])
def test_support_is_the_nucleus_mask(native, V, W, top_k, top_p):
    x, h = make_case(V, W, 300 * V + W)
    out = run(native, x, h, temperature=1.0, top_k=top_k, top_p=top_p)
    FILL = 12345.0
    masked = native.nucleus_mask(torch.from_numpy(x).to(DEV), top_p, top_k, FILL).cpu().numpy()
    kept = masked != FILL
    tok, nk, rank = out.token_logq.cpu().numpy(), out.n_kept.cpu().numpy(), out.rank.cpu().numpy()
    seen = set()
    for r in range(6):
        n, _ = Q.length_rule(h[r], PAD, EOS)
        for p in range(n):
            t = token_at(h, r, p, V)
            assert nk[r, p] == kept[r, p].sum(), (r, p)
            assert (tok[r, p] > -np.inf) == bool(kept[r, p, t]), (r, p)
            assert (rank[r, p] < nk[r, p]) == bool(kept[r, p, t]), (r, p)      # kept iff rank < n_kept: ties by the lower id
            seen.add(bool(kept[r, p, t]))
    assert True in seen and (top_k != 1 or False in seen)
    check_row_sums(out, h)


@pytest.mark.parametrize("V,W", SHAPES)
def test_rank_is_the_count(native, V, W):
    x, h = make_case(V, W, 400 * V + W)
    for dist in (dict(temperature=0.5), dict(temperature=2.0, top_k=8, top_p=0.9), dict(temperature=0.0)):
        out = run(native, x, h, **dist)
        rank = out.rank.cpu().numpy()
        for r in range(6):
            n, _ = Q.length_rule(h[r], PAD, EOS)
            for p in range(n):
                y = S.scaled(x[r, p], dist["temperature"]) if dist["temperature"] else x[r, p].astype(np.float64)
                assert rank[r, p] == Q.rank_of(y, token_at(h, r, p, V)), (dist, r, p)


@pytest.mark.parametrize("V,W", [(7, 65), (64, 66), (1000, 66)])
def test_forced_positions(native, V, W):
    x, h = make_case(V, W, 500 * V + W)
    dist = dict(temperature=0.7, top_k=2)                               # most tokens of the rows are outside this support
    free = run(native, x, h, **dist)
    forced = np.array([1, 3, 5, 100, -4, W - 1], dtype=np.int32)
    out = run(native, x, h, forced=torch.from_numpy(forced).to(DEV), **dist)
    poisoned = x.copy()
    for r in range(6):
        n, _ = Q.length_rule(h[r], PAD, EOS)
        poisoned[r, :min(max(int(forced[r]), 0), n)] = np.nan           # the logits of a forced position are not read
    again = run(native, poisoned, h, forced=torch.from_numpy(forced).to(DEV), **dist)
    assert same(out, again)
    tok, ftok = out.token_logq.cpu().numpy(), free.token_logq.cpu().numpy()
    assert (ftok == -np.inf).any()
    for r in range(6):
        n, _ = Q.length_rule(h[r], PAD, EOS)
        f = min(max(int(forced[r]), 0), n)
        assert (tok[r, :f] == 0).all() and not np.signbit(tok[r, :f]).any()
        assert (out.rank[r, :f] == -1).all() and (out.n_kept[r, :f] == 0).all()
        assert np.array_equal(tok[r, f:].view(np.int32), ftok[r, f:].view(np.int32))
        assert torch.equal(out.rank[r, f:], free.rank[r, f:]) and torch.equal(out.n_kept[r, f:], free.n_kept[r, f:])
        assert int(out.first_outside[r]) == next((p for p in range(f, n) if ftok[r, p] == -np.inf), -1)
    check_row_sums(out, h)
    assert torch.equal(out.length, free.length) and torch.equal(out.finished, free.finished)


@pytest.mark.parametrize("V,W", SHAPES)
def test_bit_identical_across_calls_rows_and_alignment(native, V, W):
    x, h = make_case(V, W, 600 * V + W)
    flat = torch.empty(x.size + 8, dtype=torch.float32, device=DEV)
    for dist in (dict(temperature=1.0), dict(temperature=0.5), dict(temperature=0.0), dict(temperature=2.0, top_k=32, top_p=0.9975),
                 dict(temperature=0.7, top_k=8)):
        a = run(native, x, h, **dist)
        run(native, x[:2], h[:2], temperature=1.3, top_k=3)                # another shape and distribution in between
        b = run(native, x, h, **dist)
        assert same(a, b), dist
        for r in (0, 3, 5):
            one = run(native, x[r:r + 1], h[r:r + 1], **dist)
            assert all(torch.equal(bits(u), bits(v[r:r + 1])) for u, v in zip(one[:7], a[:7])), (dist, r)
        for off in (1, 2, 4):                                               # bases 4, 8 and 16 bytes off the allocation's
            shifted = flat[off:off + x.size].view(x.shape)
            shifted.copy_(torch.from_numpy(x))
            assert (shifted.data_ptr() % 16 == 0) == (off == 4)
            assert same(a, run(native, shifted, h, **dist)), (dist, off)


def test_agrees_with_the_sampler_on_one_row(native):
    """4 096 keyed draws of k_sample per logits row: no drawn token is outside the support, and the counts pass the chi-square
    against exp(tok_logq) at the level tests/test_gpu_sample_kernel.py holds its frequency check to (p > 1e-6)."""
    V, n = 64, 4096
    dist = dict(temperature=0.7, top_k=8, top_p=0.9)
    rng = np.random.default_rng(11)
    flat = (0.5 * rng.standard_normal(V)).astype(np.float32)              # near flat: all 8 ranks kept
    prob = np.full(V, 0.05 / 60)
    prob[[9, 40, 3, 22]] = [0.4, 0.3, 0.15, 0.1]                           # the mass above rank 4 is 0.95: 4 ranks kept
    peaked = (0.7 * np.log(prob)).astype(np.float32)
    for row, want_kept in ((flat, 8), (peaked, 4)):
        logits = torch.from_numpy(np.tile(row, (n, 1))).to(DEV)
        key = torch.arange(n, dtype=torch.int64, device=DEV)
        zeros = torch.zeros(n, dtype=torch.int32, device=DEV)
        pred = torch.empty(n, dtype=torch.int32, device=DEV)
        native.debug_sample(logits, key, zeros.clone(), zeros.clone(), torch.zeros(1, dtype=torch.int32, device=DEV), pred, n,
                            pad=-1, eos=-1, seed=20260101, **dist)
        drawn = pred.cpu().numpy()
        # every token of the vocabulary as a one-position hypothesis under the same logits row
        h = np.stack([np.full(V, BOS), np.arange(V)], axis=1).astype(np.int64)
        out = native.hypothesis_logq(torch.from_numpy(np.tile(row, (V, 1, 1))).to(DEV), torch.from_numpy(h).to(DEV), -1, -1,
                                     check_ids=False, **dist)
        tok = out.token_logq[:, 0].cpu().numpy().astype(np.float64)
        assert (out.length == 1).all() and (out.n_kept == want_kept).all()
        q = np.exp(tok)
        assert abs(q.sum() - 1.0) < 1e-5 and int((q > 0).sum()) == want_kept
        assert (tok[drawn] > -np.inf).all(), "the sampler drew a token the stage puts outside the support"
        count = np.bincount(drawn, minlength=V).astype(np.float64)
        live = q > 0
        chi2 = float(((count[live] - n * q[live]) ** 2 / (n * q[live])).sum())
        pval = S.chi2_sf(chi2, want_kept - 1)
        print(f"kept {want_kept}: chi-square {chi2:.3f}, p {pval:.3g}; smallest expected count {n * q[live].min():.1f}")
        assert pval > 1e-6


@pytest.mark.parametrize("V,W", SHAPES)
def test_values_against_float64(native, V, W):
    x, h = make_case(V, W, 700 * V + W)
    worst = {}
    for dist in (dict(temperature=0.5), dict(temperature=2.0), dict(temperature=1.0, top_k=8), dict(temperature=0.5, top_k=32, top_p=0.9975),
                 dict(temperature=2.0, top_k=8, top_p=0.9)):
        p = S.Params(pad=PAD, eos=EOS, **dist)
        out = run(native, x, h, **dist)
        tok, nk = out.token_logq.cpu().numpy().astype(np.float64), out.n_kept.cpu().numpy()
        for r in range(6):
            ref = Q.row_logq(x[r], h[r], p, n_kept=nk[r])                 # the kernel's own kept-set sizes
            for pos in range(ref.length):
                y = S.scaled(x[r, pos], p.temperature)
                t = token_at(h, r, pos, V)
                if ref.tok[pos] == -np.inf:
                    assert tok[r, pos] == -np.inf, (dist, r, pos)
                    continue
                d_t = y.max() - y[t]
                if p.filtered:
                    kept = S.rank_order(y)[:nk[r, pos]]
                    bound = EPS * (9.2 + 1.5 * (y.max() - y[kept].min()))
                else:
                    bound = EPS * (44 + 2 * math.log(V) + d_t)
                err = abs(tok[r, pos] - ref.tok[pos])
                key = "filtered" if p.filtered else "unfiltered"
                worst[key] = max(worst.get(key, 0.0), err / bound)
                assert err <= bound, (dist, r, pos, err, bound)
    print(f"V {V} W {W}: largest error over its bound {worst}")
