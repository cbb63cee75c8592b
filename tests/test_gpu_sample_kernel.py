"""k_sample (csrc/ttx_sample.hip.h) one launch at a time through ttx_debug_sample, on operands the test builds, against the float64
restatement of tests/util_sample_checks.py (tests/test_sample_checks_host.py shows that its checker can fail).

Every live row's token must be ``consistent``: kept, and its uniform inside the token's interval of the float64 CDF taken in the
kernel's order, widened by tol = 1e-4 on either side.  Where the bound comes from: the kernel's CDF is a running fp32 sum of
V <= 1024 non-negative terms, whose rounding is at most V * 2^-24 = 6.1e-5 relative to the total, plus a few ulp of expf per term;
and it scales y = x * inv_T in fp32 where a float64 restatement may not, 3 ulp of y (about 2e-6 at |y| <= 16).  1e-4 covers both.
Beside that, exact checks: temperature 0 and top_k = 1 against k_argmax, done rows, the done flags, rows beyond the live count,
guard margins, the same row at several launch positions, two launches, the Philox words, and one chi-square frequency check.
"""
import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_sample_checks as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
PAD, EOS = 0, 2
FILTERS = [dict(), dict(top_k=1), dict(top_k=2), dict(top_k=32), dict(top_p=0.5), dict(top_p=0.9975)]
TEMPS = [0.5, 1.0, 3.0]


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def make_logits(m: int, V: int, seed: int) -> np.ndarray:
    """N(0, 2^2) rows with about a tenth of the columns -inf, never a whole row."""
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((m, V))).astype(np.float32)
    if V > 1:
        hole = rng.random((m, V)) < 0.1
        hole[np.arange(m), rng.integers(0, V, m)] = False
        x[hole] = -np.inf
    return x


class Operands:
    """The device operands of one launch, every one between guard margins."""

    def __init__(self, x: np.ndarray, seed: int, front: int = 6, done=None):
        m, V = x.shape
        rng = np.random.default_rng(seed)
        self.x, self.m, self.V = x, m, V
        self.key_np = rng.integers(-2 ** 63, 2 ** 63, m, dtype=np.int64)
        self.smp_np = rng.integers(-2 ** 31, 2 ** 31, m, dtype=np.int64).astype(np.int32)
        self.front_np = front
        self.logits = U.Buf((m, V), torch.float32, DEV, x)
        self.key = U.Buf((m,), torch.int64, DEV, self.key_np)
        self.smp = U.Buf((m,), torch.int32, DEV, self.smp_np)
        self.front = U.Buf((1,), torch.int32, DEV, [front])
        self.done_np = np.zeros(m, dtype=np.int32) if done is None else np.asarray(done, dtype=np.int32)
        self.done = U.Buf((m,), torch.int32, DEV, self.done_np)
        self.pred = U.Buf((m,), torch.int32, DEV)

    def launch(self, native, live=None, seed=0, pad=PAD, eos=EOS, **kw):
        self.pred.reset()
        self.done.reset()
        self.done.set(self.done_np)
        m_live = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
        native.debug_sample(self.logits.v, self.key.v, self.smp.v, self.done.v, self.front.v, self.pred.v, self.m, m_live,
                            pad=pad, eos=eos, seed=seed, **kw)
        torch.cuda.synchronize()
        for b in (self.logits, self.key, self.smp, self.front, self.done, self.pred):
            assert b.margins() is None, b.margins()
        return self.pred.get(), self.done.get()

    def u(self, seed=0) -> np.ndarray:
        return S.uniform(seed, self.key_np, self.smp_np, self.front_np + 1)


def check_rows(ops: Operands, tok, done, p: S.Params, seed: int, what: str, live=None):
    live = ops.m if live is None else live
    u = ops.u(seed)
    worst = 0.0
    for r in range(live):
        if ops.done_np[r]:
            assert tok[r] == p.pad and done[r] == ops.done_np[r], f"{what}: done row {r} gave {tok[r]}, done {done[r]}"
            continue
        ex = S.excess(int(tok[r]), ops.x[r], u[r], p, TOL)
        worst = max(worst, ex)
        assert ex <= TOL, f"{what}: row {r} token {tok[r]} u {u[r]!r} lies {ex:.3e} outside its interval"
        assert done[r] == int(tok[r] in (p.eos, p.pad)), f"{what}: row {r} token {tok[r]} done {done[r]}"
    assert (tok[live:] == U.SENTINEL[torch.int32]).all(), f"{what}: a row at or beyond the live count was written"
    return worst


@pytest.mark.parametrize("m_max", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 255, 256, 1023, 1024])
def test_every_row_is_consistent(native, V, m_max):
    ops = Operands(make_logits(m_max, V, seed=V * 1000 + m_max), seed=V + 7 * m_max)
    worst = 0.0
    for T in TEMPS:
        for f in FILTERS:
            seed = 0x9E3779B97F4A7C15 ^ (int(T * 8) << 40) ^ len(f)
            tok, done = ops.launch(native, seed=seed, temperature=T, **f)
            worst = max(worst, check_rows(ops, tok, done, S.Params(T, pad=PAD, eos=EOS, **f), seed, f"V {V} m {m_max} T {T} {f}"))
    print(f"V {V} m_max {m_max}: largest excess over the exact interval {worst:.3e}")


def planted(m: int, V: int, seed: int) -> np.ndarray:
    """Rows for the argmax comparison: random, the maximum twice in neighbouring columns, twice 64 columns apart, -0.0 before 0.0."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, V)).astype(np.float32)
    for r in range(m):
        c = int(rng.integers(0, V))
        if r % 4 == 1 and V >= 2:
            c = min(c, V - 2)
            x[r, [c, c + 1]] = 7.5
        elif r % 4 == 2 and V > 64:
            c = int(rng.integers(0, V - 64))
            x[r, [c, c + 64]] = 7.5
        elif r % 4 == 3 and V >= 2:
            x[r] = -np.abs(x[r]) - 1.0
            c = min(c, V - 2)
            x[r, c], x[r, c + 1] = -0.0, 0.0
    return x


@pytest.mark.parametrize("m_max", [5, 257])
@pytest.mark.parametrize("V", [1, 5, 65, 256, 1024])
def test_greedy_settings_equal_k_argmax(native, V, m_max):
    x = planted(m_max, V, seed=V + m_max)
    want = U.Buf((m_max,), torch.int32, DEV)
    settings = [dict(temperature=0.0), dict(temperature=0.0, top_k=5, top_p=0.3), dict(temperature=1.0, top_k=1),
                dict(temperature=0.5, top_k=1), dict(temperature=1.0, top_k=1, top_p=0.2)]
    for weird in (False, True):
        if weird:                                   # temperature 0 takes k_argmax's rule for rows outside the contract too
            x = x.copy()
            x[0] = -np.inf
            x[m_max - 1] = np.nan
            settings = settings[:2]
        ops = Operands(x, seed=3)
        native.debug_argmax(ops.logits.v, want.v, m_max)
        torch.cuda.synchronize()
        for kw in settings:
            tok, done = ops.launch(native, seed=11, pad=-1, eos=-2, **kw)
            d = U.first_difference(tok, want.get())
            assert d is None, f"V {V} m {m_max} {kw}: {d}"
            assert (done == 0).all()


def test_done_rows_give_pad_and_their_logits_are_not_read(native):
    m, V = 70, 65
    x = make_logits(m, V, seed=5)
    done = (np.arange(m) % 3 == 1).astype(np.int32)
    x[done != 0] = np.nan
    ops = Operands(x, seed=6, done=done)
    for kw in (dict(temperature=1.0), dict(temperature=0.0), dict(temperature=3.0, top_k=4), dict(temperature=1.0, top_p=0.9)):
        for pad in (0, 4):
            tok, dn = ops.launch(native, seed=2, pad=pad, eos=EOS, **kw)
            check_rows(ops, tok, dn, S.Params(kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), pad=pad, eos=EOS), 2,
                       f"{kw} pad {pad}")
            assert (tok[done != 0] == pad).all() and (dn[done != 0] == 1).all()


def test_eos_and_pad_set_done_and_nothing_else_does(native):
    m, V = 257, 5                                   # every token of a small vocabulary comes up
    ops = Operands(make_logits(m, V, seed=8), seed=9)
    for eos, pad in ((2, 0), (4, 1), (3, 3)):
        tok, dn = ops.launch(native, seed=5, pad=pad, eos=eos, temperature=3.0)
        assert set(tok.tolist()) >= {eos, pad} and len(set(tok.tolist())) >= 4
        assert (dn == ((tok == eos) | (tok == pad)).astype(np.int32)).all()


@pytest.mark.parametrize("live", [0, 1, 100, 256, 257])
def test_rows_beyond_the_live_count_keep_their_sentinel(native, live):
    m, V = 257, 63
    ops = Operands(make_logits(m, V, seed=21), seed=22)
    sent = U.SENTINEL[torch.int32]
    ops.done_np = np.where(np.arange(m) < live, 0, sent).astype(np.int32)       # the flags beyond the live count: sentinels too
    for kw in (dict(temperature=1.0), dict(temperature=1.0, top_k=3)):
        tok, dn = ops.launch(native, live=live, seed=4, **kw)
        check_rows(ops, tok, dn, S.Params(1.0, kw.get("top_k", 0), pad=PAD, eos=EOS), 4, f"live {live} {kw}", live=live)
        assert (dn[live:] == sent).all(), "a done flag at or beyond the live count was written"


@pytest.mark.parametrize("V", [5, 65, 1024])
def test_a_row_gives_the_same_token_wherever_it_sits(native, V):
    m = 257
    x = make_logits(m, V, seed=V)
    x[3], x[256] = x[0], x[0]
    ops = Operands(x, seed=V + 1)
    for a in (ops.key_np, ops.smp_np):
        a[3], a[256] = a[0], a[0]
    ops.key.set(ops.key_np)
    ops.smp.set(ops.smp_np)
    seen = set()
    for T in TEMPS:
        for f in FILTERS:
            for seed in (1, 2, 3):
                tok, _ = ops.launch(native, seed=seed, pad=-1, eos=-2, temperature=T, **f)
                assert tok[0] == tok[3] == tok[256], f"V {V} T {T} {f} seed {seed}: {tok[0]}, {tok[3]}, {tok[256]}"
                seen.add(int(tok[0]))
                tok2, _ = ops.launch(native, seed=seed, pad=-1, eos=-2, temperature=T, **f)
                assert (tok == tok2).all(), "two launches differ"
    assert len(seen) > 1


def test_the_uniform_is_the_philox_word(native):
    """A two-token row with equal logits gives token 1 iff u >= 0.5: changing seed, key, sample or front[0] changes the token as
    the NumPy Philox says."""
    m = 257
    x = np.zeros((m, 2), dtype=np.float32)
    ops = Operands(x, seed=33, front=0)
    base = None
    for seed, front in ((0, 0), (1, 0), (0xFFFFFFFFFFFFFFFF, 0), (0x0123456789ABCDEF, 0), (1 << 32, 0), (1, 1), (1, 149), (1, 4999)):
        ops.front_np = front
        ops.front.set([front])
        want = (ops.u(seed) >= 0.5).astype(np.int32)
        for f in (dict(), dict(top_k=2)):
            tok, _ = ops.launch(native, seed=seed, pad=-1, eos=-2, temperature=1.0, **f)
            d = U.first_difference(tok, want)
            assert d is None, f"seed {seed:#x} front {front} {f}: {d}"
        assert base is None or (want != base).any()
        base = want if base is None else base
    # key and sample: swap their words between two rows and only those rows change as predicted
    ops.key_np[:] = np.arange(m) << 32                                       # the high word alone
    ops.smp_np[:] = 0
    ops.key.set(ops.key_np)
    ops.smp.set(ops.smp_np)
    tok_hi, _ = ops.launch(native, seed=1, pad=-1, eos=-2, temperature=1.0)
    assert U.first_difference(tok_hi, (ops.u(1) >= 0.5).astype(np.int32)) is None
    ops.key_np[:] = 0
    ops.smp_np[:] = np.arange(m)
    ops.key.set(ops.key_np)
    ops.smp.set(ops.smp_np)
    tok_s, _ = ops.launch(native, seed=1, pad=-1, eos=-2, temperature=1.0)
    assert U.first_difference(tok_s, (ops.u(1) >= 0.5).astype(np.int32)) is None
    assert (tok_hi != tok_s).any() and 0 < tok_s.sum() < m


def test_frequencies_follow_the_distribution(native):
    """20 000 draws of one row against its float64 probabilities: Pearson chi-square below the 1 - 1e-6 quantile for 11 degrees of
    freedom.  A fixed seed: the run is deterministic."""
    n, V = 20000, 12
    row = np.array([0.3, -1.9, 2.4, 1.1, -0.6, 0.0, 1.7, -1.2, 0.8, -2.0, 2.0, -0.2], dtype=np.float32)
    x = np.broadcast_to(row, (n, V)).copy()
    logits = torch.from_numpy(x).to(DEV)
    key = torch.arange(n, dtype=torch.int64, device=DEV)
    smp = torch.zeros(n, dtype=torch.int32, device=DEV)
    done = torch.zeros(n, dtype=torch.int32, device=DEV)
    front = torch.zeros(1, dtype=torch.int32, device=DEV)
    pred = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    native.debug_sample(logits, key, smp, done, front, pred, n, temperature=1.0, pad=-1, eos=-2, seed=20260101)
    torch.cuda.synchronize()
    tok = pred.cpu().numpy()
    assert ((tok >= 0) & (tok < V)).all() and int(done.sum()) == 0
    prob = np.exp(row.astype(np.float64))
    prob /= prob.sum()
    count = np.bincount(tok, minlength=V).astype(np.float64)
    chi2 = float(((count - n * prob) ** 2 / (n * prob)).sum())
    print(f"chi-square {chi2:.3f} (bar {S.CHI2_11_Q1E6}); smallest expected count {n * prob.min():.1f}")
    assert chi2 < S.CHI2_11_Q1E6
    # and each draw is the one its own uniform selects
    u = S.uniform(20260101, np.arange(n), 0, 1)
    c = np.cumsum(prob)
    lo, hi = np.concatenate([[0.0], c[:-1]])[tok], c[tok]
    assert ((u >= lo - TOL) & (u <= hi + TOL)).all()


def test_refused_arguments(native):
    from translation_transformer_amd._native import TtxError
    ops = Operands(make_logits(4, 5, seed=1), seed=2)
    a = (ops.logits.v, ops.key.v, ops.smp.v, ops.done.v, ops.front.v, ops.pred.v, 4)
    for kw in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_k=-1), dict(top_k=33),
               dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(top_p=-0.5)):
        with pytest.raises(TtxError):
            native.debug_sample(*a, **kw)
    for live in (-1, 5):
        with pytest.raises(TtxError):
            native.debug_sample(*a, torch.tensor([live], dtype=torch.int32, device=DEV))
    big = torch.zeros((4, 1025), dtype=torch.float32, device=DEV)
    with pytest.raises(TtxError):
        native.debug_sample(big, *a[1:])
    with pytest.raises(TtxError):
        native.debug_sample(ops.logits.v, ops.key.v, ops.smp.v, ops.done.v, ops.front.v, ops.pred.v, 0)
    torch.cuda.synchronize()
    assert (ops.pred.get() == U.SENTINEL[torch.int32]).all() and ops.pred.margins() is None      # nothing was launched
