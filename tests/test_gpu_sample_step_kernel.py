"""k_sample_step (csrc/ttx_sample.hip.h) one launch at a time through ttx_debug_sample_step, on operands the test builds.

Every live row's token must EQUAL what ttx_debug_sample (k_sample, held to float64 by tests/test_gpu_sample_kernel.py) returns for
the same logits row with front[0] = pos - 1 and that row's key and sample id, (b, pos) being the restated mapping of
tests/util_sample_spec.py: this pins the shared arithmetic and the row mapping at once.  Beside that: ``consistent`` with float64
within the tol = 1e-4 of tests/test_gpu_sample_kernel.py (the same arithmetic on the same row lengths, so the same bound),
temperature 0 and top_k = 1 against k_argmax, rows at or beyond the live count, guard margins, refused arguments.
"""
import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_sample_checks as S
import util_sample_spec as X
from test_gpu_sample_kernel import make_logits, planted

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
B = 5
SETTINGS = [dict(temperature=1.0), dict(temperature=0.5, top_k=32, top_p=0.9975), dict(temperature=3.0, top_p=0.5),
            dict(temperature=2.0, top_k=3)]


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


class StepOperands:
    """B slots of 1 + N*D step rows: a non-identity active list, distinct fronts, keys with high words, every operand between guard
    margins."""

    def __init__(self, x: np.ndarray, N: int, D: int, seed: int):
        rng = np.random.default_rng(seed)
        self.x, self.N, self.D, self.R = x, N, D, U.rps(N, D)
        self.M, self.V = x.shape
        assert self.M == B * self.R
        self.act_np = np.array([3, 0, 4, 1, 2], dtype=np.int32)
        self.front_np = (1 + rng.permutation(40)[:B] + np.array([0, 0, 0, 0, 4900])).astype(np.int32)     # distinct; one far right
        self.front_np[self.act_np[0]] = 0
        self.key_np = rng.integers(-2 ** 63, 2 ** 63, B, dtype=np.int64)
        self.key_np[1] = (0xFFFFFFFF << 32) - 2 ** 64                   # the high word alone
        self.smp_np = rng.integers(-2 ** 31, 2 ** 31, B, dtype=np.int64).astype(np.int32)
        self.logits = U.Buf(x.shape, torch.float32, DEV, x)
        self.key = U.Buf((B,), torch.int64, DEV, self.key_np)
        self.smp = U.Buf((B,), torch.int32, DEV, self.smp_np)
        self.act = U.Buf((B,), torch.int32, DEV, self.act_np)
        self.front = U.Buf((B,), torch.int32, DEV, self.front_np)
        self.pred = U.Buf((self.M,), torch.int32, DEV)

    def launch(self, native, n_active: int, live=None, **kw) -> np.ndarray:
        self.pred.reset()
        live = n_active * self.R if live is None else live
        native.debug_sample_step(self.logits.v, self.key.v, self.smp.v, self.act.v, self.front.v, self.pred.v, B=B, n=self.N, d=self.D,
                                 n_active=n_active, m_live=torch.tensor([live], dtype=torch.int32, device=DEV), **kw)
        torch.cuda.synchronize()
        for b in (self.logits, self.key, self.smp, self.act, self.front, self.pred):
            assert b.margins() is None, b.margins()
        got = self.pred.get()
        assert (got[live:] == U.SENTINEL[torch.int32]).all(), "a row at or beyond the live count was written"
        return got

    def by_k_sample(self, native, n_active: int, **kw) -> np.ndarray:
        """The tokens ttx_debug_sample gives the live rows: one launch per distinct position, on the rows that predict it."""
        b, pos = X.step_rows(self.act_np, self.front_np, n_active, self.N, self.D)
        want = np.full(len(b), -1, dtype=np.int32)
        for p in np.unique(pos):
            rows = np.nonzero(pos == p)[0]
            m = len(rows)
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
            pred = torch.full((m,), -1, dtype=torch.int32, device=DEV)
            native.debug_sample(t(self.x[rows], torch.float32), t(self.key_np[b[rows]], torch.int64), t(self.smp_np[b[rows]], torch.int32),
                                torch.zeros(m, dtype=torch.int32, device=DEV), torch.tensor([p - 1], dtype=torch.int32, device=DEV),
                                pred, m, pad=-1, eos=-2, **kw)
            want[rows] = pred.cpu().numpy()
        return want


@pytest.mark.parametrize("n_active", [1, 3, 5])
@pytest.mark.parametrize("N,D", X.ND)
@pytest.mark.parametrize("V", [5, 64, 65, 256, 1024])
def test_rows_equal_k_sample_on_the_bits_and_are_consistent(native, V, N, D, n_active):
    ops = StepOperands(make_logits(B * U.rps(N, D), V, seed=V * 100 + N * 10 + D), N, D, seed=V + N + D)
    b, pos = X.step_rows(ops.act_np, ops.front_np, n_active, N, D)
    live = n_active * ops.R
    worst = 0.0
    for i, kw in enumerate(SETTINGS):
        seed = 0x9E3779B97F4A7C15 ^ (i << 40)
        got = ops.launch(native, n_active, seed=seed, pad=-1, eos=-2, **kw)
        want = ops.by_k_sample(native, n_active, seed=seed, **kw)
        d = U.first_difference(got[:live], want)
        assert d is None, f"V {V} N {N} D {D} n_active {n_active} {kw}: against k_sample: {d}"
        p = S.Params(kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), pad=-1, eos=-2)
        u = S.uniform(seed, ops.key_np[b], ops.smp_np[b], pos)
        for r in range(live):
            ex = S.excess(int(got[r]), ops.x[r], float(u[r]), p, TOL)
            worst = max(worst, ex)
            assert ex <= TOL, f"V {V} N {N} D {D} {kw}: row {r} token {got[r]} lies {ex:.3e} outside its interval"
    print(f"V {V} N {N} D {D} n_active {n_active}: {live} live rows, largest excess over the exact interval {worst:.3e}")


@pytest.mark.parametrize("N,D", X.ND)
@pytest.mark.parametrize("V", [5, 65, 1024])
def test_greedy_settings_equal_k_argmax(native, V, N, D):
    M = B * U.rps(N, D)
    ops = StepOperands(planted(M, V, seed=V + N), N, D, seed=3)
    want = U.Buf((M,), torch.int32, DEV)
    native.debug_argmax(ops.logits.v, want.v, M)
    torch.cuda.synchronize()
    for kw in (dict(temperature=0.0), dict(temperature=0.0, top_k=5, top_p=0.3), dict(temperature=1.0, top_k=1), dict(temperature=0.5, top_k=1)):
        got = ops.launch(native, B, seed=11, **kw)
        d = U.first_difference(got, want.get())
        assert d is None, f"V {V} N {N} D {D} {kw}: {d}"


def test_live_count_below_the_active_slots_and_zero(native):
    N, D, V = 3, 2, 65
    ops = StepOperands(make_logits(B * U.rps(N, D), V, seed=1), N, D, seed=2)
    full = ops.launch(native, B, seed=5)
    for live in (0, 1, 6, 9, 34):
        got = ops.launch(native, B, live=live, seed=5)
        assert (got[:live] == full[:live]).all()
    b = ops.launch(native, B, seed=5)
    assert (b == full).all(), "two launches differ"
    assert (ops.launch(native, B, seed=6) != full).any()


def test_refused_arguments(native):
    from translation_transformer_amd._native import TtxError
    N, D = 3, 2
    ops = StepOperands(make_logits(B * U.rps(N, D), 5, seed=1), N, D, seed=2)
    a = (ops.logits.v, ops.key.v, ops.smp.v, ops.act.v, ops.front.v, ops.pred.v)
    ok = dict(B=B, n=N, d=D, n_active=B)
    ops.pred.reset()
    for kw in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_k=33), dict(top_p=0.0), dict(n_active=B + 1),
               dict(n_active=-1), dict(n=0), dict(d=0), dict(B=0), dict(n_active=3),
               dict(m_live=torch.tensor([B * 7 + 1], dtype=torch.int32, device=DEV)), dict(m_live=torch.tensor([-1], dtype=torch.int32, device=DEV))):
        with pytest.raises(TtxError):
            native.debug_sample_step(*a, **{**ok, **kw})
    dup = torch.tensor([0, 1, 1, 2, 3], dtype=torch.int32, device=DEV)
    with pytest.raises(TtxError):
        native.debug_sample_step(ops.logits.v, ops.key.v, ops.smp.v, dup, ops.front.v, ops.pred.v, **ok)
    neg = torch.tensor([0, -1, 2, 3, 4], dtype=torch.int32, device=DEV)
    with pytest.raises(TtxError):
        native.debug_sample_step(ops.logits.v, ops.key.v, ops.smp.v, ops.act.v, neg, ops.pred.v, **ok)
    big = torch.zeros((B * 7, 1025), dtype=torch.float32, device=DEV)
    with pytest.raises(TtxError):
        native.debug_sample_step(big, *a[1:], **ok)
    torch.cuda.synchronize()
    assert (ops.pred.get() == U.SENTINEL[torch.int32]).all() and ops.pred.margins() is None      # nothing was launched
