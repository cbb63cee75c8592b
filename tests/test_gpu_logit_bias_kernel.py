"""k_logit_bias (csrc/ttx_logit_bias.hip.h), one launch at a time through ttx_debug_logit_bias, EXACT against the NumPy restatement
of tests/util_logit_bias.py (bit for bit: the rule is one rounded fp32 add per entry, skipped where the bias entry is zero).

Vocabularies 7, 64, 250, 256, 1 000 and 1 024 (a scalar tail, a non-multiple of 4, rows that are and are not 16-byte aligned, the
maximum); both row mappings; the three forms the slot pool's verify step takes (the one pass, the probe with N = 1 and D = 0, a
compacted pass under a row map); a live-row count on the device below the launch's row count; bias tables whose row stride
exceeds V; a logits view whose base is only 4-byte aligned.  Bias entries include +0.0, -0.0, -inf, +-8 and denormals, logits
include -0.0 and -inf.  Rows at or beyond the live count and the guard margins on both sides of every operand must keep their
sentinels.
"""
import numpy as np
import pytest
import torch

import util_logit_bias as L
import util_loop_checks as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = [7, 64, 250, 256, 1000, 1024]
FILL = np.array([U.FLOAT_FILL], dtype=np.int32).view(np.float32)[0]          # what a dead row holds before and after the launch


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


class Guarded:
    """A float32 [M, V] operand inside an allocation with guard margins; ``shift`` elements move its base off 16-byte alignment."""

    def __init__(self, data: np.ndarray, shift: int = 0):
        self.n = data.size
        self.buf = torch.empty(self.n + 2 * U.GUARD + shift, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(U.FLOAT_FILL)
        self.lo = U.GUARD + shift
        self.v = self.buf[self.lo:self.lo + self.n].view(data.shape)
        self.v.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)))
        assert self.v.data_ptr() % 16 == (4 * shift) % 16

    def get(self) -> np.ndarray:
        return self.v.detach().cpu().numpy().copy()

    def margins_intact(self) -> bool:
        w = self.buf.view(torch.int32)
        return bool((w[:self.lo] == U.FLOAT_FILL).all()) and bool((w[self.lo + self.n:] == U.FLOAT_FILL).all())


def ints(a) -> U.Buf:
    a = np.asarray(a)
    return U.Buf(a.shape, torch.int32, DEV, a)


def run(native, x: np.ndarray, b: np.ndarray, live: int, what: str, *, src=None, rows_per_src=1, act=None, row_map=None, N=1, D=0,
        shift=0, live_on_device=True) -> None:
    """One launch; the result must be the restatement on the bits, dead rows and every margin untouched."""
    M, V = x.shape
    x = x.copy()
    x[live:] = FILL                                                  # sentinels in the rows the kernel must not write
    lg, bias = Guarded(x, shift), Guarded(b)
    bufs = {k: ints(v) for k, v in (("src", src), ("act", act), ("row_map", row_map)) if v is not None}
    m = ints([live]) if live_on_device else None
    bufs.update({} if m is None else {"m": m})
    native.debug_logit_bias(lg.v, bias.v, src=bufs["src"].v if "src" in bufs else None, m_live=None if m is None else m.v,
                            rows_per_src=rows_per_src, act_idx=bufs["act"].v if "act" in bufs else None,
                            row_map=bufs["row_map"].v if "row_map" in bufs else None, n=N, d=D)
    torch.cuda.synchronize()
    rows = L.rows_plain(src, live, rows_per_src) if act is None else L.rows_step(act, src, live, N, D, row_map)    # of the live rows
    L.check(lg.get(), x, b, rows, live, what)
    assert lg.margins_intact() and bias.margins_intact(), f"{what}: a guard margin of the logits or the bias was written"
    assert L.first_difference(bias.get(), b) is None, f"{what}: the bias table was written"
    for name, buf in bufs.items():
        assert buf.margins() is None, f"{what}: {name}: {buf.margins()}"


@pytest.mark.parametrize("V", VS)
def test_plain_mapping(native, V):
    rng = np.random.default_rng(V)
    M, live, S = 9, 5, 4
    src = np.array([3, 0, 0, 2, 1, 1, 3, 2, 0])
    for ld in (V, V + 5, V + 8):                             # a row stride that keeps / breaks the 16-byte alignment of the bias rows
        run(native, L.make_logits(rng, M, V), L.make_bias(rng, S, V, ld), live, f"plain V {V} ld {ld}", src=src)
    run(native, L.make_logits(rng, M, V), L.make_bias(rng, S, V), M, f"plain V {V}, no live count", src=src, live_on_device=False)
    # without a map: logits row r belongs to source r // rows_per_src (the teacher-forced logits of the scoring pass)
    run(native, L.make_logits(rng, 12, V), L.make_bias(rng, 3, V), 10, f"plain V {V} rows_per_src 4", rows_per_src=4)


@pytest.mark.parametrize("V", VS)
def test_step_layout(native, V):
    rng = np.random.default_rng(100 + V)
    N, D = 2, 3                                              # RPS = 7
    act = np.array([2, 0, 3])                                # three live slots, a permutation of decoder rows (row 1 is retired)
    src = np.array([1, 0, 0, 1])                             # by decoder row: rows 0 and 3 share bias row 1
    b = L.make_bias(rng, 2, V)
    run(native, L.make_logits(rng, 21, V), b, 21, f"step V {V}", src=src, act=act, N=N, D=D)
    run(native, L.make_logits(rng, 21, V), b, 15, f"step V {V}, 15 live rows", src=src, act=act, N=N, D=D)


@pytest.mark.parametrize("V", VS)
def test_probe_layout(native, V):
    rng = np.random.default_rng(200 + V)
    act = np.array([4, 1, 0, 3, 2])
    src = np.array([2, 0, 1, 1, 2])
    run(native, L.make_logits(rng, 6, V), L.make_bias(rng, 3, V), 5, f"probe V {V}", src=src, act=act, N=1, D=0)


@pytest.mark.parametrize("V", VS)
def test_compacted_pass(native, V):
    rng = np.random.default_rng(300 + V)
    N, D = 2, 3
    act = np.array([1, 2, 0])                                # the pass's own list
    src = np.array([0, 2, 1])
    # slot 0: row 0 and draft 1; slot 1: row 0 and both drafts; slot 2: row 0 and draft 0 (layout rows of k_embed<true>)
    row_map = np.array([0, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17])
    x = L.make_logits(rng, len(row_map) + 2, V)
    run(native, x, L.make_bias(rng, 3, V), len(row_map), f"compacted V {V}", src=src, act=act, row_map=np.append(row_map, [0, 0]), N=N, D=D)


@pytest.mark.parametrize("V", VS)
def test_base_that_is_only_four_byte_aligned(native, V):
    rng = np.random.default_rng(400 + V)
    src = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1])
    for shift in (1, 2, 3):
        run(native, L.make_logits(rng, 9, V), L.make_bias(rng, 2, V), 7, f"shift {shift} V {V}", src=src, shift=shift)
    act = np.array([1, 0])
    run(native, L.make_logits(rng, 14, V), L.make_bias(rng, 2, V), 14, f"step, shift 1, V {V}", src=np.array([0, 1]), act=act, N=2, D=3, shift=1)


def test_more_rows_than_one_workgroup_and_the_special_values(native):
    rng = np.random.default_rng(7)
    V, M = 256, 131                                          # 33 workgroups, the last one with three live waves
    x, b = L.make_logits(rng, M, V), L.make_bias(rng, 5, V)
    assert np.signbit(x[x == 0]).any() and np.isinf(x).any() and (b == 0).any() and np.signbit(b[b == 0]).any() and np.isinf(b).any()
    assert (np.abs(b[:, :V]) == 8).any() and ((b != 0) & (np.abs(b) < 1e-38)).any(), "the special bias values are missing"
    run(native, x, b, 129, "131 rows", src=rng.integers(0, 5, M))
    zero = np.zeros((5, V), dtype=np.float32)
    zero[:, ::2] = -0.0
    run(native, x, zero, M, "an all-zero bias leaves every bit", src=rng.integers(0, 5, M))


def test_refused_arguments(native):
    from translation_transformer_amd._native import TtxError
    x = torch.zeros((4, 8), dtype=torch.float32, device=DEV)
    b = torch.zeros((2, 8), dtype=torch.float32, device=DEV)
    src = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(TtxError):
        native.debug_logit_bias(x, torch.zeros((2, 4), dtype=torch.float32, device=DEV), src=src)      # ld_bias < V
    with pytest.raises(TtxError):
        native.debug_logit_bias(x, b, rows_per_src=0)                      # neither a map nor a divisor
    with pytest.raises(TtxError):
        native.debug_logit_bias(x, b, act_idx=src, n=2, d=3)               # the step layout needs src
    with pytest.raises(TtxError):
        native.debug_logit_bias(x, b, src=src, act_idx=src, n=0, d=3)
