"""Comparison helpers of the kernel-level GEMM / finisher tests (tests/test_gpu_gemm_kernels.py), kept free of any GPU call
so that tests/test_gemm_checks_host.py can show on the CPU that each of them fails when it should.

Operands live inside larger allocations (``Arena``): guard bands in front and behind, the columns between the logical
width and the leading dimension, and the rows a launch must not touch are filled with NaN.  A read outside an operand that
reaches a stored value turns it into NaN; a write outside the output changes a fill word and is found by
``Arena.untouched``.  Output arenas use a NaN with a payload of their own (``OUT_FILL``), so that a NaN copied from an
input to a place it does not belong is told from the fill.
"""
from __future__ import annotations

import torch

GUARD = 64                       # floats in front of and behind every operand (a multiple of 4: 16-byte alignment is kept)
IN_FILL = 0x7FC00000             # the quiet NaN of torch.nan: everything around X, W, bias, slabs, residual
OUT_FILL = 0x7FD5AAAA            # quiet NaN with a payload: everything an output launch finds in Y
U32 = 2.0 ** -24                 # unit roundoff of fp32


class Arena:
    """[slabs][rows][ld] floats with guard bands, exposed as the strided view ``v`` [slabs, rows, cols]."""

    def __init__(self, rows: int, cols: int, ld: int | None = None, slabs: int = 1, device="cpu", fill: int = IN_FILL,
                 guard: int = GUARD):
        self.rows, self.cols, self.ld, self.slabs, self.fill, self.guard = rows, cols, ld or cols, slabs, fill, guard
        assert self.ld >= cols and guard % 4 == 0
        self.slab_stride = rows * self.ld
        self.buf = torch.empty(2 * guard + slabs * self.slab_stride, dtype=torch.float32, device=device)
        self.reset()
        self.v = self.buf.as_strided((slabs, rows, cols), (self.slab_stride, self.ld, 1), guard)

    def reset(self) -> None:
        self.buf.view(torch.int32).fill_(self.fill)

    @property
    def m(self) -> torch.Tensor:
        """The first slab as a 2-D view (row stride = leading dimension)."""
        return self.v[0]

    def untouched(self, live_rows: int, slabs: int | None = None) -> str | None:
        """None when every word outside [:slabs, :live_rows, :cols] still holds the fill; else where the first other one is."""
        words = self.buf.view(torch.int32).clone()
        inner = words.as_strided((self.slabs, self.rows, self.cols), (self.slab_stride, self.ld, 1), self.guard)
        inner[:self.slabs if slabs is None else slabs, :live_rows] = self.fill
        bad = torch.nonzero(words != self.fill)
        if bad.numel() == 0:
            return None
        at = int(bad[0]) - self.guard
        if at < 0 or at >= self.slabs * self.slab_stride:
            return f"guard band overwritten at offset {at} relative to the output (word {int(words[int(bad[0])]) & 0xFFFFFFFF:#x})"
        s, rem = divmod(at, self.slab_stride)
        r, c = divmod(rem, self.ld)
        return f"write outside the live output: slab {s} row {r} column {c} (live rows {live_rows}, columns {self.cols}, ld {self.ld})"


def first_mismatch(got: torch.Tensor, want: torch.Tensor, bits: bool = False) -> str | None:
    """None, or a description of the first element of ``got`` that is not equal to ``want`` (a NaN is never equal).  ``bits``:
    both are fp32 and must agree bit for bit."""
    assert got.shape == want.shape, (got.shape, want.shape)
    if bits:
        same = (got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)) & ~torch.isnan(got)
    else:
        same = got.to(torch.float64) == want.to(torch.float64)
    bad = torch.nonzero(~same)
    if bad.numel() == 0:
        return None
    idx = tuple(int(i) for i in bad[0])
    return f"{bad.shape[0]} of {got.numel()} elements differ; first at {idx}: got {got[idx].item()!r} expected {want[idx].item()!r}"


def gamma(n: int) -> float:
    """Higham's gamma_n for fp32: the relative error bound of any n-term fp32 sum of products, in any order, with or without FMA."""
    return n * U32 / (1.0 - n * U32)


def gemm_ref64(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, relu: bool) -> torch.Tensor:
    """act(X W^T + b) in float64 with stock torch ops (exact for the integer operands of check (a))."""
    y = x.to(torch.float64) @ w.to(torch.float64).T
    if bias is not None:
        y = y + bias.to(torch.float64)
    return torch.relu(y) if relu else y


def gemm_bound(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, K: int) -> torch.Tensor:
    """gamma(K + 2) * (|X| |W|^T + |b|): element-wise bound of check (c)."""
    b = x.to(torch.float64).abs() @ w.to(torch.float64).abs().T
    if bias is not None:
        b = b + bias.to(torch.float64).abs()
    return gamma(K + 2) * b


def finish_slabs(slabs: torch.Tensor, bias: torch.Tensor | None, relu: bool = False) -> torch.Tensor:
    """What k_finish_ln makes of raw slabs [S, M, N] before its norm: fp32 sum in slab order, bias last."""
    y = slabs[0].clone()
    for s in range(1, slabs.shape[0]):
        y = y + slabs[s]
    if bias is not None:
        y = y + bias
    return torch.relu(y) if relu else y


def check_exact(got: torch.Tensor, want: torch.Tensor, what: str, bits: bool = False) -> None:
    """Checks (a) and (b): every element equals the exact result ((b): bit for bit)."""
    bad = first_mismatch(got, want, bits)
    assert bad is None, f"{what}: {bad}"


def check_bound(got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor, what: str) -> float:
    """Check (c): |y - y64| <= bound element-wise (NaN fails).  Returns the largest used fraction of the bound."""
    err = (got.to(torch.float64) - want64).abs()
    ok = err <= bound
    if not bool(ok.all()):
        bad = torch.nonzero(~ok)
        idx = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements outside the fp32 bound; first at {idx}: got "
                             f"{got[idx].item()!r} expected {want64[idx].item()!r} (error {err[idx].item():.3e}, bound {bound[idx].item():.3e})")
    return float((err / bound.clamp_min(1e-300)).max())


def check_same(a: torch.Tensor, b: torch.Tensor, what: str) -> None:
    """Check (d): two evaluations of the same operands are bit-identical."""
    if not torch.equal(a, b):
        raise AssertionError(f"{what}: {first_mismatch(a, b, bits=True)}")


def check_untouched(y: Arena, live_rows: int, what: str, slabs: int | None = None) -> None:
    bad = y.untouched(live_rows, slabs)
    assert bad is None, f"{what}: {bad}"


# ---- operands -------------------------------------------------------------------------------------------------------
def int_operands(gen: torch.Generator, m: int, n: int, k: int):
    """Integers in [-8, 8]: every partial sum is an integer below 2^24 for K <= 8192, hence exact in fp32 in any order."""
    r = lambda *shape: torch.randint(-8, 9, shape, generator=gen).to(torch.float32)
    return r(m, k), r(n, k), r(n)


def float_operands(gen: torch.Generator, m: int, n: int, k: int):
    u = lambda *shape: torch.rand(shape, generator=gen, dtype=torch.float32) * 2.0 - 1.0
    return u(m, k), u(n, k) * 0.125, u(n)


def scaled_normals(gen: torch.Generator, rows: int, cols: int) -> torch.Tensor:
    """Random normal floats times 2^e, e uniform in [-20, 20]; no zeros, no subnormals (check (b))."""
    x = torch.randn((rows, cols), generator=gen, dtype=torch.float32)
    x = torch.where(x.abs() < 2.0 ** -10, torch.full_like(x, 0.5), x)
    e = torch.randint(-20, 21, (rows, cols), generator=gen).to(torch.float32)
    return x * torch.exp2(e)


# ---- finisher ---------------------------------------------------------------------------------------------------------
def ln64(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    x = x.to(torch.float64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)                     # biased
    return (x - mean) / torch.sqrt(var + eps) * g.to(torch.float64) + b.to(torch.float64)


def finish_ref64(pre: torch.Tensor, g1, b1, g2, b2, eps: float) -> torch.Tensor:
    """LN2?(LN(pre)) in float64 from a given pre-norm row."""
    y = ln64(pre, g1, b1, eps)
    return ln64(y, g2, b2, eps) if g2 is not None else y


def finish_pre64(slabs: torch.Tensor, bias: torch.Tensor, resid: torch.Tensor) -> torch.Tensor:
    """(resid + bias) + sum of slabs, exactly (float64)."""
    return (resid.to(torch.float64) + bias.to(torch.float64)) + slabs.to(torch.float64).sum(0)


def finish_pre32_in_order(slabs: torch.Tensor, bias: torch.Tensor, resid: torch.Tensor) -> torch.Tensor:
    """The same in fp32 the way the kernel is defined: slabs added to each other in slab order, then to (resid + bias)."""
    t = slabs[0].clone()
    for s in range(1, slabs.shape[0]):
        t = t + slabs[s]
    return (resid + bias) + t


def finish_torch32(pre32: torch.Tensor, g1, b1, g2, b2, eps: float) -> torch.Tensor:
    """Plain fp32 evaluation with stock torch ops on the CPU: the arithmetic the tolerance is taken from."""
    d = pre32.shape[-1]
    y = torch.nn.functional.layer_norm(pre32.cpu(), (d,), g1.cpu(), b1.cpu(), eps)
    if g2 is not None:
        y = torch.nn.functional.layer_norm(y, (d,), g2.cpu(), b2.cpu(), eps)
    return y


def finish_tolerance(torch32: torch.Tensor, ref64: torch.Tensor) -> tuple[float, float]:
    """(e32, tolerance): e32 = max |torch_fp32 - fp64|; tolerance = 4 e32 + 2^-22 max |fp64|."""
    e32 = float((torch32.to(torch.float64) - ref64.cpu()).abs().max())
    return e32, 4.0 * e32 + 2.0 ** -22 * float(ref64.abs().max())


def check_finish_structure(y: Arena, live_rows: int, row_valid: torch.Tensor | None, what: str) -> None:
    """Rows with row_valid == 0 are exactly 0.0, rows >= live_rows and the guard bands keep their fill, no NaN in a valid row."""
    check_untouched(y, live_rows, what)
    out = y.m[:live_rows]
    valid = torch.ones(live_rows, dtype=torch.bool, device=out.device) if row_valid is None else row_valid[:live_rows].to(out.device) != 0
    dropped = out[~valid]
    if dropped.numel():
        bad = torch.nonzero(dropped.view(torch.int32) != 0)
        assert bad.numel() == 0, f"{what}: a row with row_valid == 0 is not exactly +0.0 ({bad.shape[0]} words)"
    nan_rows = torch.nonzero(torch.isnan(out[valid]).any(-1))
    assert nan_rows.numel() == 0, f"{what}: NaN in valid row (index among valid rows) {int(nan_rows[0])}"


def check_finish_values(got: torch.Tensor, ref64: torch.Tensor, tol: float, what: str) -> float:
    err = (got.to(torch.float64) - ref64.to(got.device)).abs()
    worst = float(err.max()) if err.numel() else 0.0
    if not worst <= tol:
        idx = tuple(int(i) for i in torch.nonzero(~(err <= tol))[0])
        raise AssertionError(f"{what}: error {worst:.3e} above the tolerance {tol:.3e}; first at {idx}: got {got[idx].item()!r} "
                             f"expected {ref64[idx].item()!r}")
    return worst


def magnitude_slabs(gen: torch.Generator, n_slabs: int, rows: int, d: int) -> torch.Tensor:
    """Per column a permutation of (2^24, 1, -2^24, 1, 0, ...) over the slabs, with 2^24 placed ahead of -2^24 and at least one 1
    between them or after them in an order where fp32 loses it: the in-order fp32 sum differs from the exact sum (2)."""
    base = torch.zeros(n_slabs)
    base[:4] = torch.tensor([2.0 ** 24, 1.0, -2.0 ** 24, 1.0])
    out = torch.empty(n_slabs, rows, d)
    for r in range(rows):
        for c in range(d):
            while True:
                p = base[torch.randperm(n_slabs, generator=gen)]
                t = torch.zeros((), dtype=torch.float32)
                for v in p.to(torch.float32):
                    t = t + v
                if float(t) != 2.0:           # keep only orders that fp32 addition gets wrong
                    break
            out[:, r, c] = p
    return out
