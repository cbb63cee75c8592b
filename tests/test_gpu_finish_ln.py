"""k_finish_ln (slab sum + bias + residual + LayerNorm, optional second norm) on operands the test builds, through
ttx_debug_finish_ln: all five row widths, the two straight-line slab counts of d = 256 (1, 8) and the general loop, live row
counts around the four rows of a workgroup, against the same formula in float64.

The tolerance is taken from the plain fp32 evaluation of the formula with stock torch ops on the CPU:
e32 = max |torch_fp32 - fp64| per case, and the kernel must satisfy max |kernel - fp64| <= 4 e32 + 2^-22 max |fp64| (the factor
for the different reduction tree, the floor for cases where torch happens to be exact).  Achieved on an MI355X, worst case of
the grid per d (printed by test_finisher_table; also in DESIGN.md §5) — the kernel stays within 1.1x of torch's own fp32 error:

    d      e32 (torch fp32)   kernel error   kernel error / tolerance
    64     7.492e-07          6.989e-07      0.203
    128    9.943e-07          9.548e-07      0.213
    256    8.763e-07          9.758e-07      0.415
    512    9.892e-07          9.892e-07      0.278
    1024   1.057e-06          1.142e-06      0.305
"""
import pytest
import torch

import util_gemm_checks as G

pytestmark = pytest.mark.gpu

DS = [64, 128, 256, 512, 1024]
SLABS = [1, 2, 8, 9, 16]
MS = [1, 3, 4, 5, 257]
EPS = 1e-5
TABLE = {}               # d -> (worst e32, worst kernel error, worst error / tolerance)


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; d and eps are arguments


class Finisher:
    """Operands of one finisher launch inside NaN-filled allocations; rows at and beyond M are NaN in every row operand."""

    def __init__(self, native, d, n_slabs, M, slack=3):
        self.native, self.d, self.n_slabs, self.M, self.m_max = native, d, n_slabs, M, M + slack
        dev = "cuda"
        self.slabs = G.Arena(self.m_max, d, slabs=n_slabs, device=dev)
        self.resid = G.Arena(self.m_max, d, device=dev)
        self.vec = {k: G.Arena(1, d, device=dev) for k in ("bias", "g1", "b1", "g2", "b2")}
        self.y = G.Arena(self.m_max, d, device=dev, fill=G.OUT_FILL)
        self.m_dev = torch.full((1,), M, dtype=torch.int32, device=dev)

    def run(self, slabs, resid, bias, g1, b1, g2, b2, row_valid):
        M = self.M
        self.slabs.v[:, :M] = slabs.cuda()
        self.resid.m[:M] = resid.cuda()
        for k, t in (("bias", bias), ("g1", g1), ("b1", b1), ("g2", g2), ("b2", b2)):
            if t is not None:
                self.vec[k].m[0] = t.cuda()
        rv = None
        if row_valid is not None:
            rv = torch.full((self.m_max + 2 * G.GUARD,), 7, dtype=torch.uint8, device="cuda")     # rows >= M: neither 0 nor 1
            rv = rv[G.GUARD:G.GUARD + self.m_max]
            rv[:M] = row_valid.cuda()
        p = lambda k: self.vec[k].m[0]
        self.native.debug_finish_ln(self.slabs.v[0], self.n_slabs, self.slabs.slab_stride, p("bias"), self.resid.m, p("g1"), p("b1"),
                                    p("g2") if g2 is not None else None, p("b2") if g2 is not None else None, rv, self.y.m,
                                    self.m_max, self.d, EPS, self.m_dev)
        return self.y


def draw(gen, n_slabs, M, d):
    u = lambda *shape: torch.rand(shape, generator=gen, dtype=torch.float32) * 2.0 - 1.0
    # ranges of util_models.seeded_weights: gamma in [0.9, 1.1], beta and bias in [-0.1, 0.1]; slabs and residual in [-1, 1]
    return dict(slabs=u(n_slabs, M, d), resid=u(M, d), bias=u(d), g1=1.0 + 0.1 * u(d), b1=0.1 * u(d), g2=1.0 + 0.1 * u(d), b2=0.1 * u(d))


GRID = [(d, n, M, 25 * di + 5 * ni + mi) for di, d in enumerate(DS) for ni, n in enumerate(SLABS) for mi, M in enumerate(MS)]


@pytest.mark.parametrize("d,n_slabs,M,i", GRID, ids=[f"d{d}-s{n}-M{M}" for d, n, M, _ in GRID])
def test_finisher_against_fp64(native, d, n_slabs, M, i):
    di, ni, mi = i // 25, (i // 5) % 5, i % 5
    second, masked = bool((di + ni + mi) % 2), bool((di + mi) % 2)             # each setting meets every d, slab count and M
    gen = torch.Generator().manual_seed(500 + i)
    o = draw(gen, n_slabs, M, d)
    g2, b2 = (o["g2"], o["b2"]) if second else (None, None)
    row_valid = (torch.rand(M, generator=gen) < 0.6).to(torch.uint8) if masked else None
    if masked and M > 1:
        row_valid[0], row_valid[-1] = 0, 1
    what = f"d={d} n_slabs={n_slabs} M={M} m_max={M + 3} second norm={second} row_valid={'mixed' if masked else 'NULL'}"
    y = Finisher(native, d, n_slabs, M).run(o["slabs"], o["resid"], o["bias"], o["g1"], o["b1"], g2, b2, row_valid)
    G.check_finish_structure(y, M, row_valid, what)
    ref = G.finish_ref64(G.finish_pre64(o["slabs"], o["bias"], o["resid"]), o["g1"], o["b1"], g2, b2, EPS)
    t32 = G.finish_torch32(G.finish_pre32_in_order(o["slabs"], o["bias"], o["resid"]), o["g1"], o["b1"], g2, b2, EPS)
    e32, tol = G.finish_tolerance(t32, ref)
    keep = torch.ones(M, dtype=torch.bool) if row_valid is None else row_valid != 0
    err = G.check_finish_values(y.m[:M].cpu()[keep], ref[keep], tol, what)
    print(f"{what}: torch fp32 error {e32:.3e}, kernel error {err:.3e}, tolerance {tol:.3e}")
    w = TABLE.get(d, (0.0, 0.0, 0.0))
    TABLE[d] = (max(w[0], e32), max(w[1], err), max(w[2], err / tol))


@pytest.mark.parametrize("n_slabs", [8, 9])
def test_slabs_are_added_in_slab_order(native, n_slabs):
    """Slabs that are, per column, a permutation of (2^24, 1, -2^24, 1, 0, ...) in an order fp32 addition gets wrong: the kernel
    must give the LayerNorm of the in-order fp32 sum, and that must be told from the LayerNorm of the exact sum.  (Swapping
    slabs 0 and 1 is the one reordering no test can see: fp32 addition commutes, s0 + s1 == s1 + s0.)"""
    d, M = 256, 4
    gen = torch.Generator().manual_seed(77 + n_slabs)
    o = draw(gen, n_slabs, M, d)
    o["slabs"] = G.magnitude_slabs(gen, n_slabs, M, d)
    what = f"magnitude case n_slabs={n_slabs} d={d} M={M}"
    y = Finisher(native, d, n_slabs, M).run(o["slabs"], o["resid"], o["bias"], o["g1"], o["b1"], None, None, None)
    G.check_finish_structure(y, M, None, what)
    pre32 = G.finish_pre32_in_order(o["slabs"], o["bias"], o["resid"])
    assert 0.1 < float(pre32.var(-1).min()) and float(pre32.var(-1).max()) < 10.0          # rows keep a variance of order 1
    ref = G.finish_ref64(pre32, o["g1"], o["b1"], None, None, EPS)
    e32, tol = G.finish_tolerance(G.finish_torch32(pre32, o["g1"], o["b1"], None, None, EPS), ref)
    err = G.check_finish_values(y.m[:M].cpu(), ref, tol, what)
    exact = G.finish_ref64(G.finish_pre64(o["slabs"], o["bias"], o["resid"]), o["g1"], o["b1"], None, None, EPS)
    away = float((y.m[:M].cpu().to(torch.float64) - exact).abs().max())
    print(f"{what}: error against the in-order sum {err:.3e} (tolerance {tol:.3e}), against the exact sum {away:.3e}")
    assert away > tol, "the case does not tell the slab order from the exact sum"


def test_invalid_arguments_are_refused(native):
    from translation_transformer_amd import _native as N_
    f = Finisher(native, 256, 2, 4)
    o = draw(torch.Generator().manual_seed(1), 2, 4, 256)
    f.run(o["slabs"], o["resid"], o["bias"], o["g1"], o["b1"], None, None, None)             # the base call is fine
    p = lambda k: f.vec[k].m[0]
    base = dict(slabs=f.slabs.v[0], n_slabs=2, slab_stride=f.slabs.slab_stride, bias=p("bias"), resid=f.resid.m, g1=p("g1"), b1=p("b1"),
                g2=None, b2=None, row_valid=None, y=f.y.m, m_max=f.m_max, d=256, eps=EPS, m_live=f.m_dev)

    def refused(**kw):
        with pytest.raises(N_.TtxError) as e:
            native.debug_finish_ln(**dict(base, **kw))
        assert e.value.code == N_.TTX_ERR_INVALID, kw
        return True

    f.y.reset()
    assert refused(d=96) and refused(d=0) and refused(d=2048) and refused(d=192)
    assert refused(g2=p("g2")) and refused(b2=p("b2"))                        # half a second norm
    assert refused(n_slabs=0) and refused(m_max=0)
    assert refused(slab_stride=f.slabs.slab_stride - 256)                      # slabs overlap
    assert refused(slab_stride=f.slabs.slab_stride + 2)                        # float4 loads of the second slab
    assert refused(bias=f.vec["bias"].buf[G.GUARD + 1:][:256])                 # not 16-byte aligned
    assert refused(y=f.y.buf[G.GUARD + 2:][:f.m_max * 256].view(f.m_max, 256))
    f.m_dev.fill_(f.m_max + 1)
    assert refused()                                                           # live rows above the capacity
    f.m_dev.fill_(4)
    lib = native._lib
    assert lib.ttx_debug_finish_ln(native.session, None, 1, 0, p("bias").data_ptr(), f.resid.m.data_ptr(), p("g1").data_ptr(),
                                   p("b1").data_ptr(), None, None, None, f.y.m.data_ptr(), None, f.m_max, 256, EPS, None) == N_.TTX_ERR_INVALID
    torch.cuda.synchronize()
    assert f.y.untouched(0) is None                                            # nothing was launched


def test_finisher_table():
    """Prints the achieved errors per row width (the table of DESIGN.md §5); runs after the grid above."""
    assert set(TABLE) == set(DS), "run the whole module: this test reads what the grid measured"
    print("d      e32 (torch fp32)   kernel error   kernel error / tolerance")
    for d in DS:
        e32, err, frac = TABLE[d]
        print(f"{d:<6d} {e32:.3e}          {err:.3e}      {frac:.3f}")
        assert frac <= 1.0
