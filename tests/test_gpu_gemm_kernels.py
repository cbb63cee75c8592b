"""Every GEMM kernel of csrc/ttx_gemm.hip, one launch at a time on operands the test builds (ttx_debug_gemm), against
references that share no code with them (stock torch float64).  The LayerNorm finisher: tests/test_gpu_finish_ln.py.

Per operand case (K, N, strides, bias, ReLU, a list of live row counts) every variant x tiling x slab count that accepts the
shape is launched and
  (a) on integer operands in [-8, 8] the output equals the exact result element for element,
  (c) on random floats it lies within gamma(K + 2) (|X| |W|^T + |b|) of the float64 result,
  (d) all those launches return the same bits, and so does every row under every live row count that contains it;
(b) runs on selector operands of its own.  X, W, bias and Y are interior views of NaN-filled allocations
(util_gemm_checks.Arena): a read outside the operands poisons the result, a write outside the live output is found in the
fill.  tests/test_gemm_checks_host.py shows on the CPU that each check fails when the result carries the defect it is for.

Pruning of the issue's grid, by contract of the kernels and nothing else:
  * k_gemm3 only takes K = 256, N <= 768 and step launches without slabs; k_gemm_tn only K without canonical slices
    (32, 96, 192, 320); slabs exist only for K >= 2048 with at most 16 slices — each K class meets every N, the three
    leading dimensions, bias / ReLU and every live row count, not every other K;
  * the cross product is pairwise: every N meets every K class, every live M meets every K class (three per case, cycling),
    strides / bias / ReLU cycle with different periods.
"""
import itertools

import pytest
import torch

import util_gemm_checks as G

pytestmark = pytest.mark.gpu

GV_BIG, GV_SMALL, GV_BIG_FFN2_SLABS, GV_MID = 0, 1, 2, 3
K_GEMM3, K_TN, K_G24_4, K_G24_0, K_G2_1, K_G2_2, K_G2_4, K_G2_0, BODY_128 = 1, 2, 3, 4, 5, 6, 7, 8, 16
NAMES = {K_GEMM3: "k_gemm3", K_TN: "k_gemm_tn", K_G24_4: "k_gemm24<4>/64x64", K_G24_4 | BODY_128: "k_gemm24<4>/128x64",
         K_G24_0: "k_gemm24<0>/64x64", K_G24_0 | BODY_128: "k_gemm24<0>/128x64", K_G2_1: "k_gemm2<1>", K_G2_2: "k_gemm2<2>",
         K_G2_4: "k_gemm2<4>", K_G2_0: "k_gemm2<0>"}
TILE = {K_GEMM3: (32, 32), K_TN: (64, 64), K_G24_4: (64, 64), K_G24_4 | BODY_128: (128, 64), K_G24_0: (64, 64),
        K_G24_0 | BODY_128: (128, 64), K_G2_1: (64, 64), K_G2_2: (64, 64), K_G2_4: (64, 64), K_G2_0: (64, 64)}

K_CLASSES = {"K64": [64], "K128": [128], "K256": [256], "K64slices": [512, 768, 1024], "K256slices": [2048, 2304, 4096, 8192],
             "Ktn": [32, 96, 192, 320]}
NS = [1, 5, 30, 31, 32, 33, 63, 64, 65, 127, 129, 300, 768, 769, 1000, 2048]
MS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 257]

REACHED = set()          # (kernel id, K, M, N) of every launch of this module: the coverage condition at the end reads it


def slice_k(K):
    return 64 if K in (64, 128) else 0 if K % 256 else 256 if K >= 2048 else 64


def gemm_splits(K, step, variant):
    """The slab count the library gives a step GEMM (csrc/ttx_gemm.hip: gemm_splits)."""
    return K // 256 if step and variant == GV_SMALL and slice_k(K) == 256 and K // 256 <= 16 else 1


def expected_kernel(step, variant, N, K, splits):
    """The documented dispatch of launch_gemm: what a launch is expected to report (without the body flag)."""
    S = max(splits, 1)
    kps = K // S
    small = step and variant == GV_SMALL
    if small and K == 256 and N <= 768 and S == 1:
        return K_GEMM3
    if slice_k(K) == 0:
        return K_TN
    if kps % 256 == 0 and not small:
        return K_G24_4 if kps == 256 else K_G24_0
    return {64: K_G2_1, 128: K_G2_2, 256: K_G2_4}.get(kps, K_G2_0)


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session


def cases():
    out = []
    for ci, (cname, ks) in enumerate(K_CLASSES.items()):
        for ni, N in enumerate(NS):
            i = ci * len(NS) + ni
            K = ks[ni % len(ks)]
            ms = sorted({MS[(3 * ni + ci + j * 5) % len(MS)] for j in range(3)})
            out.append(dict(id=f"{cname}-K{K}-N{N}", K=K, N=N, ms=ms, ldx=K + 4 * (i % 2), ldw=K + 4 * ((i // 2) % 2),
                            ldy=N + (0, 1, 4)[(i + ci) % 3], bias=(i % 5 != 3), relu=bool((i // 3) % 2), seed=1000 + i))
    return out


CASES = cases()


def test_grid_is_pairwise():
    """Every N and every live M meets every K class; every K, leading dimension, bias and ReLU setting occurs per class."""
    for cname, ks in K_CLASSES.items():
        mine = [c for c in CASES if c["id"].startswith(cname + "-")]
        assert {c["N"] for c in mine} == set(NS) and {m for c in mine for m in c["ms"]} == set(MS), cname
        assert {c["K"] for c in mine} == set(ks)
        assert {c["ldx"] - c["K"] for c in mine} == {0, 4} and {c["ldw"] - c["K"] for c in mine} == {0, 4}
        assert {c["ldy"] - c["N"] for c in mine} == {0, 1, 4}
        assert {c["bias"] for c in mine} == {True, False} and {c["relu"] for c in mine} == {True, False}


class Launcher:
    """Operands of one case on the device and the launches over them."""

    def __init__(self, native, K, N, m_max, ldx, ldw, ldy, bias, relu, max_slabs):
        self.native, self.K, self.N, self.m_max, self.relu = native, K, N, m_max, relu
        self.x = G.Arena(m_max, K, ldx, device="cuda")
        self.w = G.Arena(N, K, ldw, device="cuda")
        self.b = G.Arena(1, N, device="cuda") if bias else None
        self.y = G.Arena(m_max, N, ldy, slabs=max_slabs, device="cuda", fill=G.OUT_FILL)
        self.m_dev = torch.zeros(1, dtype=torch.int32, device="cuda")

    def load(self, x, w, b):
        self.xv, self.wv, self.bv = x.cuda(), w.cuda(), (b.cuda() if self.b is not None else None)
        self.w.m[:] = self.wv
        if self.b is not None:
            self.b.m[0] = self.bv

    def run(self, M, step, variant, tiling, splits, what):
        """One launch with M live rows; returns (result [M, N] with slabs summed in order and the bias added last, the description
        extended by the kernel that ran)."""
        self.x.reset()
        self.x.m[:M] = self.xv[:M]                         # rows in [M, m_max) stay NaN
        self.y.reset()
        self.m_dev.fill_(M)
        kid = self.native.debug_gemm(self.x.m, self.w.m, None if self.b is None else self.b.m[0], self.y.m, self.N, self.K,
                                     self.m_max if step else M, self.m_dev if step else None, self.relu and splits == 0, splits,
                                     self.y.slab_stride, variant, tiling)
        assert kid & ~BODY_128 == expected_kernel(step, variant, self.N, self.K, splits), f"{what}: dispatched {NAMES.get(kid, kid)}"
        REACHED.add((kid, self.K, M, self.N))
        what = f"{what} [{NAMES[kid]}]"
        G.check_untouched(self.y, M, what, slabs=max(splits, 1))
        if splits == 0:
            return self.y.m[:M].clone(), what
        return G.finish_slabs(self.y.v[:splits, :M], self.bv, self.relu), what


def configs(K):
    """(step, variant, tiling, splits) of every launch of a case."""
    S = gemm_splits(K, True, GV_SMALL)
    out = []
    for variant, tiling in itertools.product((GV_BIG, GV_SMALL, GV_BIG_FFN2_SLABS, GV_MID), (1, 2)):
        for splits in sorted({0, 1, S} if variant in (GV_BIG, GV_SMALL) else {0, S} - {1}):
            out.append((True, variant, tiling, splits))
    out += [(False, GV_BIG, 1, 0), (False, GV_BIG, 2, 0), (False, GV_SMALL, 1, 0)]        # bulk passes: no live count on the device
    return out


def describe(c, M, cfg):
    step, variant, tiling, splits = cfg
    return (f"K={c['K']} N={c['N']} M={M} m_max={c['m_max']} ldx={c['ldx']} ldw={c['ldw']} ldy={c['ldy']} bias={c['bias']} "
            f"relu={c['relu']} {'step' if step else 'bulk'} variant={variant} tiling={tiling} splits={splits}")


def run_case(native, c, cfgs_of):
    K, N = c["K"], c["N"]
    m_top = max(c["ms"])
    c = dict(c, m_max=m_top + c.get("slack", 3))
    L = Launcher(native, K, N, c["m_max"], c["ldx"], c["ldw"], c["ldy"], c["bias"], c["relu"], max(gemm_splits(K, True, GV_SMALL), 1))
    gen = torch.Generator().manual_seed(c["seed"])
    used = 0.0
    for kind, draw in (("integers", G.int_operands), ("floats", G.float_operands)):
        x, w, b = draw(gen, m_top, N, K)
        L.load(x, w, b)
        ref = G.gemm_ref64(L.xv, L.wv, L.bv, c["relu"])
        bound = G.gemm_bound(L.xv, L.wv, L.bv, K) if kind == "floats" else None
        first = {}                                    # row count -> (result, description) of its first launch
        for M in c["ms"]:
            for cfg in cfgs_of(M):
                what = f"{kind}: " + describe(c, M, cfg)
                got, what = L.run(M, *cfg, what)
                if kind == "integers":
                    G.check_exact(got, ref[:M], "(a) " + what)
                else:
                    used = max(used, G.check_bound(got, ref[:M], bound[:M], "(c) " + what))
                if M in first:
                    G.check_same(got, first[M][0], f"(d) {what} against {first[M][1]}")
                else:
                    for lo, (res, desc) in first.items():          # batch invariance: the rows shared with every smaller live count
                        G.check_same(got[:lo], res, f"(d) rows [0, {lo}) of {what} against {desc}")
                    first[M] = (got, what)
    return used


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_gemm_case(native, case):
    cfgs = configs(case["K"])
    used = run_case(native, case, lambda M: cfgs)
    print(f"{case['id']}: largest used fraction of the fp32 bound {used:.4f}")


# The five GEMM shapes of a verify step at the benchmark model (d = 256, F = 2048, V = 256) at one live row count per
# production class, under the tile choice the library makes itself (tiling 0) and the variant its default thresholds
# (800 / 2000 / 5600 live rows) give that row count (csrc/ttx_api.hip: variant_qkv / variant_dd / variant_ffn1 / variant_ffn2).
def production_variant(M, shape):
    v = GV_SMALL if M < 800 else GV_MID if M < 2000 else GV_BIG_FFN2_SLABS if M < 5600 else GV_BIG
    if shape in ("qkv", "ffn1"):
        return GV_SMALL if v == GV_SMALL else GV_BIG
    if shape in ("dxd", "classifier"):
        return GV_SMALL if v in (GV_SMALL, GV_MID) else GV_BIG
    return GV_BIG if v == GV_BIG else GV_SMALL                                               # ffn2


LARGE_SHAPES = {"qkv": (768, 256, True, False), "dxd": (256, 256, True, False), "ffn1": (2048, 256, True, True),
                "ffn2": (256, 2048, True, False), "classifier": (256, 256, True, False)}


@pytest.mark.parametrize("M", [310, 1200, 4960, 15872])
@pytest.mark.parametrize("shape", list(LARGE_SHAPES))
def test_production_shapes(native, shape, M):
    N, K, bias, relu = LARGE_SHAPES[shape]
    variant = production_variant(M, shape)
    splits = gemm_splits(K, True, variant)
    case = dict(id=f"{shape}-M{M}", K=K, N=N, ms=[M], ldx=K, ldw=K, ldy=N, bias=bias, relu=relu, seed=7000 + M + N,
                slack=200)                # capacity beyond the live rows: whole workgroups find no row of theirs and leave at once
    # the production launch, then the 64x64 tiling walking all slices as a second evaluation for (d)
    cfgs = [(True, variant, 0, splits if splits > 1 else 0), (True, GV_BIG, 1, 0)]
    used = run_case(native, case, lambda _M: cfgs)
    print(f"{case['id']}: variant {variant}, splits {splits}, largest used fraction of the fp32 bound {used:.4f}")


# (b) selector operands: one non-zero product per sum, so every k must be visited exactly once and no value may change on its way
SELECTOR = [(K, variant, tiling, splits)
            for K in (64, 128, 256, 512, 2048, 8192, 96, 320)
            for variant, tiling in ((GV_BIG, 1), (GV_BIG, 2), (GV_SMALL, 1))
            for splits in sorted({0, gemm_splits(K, True, GV_SMALL)} - {1})]


@pytest.mark.parametrize("K,variant,tiling,splits", SELECTOR)
def test_selector_operands(native, K, variant, tiling, splits):
    gen = torch.Generator().manual_seed(31 * K + 7 * variant + tiling + splits)
    for which in ("X is the identity", "W is the identity"):
        if which.startswith("X"):
            M, N = K, 33
            w = G.scaled_normals(gen, N, K)
            x = torch.eye(K)
            want = w.T.contiguous()
        else:
            M, N = 65, K
            x = G.scaled_normals(gen, M, K)
            w = torch.eye(K)
            want = x
        L = Launcher(native, K, N, M + 3, K + 4, K, N + 4, False, False, max(splits, 1))
        L.load(x, w, None)
        what = f"(b) {which}: K={K} M={M} N={N} variant={variant} tiling={tiling} splits={splits}"
        got, what = L.run(M, True, variant, tiling, splits, what)
        G.check_exact(got, want.cuda(), what, bits=True)


def test_selector_reaches_gemm2_4(native):
    """k_gemm2<4> takes K = 256 only beyond k_gemm3's 768 columns: its selector pair at N = 769 / K = 256 slabs of K = 2048."""
    gen = torch.Generator().manual_seed(99)
    w = G.scaled_normals(gen, 769, 256)
    L = Launcher(native, 256, 769, 259, 256, 260, 769, False, False, 1)
    L.load(torch.eye(256), w, None)
    got, what = L.run(256, True, GV_SMALL, 1, 0, "(b) X is the identity: K=256 N=769")
    assert "k_gemm2<4>" in what
    G.check_exact(got, w.T.contiguous().cuda(), what, bits=True)


# ---- arguments the kernels cannot take are refused on the host ------------------------------------------------------
def test_invalid_arguments_are_refused(native):
    from translation_transformer_amd import _native as N_
    LD = 2052
    x = G.Arena(8, 2048, LD, device="cuda")
    w = G.Arena(8, 2048, LD, device="cuda")
    y = G.Arena(8, 8, 8, slabs=16, device="cuda", fill=G.OUT_FILL)
    m = torch.full((1,), 4, dtype=torch.int32, device="cuda")
    x.m[:] = 1.0
    w.m[:] = 1.0

    def view(a, k, ld=LD, shift=0):
        return a.buf[G.GUARD + shift:].as_strided((8, k), (ld, 1))

    def refused(**kw):
        a = dict(x=view(x, 256), w=view(w, 256), bias=None, y=y.m, n=8, k=256, m_max=8, m_live=m, splits=0, slab_stride=y.slab_stride)
        a.update(kw)
        if "k" in kw and "x" not in kw:
            a.update(x=view(x, kw["k"]), w=view(w, kw["k"]))
        with pytest.raises(N_.TtxError) as e:
            native.debug_gemm(**a)
        assert e.value.code == N_.TTX_ERR_INVALID, kw
        return True

    native.debug_gemm(view(x, 256), view(w, 256), None, y.m, 8, 256, 8, m)     # the base call itself is fine
    assert refused(k=48) and refused(k=40)                                     # K not a multiple of 32
    assert refused(x=view(x, 256, LD - 2)) and refused(w=view(w, 256, LD - 2))  # ldx / ldw not multiples of 4
    assert refused(x=view(x, 256, LD, 1)) and refused(w=view(w, 256, LD, 2))   # X / W not 16-byte aligned
    assert refused(bias=w.buf[G.GUARD + 1:][:8])
    assert refused(y=y.buf[G.GUARD + 1:].as_strided((8, 8), (8, 1)))           # float4 rows of k_gemm3
    assert refused(x=view(x, 256, 128))                                        # ldx < K
    assert refused(k=768, splits=4)                                            # 192-k slabs: not a shape the ring kernels walk
    assert refused(k=2048, splits=16) and refused(k=2048, splits=3)            # half slices; K not divisible
    assert refused(k=96, splits=2)                                             # 48-k slabs of a K without slices
    assert refused(k=256, splits=2, slab_stride=8)                             # slabs overlap
    assert refused(k=256, splits=1, relu=True)                                 # raw slabs are partial sums: no activation
    assert refused(variant=4) and refused(tiling=3) and refused(n=0) and refused(m_max=0) and refused(splits=-1)
    m.fill_(9)
    assert refused()                                                           # live rows above the capacity
    m.fill_(-1)
    assert refused()
    m.fill_(4)
    lib = native._lib
    for args in ((None, LD, w.m.data_ptr(), LD, None, y.m.data_ptr()), (x.m.data_ptr(), LD, None, LD, None, y.m.data_ptr()),
                 (x.m.data_ptr(), LD, w.m.data_ptr(), LD, None, None)):
        assert lib.ttx_debug_gemm(native.session, *args, 8, m.data_ptr(), 8, 8, 256, 0, 0, 0, 0, 0, None, None) == N_.TTX_ERR_INVALID
    assert lib.ttx_debug_gemm(None, x.m.data_ptr(), LD, w.m.data_ptr(), LD, None, y.m.data_ptr(), 8, m.data_ptr(), 8, 8, 256, 0, 0,
                              0, 0, 0, None, None) == N_.TTX_ERR_INVALID
    torch.cuda.synchronize()
    assert y.untouched(4) is None


def test_every_kernel_and_body_was_reached():
    """Coverage condition: each kernel / body ran at least once with a ragged M and a ragged N (runs after the grid above)."""
    assert REACHED, "run the whole module: this test reads what the others launched"

    def ragged(kid, pred=lambda K: True):
        th, tw = TILE[kid]
        return [(K, M, N) for (k, K, M, N) in REACHED if k == kid and M % th and N % tw and pred(K)]

    want = [(K_GEMM3, None), (K_TN, None), (K_G24_4, None), (K_G24_4 | BODY_128, None), (K_G24_0, None),
            (K_G24_0 | BODY_128, lambda K: K < 2048), (K_G24_0 | BODY_128, lambda K: K >= 2048),
            (K_G2_1, None), (K_G2_2, None), (K_G2_4, None), (K_G2_0, None)]
    missing = []
    for kid, pred in want:
        hits = ragged(kid, pred or (lambda K: True))
        label = NAMES[kid] + ("" if pred is None else (" K<2048" if pred(512) else " K>=2048"))
        print(f"{label}: {len(hits)} ragged launches, e.g. (K, M, N) = {sorted(hits)[:2]}")
        if not hits:
            missing.append(label)
    assert not missing, f"never run at a ragged M and N: {missing}"
