"""The exact-GELU epilogue of every GEMM kernel an FFN1 launch can reach (csrc/ttx_gemm.hip, ttx_debug_gemm_act), one launch
at a time on operands the test builds, against the float64 yardstick of tests/util_gelu.py.

Per operand case (K, N, leading dimensions, bias, three live row counts) every variant x tiling that accepts the shape is launched,
as a step launch (live row count on the device) and as a bulk launch, and
  (a) on selector operands (one non-zero per X row, so that the pre-activation x IS a chosen value: every multiple of 1/64 in
      [-12, 12], +-0, +-1e-30, +-20, +-88, +-1e30; with a bias, a multiple of 1/64 in [-1, 1] is added, which fp32 does exactly
      for the multiples and the test rounds as the kernel does for the rest) |y - gelu64(x)| <= A(x), NaN and Inf failing,
  (c) on random floats |y - gelu64(x64)| <= 1.13 * gemm_bound + A(x64): the GEMM's own fp32 bound carried through the largest
      slope of GELU (1.129), plus one evaluation of the activation,
  (d) all those launches return the same bits, and so does every row under every live row count that contains it.
Rows at or beyond the live count and everything around the output keep their fill (util_gemm_checks.Arena).  Raw split-K slabs take
no activation, so no launch of the grid has slabs; the refusal is tested at the end.

The grid is pairwise as in tests/test_gpu_gemm_kernels.py: every N and every live M meets every K.  k_gemm2<4> takes K = 256 only
beyond k_gemm3's 768 columns, so one case at N = 769 is added to the grid.  The last test requires that every kernel and body an
FFN1 can dispatch to ran with GELU at a ragged M and N and saw every chosen value.
"""
import itertools

import pytest
import torch

import util_gemm_checks as G
from util_gelu import ACT_GELU, ACT_NONE, ACT_RELU, GELU_MAX_SLOPE, act_bound, gelu64

pytestmark = pytest.mark.gpu

GV_BIG, GV_SMALL, GV_BIG_FFN2_SLABS, GV_MID = 0, 1, 2, 3
K_GEMM3, K_TN, K_G24_4, K_G24_0, K_G2_1, K_G2_2, K_G2_4, K_G2_0, BODY_128 = 1, 2, 3, 4, 5, 6, 7, 8, 16
FFN1_KERNELS = [K_GEMM3, K_TN, K_G24_4, K_G24_4 | BODY_128, K_G24_0, K_G24_0 | BODY_128, K_G2_1, K_G2_2, K_G2_4, K_G2_0]
TILE = {kid: ((32, 32) if kid == K_GEMM3 else (128, 64) if kid & BODY_128 else (64, 64)) for kid in FFN1_KERNELS}

KS = [64, 128, 192, 256, 320, 512, 1024]
NS = [1, 31, 33, 64, 65, 129, 300]
MS = [1, 31, 33, 64, 65, 129, 257]

# (a): the chosen pre-activations
CHOSEN = torch.cat([torch.arange(-12 * 64, 12 * 64 + 1, dtype=torch.float32) / 64.0,
                    torch.tensor([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, 1e30, -1e30])])

REACHED = set()          # (kernel id, K, M, N) of every GELU launch of the grid
SEEN = {}                # kernel id -> bool mask over CHOSEN: the values a GELU launch of check (a) returned an output for


def slice_k(K):
    return 64 if K in (64, 128) else 0 if K % 256 else 256 if K >= 2048 else 64


def expected_kernel(step, variant, N, K):
    """The documented dispatch of launch_gemm without slabs (without the body flag)."""
    small = step and variant == GV_SMALL
    if small and K == 256 and N <= 768:
        return K_GEMM3
    if slice_k(K) == 0:
        return K_TN
    if K % 256 == 0 and not small:
        return K_G24_4 if K == 256 else K_G24_0
    return {64: K_G2_1, 128: K_G2_2, 256: K_G2_4}.get(K, K_G2_0)


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session


def cases():
    out = []
    for ki, K in enumerate(KS):
        for ni, N in enumerate(NS):
            i = ki * len(NS) + ni
            ms = sorted({MS[(3 * ni + ki + j) % len(MS)] for j in range(3)})
            out.append(dict(id=f"K{K}-N{N}", K=K, N=N, ms=ms, ldx=K + 4 * (i % 2), ldw=K + 4 * ((i // 2) % 2),
                            ldy=N + (0, 1, 4)[(i + ki) % 3], bias=(i % 5 != 3), seed=5000 + i))
    out.append(dict(id="K256-N769", K=256, N=769, ms=[33, 65, 257], ldx=256, ldw=260, ldy=770, bias=True, seed=5999))
    return out


CASES = cases()
# (step, variant, tiling) of every launch of a case: the four variants under both tilings on a live row count, and the bulk passes
CONFIGS = [(True, v, t) for v, t in itertools.product((GV_BIG, GV_SMALL, GV_BIG_FFN2_SLABS, GV_MID), (1, 2))] + \
          [(False, GV_BIG, 1), (False, GV_BIG, 2), (False, GV_SMALL, 1)]


def test_grid_is_pairwise():
    """Every N and every live M meets every K; every distance ldy - N, bias on and off occur per K."""
    for K in KS:
        mine = [c for c in CASES if c["K"] == K and c["N"] in NS]
        assert {c["N"] for c in mine} == set(NS) and {m for c in mine for m in c["ms"]} == set(MS), K
        assert {c["ldy"] - c["N"] for c in mine} == {0, 1, 4} and {c["bias"] for c in mine} == {True, False}, K
    assert {expected_kernel(s, v, c["N"], c["K"]) for c in CASES for s, v, _ in CONFIGS} == {k & ~BODY_128 for k in FFN1_KERNELS}


class Launcher:
    """Operands of one case on the device and the launches over them (ttx_debug_gemm_act, or ttx_debug_gemm when act is None)."""

    def __init__(self, native, c, m_max):
        self.native, self.K, self.N, self.m_max = native, c["K"], c["N"], m_max
        self.x = G.Arena(m_max, self.K, c["ldx"], device="cuda")
        self.w = G.Arena(self.N, self.K, c["ldw"], device="cuda")
        self.b = G.Arena(1, self.N, device="cuda") if c["bias"] else None
        self.y = G.Arena(m_max, self.N, c["ldy"], device="cuda", fill=G.OUT_FILL)
        self.m_dev = torch.zeros(1, dtype=torch.int32, device="cuda")

    def load(self, x, w, b):
        self.xv, self.wv, self.bv = x.cuda(), w.cuda(), (b.cuda() if self.b is not None else None)
        self.w.m[:] = self.wv
        if self.b is not None:
            self.b.m[0] = self.bv

    def run(self, M, step, variant, tiling, what, act=ACT_GELU, relu=False):
        self.x.reset()
        self.x.m[:M] = self.xv[:M]                         # rows in [M, m_max) stay NaN
        self.y.reset()
        self.m_dev.fill_(M)
        kid = self.native.debug_gemm(self.x.m, self.w.m, None if self.b is None else self.b.m[0], self.y.m, self.N, self.K,
                                     self.m_max if step else M, self.m_dev if step else None, relu=relu, variant=variant,
                                     tiling=tiling, activation=act)
        assert kid & ~BODY_128 == expected_kernel(step, variant, self.N, self.K), f"{what}: dispatched kernel {kid}"
        what = f"{what} [kernel {kid}]"
        G.check_untouched(self.y, M, what)
        return self.y.m[:M].clone(), kid, what


def selector_operands(c, m_top):
    """X rows with a single 1.0 at column k(m) = (5 m + 1) mod K; W[n, k] walks CHOSEN, so Y[m, n] = act(W[n, k(m)] + b[n])."""
    K, N = c["K"], c["N"]
    x = torch.zeros(m_top, K)
    km = (5 * torch.arange(m_top) + 1) % K
    x[torch.arange(m_top), km] = 1.0
    idx = (torch.arange(K)[None, :] * N + torch.arange(N)[:, None] + c["seed"]) % CHOSEN.numel()        # [N, K]
    w = CHOSEN[idx]
    b = ((torch.arange(N) * 3) % 129 - 64).to(torch.float32) / 64.0
    pre = w.T[km]                                                                                       # [m_top, N], exact
    if c["bias"]:
        pre = pre + b                      # fp32: exact for the multiples of 1/64, rounded as the kernel's add for the rest
    return x, w, b, pre, idx.T[km]


def describe(c, M, cfg):
    step, variant, tiling = cfg
    return (f"K={c['K']} N={c['N']} M={M} ldx={c['ldx']} ldw={c['ldw']} ldy={c['ldy']} bias={c['bias']} "
            f"{'step' if step else 'bulk'} variant={variant} tiling={tiling}")


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_gelu_case(native, case):
    c = case
    m_top = max(c["ms"])
    L = Launcher(native, c, m_top + 3)
    gen = torch.Generator().manual_seed(c["seed"])
    used = {}
    for kind in ("chosen", "floats"):
        if kind == "chosen":
            x, w, b, pre, which = selector_operands(c, m_top)
            L.load(x, w, b)
            x64 = pre.cuda().to(torch.float64)
            bound = act_bound(x64)
        else:
            x, w, b = G.float_operands(gen, m_top, c["N"], c["K"])
            L.load(x, w, b)
            x64 = G.gemm_ref64(L.xv, L.wv, L.bv, False)
            bound = GELU_MAX_SLOPE * G.gemm_bound(L.xv, L.wv, L.bv, c["K"]) + act_bound(x64)
        ref = gelu64(x64)
        first = {}
        for M in c["ms"]:
            for cfg in CONFIGS:
                got, kid, what = L.run(M, *cfg, f"{kind}: " + describe(c, M, cfg))
                REACHED.add((kid, c["K"], M, c["N"]))
                tag = "(a) " if kind == "chosen" else "(c) "
                used[kind] = max(used.get(kind, 0.0), G.check_bound(got, ref[:M], bound[:M], tag + what))
                if kind == "chosen":
                    SEEN.setdefault(kid, torch.zeros(CHOSEN.numel(), dtype=torch.bool))[which[:M].reshape(-1)] = True
                if M in first:
                    G.check_same(got, first[M][0], f"(d) {what} against {first[M][1]}")
                else:
                    for lo, (res, desc) in first.items():          # the rows shared with every smaller live count
                        G.check_same(got[:lo], res, f"(d) rows [0, {lo}) of {what} against {desc}")
                    first[M] = (got, what)
    print(f"{c['id']}: largest used fraction of A on chosen values {used['chosen']:.3f}, of the bound on floats {used['floats']:.3f}")


@pytest.mark.parametrize("case", [c for c in CASES if c["id"] in ("K64-N65", "K128-N129", "K192-N33", "K256-N300", "K256-N769",
                                                                  "K512-N65", "K1024-N31")], ids=lambda c: c["id"])
def test_none_and_relu_through_the_new_entry_point_equal_ttx_debug_gemm(native, case):
    c = case
    M = max(c["ms"])
    L = Launcher(native, c, M + 3)
    L.load(*G.float_operands(torch.Generator().manual_seed(c["seed"] + 1), M, c["N"], c["K"]))
    for cfg in CONFIGS:
        for act in (ACT_NONE, ACT_RELU):
            new, kid, what = L.run(M, *cfg, f"activation {act}: " + describe(c, M, cfg), act=act)
            old, kid_old, _ = L.run(M, *cfg, "ttx_debug_gemm", act=None, relu=bool(act))
            assert kid == kid_old
            G.check_same(new, old, what + " against ttx_debug_gemm")
            if act == ACT_RELU:
                assert float(new.min()) == 0.0 and bool((new == 0).any()) and bool((new > 0).any())


def test_activation_on_raw_slabs_and_unknown_codes_are_refused(native):
    from translation_transformer_amd import _native as N_
    x = G.Arena(8, 2048, device="cuda")
    w = G.Arena(8, 2048, device="cuda")
    y = G.Arena(8, 8, 8, slabs=8, device="cuda", fill=G.OUT_FILL)
    m = torch.full((1,), 4, dtype=torch.int32, device="cuda")
    x.m[:] = 1.0
    w.m[:] = 1.0

    def refused(**kw):
        a = dict(x=x.m[:, :256], w=w.m[:, :256], bias=None, y=y.m, n=8, k=256, m_max=8, m_live=m, splits=0, slab_stride=y.slab_stride)
        a.update(kw)
        with pytest.raises(N_.TtxError) as e:
            native.debug_gemm(**a)
        assert e.value.code == N_.TTX_ERR_INVALID, kw
        return True

    assert refused(activation=3) and refused(activation=-1) and refused(activation=16)
    for act in (ACT_RELU, ACT_GELU):
        assert refused(activation=act, splits=1)
        assert refused(activation=act, x=x.m, w=w.m, k=2048, splits=8)
        assert refused(activation=act, x=x.m, w=w.m, k=2048, splits=8, variant=GV_SMALL)
    torch.cuda.synchronize()
    assert y.untouched(0) is None, "a refused call wrote to the output"
    native.debug_gemm(x.m, w.m, None, y.m, 8, 2048, 8, m, splits=8, slab_stride=y.slab_stride, activation=ACT_NONE)   # slabs without one: fine
    torch.cuda.synchronize()
    assert y.untouched(4) is None and bool((y.v[:, :4] == 256.0).all())


def test_every_ffn1_kernel_ran_with_gelu():
    """Coverage condition (runs after the grid above): every kernel / body an FFN1 launch can dispatch to ran with GELU at a ragged
    M and a ragged N, and returned an output for every chosen pre-activation."""
    assert REACHED, "run the whole module: this test reads what the others launched"
    missing = []
    for kid in FFN1_KERNELS:
        th, tw = TILE[kid]
        hits = sorted((K, M, N) for (k, K, M, N) in REACHED if k == kid and M % th and N % tw)
        seen = int(SEEN[kid].sum()) if kid in SEEN else 0
        print(f"kernel {kid}: {len(hits)} ragged GELU launches, e.g. (K, M, N) = {hits[:2]}; {seen} of {CHOSEN.numel()} chosen values")
        if not hits or seen != CHOSEN.numel():
            missing.append(kid)
    assert not missing, f"kernels without a ragged GELU launch or without every chosen value: {missing}"
