"""k_attn<MODE, 64> and k_attn2<MODE, 64> (csrc/ttx_attn.hip: ten instantiations over the five modes) on operands the test builds,
one launch at a time through ttx_debug_attn_hd, against the documented rule in float64: tests/test_gpu_attn_kernels.py at head
dimension 64, with util_attn_hd (tests/test_attn_hd_checks_host.py shows on the CPU that its checks can fail).

KL = ttx_attn_staged_key_limit(64, .) is asked of the library, not written down here; the edge cases sit around it.

  structure   rows of slots >= n_active, rows behind the launch and the guard bands keep their fill; every live word is written
  values      max |kernel - float64| <= 4 e32 + (ln nk + 2) 2^-23 max |V|: util_attn_checks' derived bound, not retuned
  bits        three launches agree; a slot alone == the slot among others; the real positions do not depend on how far the
              padding extends (24 positions padded to 40 and 64, within each kernel); the production choice == the kernel it
              reports; ttx_debug_attn_hd(head_dim = 32) == ttx_debug_attn
  routing     step modes run on k_attn2 whatever H is (H = 4 included), on k_attn beyond KL staged keys; forced k_attn3 /
              k_attn3s and k_attn2 beyond KL are refused and leave the output untouched

Achieved on an MI355X, worst case of the grid per kernel and mode (printed by test_attention_table; also in DESIGN.md §5).  As at
head dimension 32 the largest errors, torch's own included, come from the cases whose scores sit near +100:

    kernel    mode        e32 (torch fp32)   kernel error   kernel error / tolerance
    k_attn    ENC         4.392e-05          4.390e-05      0.246
    k_attn    FULL_SELF   1.296e-05          1.284e-05      0.239
    k_attn    FULL_CROSS  2.833e-05          2.833e-05      0.243
    k_attn    STEP_SELF   4.591e-05          4.591e-05      0.375
    k_attn    STEP_CROSS  4.033e-05          4.033e-05      0.374
    k_attn2   ENC         4.392e-05          5.065e-05      0.283
    k_attn2   FULL_SELF   1.296e-05          2.345e-05      0.437
    k_attn2   FULL_CROSS  1.907e-05          1.783e-05      0.227
    k_attn2   STEP_SELF   4.591e-05          4.562e-05      0.351
    k_attn2   STEP_CROSS  4.033e-05          4.146e-05      0.374
"""
import pytest
import torch

import translation_transformer_amd as tta
import util_attn_checks as A
import util_attn_hd as AH
import util_gemm_checks as G

pytestmark = pytest.mark.gpu

DH = 64
KL = int(tta.lib().ttx_attn_staged_key_limit(DH, 64))           # a host query: no device needed to build the grid
KL32 = int(tta.lib().ttx_attn_staged_key_limit(DH, 32))         # the 32-query image (step launches of up to 32 rows per slot)

SELF_LS = [1, 15, 16, 17, 31, 32, 33, 64, 65, 130]
CROSS_LKS = [1, 31, 32, 33, 64, 65, KL - 1, KL, KL + 1]
# Queries per decoder row of the FULL_CROSS cases.  util_attn_checks uses 3; here the tolerance's e32 = max |torch fp32 - float64| is
# a maximum over the case's own outputs, and over 3 queries x 1 head it is too small a sample to stand for fp32: for the peaked
# distribution at Lk = 31 it ranges from 7e-7 to 5e-6 with the seed while an fp32 evaluation with another reduction tree sits at
# 1e-6 .. 3e-6 throughout.  33 queries (a second query tile, a third 16-query chunk of k_attn) keep e32 within 3e-6 .. 9e-6.
CROSS_L = 33
F_VALUES = [0, 1, 31, 32, 33, 63, 64, 65, 200]
SRC_LENS = [1, 31, 32, 33, 70]
STEP_ND = [(1, 0), (1, 1), (3, 10), (7, 10), (64, 1), (4, 3)]
HS = [2, 1, 4]


def grid_slots(i, n):
    """Slot specs of grid case i: fronts and source lengths walk their lists, slot 1 has a PAD front token (case 0: at f = 0),
    slot 2 PADs inside its prefix and source."""
    out = []
    for j in range(n):
        f = F_VALUES[(4 * i + 2 * j) % len(F_VALUES)]
        if j == 1 and i % 4 == 0:
            f = 0
        out.append(dict(f=f, src=SRC_LENS[(i + j) % len(SRC_LENS)], front_pad=(j == 1), prefix_pads=(j == 2)))
    return out


def full_grid(mode):
    cases = []
    if mode == AH.FULL_CROSS:
        for i, Lk in enumerate(CROSS_LKS):
            cases.append(AH.full_case(DH, mode, CROSS_L, Lk, 3 if i % 2 else 1, H=HS[i % 3], dist=AH.DISTS[i % 6], seed=100 + i,
                                      shared_mem=(i % 4 == 1)))
    else:
        for i, L in enumerate(SELF_LS):
            cases.append(AH.full_case(DH, mode, L, 0, 1 if i % 2 else 3, H=HS[i % 3], dist=AH.DISTS[(i + mode) % 6], seed=10 * mode + i))
    return cases


def step_grid(mode):
    """Every (N, D) with five slots of mixed front / source length in one launch (four and a trailing inactive one where i is
    odd), the null and the non-identity indirections alternating; three of five slots active; and, for STEP_SELF, a cache whose
    capacity puts the staged key count at KL exactly and one key beyond it."""
    cases = []
    for i, (N, D) in enumerate(STEP_ND):
        cases.append(AH.step_case(DH, mode, N, D, grid_slots(i, 5), H=HS[i % 3], dist=AH.DISTS[i % 6], seed=i, extra_groups=i % 2,
                                  cache_slot=bool(i % 2), src_of=bool((i // 2) % 2), src_len=bool(i % 3)))
    cases.append(AH.step_case(DH, mode, 7, 10, grid_slots(7, 5), n_active=3, H=4, dist="ascending", seed=21, cache_slot=True, src_len=True,
                              name=f"dh64-{AH.MODE_NAMES[mode]}-3-of-5-active-H4"))
    if mode == AH.STEP_SELF:
        # N = 3, D = 10: a workgroup stages capacity + 1 + 30 keys
        for cap, tag in ((KL - 31, "at-KL"), (KL - 30, "past-KL")):
            cases.append(AH.step_case(DH, mode, 3, 10, [dict(f=200, src=1), dict(f=cap - 3, src=1, prefix_pads=True), dict(f=0, src=1)], H=2,
                                      dist="upper", seed=25, cache_len=cap, name=f"dh64-STEP_SELF-staged-keys-{tag}"))
    return cases


GRIDS = {m: (step_grid(m) if m >= AH.STEP_SELF else full_grid(m)) for m in range(5)}
ALL_CASES = [c for m in range(5) for c in GRIDS[m]]


def limit_of(case):
    return KL32 if case.q_per_group <= 32 else KL


RUNS = [(c, k) for c in ALL_CASES for k in AH.kernels_for(c, limit_of(c))]
TABLE = {}               # (kernel, mode) -> (worst e32, worst kernel error, worst error / tolerance)
_OPS = {}


@pytest.fixture(scope="module")
def native():
    from util_models import tiny_state
    assert tta.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)    # any model gives a session; H, head_dim and the shapes are arguments


def launch(native, case, kernel, make=AH.Operands):
    """One launch into a freshly filled output; returns (operands, kernel id reported)."""
    ops = _OPS.get(id(case))
    if ops is None:
        ops = _OPS[id(case)] = make(case, "cuda")
        ops.keep = case                                                  # id() stays unique while the operands are cached
    ops.out.reset()
    kid = native.debug_attn(**ops.kw, kernel=kernel)
    torch.cuda.synchronize()
    return ops, kid


def result(native, case, kernel, want_kernel=None):
    ops, kid = launch(native, case, kernel)
    assert kid == (kernel if want_kernel is None else want_kernel), f"{case.name}: asked for {AH.KERNEL_NAMES[kernel]}, ran {AH.KERNEL_NAMES[kid]}"
    AH.check_structure(ops.out, case, f"{case.name} on {AH.KERNEL_NAMES[kid]}")
    return ops.out.m[:case.live_rows].clone()


@pytest.mark.parametrize("case,kernel", RUNS, ids=[f"{c.name}-{AH.KERNEL_NAMES[k]}" for c, k in RUNS])
def test_kernel_against_fp64(native, case, kernel):
    what = f"{case.name} on {AH.KERNEL_NAMES[kernel]}"
    got = result(native, case, kernel)
    r = AH.reference(case)
    err_all = (got.cpu().to(torch.float64) - r["ref"][:case.live_rows]).abs()
    print(f"{what}: torch fp32 error {r['e32']:.3e}, kernel error {float(err_all.max()) if err_all.numel() else 0.0:.3e}, "
          f"tolerance {r['tol']:.3e} (nk {r['nk']}, max |V| {r['vmax']:.2f})")
    err = AH.check_values(got, case, what)
    dead = r["ref"][:case.live_rows].abs().sum(-1) == 0                  # a query that sees no key: exactly +0.0, not merely small
    assert not dead.any() or int((got.cpu()[dead].view(torch.int32) != 0).sum()) == 0, f"{what}: a fully masked query is not exactly 0"
    w = TABLE.get((kernel, case.mode), (0.0, 0.0, 0.0))
    TABLE[(kernel, case.mode)] = (max(w[0], r["e32"]), max(w[1], err), max(w[2], err / r["tol"]))


def test_grid_reaches_the_edges():
    """What the grid is meant to hold is in it."""
    assert KL32 >= KL > 65 and KL % 32 == 0
    for m in range(5):
        assert {c.dist for c in GRIDS[m]} == set(AH.DISTS), AH.MODE_NAMES[m]
        assert {c.H for c in GRIDS[m]} == {1, 2, 4}, AH.MODE_NAMES[m]
        dead = sum(int((AH.reference(c)["ref"][:c.live_rows].abs().sum(-1) == 0).sum()) for c in GRIDS[m])
        assert dead > 0 or m == AH.STEP_CROSS, AH.MODE_NAMES[m]
    specs = [(c, s) for c in GRIDS[AH.STEP_SELF] for s in c.specs[:c.n_active]]
    assert any(s["f"] == 0 and s["front_pad"] for _, s in specs) and any(s["f"] > 0 and s["front_pad"] for _, s in specs)
    assert set(F_VALUES) <= {s["f"] for _, s in specs}
    assert {s["src"] for c in GRIDS[AH.STEP_CROSS] for s in c.specs[:c.n_active]} == set(SRC_LENS)
    for m in (AH.STEP_SELF, AH.STEP_CROSS):
        assert {(c.N, c.D) for c in GRIDS[m]} >= set(STEP_ND)
        assert any(c.n_active < c.groups for c in GRIDS[m]) and any(c.cache_slot is not None or c.src_of is not None for c in GRIDS[m])
    # both kernels wherever k_attn2 has the capacity; k_attn alone one key beyond it
    alone = [c for c in ALL_CASES if AH.K_ATTN2 not in AH.kernels_for(c, limit_of(c))]
    assert sorted((c.mode, AH.staged_keys(c)) for c in alone) == [(AH.FULL_CROSS, KL + 1), (AH.STEP_SELF, KL + 1)], alone
    at = [c for c in ALL_CASES if c.name.endswith("staged-keys-at-KL")][0]
    assert AH.staged_keys(at) == KL


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_production_choice_is_the_kernel_it_reports(native, case):
    """k_attn2 for every mode and head count (never k_attn3 / k_attn3s, H = 4 included), k_attn beyond its capacity."""
    ops, kid = launch(native, case, AH.K_PROD)
    assert kid == (AH.K_ATTN2 if AH.staged_keys(case) <= limit_of(case) else AH.K_ATTN), (case.name, kid)
    AH.check_structure(ops.out, case, case.name)
    prod = ops.out.m[:case.live_rows].clone()
    AH.check_bits(prod, result(native, case, kid), case, f"{case.name}: production choice against forced {AH.KERNEL_NAMES[kid]}")


DET = [(GRIDS[m][3], k) for m in range(5) for k in (AH.K_ATTN, AH.K_ATTN2)]


@pytest.mark.parametrize("case,kernel", DET, ids=[f"{c.name}-{AH.KERNEL_NAMES[k]}" for c, k in DET])
def test_three_launches_are_bit_identical(native, case, kernel):
    first = result(native, case, kernel)
    for _ in range(2):
        AH.check_bits(result(native, case, kernel), first, case, f"{case.name} on {AH.KERNEL_NAMES[kernel]}: two launches")


@pytest.mark.parametrize("kernel", [AH.K_ATTN, AH.K_ATTN2], ids=AH.KERNEL_NAMES[1:3])
@pytest.mark.parametrize("mode", [AH.STEP_SELF, AH.STEP_CROSS], ids=AH.MODE_NAMES[3:])
def test_a_slot_does_not_depend_on_its_batch(native, mode, kernel):
    """The same slots alone, in another slot order and among fewer others: the same bits per slot."""
    case = GRIDS[mode][3]                                                # (7, 10): five slots of mixed fronts and source lengths
    full = result(native, case, kernel)
    rps = case.rps
    for order in [[g] for g in range(case.n_active)] + [list(range(case.n_active))[::-1], [3, 1]]:
        sub = AH.subcase(case, order)
        got = result(native, sub, kernel)
        for i, g in enumerate(order):
            AH.check_bits(got[i * rps:(i + 1) * rps], full[g * rps:(g + 1) * rps], sub, f"{sub.name} on {AH.KERNEL_NAMES[kernel]}: slot {g}")
        _OPS.pop(id(sub), None)


@pytest.mark.parametrize("kernel", [AH.K_ATTN, AH.K_ATTN2], ids=AH.KERNEL_NAMES[1:3])
@pytest.mark.parametrize("mode", [AH.ENC, AH.FULL_SELF, AH.FULL_CROSS], ids=AH.MODE_NAMES[:3])
def test_bits_do_not_depend_on_the_padding(native, mode, kernel):
    """24 real positions padded to 40 and to 64 (a 32-query image against the 64-query one, one staged key tile against two):
    the same bits at the real positions, within each kernel (the order in which a row's keys are summed does not
    depend on how far the batch's padding extends; masked keys add exact zeros)."""
    cross = mode == AH.FULL_CROSS
    small = AH.full_case(DH, mode, CROSS_L if cross else 24, 24 if cross else 0, 3, H=2, dist="ordinary", seed=60 + mode,
                         patterns=["tail", "full", "mid"])
    first = result(native, small, kernel)
    for L2 in (40, 64):
        big = AH.repad(small, L2)
        got = result(native, big, kernel)
        AH.check_values(got, big, big.name)
        for g in range(3):
            if cross:
                a, b = got[g * CROSS_L:(g + 1) * CROSS_L], first[g * CROSS_L:(g + 1) * CROSS_L]
            else:
                real = (small.tok[g] != AH.PAD).cuda()
                a, b = got[g * L2:g * L2 + 24][real], first[g * 24:(g + 1) * 24][real]
            assert a.numel() > 0
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                f"{big.name} against {small.name} on {AH.KERNEL_NAMES[kernel]}: group {g} differs in {int((a != b).sum())} of {a.numel()} values at real positions"
        _OPS.pop(id(big), None)


def _legacy(native, kw, kernel):
    """ttx_debug_attn itself (the entry point without a head dimension) on the keyword arguments of debug_attn."""
    import ctypes as C
    from translation_transformer_amd import _native as N_
    p = lambda t: None if t is None else t.data_ptr()
    kid = C.c_int32(0)
    N_.check(native._lib.ttx_debug_attn(
        native.session, kw["q"].data_ptr(), kw["q"].stride(0), kw["k"].data_ptr(), kw["v"].data_ptr(), kw["k"].stride(0),
        kw["out"].data_ptr(), kw["heads"], kw["scale"], kw["L"], kw["Lk"], p(kw["tok"]), kw["pad"], p(kw["key_pad"]), p(kw["mem_row"]),
        p(kw["act_idx"]), p(kw["front"]), p(kw["src_of"]), p(kw["src_len"]), p(kw.get("kcache")), p(kw.get("vcache")),
        kw.get("cache_seq_stride", 0), p(kw["cache_slot"]), kw["gen_ld"], kw["n"], kw["d"], kw["mode"], kw["groups"], kw["n_active"],
        kw["max_keys"], kernel, C.byref(kid), native._stream()))
    torch.cuda.synchronize()
    return int(kid.value)


HD32 = [A.full_case(A.ENC, 65, 0, 3, dist="ascending", seed=80), A.full_case(A.FULL_SELF, 33, 0, 1, H=2, dist="peaked", seed=81),
        A.full_case(A.FULL_CROSS, 3, 257, 3, dist="offset", seed=82, shared_mem=True),
        A.step_case(A.STEP_SELF, 7, 10, A.grid_slots(4, 5), dist="descending", seed=83, cache_slot=True),
        A.step_case(A.STEP_CROSS, 3, 10, A.grid_slots(2, 5), dist="ordinary", seed=84, src_of=True, src_len=True)]


@pytest.mark.parametrize("case", HD32, ids=[c.name for c in HD32])
def test_head_dim_32_is_ttx_debug_attn(native, case):
    """ttx_debug_attn_hd with head_dim = 32 and ttx_debug_attn: the same kernel, the same bits, for every kernel of the case and
    for the production choice (the step cases have H = 4: k_attn3)."""
    for kernel in [A.K_PROD] + A.kernels_for(case):
        ops, kid = launch(native, case, kernel, make=A.Operands)
        A.check_structure(ops.out, case, case.name)
        new = ops.out.m[:case.live_rows].clone()
        ops.out.reset()
        assert _legacy(native, ops.kw, kernel) == kid, (case.name, kernel)
        A.check_structure(ops.out, case, case.name)
        A.check_bits(ops.out.m[:case.live_rows], new, case, f"{case.name} on {A.KERNEL_NAMES[kid]}: ttx_debug_attn against ttx_debug_attn_hd(32)")
        A.check_values(new, case, case.name)
    _OPS.pop(id(case), None)


@pytest.mark.parametrize("mode", [AH.STEP_SELF, AH.STEP_CROSS], ids=AH.MODE_NAMES[3:])
def test_no_active_slot_writes_nothing(native, mode):
    case = AH.step_case(DH, mode, 3, 10, grid_slots(1, 2), n_active=0, seed=70)
    for kernel in (AH.K_ATTN, AH.K_ATTN2, AH.K_PROD):
        ops, _ = launch(native, case, kernel)
        assert ops.out.untouched(0) is None, f"{case.name} on {AH.KERNEL_NAMES[kernel]}: {ops.out.untouched(0)}"


def test_what_head_dimension_64_cannot_take_is_refused(native):
    from translation_transformer_amd import _native as N_
    h4 = [c for c in GRIDS[AH.STEP_SELF] if c.H == 4][0]
    x4 = [c for c in GRIDS[AH.STEP_CROSS] if c.H == 4][0]
    enc = GRIDS[AH.ENC][3]
    fc = [c for c in GRIDS[AH.FULL_CROSS] if c.Lk == KL + 1][0]
    past = [c for c in GRIDS[AH.STEP_SELF] if c.name.endswith("past-KL")][0]
    bases = {}
    for c in (h4, x4, enc, fc, past):
        result(native, c, AH.K_ATTN)                                     # the base calls are fine
        bases[id(c)] = _OPS[id(c)]
        bases[id(c)].out.reset()

    def refused(case, **kw):
        with pytest.raises(N_.TtxError) as e:
            native.debug_attn(**dict(bases[id(case)].kw, **kw))
        assert e.value.code == N_.TTX_ERR_INVALID, (case.name, list(kw))
        return True

    # k_attn3 / k_attn3s exist at head dimension 32 only: refused, never rerouted, whatever the mode and H
    for c in (h4, x4, enc):
        assert refused(c, kernel=AH.K_ATTN3) and refused(c, kernel=AH.K_ATTN3S), c.name
    assert refused(fc, kernel=AH.K_ATTN2) and refused(past, kernel=AH.K_ATTN2)           # one key beyond what k_attn2 stages
    assert refused(enc, head_dim=16) and refused(enc, head_dim=128) and refused(enc, head_dim=0) and refused(enc, head_dim=48)
    d = enc.d
    narrow = bases[id(enc)].qa.buf[G.GUARD:].as_strided((enc.groups * enc.L, d // 2), (d // 2, 1))   # a leading dimension below d = 64 H
    assert refused(enc, q=narrow) and refused(enc, k=narrow, v=narrow)
    torch.cuda.synchronize()
    for c in (h4, x4, enc, fc, past):
        assert bases[id(c)].out.untouched(0) is None, c.name                             # nothing was launched


def test_attention_table():
    """Prints the achieved errors per kernel and mode (the table of DESIGN.md); runs after the grid above."""
    want = {(k, m) for m in range(5) for k in (AH.K_ATTN, AH.K_ATTN2)}
    assert set(TABLE) == want, "run the whole module: this test reads what the grid measured (all 10 instantiations)"
    print("kernel    mode        e32 (torch fp32)   kernel error   kernel error / tolerance")
    for k, m in sorted(TABLE):
        e32, err, frac = TABLE[(k, m)]
        print(f"{AH.KERNEL_NAMES[k]:<9s} {AH.MODE_NAMES[m]:<11s} {e32:.3e}          {err:.3e}      {frac:.3f}")
        assert frac <= 1.0
