"""Every kernel of csrc/ttx_attn.hip (k_attn, k_attn2, k_attn3, k_attn3s: fourteen instantiations over the five modes) on
operands the test builds, one launch at a time through ttx_debug_attn, against the documented rule in float64.

What is checked, with util_attn_checks (reference, tolerance, operand layout and the checkers; tests/test_attn_checks_host.py
shows on the CPU that each checker can fail):
  structure   rows of slots >= n_active, rows behind the launch and the guard bands keep their fill; every live word is written
  values      max |kernel - float64| <= tol = 4 e32 + (ln nk + 2) 2^-23 max |V| with e32 the error of stock fp32 torch ops on the
              same case: derived in util_attn_checks, not tuned on the kernels
  bits        k_attn3 == k_attn3s; the production choice == the kernel it reports; launch-to-launch determinism; a slot's bits do
              not depend on the other slots of its launch (k_attn2, k_attn3, k_attn3s); k_attn2's bits at the real positions do
              not depend on how far the padding extends

Padding invariance (ENC, FULL_SELF, FULL_CROSS) is claimed for k_attn2 within one query-tile capacity and one workgroup tiling
(L or Lk of 40 against 64).  Observed on the MI355X and asserted here: it holds for every extent k_attn2 serves (24 real
positions padded to 40, 64 and 130; Lk of 24 against 40, 64 and 290) and for k_attn as well (24 against 40, 130 and 390), as the
kernels' fixed key-to-wave and key-to-lane interleaves say it must.  It does not hold ACROSS the two kernels, whose summation
orders differ: a batch padded beyond k_attn2's 384 keys is not bit-identical to the same rows in a narrower batch.

Achieved on an MI355X, worst case of the grid per kernel and mode (printed by test_attention_table; also in DESIGN.md §5).  The
largest errors, torch's own included, come from the cases whose scores sit near +100; the ordinary cases lie near 1e-6:

    kernel    mode        e32 (torch fp32)   kernel error   kernel error / tolerance
    k_attn    ENC         3.37e-05           3.37e-05       0.25
    k_attn    FULL_SELF   3.11e-05           3.11e-05       0.25
    k_attn    FULL_CROSS  1.34e-05           1.87e-05       0.75
    k_attn    STEP_SELF   3.07e-05           3.08e-05       0.32
    k_attn    STEP_CROSS  3.33e-05           3.34e-05       0.25
    k_attn2   ENC         3.37e-05           2.74e-05       0.25
    k_attn2   FULL_SELF   3.11e-05           2.77e-05       0.29
    k_attn2   FULL_CROSS  1.34e-05           2.12e-05       0.49
    k_attn2   STEP_SELF   3.07e-05           3.09e-05       0.41
    k_attn2   STEP_CROSS  3.33e-05           2.68e-05       0.22
    k_attn3   STEP_SELF   3.07e-05           2.54e-05       0.31
    k_attn3   STEP_CROSS  3.33e-05           3.17e-05       0.31
    k_attn3s  STEP_SELF   3.07e-05           2.54e-05       0.31
    k_attn3s  STEP_CROSS  3.33e-05           3.17e-05       0.31
"""
import pytest
import torch

import util_attn_checks as A
import util_gemm_checks as G

pytestmark = pytest.mark.gpu

GRIDS = {m: (A.step_grid(m) if m >= A.STEP_SELF else A.full_grid(m)) for m in range(5)}
ALL_CASES = [c for m in range(5) for c in GRIDS[m]]
RUNS = [(c, k) for c in ALL_CASES for k in A.kernels_for(c)]
TABLE = {}               # (kernel, mode) -> (worst e32, worst kernel error, worst error / tolerance)
_OPS = {}


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; H and the shapes are arguments


def launch(native, case, kernel):
    """One launch into a freshly filled output; returns (operands, kernel id reported)."""
    ops = _OPS.get(id(case))
    if ops is None:
        ops = _OPS[id(case)] = A.Operands(case, "cuda")
        ops.keep = case                                                  # id() stays unique while the operands are cached
    ops.out.reset()
    kid = native.debug_attn(**ops.kw, kernel=kernel)
    torch.cuda.synchronize()
    return ops, kid


def result(native, case, kernel, want_kernel=None):
    ops, kid = launch(native, case, kernel)
    assert kid == (kernel if want_kernel is None else want_kernel), f"{case.name}: asked for {A.KERNEL_NAMES[kernel]}, ran {A.KERNEL_NAMES[kid]}"
    A.check_structure(ops.out, case, f"{case.name} on {A.KERNEL_NAMES[kid]}")
    return ops.out.m[:case.live_rows].clone()


@pytest.mark.parametrize("case,kernel", RUNS, ids=[f"{c.name}-{A.KERNEL_NAMES[k]}" for c, k in RUNS])
def test_kernel_against_fp64(native, case, kernel):
    what = f"{case.name} on {A.KERNEL_NAMES[kernel]}"
    got = result(native, case, kernel)
    r = A.reference(case)
    err_all = (got.cpu().to(torch.float64) - r["ref"][:case.live_rows]).abs()
    print(f"{what}: torch fp32 error {r['e32']:.3e}, kernel error {float(err_all.max()):.3e}, tolerance {r['tol']:.3e} "
          f"(nk {r['nk']}, max |V| {r['vmax']:.2f})")
    err = A.check_values(got, case, what)
    # a query that sees no key: exactly +0.0, not merely small
    dead = r["ref"][:case.live_rows].abs().sum(-1) == 0
    assert not dead.any() or int((got.cpu()[dead].view(torch.int32) != 0).sum()) == 0, f"{what}: a fully masked query is not exactly 0"
    w = TABLE.get((kernel, case.mode), (0.0, 0.0, 0.0))
    TABLE[(kernel, case.mode)] = (max(w[0], r["e32"]), max(w[1], err), max(w[2], err / r["tol"]))


def test_grid_reaches_the_edges():
    """The cases the grid is meant to hold are in it: an all-PAD group and exact-zero queries in every non-step mode, a PAD front
    token at f = 0, k_attn3 tile counts 1, 2, 4, 5 and 9, every score distribution in every mode."""
    for m in range(5):
        assert {c.dist for c in GRIDS[m]} == set(A.DISTS), A.MODE_NAMES[m]
        dead = sum(int((A.attn_ref64(c)[:c.live_rows].abs().sum(-1) == 0).sum()) for c in GRIDS[m])
        assert dead > 0 or m == A.STEP_CROSS, A.MODE_NAMES[m]
    specs = [(c, s) for c in GRIDS[A.STEP_SELF] for s in c.specs[:c.n_active]]
    assert any(s["f"] == 0 and s["front_pad"] for _, s in specs) and any(s["f"] > 0 and s["front_pad"] for _, s in specs)
    assert {s["f"] for _, s in specs} == set(A.F_VALUES) | {110, 230}
    ntiles = set()
    for c, s in specs:
        for r0 in range(0, c.rps, 32):                                   # k_attn3's unit: 32 step rows and the drafts they touch
            last = min(r0 + 32, c.rps) - 1
            drafts = 0 if last == 0 or c.D == 0 else (last - 1) // c.D - (0 if r0 == 0 else (r0 - 1) // c.D) + 1
            ntiles.add((s["f"] + 1 + drafts * c.D + 31) // 32)
    assert {1, 2, 4, 5, 9} <= ntiles, sorted(ntiles)
    assert {s["src"] for c in GRIDS[A.STEP_CROSS] for s in c.specs[:c.n_active]} == set(A.SRC_LENS)


STEP34 = [c for m in (A.STEP_SELF, A.STEP_CROSS) for c in GRIDS[m] if c.H % 4 == 0]


@pytest.mark.parametrize("case", STEP34, ids=[c.name for c in STEP34])
def test_attn3_and_attn3s_are_bit_identical(native, case):
    A.check_bits(result(native, case, A.K_ATTN3), result(native, case, A.K_ATTN3S), case, f"{case.name}: k_attn3 against k_attn3s")


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_production_choice_is_the_kernel_it_reports(native, case):
    ops, kid = launch(native, case, A.K_PROD)
    if case.step:
        assert kid == (A.K_ATTN3 if case.H % 4 == 0 else A.K_ATTN2), (case.name, kid)      # few units: the split kernel
    else:
        assert kid == (A.K_ATTN if case.mode == A.FULL_CROSS and case.Lk > 384 else A.K_ATTN2), (case.name, kid)
    A.check_structure(ops.out, case, case.name)
    prod = ops.out.m[:case.live_rows].clone()
    A.check_bits(prod, result(native, case, kid), case, f"{case.name}: production choice against forced {A.KERNEL_NAMES[kid]}")


DET = [(GRIDS[m][4], k) for m in range(5) for k in A.kernels_for(GRIDS[m][4])]


@pytest.mark.parametrize("case,kernel", DET, ids=[f"{c.name}-{A.KERNEL_NAMES[k]}" for c, k in DET])
def test_launches_are_deterministic(native, case, kernel):
    first = result(native, case, kernel)
    for _ in range(2):
        A.check_bits(result(native, case, kernel), first, case, f"{case.name} on {A.KERNEL_NAMES[kernel]}: two launches")


@pytest.mark.parametrize("kernel", [A.K_ATTN2, A.K_ATTN3, A.K_ATTN3S], ids=A.KERNEL_NAMES[2:])
@pytest.mark.parametrize("mode", [A.STEP_SELF, A.STEP_CROSS], ids=A.MODE_NAMES[3:])
def test_a_slot_does_not_depend_on_its_batch(native, mode, kernel):
    """The same slots alone, in another slot order and among fewer others: the same bits per slot."""
    case = GRIDS[mode][4]                                                # (7, 10): five slots of mixed fronts and source lengths
    full = result(native, case, kernel)
    rps = case.rps
    for order in [[g] for g in range(case.n_active)] + [list(range(case.n_active))[::-1], [3, 1]]:
        sub = A.subcase(case, order)
        got = result(native, sub, kernel)
        for i, g in enumerate(order):
            A.check_bits(got[i * rps:(i + 1) * rps], full[g * rps:(g + 1) * rps], sub, f"{sub.name} on {A.KERNEL_NAMES[kernel]}: slot {g}")
        _OPS.pop(id(sub), None)


# (kernel, real extent, padded extents): the claim; what holds beyond it; the same for k_attn, across k_attn2's 384-key limit
PADDINGS = [(A.K_ATTN2, 40, [64]), (A.K_ATTN2, 24, [40, 64, 130]), (A.K_ATTN, 24, [40, 130, 390])]


@pytest.mark.parametrize("kernel,base,wider", PADDINGS, ids=["k_attn2-40-to-64", "k_attn2-24-to-40-64-130", "k_attn-24-to-40-130-390"])
@pytest.mark.parametrize("mode", [A.ENC, A.FULL_SELF, A.FULL_CROSS], ids=A.MODE_NAMES[:3])
def test_bits_do_not_depend_on_the_padding(native, mode, kernel, base, wider):
    """The same real tokens in a batch padded further give the same bits at the real positions (what scoring's "bit-identical
    across batching, chunking and trimming" rests on).  Claimed for k_attn2 within one query-tile capacity and one workgroup
    tiling (L or Lk of 40 against 64); observed on the MI355X, and asserted here, for every extent either kernel serves: a
    32-query tile against a 64-query one against three workgroups per group, 32 to 288 staged keys, and k_attn up to 390 keys.
    The two kernels do NOT agree with each other in their bits (the k_attn run prints how many values differ): a batch whose
    extent crosses k_attn2's 384 keys changes kernel and with it the summation order."""
    cross = mode == A.FULL_CROSS
    small = A.full_case(mode, 3 if cross else base, base if cross else 0, 3, dist="ordinary", seed=60 + mode,
                        patterns=["tail", "full", "mid"])
    first = result(native, small, kernel)
    if kernel == A.K_ATTN:
        other = result(native, small, A.K_ATTN2)
        print(f"{small.name}: k_attn and k_attn2 differ in {int((other != first).sum())} of {first.numel()} values "
              f"(largest difference {float((other - first).abs().max()):.3e})")
    for L2 in wider:
        L2 = 290 if cross and L2 == 130 and kernel == A.K_ATTN2 else L2
        big = A.repad(small, L2)
        got = result(native, big, kernel)
        A.check_values(got, big, big.name)
        for g in range(3):
            if cross:
                a, b = got[g * 3:(g + 1) * 3], first[g * 3:(g + 1) * 3]
            else:
                real = (small.tok[g] != A.PAD).cuda()
                a, b = got[g * L2:g * L2 + base][real], first[g * base:(g + 1) * base][real]
            assert a.numel() > 0
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                f"{big.name} against {small.name} on {A.KERNEL_NAMES[kernel]}: group {g} differs in {int((a != b).sum())} of {a.numel()} values at real positions"
        _OPS.pop(id(big), None)


@pytest.mark.parametrize("mode", [A.STEP_SELF, A.STEP_CROSS], ids=A.MODE_NAMES[3:])
def test_attn3s_streams_more_units_than_waves(native, mode):
    """One k_attn3s launch with about 1.5 units per wave of its grid: every wave carries its state (running maximum, sum, output,
    prefetched tile and queries, the next unit's scalars) from one unit into a next one of another front, tile count and source
    length.  Checked against float64, and bit for bit against k_attn3, which has one workgroup per unit and nothing to carry."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    case = A.stream_case(mode, n_cu)
    units = case.n_active * case.H * 2
    assert 8 * n_cu < units < 16 * n_cu and units % (8 * n_cu) not in (0, 4 * n_cu)
    step = max(1, n_cu // 2)
    s = case.specs
    assert all(s[g]["f"] != s[g + step]["f"] and s[g]["src"] != s[g + step]["src"] for g in range(len(s) - step))
    streamed = result(native, case, A.K_ATTN3S)
    err = A.check_values(streamed, case, f"{case.name} on k_attn3s")
    r = A.reference(case)
    print(f"{case.name}: {units} units on {8 * n_cu} waves, kernel error {err:.3e}, tolerance {r['tol']:.3e}")
    A.check_bits(streamed, result(native, case, A.K_ATTN3), case, f"{case.name}: k_attn3s against k_attn3")
    _OPS.pop(id(case), None)


@pytest.mark.parametrize("mode", [A.STEP_SELF, A.STEP_CROSS], ids=A.MODE_NAMES[3:])
def test_no_active_slot_writes_nothing(native, mode):
    case = A.step_case(mode, 3, 10, A.grid_slots(1, 2), n_active=0, seed=70)
    for kernel in A.kernels_for(case) + [A.K_PROD]:
        ops, _ = launch(native, case, kernel)
        assert ops.out.untouched(0) is None, f"{case.name} on {A.KERNEL_NAMES[kernel]}: {ops.out.untouched(0)}"


def test_invalid_arguments_are_refused(native):
    from translation_transformer_amd import _native as N_
    step = GRIDS[A.STEP_SELF][2]
    cross = GRIDS[A.STEP_CROSS][2]
    enc = GRIDS[A.ENC][3]
    fc385 = [c for c in GRIDS[A.FULL_CROSS] if c.Lk == 385][0]
    h2 = [c for c in GRIDS[A.STEP_SELF] if c.H == 2][0]
    bases = {}
    for c in (step, cross, enc, fc385, h2):
        result(native, c, A.K_ATTN)                                      # the base calls are fine
        bases[id(c)] = _OPS[id(c)]
        bases[id(c)].out.reset()

    def refused(case, **kw):
        with pytest.raises(N_.TtxError) as e:
            native.debug_attn(**dict(bases[id(case)].kw, **kw))
        assert e.value.code == N_.TTX_ERR_INVALID, (case.name, list(kw))
        return True

    for case, required in ((step, ["q", "k", "v", "out", "tok", "act_idx", "front", "kcache", "vcache"]),
                           (cross, ["q", "k", "v", "out", "key_pad", "act_idx"]), (enc, ["q", "k", "v", "out", "tok"]),
                           (fc385, ["q", "k", "v", "out", "key_pad"])):
        for name in required:
            if name in ("q", "k", "v", "out"):                           # the wrapper reads their strides: go through the C entry point
                continue
            assert refused(case, **{name: None}), name
    kw = bases[id(enc)].kw
    lib = native._lib
    z = kw["q"].data_ptr()
    for hole in range(4):                                                # q, k, v, out in turn
        ptrs = [kw["q"].data_ptr(), kw["k"].data_ptr(), kw["v"].data_ptr(), kw["out"].data_ptr()]
        ptrs[hole] = None
        rc = lib.ttx_debug_attn(native.session, ptrs[0], kw["q"].stride(0), ptrs[1], ptrs[2], kw["k"].stride(0), ptrs[3], enc.H, A.SCALE,
                                enc.L, 0, kw["tok"].data_ptr(), 0, None, None, None, None, None, None, None, None, 0, None, 0, 1, 0,
                                A.ENC, enc.groups, 0, enc.L, 0, None, None)
        assert rc == N_.TTX_ERR_INVALID, hole
    assert z and refused(enc, heads=0) and refused(enc, heads=-4) and refused(enc, mode=5) and refused(enc, kernel=5)
    qa = bases[id(enc)].qa
    d = enc.d
    odd = qa.buf[G.GUARD:].as_strided((enc.groups * enc.L, d), (3 * d - 2, 1))          # a leading dimension that is no multiple of 4
    assert refused(enc, q=odd) and refused(enc, k=odd, v=odd)
    off = qa.buf[G.GUARD + 1:].as_strided((enc.groups * enc.L - 1, d), (3 * d, 1))      # not 16-byte aligned
    assert refused(enc, q=off) and refused(enc, k=off) and refused(enc, v=off[:, :]) and refused(enc, out=bases[id(enc)].out.buf[G.GUARD + 2:])
    kc = bases[id(step)].kc
    assert refused(step, kcache=kc.buf[G.GUARD + 3:]) and refused(step, vcache=kc.buf[G.GUARD + 1:])
    assert refused(step, n_active=-1) and refused(step, n_active=step.groups + 1) and refused(cross, n_active=cross.groups + 1)
    assert refused(enc, max_keys=enc.L - 1) and refused(cross, max_keys=cross.Lk - 1)
    # a forced kernel that cannot serve the request is refused, never rerouted
    assert refused(enc, kernel=A.K_ATTN3) and refused(enc, kernel=A.K_ATTN3S)            # not a step mode
    assert refused(h2, kernel=A.K_ATTN3) and refused(h2, kernel=A.K_ATTN3S)              # H % 4 != 0
    assert refused(step, kernel=A.K_ATTN3, max_keys=16 * 32)                             # 17 parked tile partials: more than 64 KB
    assert refused(fc385, kernel=A.K_ATTN2)                                              # 416 staged keys: beyond the 384 of its registers
    assert refused(step, kernel=A.K_ATTN2, max_keys=400)
    assert refused(step, kernel=A.K_ATTN, max_keys=3000)                                 # scores beyond k_attn's LDS limit
    assert refused(fc385, kernel=A.K_ATTN2, max_keys=1200, Lk=385)                       # k_attn2's LDS limit as well
    torch.cuda.synchronize()
    for c in (step, cross, enc, fc385, h2):
        assert bases[id(c)].out.untouched(0) is None, c.name                             # nothing was launched


def test_attention_table():
    """Prints the achieved errors per kernel and mode (the table of DESIGN.md); runs after the grid above."""
    want = {(k, m) for m in range(5) for k in (A.K_ATTN, A.K_ATTN2)} | {(k, m) for m in (3, 4) for k in (A.K_ATTN3, A.K_ATTN3S)}
    assert set(TABLE) == want, "run the whole module: this test reads what the grid measured (all 14 instantiations)"
    print("kernel    mode        e32 (torch fp32)   kernel error   kernel error / tolerance")
    for k, m in sorted(TABLE):
        e32, err, frac = TABLE[(k, m)]
        print(f"{A.KERNEL_NAMES[k]:<9s} {A.MODE_NAMES[m]:<11s} {e32:.3e}          {err:.3e}      {frac:.3f}")
        assert frac <= 1.0
