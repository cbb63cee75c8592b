"""k_attn1 (csrc/ttx_attn.hip): the attention of a step launch with ONE row per slot, the (N, D) = (1, 0) layout of the probe of a
two-phase verify step.  It runs on the VALU the fmaf chains the 32x32 MFMA tiles of k_attn3 / k_attn3s contract, in their order,
so every check of bits is exact equality with those two kernels; values are checked against float64 with the tolerance
tests/util_attn_checks.py derives.

  bits          forced 5 == forced k_attn3s == forced k_attn3, STEP_SELF and STEP_CROSS, H 4 and 8, every score distribution:
                fronts {0, 1, 30, 31, 32, 33, 63, 64, 65, 110, 200, 230} (1 to 8 key tiles, nk on both sides of a tile edge), the
                source lengths of A.SRC_LENS, a PAD front token at f = 0 (nothing visible: zeros) and at f > 0, PAD tokens inside
                prefix and source, a slot whose whole third tile is PAD between real tiles (a fold that changes nothing), dead
                slots behind the live ones, cache_slot and src_of indirection
  row 0         of a (3, 10), (7, 10), (2, 16) launch on k_attn3s == the (1, 0) launch on k_attn1
  batch         a slot's bits do not depend on the other slots of its launch; three launches give the same bits
  launch rule   256 slots x 4 heads take k_attn1 and 255 the split kernel k_attn3; TTX_ATTN_ROW=0 keeps k_attn3s, TTX_ATTN_ROW=1
                takes k_attn1 for five slots; the production choice gives the bits of the kernel it reports
  refusals      forced 5 outside the step modes, with H % 4 != 0, at head dimension 64, with N * D > 0; ttx_debug_attn_select
  end to end    the trained four-head model: slot pool with every step split, capacities 3 and 64, graphs and eager,
                TTX_ATTN_ROW=1 against =0, with the kernels the session dispatched read back (ttx_debug_attn_kernels_seen: k_attn1
                ran under =1 and not under =0); plain greedy generate; one pool run on NaN-filled workspaces (a child process)

k_attn1 gives a wave one (slot, pair of heads) and walks nothing: there is no unit stream to test.
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import util_attn_checks as A
import util_attn_hd as AH
import util_draft_select as S
import util_gemm_checks as G
from test_gpu_two_phase import COUNTERS, LAYOUTS, fixture_rows, layout_cases, pool_call, row0_case
from util_models import BOS, EOS, PAD, fixture_tokens, tiny_state, upto_eos

pytestmark = pytest.mark.gpu
DEV = "cuda"
K_ATTN_ROW = 5
NAMES = A.KERNEL_NAMES + ["k_attn1"]
MODES = [A.STEP_SELF, A.STEP_CROSS]
MODE_IDS = A.MODE_NAMES[3:]
FRONTS = [0, 1, 30, 31, 32, 33, 63, 64, 65, 110, 200, 230]
HOLE = 192            # a prefix / source of 192 positions with PADs "mid": positions 64 .. 96 are PAD, the whole tile of keys 64 .. 95


def row_slots(i):
    """Every front of FRONTS, the source lengths walking A.SRC_LENS from i on; slot 0 (f = 0) and slot 5 (f = 33) have a PAD front
    token, slots 8, 11 (f = 65, 230) PADs inside prefix and source; the last slot has its third key tile all PAD."""
    slots = [dict(f=f, src=A.SRC_LENS[(i + j) % len(A.SRC_LENS)], front_pad=j in (0, 5), prefix_pads=j in (8, 11)) for j, f in enumerate(FRONTS)]
    slots[10]["src"] = 70                                                 # f = 200: the longest of A.SRC_LENS in every case
    return slots + [dict(f=HOLE, src=HOLE, prefix_pads=True)]


def _grid():
    cases = []
    for mode in MODES:
        for hi, H in enumerate((4, 8)):
            for i, dist in enumerate(A.DISTS):
                cases.append(A.step_case(mode, 1, 0, row_slots(i), H=H, dist=dist, seed=300 + 10 * hi + i, extra_groups=1 + i % 2,
                                         cache_slot=True, src_of=True, src_len=bool((i + hi) % 2)))
    return cases


GRID = _grid()
_OPS = {}


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def native(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; H and the shapes are arguments


def launch(native, case, kernel, make=A.Operands):
    ops = _OPS.get(id(case))
    if ops is None:
        ops = _OPS[id(case)] = make(case, DEV)
        ops.keep = case
    ops.out.reset()
    kid = native.debug_attn(**ops.kw, kernel=kernel)
    torch.cuda.synchronize()
    return ops, kid


def result(native, case, kernel, want_kernel=None):
    ops, kid = launch(native, case, kernel)
    want = kernel if want_kernel is None else want_kernel
    assert kid == want, f"{case.name}: asked for {NAMES[kernel]}, expected {NAMES[want]}, ran {NAMES[kid]}"
    A.check_structure(ops.out, case, f"{case.name} on {NAMES[kid]}")       # rows of dead slots and the guard bands keep their fill
    return ops.out.m[:case.live_rows].clone()


def test_grid_reaches_the_edges():
    assert {c.dist for c in GRID} == set(A.DISTS) and {c.H for c in GRID} == {4, 8}
    for c in GRID:
        assert c.n_active < c.groups and c.rps == 1
        specs = c.specs
        assert [s["f"] for s in specs[:len(FRONTS)]] == FRONTS
        assert specs[0]["f"] == 0 and specs[0]["front_pad"] and specs[5]["f"] > 0 and specs[5]["front_pad"]
        b = int(c.act_idx[len(specs) - 1])                                   # the slot with the hole
        if c.mode == A.STEP_SELF:
            assert c.cache_slot is not None and not torch.equal(c.cache_slot, torch.arange(len(c.cache_slot), dtype=torch.int32))
            real = c.tok[b, :HOLE + 1] != A.PAD
        else:
            assert c.src_of is not None
            real = c.key_pad[int(c.src_of[b]), :HOLE] != 0
        assert not real[64:96].any() and real[32:64].any() and real[96:128].any(), "the third key tile is not a PAD tile between real ones"
        dead = A.attn_ref64(c)[:c.live_rows].abs().sum(-1) == 0
        assert bool(dead[0]) == (c.mode == A.STEP_SELF)                      # f = 0 with a PAD front token: nothing visible
    assert {s["src"] for c in GRID if c.mode == A.STEP_CROSS for s in c.specs[:len(FRONTS)]} == set(A.SRC_LENS)
    assert any(c.src_len is None for c in GRID if c.mode == A.STEP_CROSS) and any(c.src_len is not None for c in GRID if c.mode == A.STEP_CROSS)


@pytest.mark.parametrize("case", GRID, ids=[c.name for c in GRID])
def test_bits_equal_attn3s_and_attn3_and_values_float64(native, case):
    got = result(native, case, K_ATTN_ROW)
    r = A.reference(case)
    err = A.check_values(got, case, f"{case.name} on k_attn1")
    print(f"{case.name}: torch fp32 error {r['e32']:.3e}, kernel error {err:.3e}, tolerance {r['tol']:.3e} (nk {r['nk']}, max |V| {r['vmax']:.2f})")
    dead = r["ref"][:case.live_rows].abs().sum(-1) == 0                       # a query that sees no key: exactly +0.0
    assert int((got.cpu()[dead].view(torch.int32) != 0).sum()) == 0, f"{case.name}: a fully masked query is not exactly 0"
    A.check_bits(got, result(native, case, A.K_ATTN3S), case, f"{case.name}: k_attn1 against k_attn3s")
    A.check_bits(got, result(native, case, A.K_ATTN3), case, f"{case.name}: k_attn1 against k_attn3")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_row0_of_a_full_step_is_the_one_row_launch(native, mode):
    """What the two-phase step rests on (tests/test_gpu_two_phase.py): row 0 of a slot in the (N, D) launch, here on k_attn3s,
    equals the slot's row in the (1, 0) launch on k_attn1, bit for bit."""
    cases = layout_cases(32, mode)
    assert {(c.N, c.D) for c in cases} == set(LAYOUTS)
    for case in cases:
        outs = []
        for c, kernel in ((case, A.K_ATTN3S), (row0_case(case), K_ATTN_ROW)):
            ops = A.Operands(c, DEV)
            kid = native.debug_attn(**ops.kw, kernel=kernel)
            torch.cuda.synchronize()
            assert kid == kernel, (c, kid)
            A.check_structure(ops.out, c, f"{c} on {NAMES[kernel]}")
            outs.append(ops.out.m[:c.live_rows].clone())
        full, probe = outs
        A.check_bits(full[::case.rps].contiguous(), probe, case, f"{case}: row 0 on k_attn3s against the (1, 0) launch on k_attn1")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_slot_does_not_depend_on_its_batch(native, mode):
    """The same slots alone, in reversed order and among fewer others: the same bits per slot."""
    case = [c for c in GRID if c.mode == mode and c.H == 8][1]
    full = result(native, case, K_ATTN_ROW)
    n = case.n_active
    for order in [[g] for g in range(n)] + [list(range(n))[::-1], [3, 1], [12, 0, 11]]:
        sub = A.subcase(case, order)
        got = result(native, sub, K_ATTN_ROW)
        for i, g in enumerate(order):
            A.check_bits(got[i:i + 1], full[g:g + 1], sub, f"{sub.name} on k_attn1: slot {g}")
        _OPS.pop(id(sub), None)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_launches_are_deterministic(native, mode):
    case = [c for c in GRID if c.mode == mode and c.H == 4][0]
    first = result(native, case, K_ATTN_ROW)
    for _ in range(2):
        A.check_bits(result(native, case, K_ATTN_ROW), first, case, f"{case.name} on k_attn1: two launches")


# -- launch rule -----------------------------------------------------------------------------------------------------------------
_BIG = {}


def big_case(mode):
    """256 slots x 4 heads = 1 024 units, the size from which a launch leaves the split kernel; short keys."""
    if mode not in _BIG:
        slots = [dict(f=A.F_VALUES[g % 6], src=A.SRC_LENS[g % 4], front_pad=(g % 11 == 3), prefix_pads=(g % 7 == 2)) for g in range(256)]
        _BIG[mode] = A.step_case(mode, 1, 0, slots, H=4, dist="ordinary", seed=400, cache_slot=True, src_len=True, name=f"{A.MODE_NAMES[mode]}-256-slots")
    return _BIG[mode]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_launch_rule(tta, native, monkeypatch, mode):
    big = big_case(mode)
    assert big.groups * big.H == 1024
    prod = result(native, big, A.K_PROD, want_kernel=K_ATTN_ROW)             # 1 024 units: the launch k_attn3s used to get
    A.check_values(prod, big, f"{big.name} on k_attn1")
    A.check_bits(prod, result(native, big, K_ATTN_ROW), big, f"{big.name}: production choice against forced k_attn1")
    A.check_bits(prod, result(native, big, A.K_ATTN3S), big, f"{big.name}: k_attn1 against k_attn3s")
    small = A.subcase(big, list(range(255)))                                 # 1 020 units: the split kernel, as before
    got = result(native, small, A.K_PROD, want_kernel=A.K_ATTN3)
    A.check_bits(got, prod[:255], small, f"{small.name}: k_attn3 against the same slots of the larger launch")
    five = A.step_case(mode, 1, 0, A.grid_slots(2, 5), H=4, dist="peaked", seed=410, src_of=True)
    st, cfg = tiny_state()
    for flag, case, want in (("0", big, A.K_ATTN3S), ("0", five, A.K_ATTN3), ("1", five, K_ATTN_ROW), ("1", big, K_ATTN_ROW)):
        monkeypatch.setenv("TTX_ATTN_ROW", flag)                             # read when the session is created
        model = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
        monkeypatch.delenv("TTX_ATTN_ROW")
        got = result(model, case, A.K_PROD, want_kernel=want)
        A.check_bits(got, result(model, case, want), case, f"{case.name}, TTX_ATTN_ROW={flag}: production choice against forced {NAMES[want]}")
        A.check_bits(got, result(native, case, K_ATTN_ROW), case, f"{case.name}, TTX_ATTN_ROW={flag}: against k_attn1")
        model.close()
    # a one-row launch with drafts in its layout is no one-row launch: TTX_ATTN_ROW=1 leaves it where it was
    monkeypatch.setenv("TTX_ATTN_ROW", "1")
    model = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    monkeypatch.delenv("TTX_ATTN_ROW")
    drafts = layout_cases(32, mode)[0]
    assert launch(model, drafts, A.K_PROD)[1] == A.K_ATTN3
    model.close()
    for c in (small, five, drafts):
        _OPS.pop(id(c), None)


# -- refusals --------------------------------------------------------------------------------------------------------------------
def test_a_forced_row_kernel_is_refused_where_it_cannot_serve(tta, native):
    slots = A.grid_slots(1, 3)
    enc = A.full_case(A.ENC, 17, 0, 3, seed=500)
    full_cross = A.full_case(A.FULL_CROSS, 3, 33, 3, seed=501)
    h2 = A.step_case(A.STEP_SELF, 1, 0, slots, H=2, seed=502)
    h6 = A.step_case(A.STEP_CROSS, 1, 0, slots, H=6, seed=503)
    hd64 = [AH.step_case(64, m, 1, 0, slots, H=4, seed=504) for m in MODES]
    drafts = [A.step_case(m, N, D, slots, H=4, seed=505) for m in MODES for N, D in ((3, 10), (1, 1))]
    for case in [enc, full_cross, h2, h6] + hd64 + drafts:
        make = AH.Operands if hasattr(case, "dh") else A.Operands
        ops, kid = launch(native, case, A.K_PROD, make)                      # the case itself is fine
        assert kid in (A.K_ATTN, A.K_ATTN2, A.K_ATTN3), (case.name, kid)
        ops.out.reset()
        with pytest.raises(tta.TtxError) as e:
            native.debug_attn(**ops.kw, kernel=K_ATTN_ROW)
        assert e.value.code == -1, case.name
        with pytest.raises(tta.TtxError):
            native.debug_attn(**ops.kw, kernel=6)
        torch.cuda.synchronize()
        assert ops.out.untouched(0) is None, f"{case.name}: a refused launch wrote {ops.out.untouched(0)}"
    # draft select keeps refusing everything but 0 / 3 / 4
    case = layout_cases(32, A.STEP_SELF)[0]
    ops = A.Operands(case, DEV)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    mask, base = i32(1, 2, 3, 4, 5), i32(0, 11, 22, 43, 54)
    assert native.debug_attn_select(**ops.kw, kernel=A.K_ATTN3S, row_base=base, draft_mask=mask) == A.K_ATTN3S
    ops.out.reset()
    with pytest.raises(tta.TtxError) as e:
        native.debug_attn_select(**ops.kw, kernel=K_ATTN_ROW, row_base=base, draft_mask=mask)
    assert e.value.code == -1
    torch.cuda.synchronize()
    G.check_untouched(ops.out, 0, "ttx_debug_attn_select with kernel 5")


# -- end to end --------------------------------------------------------------------------------------------------------------------
def row_forms(tta, monkeypatch, run, no_graph=False):
    """``run(model)`` on models created under TTX_ATTN_ROW=0 and =1 (every step of a pool call split)."""
    if no_graph:
        monkeypatch.setenv("TTX_NO_GRAPH", "1")
    monkeypatch.setenv("TTX_TWO_PHASE", "1")
    monkeypatch.setenv("TTX_TWO_PHASE_MIN_ROWS", "0")
    st, cfg = S.h4_state()
    res = []
    for flag in ("0", "1"):
        monkeypatch.setenv("TTX_ATTN_ROW", flag)
        model = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
        res.append(run(model))
        model.close()
    return res


@pytest.mark.parametrize("no_graph", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("capacity,n_rows", [(3, 12), (64, 150)])
def test_pool_is_unchanged_by_the_row_kernel(tta, monkeypatch, capacity, n_rows, no_graph):
    """The trained four-head model (head dimension 32: its step attention is k_attn3 / k_attn3s, its probes k_attn1 under
    TTX_ATTN_ROW=1): outputs, traces, finishing steps and every counter identical, the golden tokens up to EOS."""
    gold = S.h4_gen()["b1_n3_d10_tokens"]
    rows, idx, c = fixture_rows(n_rows, seed=capacity)
    run = lambda model: pool_call(tta, model, rows, capacity, 150, 3, 10, c) + (model.pool_last_counters(), model.attn_kernels_seen())
    (rc0, out0, traj0, fin0, st0, cnt0, seen0), (rc1, out1, traj1, fin1, st1, cnt1, seen1) = row_forms(tta, monkeypatch, run, no_graph)
    assert rc0 == rc1 == 0
    # the switch reached the pool's steps: the probes ran on k_attn1 under =1 (the draft passes and the encoder on their own
    # kernels), on no launch under =0
    assert K_ATTN_ROW in seen1 and A.K_ATTN3 in seen1 and K_ATTN_ROW not in seen0 and A.K_ATTN3 in seen0, (seen0, seen1)
    assert torch.equal(out0, out1) and torch.equal(traj0, traj1) and torch.equal(fin0, fin1)
    for k in COUNTERS + ["verified_positions"]:
        assert getattr(st0, k) == getattr(st1, k), k
    assert cnt0 == cnt1 and cnt1["steps"] == cnt1["split_steps"] == st1.model_calls > 0      # every step ran a probe
    out = out1.cpu().numpy()
    for j, r in enumerate(idx):
        assert upto_eos(out[j]) == upto_eos(gold[r, 0]), (capacity, r)


def test_greedy_generate_is_unchanged_by_the_row_kernel(tta, monkeypatch):
    """Plain greedy decoding is a (1, 0) step per token: under TTX_ATTN_ROW=1 every one of them runs on k_attn1."""
    src, _, _, _ = fixture_tokens()
    src = src[:, :int((src != PAD).sum(1).max())]
    run = lambda model: (tta.TranslationInferenceGreedy(model, 150, PAD, BOS, EOS).generate(src), model.attn_kernels_seen())
    (a, seen0), (b, seen1) = row_forms(tta, monkeypatch, run)
    assert torch.equal(a, b)
    assert seen0 == {A.K_ATTN2, A.K_ATTN3} and seen1 == {A.K_ATTN2, K_ATTN_ROW}, (seen0, seen1)      # encoder; every step
    assert int((a != PAD).sum()) > a.shape[0]                                 # it decoded something


CHILD = r"""
import sys, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import translation_transformer_amd as tta
import util_draft_select as S
from test_gpu_two_phase import fixture_rows, pool_call
st, cfg = S.h4_state()
rows, idx, c = fixture_rows(12, seed=3)
model = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
rc, out, traj, fin, stats = pool_call(tta, model, rows, 3, 150, 3, 10, c)
assert rc == 0
torch.save(dict(out=out.cpu(), traj=traj.cpu(), fin=fin.cpu()), %(dump)r)
print("poisoned row-kernel run ok")
"""


def test_pool_on_poisoned_workspaces(tta, monkeypatch, tmp_path):
    """TTX_POISON_WORKSPACES=1 (read when the library first allocates: a child process) with every probe on k_attn1: the keys a
    tile holds past nk are clamped loads of finite data, so the outputs are those of the run without the poison."""
    root = Path(__file__).resolve().parent.parent
    dump = tmp_path / "poisoned.pt"
    env = dict(os.environ, TTX_POISON_WORKSPACES="1", TTX_ATTN_ROW="1", TTX_TWO_PHASE="1", TTX_TWO_PHASE_MIN_ROWS="0")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": str(root), "tests": str(root / "tests"), "dump": str(dump)}], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "poisoned row-kernel run ok" in r.stdout
    got = torch.load(dump)
    rows, idx, c = fixture_rows(12, seed=3)
    run = lambda model: pool_call(tta, model, rows, 3, 150, 3, 10, c)
    _, (rc, out, traj, fin, _) = row_forms(tta, monkeypatch, run)
    assert rc == 0
    assert torch.equal(got["out"], out.cpu()) and torch.equal(got["traj"], traj.cpu()) and torch.equal(got["fin"], fin.cpu())
