"""The two-phase verify step of the slot pool (DESIGN.md "Two-phase verify step"): a probe over the front rows of all live slots,
the full step on the slots whose probe prediction equals the first token of one of their drafts, and the merge that hands
k_accept the predictions in the layout it reads.  Every check is exact equality.

  row 0 across layouts   the identity the split rests on: row 0 of a slot in an (N, D) launch == the row of the same slot in the
                         (1, 0) launch on the same cache, bit for bit, for every kernel that serves the step modes (k_attn3,
                         k_attn3s, k_attn2, k_attn at head dimension 32; k_attn2, k_attn at 64), STEP_SELF and STEP_CROSS, fronts
                         {0, 1, 30, 31, 32, 33, 63, 64, 65, 200} and source lengths {1, 31, 32, 33, 70} over five slots a launch
  k_probe_split,         against tests/util_two_phase.py: no match, all match, the last draft only, two drafts sharing the token, the
  k_merge_pred           replacement token, a permuted active list; 0, 1, 3, 257 and 1 100 live slots (one round of 256 threads,
                         one and two rounds of 1 024); entries past the counts untouched, guard margins intact
  k_kvcopy               with the indirection: probe row 0 for a slot without a match, the draft pass's rows for a matching one,
                         nothing else written, null pointers == ttx_debug_kvcopy
  kernel choice          where an (N, D) launch runs on k_attn and a (1, 0) launch alone would take k_attn2, the probe chooses as the
                         (N, D) layout does (production choice, kernel = 0): same kernel id, same bits; end to end at such a max_len
  end to end             ttx_greedy_speculative_generate_pool and generate_many(reorder=True) with every step split
                         (TTX_TWO_PHASE_MIN_ROWS=0) against TTX_TWO_PHASE=0: outputs, traces and counters identical, the golden
                         tokens, verified_positions == the executed rows read off the traces, both branches taken
"""
import ctypes as C

import numpy as np
import pytest
import torch

import util_attn_checks as A
import util_attn_hd as AH
import util_loop_checks as U
import util_two_phase as T
from util_hd64 import hd64_gen, hd64_state
from util_models import BOS, EOS, PAD, fixture_tokens, full_state, load_npz, tiny_state, upto_eos

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def native(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


# -- row 0 across layouts ------------------------------------------------------------------------------------------------------
FRONTS = [[0, 30, 32, 63, 200], [1, 31, 33, 64, 65]]
SRC_LENS = [1, 31, 32, 33, 70]
LAYOUTS = [(3, 10), (7, 10), (2, 16)]
ROW0_RUNS = [(32, A.K_ATTN3), (32, A.K_ATTN3S), (32, A.K_ATTN2), (32, A.K_ATTN), (64, A.K_ATTN2), (64, A.K_ATTN)]


_LAYOUT_CASES = {}


def layout_cases(dh, mode):
    if (dh, mode) not in _LAYOUT_CASES:
        _LAYOUT_CASES[dh, mode] = _layout_cases(dh, mode)
    return _LAYOUT_CASES[dh, mode]


def _layout_cases(dh, mode):
    """Five slots with different fronts and source lengths, slot 1 with a PAD front token and slot 2 with PADs inside its prefix
    and source, for every layout; the operands follow util_attn_checks' guard conventions (NaN where nothing may be read)."""
    cases = []
    for i, fronts in enumerate(FRONTS):
        slots = [dict(f=f, src=SRC_LENS[(j + i) % 5], front_pad=(j == 1), prefix_pads=(j == 2)) for j, f in enumerate(fronts)]
        for N, D in LAYOUTS:
            kw = dict(dist=AH.DISTS[(i + N) % 5], seed=40 + i, cache_slot=bool(i), src_len=not i, src_of=bool(i))
            cases.append(A.step_case(mode, N, D, slots, H=4, **kw) if dh == 32 else AH.step_case(dh, mode, N, D, slots, H=2, **kw))
    return cases


def row0_case(case):
    """The (1, 0) launch over the same slots, caches and sources: every slot's row 0 alone."""
    rows = torch.arange(case.groups) * case.rps
    kw = {k: v for k, v in case.__dict__.items() if k not in ("_ref", "d", "dh")}
    kw.update(N=1, D=0, q=case.q[rows].clone(), name=f"{case.name}[row 0 as (1, 0)]")
    if case.mode == A.STEP_SELF:
        kw.update(k=case.k[rows].clone(), v=case.v[rows].clone())
    return AH.Case(case.dh, **kw) if hasattr(case, "dh") else A.Case(**kw)


@pytest.mark.parametrize("mode", [A.STEP_SELF, A.STEP_CROSS], ids=["STEP_SELF", "STEP_CROSS"])
@pytest.mark.parametrize("dh,kernel", ROW0_RUNS, ids=[f"dh{d}-{A.KERNEL_NAMES[k]}" for d, k in ROW0_RUNS])
def test_row0_is_the_same_in_every_layout(native, dh, kernel, mode):
    make = A.Operands if dh == 32 else AH.Operands
    for case in layout_cases(dh, mode):
        outs = []
        for c in (case, row0_case(case)):
            ops = make(c, DEV)
            kid = native.debug_attn(**ops.kw, kernel=kernel)
            torch.cuda.synchronize()
            assert kid == kernel, (c, kid)
            A.check_structure(ops.out, c, f"{c} on {A.KERNEL_NAMES[kernel]}")
            outs.append(ops.out.m[:c.live_rows].clone())
        full, probe = outs
        A.check_bits(full[::case.rps].contiguous(), probe, case, f"{case} on {A.KERNEL_NAMES[kernel]}: row 0 against the (1, 0) launch")


WINDOW = [(64, 3, 10), (32, 3, 10), (64, 7, 10)]


@pytest.mark.parametrize("dh,N,D", WINDOW, ids=[f"dh{w[0]}-N{w[1]}-D{w[2]}" for w in WINDOW])
def test_probe_takes_the_kernel_the_full_layout_takes(tta, native, dh, N, D):
    """The production choice (kernel = 0) where the two layouts alone would disagree: a cache capacity at which the (N, D) launch
    stages more keys than k_attn2 holds and runs on k_attn, while a (1, 0) launch on the same cache still fits k_attn2.  The two
    kernels do not give the same bits, so the probe chooses as the (N, D) layout does: same kernel id, same bits in row 0."""
    KL = int(tta.lib().ttx_attn_staged_key_limit(dh, 1 + N * D))
    draft = min(N, (64 + D - 2) // D + 1) * D
    cap = KL - 1 - draft + 5                                        # (N, D): cap + 1 + draft = KL + 5 keys; (1, 0): cap + 1 <= KL
    slots = [dict(f=0, src=1), dict(f=33, src=33, front_pad=True), dict(f=cap - 3, src=70, prefix_pads=True)]
    case = AH.step_case(dh, A.STEP_SELF, N, D, slots, H=2, dist="ordinary", seed=77, cache_len=cap)
    probe = row0_case(case)
    assert AH.staged_keys(case) > KL >= AH.staged_keys(probe)
    ops_f, ops_p = AH.Operands(case, DEV), AH.Operands(probe, DEV)
    kid_f = native.debug_attn(**ops_f.kw, kernel=0)
    kid_alone = native.debug_attn(**ops_p.kw, kernel=0)
    torch.cuda.synchronize()
    assert (kid_f, kid_alone) == (A.K_ATTN, A.K_ATTN2), "the capacity does not lie where the layouts disagree"
    ops_p.out.reset()
    kid_p = native.debug_attn(**ops_p.kw, kernel=0, choose_as=(N, D))
    torch.cuda.synchronize()
    assert kid_p == kid_f
    A.check_structure(ops_p.out, probe, f"{probe}")
    A.check_bits(ops_f.out.m[:case.live_rows:case.rps].contiguous(), ops_p.out.m[:probe.live_rows].clone(), case,
                 f"{case}: row 0 against the (1, 0) launch that chooses as ({N}, {D})")
    # where both layouts fit k_attn2 the choice is k_attn2 with and without the hint
    low = AH.step_case(dh, A.STEP_SELF, N, D, slots[:2], H=2, dist="ordinary", seed=78, cache_len=64)
    ops_l = AH.Operands(row0_case(low), DEV)
    assert native.debug_attn(**ops_l.kw, kernel=0, choose_as=(N, D)) == A.K_ATTN2 == native.debug_attn(**AH.Operands(low, DEV).kw, kernel=0)


# -- k_probe_split and k_merge_pred ----------------------------------------------------------------------------------------------
SPLIT_CASES = [  # B, n_active, N, D, kinds, identity
    (8, 0, 3, 10, None, False), (8, 1, 3, 10, ["last_only"], False), (8, 3, 3, 10, None, False), (300, 257, 3, 10, None, False),
    (1100, 1100, 3, 10, None, False), (1100, 257, 2, 16, None, True), (257, 257, 3, 10, ["none"], False),
    (257, 257, 3, 10, ["first", "last_only", "shared_first", "replacement"], False), (1100, 1100, 7, 10, ["none", "random"], False),
    (40, 33, 1, 1, None, False), (5, 3, 2, 1, ["shared_first", "none"], False)]


@pytest.mark.parametrize("B,n_active,N,D,kinds,identity", SPLIT_CASES, ids=[f"B{c[0]}-live{c[1]}-N{c[2]}-D{c[3]}-{i}" for i, c in enumerate(SPLIT_CASES)])
def test_probe_split_and_merge_pred(native, B, n_active, N, D, kinds, identity):
    act, pred_probe, drafts, kind = T.split_case(B, n_active, N, D, seed=B + n_active, kinds=kinds, identity=identity)
    R = U.rps(N, D)
    i32 = torch.int32
    b_act, b_probe, b_drafts = U.Buf((B,), i32, DEV, act), U.Buf((B,), i32, DEV, pred_probe), U.Buf((B, N, D), i32, DEV, drafts)
    b_act2, b_pos2 = U.Buf((B,), i32, DEV), U.Buf((B,), i32, DEV)
    sent = U.sentinel_array((B,), i32)
    want_act2, want_pos2, want_words = T.probe_split(act, pred_probe, drafts, n_active, sent, sent, probes_before=41)
    words = native.debug_probe_split(b_act.v, b_probe.v, b_drafts.v, n_active, b_act2.v, b_pos2.v, probes_before=41)
    torch.cuda.synchronize()
    what = f"B {B} live {n_active} N {N} D {D}"
    assert words == want_words, (what, words, want_words)
    U.check_buf(b_act2, want_act2, f"{what}: matching sequences")           # the order of act_idx; the sentinel past the count
    U.check_buf(b_pos2, want_pos2, f"{what}: slot -> position")
    for b, w in ((b_act, act), (b_probe, pred_probe), (b_drafts, drafts)):
        U.check_buf(b, w, f"{what}: an input")
    m = want_words[0]
    if kinds == ["none"]:
        assert m == 0
    if kinds and "none" not in kinds and "random" not in kinds:
        assert m == n_active
    # the draft pass's predictions for the m matching slots, then the merge
    rng = np.random.default_rng(7)
    pred2 = U.sentinel_array((B * R,), i32)
    pred2[:m * R] = rng.integers(0, 40, size=m * R)
    b_pred2, b_pred = U.Buf((B * R,), i32, DEV, pred2), U.Buf((B * R,), i32, DEV)
    native.debug_merge_pred(b_pos2.v, b_probe.v, b_pred2.v, b_pred.v, B, N, D, n_active)
    torch.cuda.synchronize()
    U.check_buf(b_pred, T.merge_pred(want_pos2, pred_probe, pred2, n_active, N, D, U.sentinel_array((B * R,), i32)), f"{what}: merged predictions")
    U.check_buf(b_pred2, pred2, f"{what}: the draft pass's predictions")


# -- the K/V commit with the indirection -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,Ld", [(64, 1), (256, 3)])
def test_commit_takes_probe_rows_and_draft_pass_rows(native, d, Ld):
    B, N, D, max_len = 12, 3, 10, 40
    rng = np.random.default_rng(d)
    s = U.make_state(B, N, D, max_len, rng.integers(0, max_len - D - 1, size=B), n_active=9, seed=d, pool=True)
    pred = U.new_pred(s)
    accs = [[0, 0, 0], [D, 2, 0], [0, 0, 0], [1, 0, 3], [0, 0, 0], [0, 0, D], [2, 2, 2], [0, 0, 0], [0, 1, 0]]
    for slot, acc in enumerate(accs):
        U.plant(s, pred, slot, acc, rng)
    want = U.accept_step(s, pred)
    rec, n_copy, Lc = want.rec, int(want.words["n_copy"]), max_len + D + 1
    assert n_copy == 9 and sorted(set(rec[:9, 2])) == [0, 1, 2, 3, D]
    _, _, pos2, _, words = T.two_passes(s.act_idx, s.drafts, pred, 9)
    assert words[0] == 5 and (pos2[:9] >= 0).tolist() == [bool(max(a)) for a in accs]
    ops = U.kv_operands(rec, n_copy, B, N, D, d, Ld, Lc, seed=d + Ld)
    probe = rng.integers(-2 ** 31, 2 ** 31, size=(Ld, B, 3 * d), dtype=np.int64).astype(np.int32).view(np.float32)
    f32 = torch.float32
    b_rec, b_pos2 = U.Buf((B, 5), torch.int32, DEV, rec), U.Buf((B,), torch.int32, DEV, pos2)
    qkv, qp = U.Buf(ops["qkv"].shape, f32, DEV, ops["qkv"]), U.Buf(probe.shape, f32, DEV, probe)
    kc, vc = U.Buf(ops["k0"].shape, f32, DEV), U.Buf(ops["v0"].shape, f32, DEV)
    native.debug_kvcopy_split(b_rec.v, n_copy, qkv.v, kc.v, vc.v, N, D, d, B, pos2=b_pos2.v, qkv_probe=qp.v)
    torch.cuda.synchronize()
    wk, wv = T.kv_commit_split(rec, n_copy, ops["qkv"], probe, pos2, ops["k0"], ops["v0"], N, D)
    U.check_buf(kc, wk, f"K cache, d {d} Ld {Ld}")                      # every word: the committed rows' bits, the fill everywhere else
    U.check_buf(vc, wv, f"V cache, d {d} Ld {Ld}")
    for b, w in ((qkv, ops["qkv"]), (qp, probe)):
        U.check_buf(b, w, "a source buffer")
    # what moved really came from two places
    plain_k, _ = U.kv_commit(rec, n_copy, ops["qkv"], ops["k0"], ops["v0"], N, D)
    assert not np.array_equal(plain_k.view(np.int32), wk.view(np.int32))
    # null pointers: ttx_debug_kvcopy's result
    k1, v1, k2, v2 = (U.Buf(ops["k0"].shape, f32, DEV) for _ in range(4))
    native.debug_kvcopy_split(b_rec.v, n_copy, qkv.v, k1.v, v1.v, N, D, d, B)
    native.debug_kvcopy(b_rec.v, n_copy, qkv.v, k2.v, v2.v, N, D, d, B)
    torch.cuda.synchronize()
    pk, pv = U.kv_commit(rec, n_copy, ops["qkv"], ops["k0"], ops["v0"], N, D)
    for got, w in ((k1, pk), (k2, pk), (v1, pv), (v2, pv)):
        U.check_buf(got, w, "without the indirection")


def test_split_arguments_are_refused(native, tta):
    def refused(fn, *a, **kw):
        with pytest.raises(tta.TtxError) as e:
            fn(*a, **kw)
        assert e.value.code == -1

    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    drafts = torch.zeros(2, 1, 2, dtype=torch.int32, device=DEV)
    out = torch.full((2,), 9, dtype=torch.int32, device=DEV)
    refused(native.debug_probe_split, i32(0, 1), i32(0, 0), drafts, 3, out, out.clone())            # n_active > B
    refused(native.debug_probe_split, i32(0, 0), i32(0, 0), drafts, 2, out, out.clone())            # act_idx repeats a row
    refused(native.debug_merge_pred, i32(0, 2), i32(0, 0), i32(*[0] * 6), torch.zeros(6, dtype=torch.int32, device=DEV), 2, 1, 2, 2)   # pos2 >= B
    rec = torch.tensor([[0, 0, 1, 0, 0], [1, 0, 0, 0, 0]], dtype=torch.int32, device=DEV)
    qkv, probe, cache = torch.zeros(1, 2 * 3, 3 * 64, device=DEV), torch.zeros(1, 2, 3 * 64, device=DEV), torch.zeros(1, 2, 11, 64, device=DEV)
    refused(native.debug_kvcopy_split, rec, 2, qkv, cache, cache.clone(), 1, 2, 64, 2, pos2=i32(-1, 0), qkv_probe=probe)   # accepts a token without a draft pass
    refused(native.debug_kvcopy_split, rec, 2, qkv, cache, cache.clone(), 1, 2, 64, 2, pos2=i32(0, 1))                     # pos2 without the probe buffer
    assert float(cache.abs().sum()) == 0.0 and out.tolist() == [9, 9]


# -- end to end ------------------------------------------------------------------------------------------------------------------
def pool_call(tta, model, src_rows, capacity, max_len, N, D, c_token):
    """ttx_greedy_speculative_generate_pool on ONE session over the rows in the order given: (rc, out, traj, fin_step, stats)."""
    from translation_transformer_amd import _native as NA
    src = src_rows.to(model.device, torch.int64).contiguous()
    R, width = src.shape
    lengths = ((src != PAD) * torch.arange(1, width + 1, device=src.device)).amax(dim=1).cpu().numpy()
    out = torch.empty((R, max_len), dtype=torch.int64, device=src.device)
    traj = torch.empty((R, max_len + 1), dtype=torch.int16, device=src.device)
    fin = torch.empty((R,), dtype=torch.int32, device=src.device)
    sessions = model.session_pool(1)
    sess = (C.c_void_p * 1)(sessions[0].value)
    p = NA.GenParams(max_len, D, N, PAD, BOS, EOS, c_token, 0)
    st = NA.GenStats()
    rc = model._lib.ttx_greedy_speculative_generate_pool(sess, 1, src.data_ptr(), R, width, (C.c_int32 * R)(*[int(x) for x in lengths]),
                                                         capacity, C.byref(p), out.data_ptr(), traj.data_ptr(), fin.data_ptr(),
                                                         C.byref(st), model._stream())
    torch.cuda.synchronize()
    return rc, out, traj, fin, st


COUNTERS = ["model_calls", "accepted_tokens", "produced_tokens", "kv_prefix_positions", "src_positions", "src_tokens_padded"]


def both_forms(tta, monkeypatch, make_model, src_rows, capacity, max_len, N, D, c_token, no_graph):
    """The same pool call with every step in one pass and with every step split, on models created under the same graph setting."""
    res = {}
    if no_graph:
        monkeypatch.setenv("TTX_NO_GRAPH", "1")
    for form, env in (("single", {"TTX_TWO_PHASE": "0"}), ("split", {"TTX_TWO_PHASE": "1", "TTX_TWO_PHASE_MIN_ROWS": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model = make_model()
        res[form] = pool_call(tta, model, src_rows, capacity, max_len, N, D, c_token)
        model.close()
    return res["single"], res["split"]


def check_forms(single, split, capacity, N, D, expect_matches):
    (rc1, out1, traj1, fin1, st1), (rc2, out2, traj2, fin2, st2) = single, split
    assert rc1 == rc2
    assert torch.equal(out1, out2) and torch.equal(traj1, traj2) and torch.equal(fin1, fin2)
    for k in COUNTERS:
        assert getattr(st1, k) == getattr(st2, k), k
    R = U.rps(N, D)
    life, adv = T.slot_steps(traj2.cpu().numpy())
    n_slot_steps, n_matched = int(life.sum()), int((adv > 1).sum())
    steps = T.pool_schedule(traj2.cpu().numpy(), capacity)
    assert len(steps) == st1.model_calls == st2.model_calls, "the schedule read off the traces is not the one the pool ran"
    assert sum(s[0] for s in steps) == n_slot_steps and sum(s[1] for s in steps) == n_matched
    assert st1.verified_positions == n_slot_steps * R                       # one pass: every live slot's RPS rows
    assert st2.verified_positions == n_slot_steps + n_matched * R           # split: a row per live slot + RPS per matching slot
    assert st2.accepted_tokens == int(np.where(adv > 1, adv - 1, 0).sum())
    print(f"capacity {capacity}: {len(steps)} steps, {n_slot_steps} slot-steps, {n_matched} matched ({n_matched / max(1, n_slot_steps):.1%}), "
          f"{sum(1 for s in steps if s[1] == 0)} steps without a match")
    if expect_matches:
        # both branches must have run: a step whose draft pass is skipped, and a slot-step that went through the draft pass
        assert any(s[1] == 0 for s in steps), "no step without a match: the skip path did not run"
        assert n_matched > 0, "no slot-step with a match: the draft pass did not run"
        if capacity >= 8:
            assert any(0 < s[1] < s[0] for s in steps), "no step mixes matching and other slots"
    else:
        assert n_matched == 0 and st2.accepted_tokens == 0, "this model was expected to accept no draft"
    return out2


def fixture_rows(n_rows, seed):
    fsrc, _, c, _ = fixture_tokens()
    idx = torch.randperm(n_rows, generator=torch.Generator().manual_seed(seed)) % 10
    return fsrc[idx], idx.tolist(), c


@pytest.mark.parametrize("no_graph", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("capacity,n_rows", [(3, 12), (64, 150)])
@pytest.mark.parametrize("which", ["tiny", "hd64"])
def test_split_steps_equal_single_pass(tta, monkeypatch, which, capacity, n_rows, no_graph):
    if which == "tiny":
        st, cfg = tiny_state()
        gold = load_npz("gen_spec_greedy.npz")["b1_n3_d10_tokens"]
    else:
        st, cfg = hd64_state()
        gold = hd64_gen("spec_greedy")["b1_n3_d10_tokens"]
    rows, idx, c = fixture_rows(n_rows, seed=capacity)
    make = lambda: tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    single, split = both_forms(tta, monkeypatch, make, rows, capacity, 150, 3, 10, c, no_graph)
    assert single[0] == 0
    out = check_forms(single, split, capacity, 3, 10, expect_matches=True).cpu().numpy()
    for j, r in enumerate(idx):                                                # the golden holds every fixture row decoded alone
        assert upto_eos(out[j]) == upto_eos(gold[r, 0]), (which, capacity, r)


def test_split_steps_equal_single_pass_where_the_layouts_alone_would_disagree_on_the_kernel(tta, monkeypatch):
    """Head dimension 64, max_len 300: the (3, 10) step stages 331 keys and runs its self-attention on k_attn, a (1, 0) step alone
    would stage 301 and take k_attn2 (k_attn2 holds 320).  The probe takes the draft pass's choice, so the split stays identical."""
    st, cfg = hd64_state()
    assert tta.NativeTransformer.attn_staged_key_limit(64, 31) == 320
    rows, idx, c = fixture_rows(60, seed=5)
    make = lambda: tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    single, split = both_forms(tta, monkeypatch, make, rows, 16, 300, 3, 10, c, no_graph=False)
    assert single[0] == 0
    check_forms(single, split, 16, 3, 10, expect_matches=True)


def test_generate_many_is_unchanged_by_the_split(tta, monkeypatch):
    st, cfg = tiny_state()
    rows, idx, c = fixture_rows(70, seed=11)
    batches = [rows[i:i + 7] for i in range(0, 70, 7)]
    batches = [b[:, :int((b != PAD).sum(1).max())].cuda() for b in batches]
    res = {}
    for form, env in (("single", {"TTX_TWO_PHASE": "0"}), ("split", {"TTX_TWO_PHASE": "1", "TTX_TWO_PHASE_MIN_ROWS": "0"}),
                      ("default", {"TTX_TWO_PHASE": "1", "TTX_TWO_PHASE_MIN_ROWS": "800"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
        g = tta.TranslationInferenceGreedySpeculative(model, 150, 10, 3, PAD, BOS, EOS, c)
        out = g.generate_many(batches, in_flight=3, reorder=True, group_size=16)
        # three pools share the list: which pool takes which rows, and so the pools' step counts, follow the timing of the run;
        # what is summed over rows and slot-steps does not
        tot = {k: v for k, v in g.stats_total.items() if not k.endswith("_ms") and k not in ("device", "device_model_calls")}
        dev = {k: g.stats_total["device"][k] for k in ("accepted_tokens", "produced_tokens", "kv_prefix_positions", "src_positions")}
        res[form] = (out, g.model_calls_num, tot, dev, g.stats_total["device"]["verified_positions"])
        model.close()
    for form in ("split", "default"):
        for a, b in zip(res[form][0], res["single"][0]):
            assert torch.equal(a, b), form
        assert res[form][1:4] == res["single"][1:4], form
    assert res["split"][4] < res["single"][4]                                  # fewer rows went through the decoder


def test_a_model_that_accepts_nothing_skips_every_draft_pass(tta, monkeypatch):
    """Seeded (untrained) d = 256 weights at head dimension 32 accept no draft on the synthetic reactions (189 verify
    steps per batch of 32 at max_len 200, one token a step): every step of the split form is a probe followed by the accept graph
    alone, and verified_positions is the number of slot-steps."""
    from tools.synth import SynthReactions, batches, C_TOK, V
    from util_models import seeded_weights, state_shapes
    st = seeded_weights(state_shapes(V, 256, 2048, 4, 4), 20250725)
    st["tgt_token_featurizer.embedding.weight"] = st["src_token_featurizer.embedding.weight"]
    make = lambda: tta.NativeTransformer(st, 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(32)                     # the first batch of that measurement
    src = torch.from_numpy(next(iter(batches(src_rows, 32)))).to(torch.int64)
    single, split = both_forms(tta, monkeypatch, make, src, 16, 200, 3, 10, C_TOK, no_graph=False)
    check_forms(single, split, 16, 3, 10, expect_matches=False)
    life, _ = T.slot_steps(split[2].cpu().numpy())
    assert split[4].verified_positions == int(life.sum())
