"""Draft select, the third mode of the slot pool's verify step (DESIGN.md "Two-phase verify step"): the draft pass runs row 0 and
the D rows of each draft whose first token is the probe's prediction, stored compacted.  Every check is exact equality.

  attention        k_attn3 and k_attn3s, STEP_SELF and STEP_CROSS, five slots a launch (fronts {0, 1, 30, 31, 32, 33, 63, 64, 65,
                   200}, source lengths {1, 31, 32, 33, 70}, a PAD front token, PADs in a prefix), layouts (3, 10), (7, 10), (2, 16):
                   the rows a compacted launch stores equal, bit for bit, the same rows of the full-layout launch on the same cache;
                   every non-zero mask at N = 3; at (7, 10) masks that leave a whole 32-row unit absent and masks whose present
                   drafts straddle the unit edges (drafts 2 | 3 and 5 | 6); rows past the compacted count and the guard margins
                   untouched, the compacted inputs NaN past their live rows
  loop kernels     k_probe_split with its optional outputs (masks, row bases, row map, compacted count), k_embed<true> with the
                   row map, k_merge_pred and k_kvcopy on compacted rows, against tests/util_draft_select.py: 0, 1, 3, 257 and
                   1 100 live slots; no match, all drafts, the last draft only, two drafts sharing the token, a permuted list;
                   entries past the counts untouched; null operands == the existing entry points; the commit writes positions
                   front_old .. front_old + n_acc and nothing else
  end to end       ttx_greedy_speculative_generate_pool with every step split, draft select on against TTX_DRAFT_SELECT=0: outputs,
                   traces and every counter identical, the golden tokens, the executed rows of ttx_pool_last_counters == what the
                   traces, the drafts and the tokens say, both a slot-step with fewer than N drafts present and one with more than
                   one in the run, on the trained four-head model of tests/golden/h4_* (head dimension 32, H % 4 == 0); the trained
                   tiny model (2 heads) and the head-dimension-64 model, whose step attention runs on k_attn2 / k_attn, report the
                   all-drafts pass and decode identically; the four-head model under the default TTX_TWO_PHASE_MIN_ROWS, where one-pass
                   and split steps mix
"""
import numpy as np
import pytest
import torch

import util_attn_checks as A
import util_draft_select as S
import util_gemm_checks as G
import util_loop_checks as U
import util_two_phase as T
from test_gpu_loop_kernels import tables
from test_gpu_two_phase import COUNTERS, fixture_rows, layout_cases, pool_call
from util_hd64 import hd64_gen, hd64_state
from util_models import load_npz, tiny_state, upto_eos

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def native(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)


# -- attention -------------------------------------------------------------------------------------------------------------------
# masks of the five slots of a launch, per layout.  (7, 10): RPS = 71 rows are three 32-row units: rows 0 .. 31 (row 0, drafts 0 - 2
# and the first row of draft 3), 32 .. 63 (the rest of draft 3, drafts 4 and 5, three rows of draft 6), 64 .. 70 (draft 6).
MASKS = {
    (3, 10): [[1, 2, 3, 4, 5], [6, 7, 4, 1, 2], [7, 7, 7, 7, 7]],
    (7, 10): [[0b0000111, 0b0111111, 0b0001100, 0b1100000, 0b1111111],        # units 1 and 2 absent; unit 2 absent; 2 | 3; 5 | 6; all
              [0b1000000, 0b0001000, 0b1010101, 0b0000001, 0b0100100]],       # unit 0 holds row 0 alone; draft 3 alone straddles 0 | 1
    (2, 16): [[1, 2, 3, 2, 1]],
}


def compacted_launch(native, case, ops, masks, kernel):
    """The launch of ``case`` on compacted rows: (out arena, total rows, mask, row_base)."""
    c, d, R = case, case.d, case.rps
    n = c.n_active
    mask = np.zeros(c.groups, dtype=np.int32)
    mask[:n] = masks[:n]
    base = np.zeros(c.groups, dtype=np.int32)
    total = 0
    for p in range(n):
        base[p] = total
        total += S.sel_rows(int(mask[p]), c.D)
    keep = [p * R + rs for p in range(n) for rs in range(R) if S.sel_row(int(mask[p]), rs, c.D) is not None]
    assert len(keep) == total
    idx = torch.tensor(keep, dtype=torch.int64, device=DEV)
    kw = dict(ops.kw)
    if c.mode == A.STEP_CROSS:
        qa = G.Arena(c.q.shape[0], d, device=DEV)                        # NaN past the compacted rows
        qa.m[:total] = ops.kw["q"][idx]
        kw.update(q=qa.m)
    else:
        qa = G.Arena(c.q.shape[0], 3 * d, device=DEV)
        qa.m[:total] = ops.qa.m[idx]
        kw.update(q=qa.m[:, :d], k=qa.m[:, d:2 * d], v=qa.m[:, 2 * d:])
    out = G.Arena(c.out_rows, d, device=DEV, fill=G.OUT_FILL)
    kw.update(out=out.m)
    mb, bb = U.Buf((c.groups,), I32, DEV, mask), U.Buf((c.groups,), I32, DEV, base)
    kid = native.debug_attn_select(**kw, kernel=kernel, row_base=bb.v, draft_mask=mb.v)
    torch.cuda.synchronize()
    assert kid == kernel
    assert mb.margins() is None and bb.margins() is None and (mb.get() == mask).all() and (bb.get() == base).all()
    return out, total, idx


@pytest.mark.parametrize("mode", [A.STEP_SELF, A.STEP_CROSS], ids=["STEP_SELF", "STEP_CROSS"])
@pytest.mark.parametrize("kernel", [A.K_ATTN3, A.K_ATTN3S], ids=["k_attn3", "k_attn3s"])
def test_compacted_rows_equal_the_full_layout(native, kernel, mode):
    seen = set()
    for case in layout_cases(32, mode):
        ops = A.Operands(case, DEV)
        assert native.debug_attn(**ops.kw, kernel=kernel) == kernel
        torch.cuda.synchronize()
        A.check_structure(ops.out, case, f"{case}")
        full = ops.out.m[:case.live_rows].clone()
        for masks in MASKS[case.N, case.D]:
            out, total, idx = compacted_launch(native, case, ops, masks, kernel)
            what = f"{case} on {A.KERNEL_NAMES[kernel]}, masks {[bin(m) for m in masks]}"
            G.check_untouched(out, total, what)                            # rows past the compacted count, guard bands
            got = out.m[:total].clone()
            assert not bool((got.contiguous().view(torch.int32) == G.OUT_FILL).any()), f"{what}: a stored row was never written"
            A.check_bits(got, full[idx].contiguous(), case, what)
            seen.update((case.N, m) for m in masks)
    assert {(3, m) for m in range(1, 8)} <= seen


def test_select_arguments_are_refused(native, tta):
    def refused(fn, *a, **kw):
        with pytest.raises(tta.TtxError) as e:
            fn(*a, **kw)
        assert e.value.code == -1

    case = layout_cases(32, A.STEP_SELF)[0]
    ops = A.Operands(case, DEV)
    i32 = lambda *v: torch.tensor(v, dtype=I32, device=DEV)
    good_mask, good_base = i32(1, 2, 3, 4, 5), i32(0, 11, 22, 43, 54)
    assert native.debug_attn_select(**ops.kw, kernel=A.K_ATTN3S, row_base=good_base, draft_mask=good_mask) == A.K_ATTN3S
    ops.out.reset()
    refused(native.debug_attn_select, **ops.kw, kernel=A.K_ATTN3S, row_base=good_base, draft_mask=i32(1, 0, 3, 4, 5))       # a mask of 0
    refused(native.debug_attn_select, **ops.kw, kernel=A.K_ATTN3S, row_base=good_base, draft_mask=i32(1, 8, 3, 4, 5))       # a bit at N
    refused(native.debug_attn_select, **ops.kw, kernel=A.K_ATTN3S, row_base=i32(0, 10, 21, 42, 53), draft_mask=good_mask)   # no + 1 for row 0
    refused(native.debug_attn_select, **ops.kw, kernel=A.K_ATTN2, row_base=good_base, draft_mask=good_mask)                 # k_attn2 cannot
    refused(native.debug_attn_select, **ops.kw, kernel=0, row_base=good_base, draft_mask=None)                              # one without the other
    torch.cuda.synchronize()
    G.check_untouched(ops.out, 0, "refused launches")
    # the loop kernels' entry points: the same three refusals
    drafts = torch.zeros(2, 3, 2, dtype=I32, device=DEV)
    out = torch.full((2,), 9, dtype=I32, device=DEV)
    refused(native.debug_probe_split_select, i32(0, 1), i32(0, 0), drafts, 2, out, out.clone(), out.clone(), out.clone(), None)
    pred = torch.full((14,), 9, dtype=I32, device=DEV)
    refused(native.debug_merge_pred_select, i32(0, -1), i32(0, 0), i32(*[0] * 14), pred, 2, 3, 2, 2, i32(0, 0), i32(0, 0))   # mask 0
    refused(native.debug_merge_pred_select, i32(0, 1), i32(0, 0), i32(*[0] * 14), pred, 2, 3, 2, 2, i32(0, 2), i32(1, 1))    # not the prefix sum
    rec = torch.tensor([[0, 1, 1, 0, 0], [1, 0, 0, 0, 0]], dtype=I32, device=DEV)
    qkv, probe, cache = torch.zeros(1, 2 * 7, 3 * 64, device=DEV), torch.zeros(1, 2, 3 * 64, device=DEV), torch.zeros(1, 2, 11, 64, device=DEV)
    refused(native.debug_kvcopy_select, rec, 2, qkv, cache, cache.clone(), 3, 2, 64, 2, i32(0, -1), probe, i32(0, 0), i32(0b101, 0))   # best draft absent
    refused(native.debug_kvcopy_select, rec, 2, qkv, cache, cache.clone(), 3, 2, 64, 2, i32(0, -1), probe, i32(1, 0), i32(0b010, 0))   # row_base
    refused(native.debug_kvcopy_select, rec, 2, qkv, cache, cache.clone(), 3, 2, 64, 2, i32(0, -1), probe, i32(0, 0), i32(0, 0))       # mask 0
    assert float(cache.abs().sum()) == 0.0 and pred.tolist() == [9] * 14 and out.tolist() == [9, 9]


# -- the loop kernels on compacted rows --------------------------------------------------------------------------------------------
KINDS = {"none": lambda rng, N, D: np.zeros(N, dtype=np.int64),
         "all": lambda rng, N, D: rng.integers(1, D + 1, size=N),
         "last_only": lambda rng, N, D: np.concatenate([np.zeros(N - 1, dtype=np.int64), rng.integers(1, D + 1, size=1)]),
         "two_share": lambda rng, N, D: np.concatenate([rng.integers(1, D + 1, size=1), np.zeros(N - 2, dtype=np.int64), rng.integers(1, D + 1, size=1)]),
         "random": lambda rng, N, D: rng.integers(0, D + 1, size=N) * rng.integers(0, 2, size=N)}
LOOP_CASES = [  # B, live slots, N, D, kinds, permuted
    (8, 0, 3, 10, ["random"], True), (8, 1, 3, 10, ["last_only"], True), (8, 3, 3, 10, ["none", "all", "two_share"], True),
    (300, 257, 3, 10, ["random", "two_share", "last_only"], True), (1100, 1100, 3, 10, ["random", "none", "all"], True),
    (1100, 257, 7, 10, ["random"], False), (257, 257, 3, 10, ["none"], True), (257, 257, 3, 10, ["all"], True), (40, 33, 2, 16, ["random", "all"], True)]


def loop_case(B, live, N, D, kinds, permuted, seed):
    rng = np.random.default_rng(seed)
    max_len = 40
    s = U.make_state(B, N, D, max_len, rng.integers(0, max_len - D - 1, size=B), n_active=live, seed=seed, pool=True, permute=permuted)
    pred = U.new_pred(s)
    for slot in range(live):
        k = kinds[slot % len(kinds)] if len(kinds) > 1 and slot < len(kinds) else kinds[int(rng.integers(0, len(kinds)))]
        U.plant(s, pred, slot, KINDS[k](rng, N, D), rng)
    return s, pred


@pytest.mark.parametrize("B,live,N,D,kinds,permuted", LOOP_CASES, ids=[f"B{c[0]}-live{c[1]}-N{c[2]}-D{c[3]}-{i}" for i, c in enumerate(LOOP_CASES)])
def test_loop_kernels_on_compacted_rows(native, B, live, N, D, kinds, permuted):
    s, pred = loop_case(B, live, N, D, kinds, permuted, seed=B + live + N)
    R = U.rps(N, D)
    what = f"B {B} live {live} N {N} D {D}"
    sent = lambda n: U.sentinel_array((n,), I32)
    pred_probe, want_act2, want_pos2, want_mask, want_base, want_map, pred2c, _ = S.two_passes_select(s.act_idx, s.drafts, pred, live)
    before = dict(act2=sent(B), pos2=sent(B), mask=sent(B), row_base=sent(B), row_map=sent(B * R))
    want = S.select_split(s.act_idx, pred_probe, s.drafts, live, before, probes_before=41)
    m, total = want[5][0], want[5][2]
    if kinds == ["none"]:
        assert m == 0 and total == 0
    if kinds == ["all"]:
        assert m == live and total == live * R
    if "two_share" in kinds:
        assert any(int(x) == (1 | 1 << (N - 1)) for x in want[2][:m])
    if "last_only" in kinds:
        assert any(int(x) == 1 << (N - 1) for x in want[2][:m])

    # k_probe_split with the optional outputs
    b = {k: U.Buf(a.shape, I32, DEV, a) for k, a in (("act", s.act_idx), ("probe", pred_probe), ("drafts", s.drafts))}
    o = {k: U.Buf((B * R if k == "row_map" else B,), I32, DEV) for k in before}
    words = native.debug_probe_split_select(b["act"].v, b["probe"].v, b["drafts"].v, live, o["act2"].v, o["pos2"].v, o["mask"].v,
                                            o["row_base"].v, o["row_map"].v, probes_before=41)
    torch.cuda.synchronize()
    assert words == want[5], (what, words, want[5])
    for k, w in zip(("act2", "pos2", "mask", "row_base", "row_map"), want[:5]):
        U.check_buf(o[k], w, f"{what}: {k}")                               # the sentinel past the counts, margins intact
    # the optional outputs null: the existing entry point's result, from both entry points
    for fn, extra in ((native.debug_probe_split, ()), (native.debug_probe_split_select, (None, None, None))):
        a2, p2 = U.Buf((B,), I32, DEV), U.Buf((B,), I32, DEV)
        w7 = fn(b["act"].v, b["probe"].v, b["drafts"].v, live, a2.v, p2.v, *extra, probes_before=41)
        torch.cuda.synchronize()
        t_act2, t_pos2, t_words = T.probe_split(s.act_idx, pred_probe, s.drafts, live, sent(B), sent(B), probes_before=41)
        assert w7[:7] == t_words
        U.check_buf(a2, t_act2, f"{what}: act2 without the optional outputs")
        U.check_buf(p2, t_pos2, f"{what}: pos2 without the optional outputs")
    for k, w in (("act", s.act_idx), ("probe", pred_probe), ("drafts", s.drafts)):
        U.check_buf(b[k], w, f"{what}: an input")

    # k_embed<true> with the row map: row i holds what the full layout's row row_map[i] holds
    d_model, V = 64, 37
    table, pe = tables(V, d_model, int(s.front.max()) + D + 2, seed=B)
    act2 = np.where(want[0] == U.SENTINEL[I32], 0, want[0]).astype(np.int32)          # the draft pass's list (entries past m unread)
    act2[m:] = [x for x in range(B) if x not in set(act2[:m].tolist())][:B - m]
    eb = {k: U.Buf(a.shape, I32, DEV, a) for k, a in (("act2", act2), ("front", s.front), ("gen", s.gen))}
    tb, pb = U.Buf(table.shape, torch.float32, DEV, table), U.Buf(pe.shape, torch.float32, DEV, pe)
    x = U.Buf((B * R, d_model), torch.float32, DEV)
    x_before = x.get().view(np.float32)
    full = U.embed_step(table, pe, act2, s.front, s.gen, s.drafts, m, x_before.copy())
    want_x = x_before.copy()
    want_x[:total] = full[want[4][:total]]
    rmap = U.Buf((B * R,), I32, DEV, np.where(want[4] == U.SENTINEL[I32], 0, want[4]))
    native.debug_embed_select(tb.v, pb.v, x.v, eb["act2"].v, eb["front"].v, eb["gen"].v, b["drafts"].v, B, N, D, m, rmap.v, total)
    torch.cuda.synchronize()
    U.check_buf(x, want_x, f"{what}: embedding through the row map")
    x.reset()
    native.debug_embed_select(tb.v, pb.v, x.v, eb["act2"].v, eb["front"].v, eb["gen"].v, b["drafts"].v, B, N, D, m, None, 0)
    torch.cuda.synchronize()
    U.check_buf(x, full, f"{what}: embedding without a row map")

    # k_merge_pred on the compacted predictions
    b_pred2, b_pred = U.Buf((B * R,), I32, DEV, pred2c), U.Buf((B * R,), I32, DEV)
    native.debug_merge_pred_select(o["pos2"].v, b["probe"].v, b_pred2.v, b_pred.v, B, N, D, live, o["row_base"].v, o["mask"].v)
    torch.cuda.synchronize()
    merged = S.merge_pred_select(want[1], pred_probe, pred2c, want[2], want[3], live, N, D, sent(B * R))
    U.check_buf(b_pred, merged, f"{what}: merged predictions")
    U.check_buf(b_pred2, pred2c, f"{what}: the draft pass's predictions")
    b_pred.reset()
    pred2_full = T.two_passes(s.act_idx, s.drafts, pred, live)[3]
    b_full = U.Buf((B * R,), I32, DEV, pred2_full)
    native.debug_merge_pred_select(o["pos2"].v, b["probe"].v, b_full.v, b_pred.v, B, N, D, live, None, None)
    torch.cuda.synchronize()
    U.check_buf(b_pred, T.merge_pred(want[1], pred_probe, pred2_full, live, N, D, sent(B * R)), f"{what}: merged predictions, null operands")

    # k_kvcopy on the compacted QKV rows: the state the accept rule reaches from the merged predictions gives the records
    after = U.accept_step(s, merged)
    rec, n_copy, Lc, Ld = after.rec, int(after.words["n_copy"]), s.max_len + D + 1, 2
    assert n_copy == live
    ops = U.kv_operands(rec, n_copy, B, N, D, d_model, Ld, Lc, seed=B + 1)
    qkv_c = U.sentinel_array((Ld, B * R, 3 * d_model), torch.float32)
    for l in range(Ld):
        qkv_c[l] = S.compact_rows(ops["qkv"][l], want[2], want[3], m, N, D, qkv_c[l])
    rng = np.random.default_rng(B)
    probe = rng.integers(-2 ** 31, 2 ** 31, size=(Ld, B, 3 * d_model), dtype=np.int64).astype(np.int32).view(np.float32)
    f32 = torch.float32
    b_rec = U.Buf((B, 5), I32, DEV, rec)
    qc, qp = U.Buf(qkv_c.shape, f32, DEV, qkv_c), U.Buf(probe.shape, f32, DEV, probe)
    kc, vc = U.Buf(ops["k0"].shape, f32, DEV), U.Buf(ops["v0"].shape, f32, DEV)
    native.debug_kvcopy_select(b_rec.v, n_copy, qc.v, kc.v, vc.v, N, D, d_model, B, o["pos2"].v, qp.v, o["row_base"].v, o["mask"].v)
    torch.cuda.synchronize()
    wk, wv = S.kv_commit_select(rec, n_copy, qkv_c, probe, want[1], want[2], want[3], ops["k0"], ops["v0"], N, D)
    U.check_buf(kc, wk, f"{what}: K cache")                                # positions front_old .. front_old + n_acc, the fill elsewhere
    U.check_buf(vc, wv, f"{what}: V cache")
    tk, tv = T.kv_commit_split(rec, n_copy, ops["qkv"], probe, want[1], ops["k0"], ops["v0"], N, D)
    assert np.array_equal(wk.view(np.int32), tk.view(np.int32)) and np.array_equal(wv.view(np.int32), tv.view(np.int32))
    for buf, w in ((qc, qkv_c), (qp, probe)):
        U.check_buf(buf, w, f"{what}: a source buffer")
    written = (wk.view(np.int32) != U.FLOAT_FILL).any(axis=(0, 3))         # [B, Lc]
    for slot in range(n_copy):
        bb, _, n_acc, f = (int(v) for v in rec[slot, :4])
        assert written[bb].nonzero()[0].tolist() == list(range(f, f + n_acc + 1)), (what, slot)
    # null draft-select operands: ttx_debug_kvcopy_split's result on the full layout
    k1, v1 = U.Buf(ops["k0"].shape, f32, DEV), U.Buf(ops["v0"].shape, f32, DEV)
    qf = U.Buf(ops["qkv"].shape, f32, DEV, ops["qkv"])
    native.debug_kvcopy_select(b_rec.v, n_copy, qf.v, k1.v, v1.v, N, D, d_model, B, o["pos2"].v, qp.v, None, None)
    torch.cuda.synchronize()
    U.check_buf(k1, tk, f"{what}: K cache, null operands")
    U.check_buf(v1, tv, f"{what}: V cache, null operands")


# -- end to end ------------------------------------------------------------------------------------------------------------------
def select_forms(tta, monkeypatch, make_model, rows, capacity, max_len, N, D, c_token, no_graph, min_rows="0"):
    """The same pool call with TTX_DRAFT_SELECT=0 and with draft select requested: per form the call's result and the counters of
    ttx_pool_last_counters.  ``min_rows``: TTX_TWO_PHASE_MIN_ROWS ("0": every step split; None: the default threshold)."""
    res = {}
    if no_graph:
        monkeypatch.setenv("TTX_NO_GRAPH", "1")
    monkeypatch.setenv("TTX_TWO_PHASE", "1")
    if min_rows is None:
        monkeypatch.delenv("TTX_TWO_PHASE_MIN_ROWS", raising=False)
    else:
        monkeypatch.setenv("TTX_TWO_PHASE_MIN_ROWS", min_rows)
    for form, flag in (("all_drafts", "0"), ("select", "1")):
        monkeypatch.setenv("TTX_DRAFT_SELECT", flag)
        model = make_model()
        res[form] = pool_call(tta, model, rows, capacity, max_len, N, D, c_token) + (model.pool_last_counters(),)
        model.close()
    return res["all_drafts"], res["select"]


def check_select_forms(a, b, N, D):
    (rc1, out1, traj1, fin1, st1, c1), (rc2, out2, traj2, fin2, st2, c2) = a, b
    assert rc1 == rc2 == 0
    assert torch.equal(out1, out2) and torch.equal(traj1, traj2) and torch.equal(fin1, fin2)
    for k in COUNTERS + ["verified_positions"]:
        assert getattr(st1, k) == getattr(st2, k), k
    R = U.rps(N, D)
    life, adv = T.slot_steps(traj2.cpu().numpy())
    n_slot_steps, n_matched = int(life.sum()), int((adv > 1).sum())
    assert st2.verified_positions == n_slot_steps + n_matched * R          # the positions of matching slots, run or not
    for c in (c1, c2):
        assert c["steps"] == c["split_steps"] == st2.model_calls
        assert c["slot_steps_probed"] == n_slot_steps and c["slots_matched"] == n_matched
    assert c1["draft_select"] == 0 and c1["rows_executed"] == n_slot_steps + n_matched * R and c1["drafts_matched"] == n_matched * N
    return life, n_slot_steps, n_matched


@pytest.mark.parametrize("no_graph", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("capacity,n_rows", [(3, 12), (64, 150)])
@pytest.mark.parametrize("which", ["h4", "tiny"])
def test_draft_select_equals_the_all_drafts_pass(tta, monkeypatch, which, capacity, n_rows, no_graph):
    """h4: the trained four-head model (head dimension 32), whose step attention runs on k_attn3 / k_attn3s: draft select runs.
    tiny: the trained tiny model has 2 heads, so its step attention runs on k_attn2 / k_attn and the pool keeps the all-drafts pass
    when draft select is requested (scope of the mode): same outputs, and the query says so."""
    if which == "h4":
        st, cfg = S.h4_state()
        gold = S.h4_gen()["b1_n3_d10_tokens"]
    else:
        st, cfg = tiny_state()
        gold = load_npz("gen_spec_greedy.npz")["b1_n3_d10_tokens"]
    drafts10 = load_npz("drafts.npz")["nobos_d10_n3"]                        # the drafts of the ten fixture rows
    rows, idx, c = fixture_rows(n_rows, seed=capacity)
    N, D = 3, 10
    make = lambda: tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    a, b = select_forms(tta, monkeypatch, make, rows, capacity, 150, N, D, c, no_graph)
    life, n_slot_steps, n_matched = check_select_forms(a, b, N, D)
    out = b[1].cpu().numpy()
    for j, r in enumerate(idx):
        assert upto_eos(out[j]) == upto_eos(gold[r, 0]), (which, capacity, r)
    cnt = b[5]
    tokens = np.zeros((len(idx), 151), dtype=np.int64)
    tokens[:, :gold.shape[2]] = gold[idx, 0]
    rows_want, fewer, several, matched = S.executed_rows(b[2].cpu().numpy(), tokens, drafts10[idx])
    print(f"{which} capacity {capacity}: {n_slot_steps} slot-steps, {n_matched} matched, {matched} drafts matched, {rows_want} rows under "
          f"draft select against {n_slot_steps + n_matched * U.rps(N, D)}; {fewer} slot-steps with fewer than N drafts present, "
          f"{several} with several")
    assert fewer > 0, "no slot-step with fewer than N drafts present"
    assert several > 0, "no slot-step with more than one draft present"
    if which == "tiny":
        assert cnt == a[5] and cnt["draft_select"] == 0
        return
    assert cnt["draft_select"] == 1
    assert cnt["rows_executed"] == rows_want and cnt["drafts_matched"] == matched
    assert rows_want < a[5]["rows_executed"]


def test_default_threshold_mixes_one_pass_and_draft_select_steps(tta, monkeypatch):
    """The four-head model under the default TTX_TWO_PHASE_MIN_ROWS (800 live rows = 26 slots of 31): the full pool's steps are split
    and run draft select, the steps of the draining pool run in one pass.  Same outputs, traces and counters as with
    TTX_DRAFT_SELECT=0 and as with every step split; fewer rows through the decoder."""
    st, cfg = S.h4_state()
    gold = S.h4_gen()["b1_n3_d10_tokens"]
    rows, idx, c = fixture_rows(150, seed=64)
    N, D, R = 3, 10, U.rps(3, 10)
    make = lambda: tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    a, b = select_forms(tta, monkeypatch, make, rows, 64, 150, N, D, c, no_graph=False, min_rows=None)
    (rc1, out1, traj1, fin1, st1, c1), (rc2, out2, traj2, fin2, st2, c2) = a, b
    assert rc1 == rc2 == 0
    assert torch.equal(out1, out2) and torch.equal(traj1, traj2) and torch.equal(fin1, fin2)
    for k in COUNTERS + ["verified_positions"]:
        assert getattr(st1, k) == getattr(st2, k), k
    out = out2.cpu().numpy()
    for j, r in enumerate(idx):
        assert upto_eos(out[j]) == upto_eos(gold[r, 0]), r
    assert (c1["draft_select"], c2["draft_select"]) == (0, 1)
    for k in ("steps", "split_steps", "slot_steps_probed", "slots_matched"):
        assert c1[k] == c2[k], k
    assert 0 < c2["split_steps"] < c2["steps"] == st2.model_calls, "the run does not mix split and one-pass steps"
    life, _ = T.slot_steps(traj2.cpu().numpy())
    one_pass_rows = (int(life.sum()) - c2["slot_steps_probed"]) * R              # slot-steps of the one-pass steps, RPS rows each
    assert c1["rows_executed"] == one_pass_rows + c1["slot_steps_probed"] + c1["slots_matched"] * R
    assert c1["drafts_matched"] == c1["slots_matched"] * N
    assert c2["slots_matched"] <= c2["drafts_matched"] < c1["drafts_matched"]
    assert c2["rows_executed"] == one_pass_rows + c2["slot_steps_probed"] + c2["slots_matched"] + D * c2["drafts_matched"]
    every = select_forms(tta, monkeypatch, make, rows, 64, 150, N, D, c, no_graph=False)[1]
    assert torch.equal(every[1], out2) and torch.equal(every[2], traj2) and torch.equal(every[3], fin2)


def test_head_dimension_64_keeps_the_all_drafts_pass(tta, monkeypatch):
    st, cfg = hd64_state()
    gold = hd64_gen("spec_greedy")["b1_n3_d10_tokens"]
    rows, idx, c = fixture_rows(24, seed=7)
    make = lambda: tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    a, b = select_forms(tta, monkeypatch, make, rows, 8, 150, 3, 10, c, no_graph=False)
    check_select_forms(a, b, 3, 10)
    assert b[5] == a[5] and b[5]["draft_select"] == 0                        # requested, not run: its attention is k_attn2 / k_attn
    out = b[1].cpu().numpy()
    for j, r in enumerate(idx):
        assert upto_eos(out[j]) == upto_eos(gold[r, 0]), r
