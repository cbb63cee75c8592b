"""The bookkeeping kernels of the beam-speculative batch pool (csrc/ttx_loop_kernels.hip.h: k_bsp_init, k_bsp_admit, k_bsp_fill,
k_bsp_prep, k_bsp_select, k_bsp_batches, k_bsp_retire, k_bsp_publish), one launch at a time through ttx_debug_bsp, which launches
through the pool's own launch functions (csrc/ttx_api.hip: launch_bsp_*), against the plain restatement of tests/util_bsp_checks.py.
After EVERY launch the whole State is compared: every array of the kernels' argument block and the 12 words (BeamCounters,
BeamPoolHost) — the restatement's value where a rule writes, what was there before (the sentinel in the constructed cases) where
none does — guard margins intact, the staged operands of an admission untouched.  Everything is an integer, a flag or a bit copy:
every comparison is exact.  tests/test_bsp_checks_host.py pins the restatement to a per-batch loop written from the reference's
scalars, asserts that the chained scenarios reach the rare branches, and shows that each checker can fail.

Paths of the kernels these cases execute on purpose:
  k_bsp_init     (C, K) = (1, 1), (5, 3), (300, 2) and (1 024, 32): 32 768 candidates against 16 384 threads, the grid stride;
                 every array blank before; every counter and host word
  k_bsp_admit    free source slots with holes; a hole among the batch slots; R spanning one, two and three batches; R = 1; a pool
                 with exactly R free slots; one source more than free slots (error words set, earlier rows admitted, the rest
                 untouched); max_len - 2 below D0 (the first draft length)
  k_bsp_fill     Ls_new = 2, below and equal to Ls_cap; drafts_new null (smart: drafts_all untouched) and given; K * ld below and
                 above 256; T_cap 3 and 700 (past one pass of the block); kv_row 128 and 2 048 (one and two passes of 256 float4);
                 R = 1 and 5 with scattered new_slot; neighbouring slots, their K/V and other sources' caller rows untouched
  k_bsp_prep     an empty slot; a batch's first iteration (candidates 1 .. K-1 dead); K = 1, 5, 32; all drafts with N = 1, 3, 64;
                 smart libraries of 1, 255, 256, 257 and 600 windows (one to three scan rounds); keys with no window, fewer than
                 N, exactly N, more than N with the (N+1)-th in the next round; a given width above Ls_cap (windows run into the
                 replace token); D0 = 0; two batches (bat_grp over a batch's own candidates, on top of the value publish left);
                 cand_dl from a shrunk bat_dl
  k_bsp_select   (K, D0) = (1, 0), (2, 10), (10, 10), (5, 17), (32, 17) (144 KiB of LDS); beam 1 and K in one launch; ties inside
                 and across segments; finished roots with their PAD leaf; EOS leaves only (BP_DONE); exactly K leaves; K - 1
                 leaves (record, state and bat_state only); T_cap reached; all children of one parent, one child per parent, a
                 finished child listed before a running child of the same parent; empty slots between live ones; two batches
                 (bat_longest_cur per batch)
  k_bsp_batches  C = 5 and 300 (two blocks); room below 1, 1, and above bat_dl; max_steps reached, not reached and 0; a raised
                 batch (bat_iter only); free batch slots
  k_bsp_retire   every (source state, batch state) pair; `out` for BP_DONE / BP_STOPPED only; the last source of a batch frees
                 its slot, with others live it does not; dev_summary over several live sources
  k_bsp_publish  C = 5 and 300; bat_grp 1 only for live batches with a finished source; the host words and the order of their
                 contents (steps_done from the counters); the error word; dev_summary reset
  chained        util_bsp_checks.CHAINS: init, then per iteration admit + fill when the schedule says so, prep, the synthetic
                 step from the downloaded state, select, batches, retire, publish; the State after every launch, and `out`,
                 `summary`, `trace_len` against the per-batch loop at the end
  refusals       everything ttx_debug_bsp refuses: TTX_ERR_INVALID and nothing written
"""
import numpy as np
import pytest
import torch

import util_beam_checks as B
import util_bsp_checks as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


class Pool:
    """A State on the device: one guarded buffer per array, the words on the host."""

    def __init__(self, native, S: P.State):
        self.native, self.p = native, S.p
        self.bufs = B.upload(S.a, DEV)
        self.words = list(S.w)

    def put(self, S: P.State, names) -> None:
        for k in names:
            self.bufs[k].set(S.a[k])

    def arrays(self) -> dict:
        return B.download(self.bufs, list(self.bufs))

    def launch(self, op: str, want: P.State, what: str, R: int = 0, first_row: int = 0, stage: dict | None = None) -> None:
        """One launch of ``op``; afterwards the device holds ``want``, exactly and everywhere."""
        extra, staged = {}, {}
        if stage is not None:
            staged = B.upload({k: v for k, v in stage.items() if v is not None}, DEV)
            extra = dict(Ls_new=stage["tok_new"].shape[1], kv_row=stage["memkv_new"].shape[2])
        ops = {k: B.dev(b) for k, b in {**self.bufs, **staged}.items()}
        self.words = self.native.debug_bsp(op, self.words, **P.scalars(self.p), R=R, first_row=first_row, **extra, **ops)
        if DEV == "cuda":
            torch.cuda.synchronize()
        B.check_margins(self.bufs)
        B.check_margins(staged)
        B.check_inputs(staged, stage or {}, list(staged))
        P.compare(self.arrays(), self.words, want, f"{what}: after {op}")

    def refused(self, op: str, S: P.State, what: str, stage: dict | None = None, null=(), R: int = 0, first_row: int = 0, **change) -> None:
        import translation_transformer_amd as t
        staged = B.upload({k: v for k, v in (stage or {}).items() if v is not None}, DEV)
        ops = {k: B.dev(b) for k, b in {**self.bufs, **staged}.items() if k not in null}
        kw = {**P.scalars(self.p), "R": R, "first_row": first_row}
        if stage is not None:
            kw.update(Ls_new=stage["tok_new"].shape[1], kv_row=stage["memkv_new"].shape[2])
        unaligned = change.pop("unaligned", None)
        if unaligned:
            ops[unaligned] = ops[unaligned].reshape(-1)[1:]
        kw.update(change)
        with pytest.raises(t._native.TtxError) as e:
            self.native.debug_bsp(op, self.words, **kw, **ops)
        assert e.value.code == t._native.TTX_ERR_INVALID, f"{what}: {e.value}"
        B.check_margins(self.bufs)
        P.compare(self.arrays(), self.words, S, f"{what}: refused {op} wrote")


def run(native, op: str, S: P.State, what: str, *args) -> P.State:
    """Upload S, launch, compare with the rule's State; (R, first_row[, stage]) for admit / fill."""
    want = P.RULES[op](S, *args)
    kw = dict(zip(("R", "first_row", "stage"), args))
    Pool(native, S).launch(op, want, what, **kw)
    return want


# -- k_bsp_init --------------------------------------------------------------------------------------------------------------
INIT = [(1, 1), (5, 3), (300, 2), (1024, 32)]


@pytest.mark.parametrize("C,K", INIT)
def test_init(native, C, K):
    p = P.params(C=C, K=K, N=1 if C > 300 else 3, D0=1 if C > 300 else 4, Ls_cap=6, max_len=8, smart=False, T_cap=4)
    assert (C * K > 64 * 256) == (C == 1024), "the last case alone needs the grid stride"
    run(native, "init", P.blank(p, 3, 2, kv_row=4), f"C {C} K {K}")


# -- k_bsp_admit -------------------------------------------------------------------------------------------------------------
def admit_state(case: str):
    """-> (State, R, first_row).  Work list: batches of 2, 1, 3, 2 sources (rows 0-1, 2, 3-5, 6-7), then what the pool holds."""
    p = P.params(C=8, K=3, N=2, D0=4, Ls_cap=9, max_len=5 if case == "tiny" else 12, smart=False, T_cap=5)
    held = dict(holes=[dict(slot=0, id=4, srcs=[0, 3], it=2), dict(slot=2, id=5, srcs=[5], it=1)],        # free: 1 2 4 6 7; batch slot 1 free between 0 and 2
                exact=[dict(slot=1, id=4, srcs=[0, 1, 2, 4, 7], it=3)],                                  # free: 3 5 6
                empty=[])
    S = P.build(p, held["holes" if case in ("holes2", "holes3", "one", "over") else ("exact" if case == "exact" else "empty")], rows=14,
                n_batches=6, seed=len(case))
    S.a["batch_all"][:8], S.a["len_all"][:8], S.a["given_all"][:4] = [0, 0, 1, 2, 2, 2, 3, 3], [5, 9, 7, 6, 8, 9, 4, 9], [9, 8, 11, 9]
    R, first = dict(holes2=(3, 0), holes3=(5, 1), one=(1, 2), exact=(3, 3), empty=(8, 0), over=(6, 0), tiny=(2, 0))[case]
    return S, R, first


ADMIT = ["holes2", "holes3", "one", "exact", "empty", "over", "tiny"]


@pytest.mark.parametrize("case", ADMIT)
def test_admit(native, case):
    S, R, first = admit_state(case)
    want = run(native, "admit", S, case, R, first)
    free = int((S.a["row_of"] < 0).sum())
    if case == "over":
        assert R == free + 1 and want.w[P.W_ERROR] == 1 and want.a["dev_summary"][2] == 1
        assert (want.a["row_of"] >= 0).all() and want.a["new_slot"][R - 1] == S.a["new_slot"][R - 1], "earlier rows admitted, the last untouched"
    else:
        assert want.w[P.W_ERROR] == S.w[P.W_ERROR] and want.a["dev_summary"][2] == 0
        assert (case != "exact" or free == R) and sorted(want.a["new_slot"][:R]) == sorted(np.flatnonzero(S.a["row_of"] < 0)[:R])
    if case == "tiny":
        assert want.a["bat_dl"][0] == 3 < S.p.D0, "max_len 5 leaves room for 3 draft tokens after <BOS>"
    if case.startswith("holes"):
        assert want.a["bat_id"][1] == S.a["batch_all"][first], "the hole among the batch slots is taken first"
        assert len(set(S.a["batch_all"][first:first + R])) == int(case[-1])


# -- k_bsp_fill --------------------------------------------------------------------------------------------------------------
FILL = [dict(K=2, max_len=8, D0=2, T_cap=3, kv_row=128, R=1, Ls_new=2, smart=True),              # K * ld = 24
        dict(K=2, max_len=8, D0=2, T_cap=3, kv_row=128, R=5, Ls_new=6, smart=False),
        dict(K=5, max_len=60, D0=5, T_cap=700, kv_row=2048, R=5, Ls_new=9, smart=False),         # K * ld = 335, Ls_new = Ls_cap
        dict(K=5, max_len=60, D0=5, T_cap=700, kv_row=128, R=1, Ls_new=9, smart=True)]


@pytest.mark.parametrize("kw", FILL, ids=lambda k: "-".join(f"{a}{v}" for a, v in k.items()))
def test_fill(native, kw):
    p = P.params(C=8, K=kw["K"], N=3, D0=kw["D0"], Ls_cap=9, max_len=kw["max_len"], smart=kw["smart"], T_cap=kw["T_cap"])
    assert (p.K * p.ld > 256) == (kw["K"] == 5)
    R, first = kw["R"], 4
    S = P.blank(p, 12, 3, kv_row=kw["kv_row"])
    slots = [6, 1, 3, 7, 0][:R]                                            # scattered, not ascending
    S.a["new_slot"][:R] = slots
    rng = np.random.default_rng(R)
    tok = rng.integers(5, 30, size=(R, kw["Ls_new"])).astype(np.int32)
    tok[:, -1] = P.PAD
    stage = dict(tok_new=tok, valid_new=(tok != P.PAD).astype(np.uint8),
                 drafts_new=None if p.smart else rng.integers(5, 30, size=(R, p.N, p.D0)).astype(np.int32),
                 memkv_new=rng.standard_normal((R, kw["Ls_new"], kw["kv_row"])).astype(np.float32))
    want = run(native, "fill", S, str(kw), R, first, stage)
    for s in set(range(p.C)) - set(slots):                                 # what `compare` has shown already, said once in words
        B.same(want.a["memkv"][s], S.a["memkv"][s], f"K/V of the neighbouring slot {s}")
        B.same(want.a["cand_next"][s * p.K:(s + 1) * p.K], S.a["cand_next"][s * p.K:(s + 1) * p.K], f"rows of slot {s}")
    B.same(want.a["out"][:first], S.a["out"][:first], "caller rows of earlier sources")
    B.same(want.a["trace_len"][first + R:], S.a["trace_len"][first + R:], "caller rows of later sources")
    if p.smart:
        B.same(want.a["drafts_all"], S.a["drafts_all"], "drafts_all in smart mode")


# -- k_bsp_prep --------------------------------------------------------------------------------------------------------------
PREP = [dict(K=1, N=1, D0=5, smart=False), dict(K=5, N=3, D0=4, smart=False), dict(K=32, N=64, D0=3, smart=False),
        dict(K=5, N=3, D0=0, smart=False), dict(K=5, N=3, D0=0, smart=True, n_lib=300)] + \
       [dict(K=5, N=3, D0=5, smart=True, n_lib=n) for n in (1, 255, 256, 257, 600)] + \
       [dict(K=4, N=1, D0=4, smart=True, n_lib=257), dict(K=4, N=64, D0=2, smart=True, n_lib=600),
        dict(K=5, N=3, D0=5, smart=True, n_lib=40, Ls_cap=30)]              # the given width 45 is above the slot width 30


@pytest.mark.parametrize("kw", PREP, ids=lambda k: "-".join(f"{a}{v}" for a, v in k.items()))
def test_prep(native, kw):
    n_lib = kw.get("n_lib", 20)
    given = n_lib + 5
    p = P.params(C=6, K=kw["K"], N=kw["N"], D0=kw["D0"], Ls_cap=kw.get("Ls_cap", given), max_len=20, smart=kw["smart"], T_cap=4)
    # slot 0: batch A in its first iteration; 1: empty; 2, 3: batch B (draft length shrunk to 2, a finished source before);
    # 4: empty; 5: batch A.  Batch slots 3 (A) and 0 (B).
    layout = [dict(slot=3, id=0, srcs=[0, 5], it=0, given=given, grp=0),
              dict(slot=0, id=1, srcs=[2, 3], it=4, given=given, dl=min(2, p.D0), grp=1, nfin=1)]
    S = P.build(p, layout, rows=5, n_batches=2, seed=n_lib + p.K)
    rng = np.random.default_rng(p.K)
    if p.smart:
        for s in (0, 2, 3, 5):
            P.plant_keys(S, s, n_lib, rng)
        for k in range(p.K):                                               # slot 3 keeps its keys; slot 2 ends in the key without a window
            S.a["cand_next"][2 * p.K + k, S.a["len_next"][2 * p.K + k] - 1] = 10
    want = run(native, "prep", S, str(kw))
    a = want.a
    assert not a["live"][p.K:2 * p.K].any() and not a["live"][1:p.K].any() and a["live"][0] == 1, "empty slot / first iteration"
    assert (a["cand_dl"][2 * p.K:4 * p.K] == min(2, p.D0)).all() and a["cand_dl"][0] == p.D0
    if p.smart and n_lib >= 255 and 1 < p.N < 64 and p.K >= 4:
        assert set(a["per_cand"][3 * p.K:4 * p.K]) == {1, p.N - 1, p.N}, "the keys no longer cover none / fewer / N / more"
        assert a["bat_grp"][0] == p.N and a["bat_grp"][3] == 1, "each batch's group width over its own candidates"


# -- k_bsp_select ------------------------------------------------------------------------------------------------------------
SELECT = [(1, 0), (2, 10), (10, 10), (5, 17), (32, 17)]
PATTERNS = ["random", "ties", "exact", "short", "done", "one_parent", "one_each", "fin_first"]


@pytest.mark.parametrize("K,D0", SELECT)
def test_select(native, K, D0):
    C = 12
    p = P.params(C=C, K=K, N=3, D0=D0, Ls_cap=8, max_len=40, smart=False, T_cap=3)
    assert (2 * K * (D0 + 1) * K * 4 > 64 * 1024) == (K == 32)
    # batch A (slot 4, first iteration: beam 1) in source slots 0 and 9; batch B (slot 0, 6th iteration, past T_cap) in 2, 3, 5, 6,
    # 7, 8, 10, 11, one pattern each; slots 1 and 4 empty.
    mates = [2, 3, 5, 6, 7, 8, 10, 11]
    layout = [dict(slot=4, id=0, srcs=[0, 9], it=0, longest_cur=0), dict(slot=0, id=1, srcs=mates, it=5, longest_cur=0)]
    S = P.prep(P.build(p, layout, rows=10, n_batches=2, seed=K * 100 + D0))
    rng = np.random.default_rng(K + D0)
    for k in P.STEP_OUT:                                                   # the step has written every candidate's record
        S.a[k][...] = 0
    for s, pattern in zip([0, 9] + mates, ["random", "ties"] + PATTERNS):
        P.plant_leaves(S, s, pattern, rng)
    cov = set()
    want = P.select(S, cov=cov)
    P.check_cache_slots(S, want)
    Pool(native, S).launch("select", want, f"K {K} D0 {D0}")
    a = want.a
    assert a["src_state"][6] == P.ERR_LEAVES and a["bat_state"][0] == 2 and a["src_state"][7] == P.DONE, "K - 1 leaves / EOS leaves only"
    B.same(a["cand_next"][6 * K:7 * K], S.a["cand_next"][6 * K:7 * K], "rows of the source that ran short")
    assert "it - 1 >= T_cap" in cov and a["trace_len"][0, 0] > 0
    assert a["bat_longest_cur"][4] == a["src_acc"][[0, 9], 5].max() and a["bat_longest_cur"][0] == a["src_acc"][mates, 5].max()
    if K > 1:
        assert {"cache slot: running", "cache slot: finished", "cache slot: spare"} <= cov
        assert len(set(a["parent"][8 * K:9 * K])) == 1 and len(set(a["parent"][10 * K:11 * K])) == K, "all of one parent / one each"
        first_two = a["parent"][11 * K] == a["parent"][11 * K + 1] and a["fin_next"][11 * K] == 1 and a["fin_next"][11 * K + 1] == 0
        assert first_two and a["cache_slot"][11 * K + 1] == S.a["cache_slot"][a["parent"][11 * K]], "the running child inherits, not the first"


# -- k_bsp_batches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_steps", [0, 3, 100])
@pytest.mark.parametrize("C", [5, 300])
def test_batches(native, C, max_steps):
    p = P.params(C=C, K=2, N=1, D0=5, Ls_cap=6, max_len=20, smart=False, T_cap=4, max_steps=max_steps)
    S = P.blank(p, 2, 2, kv_row=4)
    a, rng = S.a, np.random.default_rng(C)
    a["bat_id"][:] = np.where(rng.random(C) < 0.7, np.arange(C), -1)
    a["bat_id"][:5] = [0, -1, 2, 3, 4]
    a["bat_iter"][:] = rng.integers(0, 5, size=C)
    a["bat_state"][:] = np.where(rng.random(C) < 0.2, 2, 0)
    a["bat_dl"][:] = rng.integers(1, 6, size=C)
    a["bat_longest_fin"][:], a["bat_longest_cur"][:] = rng.integers(0, 22, size=C), rng.integers(0, 22, size=C)
    # slot 0: room 0; slot 2: room 1 under a draft length of 4; slot 3: room above the draft length, iteration 3 next; slot 4: raised
    a["bat_longest_fin"][:5], a["bat_longest_cur"][:5] = [19, 0, 3, 7, 19], [12, 0, 18, 9, 19]
    a["bat_dl"][:5], a["bat_iter"][:5], a["bat_state"][:5] = [3, 9, 4, 2, 3], [1, 9, 1, 2, 2], [0, 0, 0, 0, 2]
    want = run(native, "batches", S, f"C {C} max_steps {max_steps}")
    w = want.a
    assert w["bat_state"][0] == 1 and w["bat_dl"][0] == 1 and w["bat_dl"][2] == 1 and w["bat_dl"][3] == 2
    assert w["bat_state"][2] == 0 and w["bat_state"][3] == (3 if max_steps == 3 else 0)
    assert w["bat_iter"][4] == 3 and w["bat_dl"][4] == 3 and w["bat_longest_cur"][4] == 19, "a raised batch only counts the iteration"
    assert w["bat_iter"][1] == 9, "a free batch slot is left alone"


# -- k_bsp_retire ------------------------------------------------------------------------------------------------------------
def test_retire(native):
    K = 3
    p = P.params(C=18, K=K, N=2, D0=3, Ls_cap=7, max_len=14, smart=False, T_cap=4)
    pairs = [(st, bst) for st in (P.RUNNING, P.DONE, P.ERR_LEAVES) for bst in (0, 1, 2, 3)]
    layout = [dict(slot=i, id=i, srcs=[i], it=3 + i, state=bst) for i, (st, bst) in enumerate(pairs)]
    layout += [dict(slot=14, id=12, srcs=[12, 13, 16], it=2, state=0, nfin=1, longest_fin=4),     # one of three retires: the batch stays
               dict(slot=12, id=13, srcs=[14, 17], it=4, state=1)]                                 # both retire: the batch slot is freed
    S = P.build(p, layout, rows=17, n_batches=14, seed=5)
    for i, (st, bst) in enumerate(pairs):
        S.a["src_state"][i] = st
    S.a["src_state"][[12, 13, 16, 14, 17]] = [P.RUNNING, P.DONE, P.RUNNING, P.DONE, P.RUNNING]
    S.a["src_acc"][:, 5] = np.arange(18) % 9 + 2
    S.a["dev_summary"][:] = [0, 0, 0, -9]
    cov = set()
    want = P.retire(S, cov=cov)
    Pool(native, S).launch("retire", want, "every pair")
    a = want.a
    assert {f"status {i}" for i in range(5)} <= cov and "BP_DONE turned into BP_ERR_LEAVES" in cov
    written = [r for r in range(17) if (a["out"][r] != S.a["out"][r]).any()]
    assert written == [r for r in range(17) if a["summary"][r, 1] in (P.DONE, P.STOPPED) and a["row_of"].tolist().count(r) == 0]
    assert a["bat_id"][14] == 12 and a["bat_live"][14] == 2 and a["bat_longest_fin"][14] == max(4, S.a["src_acc"][13, 5])
    assert a["bat_id"][12] == -1 and a["bat_live"][12] == 0
    live = [s for s in range(18) if a["row_of"][s] >= 0]
    assert len(live) >= 3 and a["dev_summary"][0] == len(live) and a["dev_summary"][1] == S.a["src_acc"][live, 6].sum()


# -- k_bsp_publish -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("error", [0, 1])
@pytest.mark.parametrize("C", [5, 300])
def test_publish(native, C, error):
    p = P.params(C=C, K=2, N=1, D0=5, Ls_cap=6, max_len=20, smart=True, T_cap=4)
    S = P.blank(p, 2, 2, kv_row=4)
    a, rng = S.a, np.random.default_rng(C)
    a["bat_id"][:] = np.where(rng.random(C) < 0.6, np.arange(C), -1)
    a["bat_nfin"][:] = rng.integers(0, 3, size=C)
    a["bat_grp"][:] = rng.integers(0, 4, size=C)
    a["bat_id"][:4], a["bat_nfin"][:4], a["bat_grp"][:4] = [0, 1, -1, -1], [0, 2, 0, 2], 3
    a["dev_summary"][:] = [11, 29, error, -9]
    S.w = [41, 1, 2, 3, 4, 5, 6, 7, 40, 8, 9, 0]
    want = run(native, "publish", S, f"C {C}")
    assert want.a["bat_grp"][:4].tolist() == [0, 1, 0, 0] and want.a["dev_summary"].tolist() == [0, 0, error, -9]
    assert want.w[8:] == [41, 11, 29, error] and want.w[:8] == S.w[:8]


# -- the chained scenarios ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", P.CHAINS, ids=lambda k: "-".join(str(v) for v in k))
def test_chain(native, key):
    pool, launches = [], [0]

    def apply(op, before, after, *args):
        what = f"{key} launch {launches[0]}"
        if op == "init":
            pool.append(Pool(native, before))
        if op == "synth":                                                  # the step, computed on the host from the downloaded state
            got = pool[0].arrays()
            P.compare(got, pool[0].words, before, f"{what}: before the step")
            pool[0].put(after, P.STEP_OUT)
            pool[0].words = list(after.w)
            return
        kw = dict(zip(("R", "first_row", "stage"), args))
        pool[0].launch(op, after, what, **kw)
        launches[0] += 1

    S, log, p, w, kn = P.run_chain(*key, apply=apply)
    final = pool[0].arrays()
    dev = P.State(p, final, pool[0].words)
    P.check_against_per_batch(dev, log, p, w, kn)
    print(f"{key}: {launches[0]} launches, {S.w[P.W_CALLS]} iterations")


# -- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(native):
    p = P.params(C=4, K=2, N=2, D0=3, Ls_cap=6, max_len=10, smart=False, T_cap=4)
    S = P.build(p, [dict(slot=0, id=0, srcs=[0], it=1)], rows=4, n_batches=2, seed=1)
    S.a["new_slot"][:2] = [1, 2]
    rng = np.random.default_rng(0)
    tok = rng.integers(5, 9, size=(2, 4)).astype(np.int32)
    stage = dict(tok_new=tok, valid_new=np.ones((2, 4), np.uint8), drafts_new=rng.integers(5, 9, size=(2, 2, 3)).astype(np.int32),
                 memkv_new=rng.standard_normal((2, 4, 8)).astype(np.float32))
    S.a["memkv"] = B.sent((4, 6, 8), np.float32)
    pool = Pool(native, S)
    for op in P.OPS:
        adm = dict(R=2, first_row=1, stage=stage) if op in ("admit", "fill") else {}
        for name in ("row_of", "bat_dl", "cand_next", "leaf_cnt", "dev_summary", "drafts_all", "out", "trace_len", "given_all"):
            pool.refused(op, S, f"{op} without {name}", null=(name,), **adm)
        for change in (dict(C_=0), dict(K=0), dict(n=0), dict(D0=-1), dict(Ls_cap=0), dict(max_len=0), dict(T_cap=0), dict(max_steps=-1),
                       dict(C_=1025), dict(K=33), dict(n=65), dict(K=32, D0=31, ld=64), dict(K=32, D0=18, ld=64), dict(ld=p.ld - 1)):
            pool.refused(op, S, f"{op} with {change}", **{**adm, **change})
    pool.refused("init", S, "init without src_of", null=("src_of",))
    pool.refused("init", S, "init without cand_src_len", null=("cand_src_len",))
    pool.refused("admit", S, "admit without new_slot", null=("new_slot",), R=2, first_row=1)
    pool.refused("admit", S, "admit without cand_src_len", null=("cand_src_len",), R=2, first_row=1)
    for name in ("new_slot", "tok_new", "valid_new", "src_valid", "memkv", "memkv_new"):
        pool.refused("fill", S, f"fill without {name}", stage=stage, null=(name,), R=2, first_row=1)
    for op in ("admit", "fill"):
        for change in (dict(R=0), dict(R=5), dict(first_row=-1)):
            pool.refused(op, S, f"{op} with {change}", stage=stage, **{"R": 2, "first_row": 1, **change})
    for change in (dict(Ls_new=7), dict(Ls_new=0), dict(kv_row=6), dict(kv_row=0), dict(unaligned="memkv"), dict(unaligned="memkv_new")):
        pool.refused("fill", S, f"fill with {change}", stage=stage, R=2, first_row=1, **change)
    for op in (-1, len(P.OPS)):
        pool.refused(op, S, f"op {op}")
