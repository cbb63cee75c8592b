"""The beam family of csrc/ttx_loop_kernels.hip.h, one launch at a time: k_bs_prep, k_bs_list, k_bs_hits, k_bs_leaves (beam_leaves_core),
k_beam_select (select_best_leaves), k_beam_step and k_tree_cache through ttx_debug_bs_prep .. ttx_debug_tree_cache, which launch through
the production launch functions of csrc/ttx_api.hip, on operands the test builds, against the plain restatement of
tests/util_beam_checks.py: the restatement's value in every element a rule writes, the sentinel in every element it does not, intact
guard margins, untouched inputs.  Integer, flag and bit-copy outputs are exact; the flags of k_bs_hits may differ from the float64
nucleus only inside its 1e-5 margin (at most 1 % of a case's pairs, planted rows never); leaf scores and k_beam_step's scores lie
within the bound derived in util_beam_checks' docstring, and every case prints its largest error / bound.
tests/test_beam_checks_host.py pins the restatement to the oracle and shows that each checker can fail.

Paths of the kernels these cases execute on purpose:
  k_bs_prep      beam 1 and K; n_cand < the grid (tail workgroups write active / per_cand only); all drafts with dl < D0 (the stride)
                 and dl = D0; smart mode with libraries of 1, 255, 256, 257 and 600 windows (one to three scan rounds), keys with no
                 window (window 0), fewer than N (slots repeat the first), exactly N, more than N with the (N+1)-th in the next round;
                 N = 1 and 64; dl = 0
  k_bs_list      1 .. 600 candidates (one wave, four waves, a second and third round of 256); nobody, everybody, every other one
                 running, one wave of a round empty, only the last candidate; two launches on one counters image; the summary reset;
                 every DecState word
  k_bs_hits      V = 30 .. 1 024 under every logits-per-lane count that covers it (bit-identical flags); K = 1 .. 32, also above V;
                 N = 1 .. 64; planted rows with the draft token at the last kept rank, the first dropped one, rank K-1, rank K and on
                 either token of a duplicated logit; finished candidates, shorter groups, slot_of not the identity; the pool's dl_of
  k_bs_leaves    the same shapes and VPLs (bit-identical outputs); dl + 1 = 1, 2, 12 (one pass of the 12 waves), 13 (wraps), 41;
                 accepted lengths 0 .. dl; <BOS> excluded at the first rejected position and kept at position dl; the accepted token
                 excluded; an exact-zero logit inside the top K; finished candidates (one PAD leaf); 64 drafts (topk(1)'s other
                 branch); smart mode's -1-padded table; the pool's dead slots, dl_of < dl and a grp_of under which the choice differs
  k_beam_select  L = nseg * K of 1, 2 and 4; beam 1 and K; K = 1, 2, 10, 32; dl = 0, 10, 17 (K = 32: 576 segments, 144 KiB of LDS),
                 203 (K = 5: 1 020 segments); ties inside a segment, across segments and across the waves' quarters; every winner in
                 one quarter; a quarter with fewer than K leaves; -inf leaves; exactly K leaves; K - 1 leaves (summary[4], nothing
                 else); PAD / EOS / other leaf tokens; finished roots; ld_in != ld_out; all five summary words
  k_beam_step    V = 30 .. 1 024; beam 1, 3, 20 (80 KiB of LDS); K = beam and K > beam; finished parents; totals a gap apart (the
                 float64 order, exactly); bit-equal totals in two beams, two lanes, two waves and two passes of a thread (lower flat
                 index first); width 1 and ld - 2
  k_tree_cache   d = 64 and 256; 1 and 3 layers; fresh and inactive candidates; 0, 1 and 1 + prev_D new rows; parent drafts 0 and
                 N - 1; a parent that was not running; prev_D = 0; two buffers, and one buffer with slot maps (a child in its
                 parent's slot only appends, the others move)
"""
import numpy as np
import pytest
import torch

import util_beam_checks as B
import util_loop_checks as U

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def launch(fn, arrays: dict, names, outs, **scalars):
    """Upload, launch ``fn`` on the operands ``names``, and hand back the outputs ``outs``; margins and inputs are checked."""
    bufs = B.upload({k: arrays[k] for k in names}, DEV)
    res = fn(**scalars, **{k: B.dev(bufs[k]) for k in names})
    torch.cuda.synchronize()
    B.check_margins(bufs)
    B.check_inputs(bufs, arrays, [k for k in names if k not in outs])
    return B.download(bufs, outs), res


# -- k_bs_prep ---------------------------------------------------------------------------------------------------------------
PREP = [dict(B=3, beam=1, n_cand=3, max_cand=12, dl=5, N=3, smart=False, D0=9),          # first iteration: beam 1, tail workgroups, dl < D0
        dict(B=3, beam=4, n_cand=12, max_cand=12, dl=7, N=3, smart=False, D0=7),
        dict(B=2, beam=2, n_cand=4, max_cand=5, dl=0, N=1, smart=False, D0=0),           # standard beam search's shape
        dict(B=1, beam=4, n_cand=4, max_cand=4, dl=3, N=64, smart=False, D0=5)] + \
       [dict(B=2, beam=4, n_cand=8, max_cand=9, dl=5, N=3, smart=True, n_lib=n) for n in (1, 255, 256, 257, 600)] + \
       [dict(B=2, beam=4, n_cand=8, max_cand=8, dl=4, N=1, smart=True, n_lib=257),
        dict(B=1, beam=4, n_cand=4, max_cand=4, dl=2, N=64, smart=True, n_lib=600),
        dict(B=2, beam=4, n_cand=8, max_cand=8, dl=0, N=3, smart=True, n_lib=300)]


@pytest.mark.parametrize("kw", PREP, ids=lambda k: "-".join(f"{a}{v}" for a, v in k.items()))
def test_bs_prep(native, kw):
    c = B.prep_case(seed=len(str(kw)), **kw)
    want = B.bs_prep(c)
    if c.smart and c.n_lib >= 257 and c.N < 64:
        assert set(want["per_cand"][:c.n_cand]) == {1, c.N - 1, c.N} or c.N == 1, "the keys no longer cover none / fewer / N / more"
    names = [k for k in B.PREP_IN if k != ("drafts_all" if c.smart else "lib")] + B.PREP_OUT
    got, _ = launch(native.debug_bs_prep, B.prep_arrays(c), names, B.PREP_OUT, ld=c.ld, max_cand=c.max_cand, n_cand=c.n_cand, beam=c.beam,
                    dl=c.dl, n=c.N, pad=c.pad, smart=c.smart, n_lib=c.n_lib, lib_ld=c.lib_ld, D0=c.D0)
    B.check_exact(got, want, str(kw))


# -- k_bs_list ---------------------------------------------------------------------------------------------------------------
def activity(pattern: str, n: int) -> np.ndarray:
    a = np.zeros(n, np.uint8)
    if pattern == "all":
        a[:] = 1
    elif pattern == "alternate":
        a[::2] = 1
    elif pattern == "wave_empty":                                          # lanes 64 .. 127 of every round of 256 idle
        a[:] = 1
        a[(np.arange(n) % 256 >= 64) & (np.arange(n) % 256 < 128)] = 0
    elif pattern == "last":
        a[-1] = 1
    return a


@pytest.mark.parametrize("pattern", ["none", "all", "alternate", "wave_empty", "last"])
@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 255, 256, 257, 600])
def test_bs_list(native, n_cand, pattern):
    rng = np.random.default_rng(n_cand)
    rows, N, dl = n_cand + 3, 5, 4
    arrays = dict(active=np.ones(rows, np.uint8), per_cand=rng.integers(1, N + 1, size=rows).astype(np.int32),
                  len=rng.integers(1, 40, size=rows).astype(np.int32), act_idx=B.sent(rows, np.int32), slot_of=B.sent(rows, np.int32),
                  prev_len=B.sent(rows, np.int32), summary=np.array([9, 8, 7, 6, 5], np.int32))
    arrays["active"][:n_cand] = activity(pattern, n_cand)
    counters = [3, 1000, 900, 2 ** 33, 2 ** 34, 77, 12, 4]                 # sums beyond 32 bits stay sums
    names = list(arrays)
    for step in range(2):                                                  # the second launch continues the first one's image
        want, cnt, state = B.bs_list(arrays["active"], arrays["per_cand"], arrays["len"], n_cand, N, dl, counters, rows)
        got, words = launch(native.debug_bs_list, arrays, names, B.LIST_OUT, counters=counters, n_cand=n_cand, n=N, dl=dl)
        B.check_exact(got, want, f"n_cand {n_cand} {pattern} launch {step}")
        assert words[:8] == cnt, f"counters {words[:8]} expected {cnt}"
        assert words[8:] == state, f"DecState {words[8:]} expected {state}"
        counters = cnt
        arrays["active"][:n_cand] = activity("alternate" if pattern != "alternate" else "all", n_cand)
        arrays["summary"] = np.array([1, 2, 3, 4, 5], np.int32)


# -- k_bs_hits / k_bs_leaves -------------------------------------------------------------------------------------------------
LEAF_IDS = [f"V{c[0]}-K{c[1]}-N{c[2]}-dl{c[3]}" + ("-smart" if c[5] else "") + ("-pool" if c[6] else "") for c in B.LEAVES_CASES]


@pytest.mark.parametrize("kw", list(B.hits_cases()), ids=LEAF_IDS)
def test_bs_hits(native, kw):
    c = B.hits_case(**kw)
    ref = B.bs_hits(c)
    arrays = {k: getattr(c, k) for k in B.HITS_IN}
    arrays["hit"] = B.sent(ref.want.shape, np.uint8)
    names = [k for k in B.HITS_IN if k != "dl_of" or c.pool] + ["hit"]
    first = None
    for vpl in [0] + B.vpls_for(c.V):
        got, _ = launch(native.debug_bs_hits, arrays, names, ["hit"], V=c.V, max_cand=c.max_cand, n_cand=c.n_cand, n=c.N, dl=c.dl, K=c.K,
                        vpl=vpl)
        differ = B.check_hits(got["hit"], c, ref, f"{kw} vpl {vpl}")
        print(f"k_bs_hits {kw} vpl {vpl}: {int(ref.written.sum())} pairs, {len(c.plans)} planted, "
              f"{int((ref.near & ~c.planted).sum())} inside the margin, {differ} differ")
        first = got["hit"] if first is None else first
        B.same(got["hit"], first, f"{kw}: vpl {vpl} against the production choice")


@pytest.mark.parametrize("kw", list(B.leaves_cases()), ids=LEAF_IDS)
def test_bs_leaves(native, kw):
    c = B.leaves_case(**kw)
    arrays = B.leaves_arrays(c)
    names = [k for k in B.LEAVES_IN if c.pool or k not in ("live", "dl_of", "grp_of", "cand_batch")] + B.LEAVES_OUT
    if c.pool and not c.smart:
        names = [k for k in names if k not in ("grp_of", "cand_batch")]
    first = None
    for vpl in [0] + B.vpls_for(c.V):
        c.vpl = vpl
        ref = B.bs_leaves(c)
        got, _ = launch(native.debug_bs_leaves, arrays, names, B.LEAVES_OUT, V=c.V, max_cand=c.max_cand, n_cand=c.n_cand, n=c.N, dl=c.dl,
                        K=c.K, bos=c.bos, pad=c.pad, smart=c.smart, max_group=c.max_group, vpl=vpl)
        worst = B.check_leaves(got, c, ref, f"{kw} vpl {vpl}")
        print(f"k_bs_leaves {kw} vpl {vpl}: {int((~np.isnan(ref.score)).sum())} leaves, {sorted(c.features)}, error / bound {worst:.3f}")
        first = got if first is None else first
        B.check_exact(got, first, f"{kw}: vpl {vpl} against the production choice")
    if c.pool and c.smart:
        cc, W = c.sensitive
        own = int(ref.out["best_slot"][cc])
        c.grp_of = np.full(2, int(c.per_cand[cc]), np.int32)
        assert B.best_draft(c, cc)[0] != own, "the planted draft table no longer depends on the padded width"


def test_debug_entries_refuse_what_production_refuses(native):
    c = B.leaves_case(V=65, K=5, N=3, dl=2, n_cand=3, max_cand=3)
    arrays = B.leaves_arrays(c)
    names = [k for k in B.LEAVES_IN if k not in ("live", "dl_of", "grp_of", "cand_batch")] + B.LEAVES_OUT
    bufs = B.upload({k: arrays[k] for k in names}, DEV)
    ops = {k: B.dev(bufs[k]) for k in names}
    base = dict(V=c.V, max_cand=3, n_cand=3, n=3, dl=2, K=5, bos=1, pad=0)
    import translation_transformer_amd as t
    for change in (dict(K=33), dict(n=65), dict(V=1025), dict(K=32, dl=31), dict(vpl=4, V=257), dict(vpl=5)):
        with pytest.raises(t._native.TtxError):
            native.debug_bs_leaves(**{**base, **change}, **ops)
    for k, b in bufs.items():
        if k in B.LEAVES_OUT:
            B.same(b.get(), B.bits(arrays[k]), f"{k} after refused launches")


# -- k_beam_select -----------------------------------------------------------------------------------------------------------
ALL_PATTERNS = ["random", "ties", "one_quarter", "sparse", "neg_inf", "exact", "short"]
SELECT = [dict(B=1, beam=1, K=1, dl=0, pattern=p) for p in ("random", "short")] + \
         [dict(B=3, beam=1, K=2, dl=0, pattern=p, ld_extra=3) for p in ("random", "exact", "short")] + \
         [dict(B=3, beam=2, K=2, dl=0, pattern=p) for p in ("ties", "neg_inf", "sparse")] + \
         [dict(B=3, beam=10, K=10, dl=10, pattern=p, ld_extra=3) for p in ALL_PATTERNS] + \
         [dict(B=3, beam=1, K=10, dl=10, pattern=p) for p in ("random", "ties", "exact", "short")] + \
         [dict(B=1, beam=32, K=32, dl=17, pattern=p) for p in ("random", "ties", "one_quarter", "sparse")] + \
         [dict(B=1, beam=5, K=5, dl=203, pattern=p) for p in ("random", "ties", "neg_inf")]


@pytest.mark.parametrize("kw", SELECT, ids=lambda k: "-".join(f"{a}{v}" for a, v in k.items()))
def test_beam_select(native, kw):
    c = B.select_case(seed=len(str(kw)) + kw["K"], **kw)
    want = B.beam_select(c)
    if kw["pattern"] == "short":
        assert want["summary"][4] == 1
    else:
        assert want["summary"][4] == 0 and want["parent"][0] >= 0
    got, _ = launch(native.debug_beam_select, B.select_arrays(c), B.SELECT_IN + B.SELECT_OUT, B.SELECT_OUT, width=c.width, ld_in=c.ld_in,
                    ld_out=c.ld_out, B=c.B, beam=c.beam, dl=c.dl, K=c.K, pad=c.pad, eos=c.eos)
    B.check_exact(got, want, str(kw))


# -- k_beam_step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", list(B.step_cases()), ids=lambda k: "-".join(f"{a}{v}" for a, v in k.items() if a != "seed"))
def test_beam_step(native, kw):
    c = B.step_case(**kw)
    got, _ = launch(native.debug_beam_step, B.step_arrays(c), B.STEP_IN + B.STEP_OUT, B.STEP_OUT, V=c.V, ld=c.ld, width=c.width, B=c.B,
                    beam=c.beam, K=c.K, pad=c.pad, eos=c.eos)
    worst = B.check_step(got, c, str(kw), exact=c.kind != "random")
    print(f"k_beam_step {kw}: error / bound {worst:.3f}")


# -- k_tree_cache ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [False, True])
@pytest.mark.parametrize("d,layers,prev_N,prev_D", [(64, 1, 3, 4), (64, 3, 1, 0), (256, 3, 3, 4), (256, 1, 64, 1), (64, 1, 2, 10)])
def test_tree_cache(native, d, layers, prev_N, prev_D, slots):
    c = B.tree_case(d=d, layers=layers, n_cand=11, prev_N=prev_N, prev_D=prev_D, slots=slots, seed=d + prev_N)
    k_want, v_want = B.tree_cache(c)
    arrays = dict(len=c.len, parent=c.parent, parent_draft=c.parent_draft, prev_len=c.prev_len, active=c.active, qkv_prev=c.qkv,
                  prev_slot_of=c.prev_slot_of)
    if slots:
        arrays.update(k_new=c.k_old, v_new=c.v_old, slot_parent=c.slot_parent, slot_self=c.slot_self)
    else:
        arrays.update(k_old=c.k_old, v_old=c.v_old, k_new=B.sent(c.k_old.shape, np.float32), v_new=B.sent(c.k_old.shape, np.float32))
    bufs = B.upload(arrays, DEV)
    ops = {k: bufs[k].v for k in arrays}
    if slots:
        ops.update(k_old=ops["k_new"], v_old=ops["v_new"])
    kb = bufs["k_new"].v
    native.debug_tree_cache(max_cand=c.max_cand, layers=layers, prev_n=prev_N, prev_d=prev_D, d=d, cache_layer_stride=kb.stride(0),
                            cache_seq_stride=kb.stride(1), qkv_layer_stride=bufs["qkv_prev"].v.stride(0), **ops)
    torch.cuda.synchronize()
    B.check_margins(bufs)
    B.check_inputs(bufs, arrays, [k for k in arrays if k not in ("k_new", "v_new")])
    got = B.download(bufs, ["k_new", "v_new"])
    B.same(got["k_new"], k_want, "K cache")
    B.same(got["v_new"], v_want, "V cache")
