"""k_sbs_step_masked (csrc/ttx_sbs.hip.h) one launch at a time through ttx_debug_sbs_step_ex, on the operands of
util_sbs_mask_checks.kernel_case, against the float64 restatement of tests/util_sbs_mask_checks.py with its checker
(tests/test_sbs_mask_checks_host.py shows that the checker can fail, and that these inputs keep float64 alone under half the cap).

The margin: max |G'_fp32 - G'_float64| over the selected, well-conditioned children of these very inputs, NumPy restatement in
float32 against float64 on the CPU, is 1.07e-5 (FP32_GAP = 1.1e-5 bounds it); ten times that, MARGIN = 1.1e-4.  A rank is excused
where a neighbouring rank's float64 G' is within MARGIN, a child is ill-conditioned (0 < Z - g < 1e-2), or its token changes between
kept and not kept when top_p moves by the sampler kernel test's TOL; at most 5 % of the ranks of a parametrisation (float64 alone:
at most 2.1 %).  Exact beside that: every integer output given the selected (parent, token) pairs, finished parents (the -inf ones
among them) carried bit for bit, sentinels in everything the rule does not write, guard margins, inputs untouched, a source alone
against the same source among others, 4 / 8 / 16 waves per source; V = 7 under a full mask against ttx_debug_sbs_step and top_k = 1
bit for bit; forced positions (token in range, out of range, EOS) with NaN logits that must not be read.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import util_beam_checks as B
import util_sbs_mask_checks as M
from test_gpu_sample_kernel import TOL
from test_gpu_sbs_kernel import IN, OUT, TRACE, SUMMARY0, arrays_of, sub_case, launch as launch_plain

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32, I64, F32, U8 = np.int32, np.int64, np.float32, np.uint8
PFX = ["pfx_tok", "pfx_len", "pfx_src"]


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def launch(native, mc: M.MaskCase, trace: bool = False, waves: int = 0, **over) -> dict:
    """Upload, one launch of the masked kernel, margins and inputs checked, the outputs back."""
    c = mc.c
    arrays = arrays_of(c, trace)
    names = IN + OUT + (TRACE if trace else [])
    extra = {}
    if mc.pfx_tok is not None:
        arrays.update(pfx_tok=mc.pfx_tok, pfx_len=mc.pfx_len, pfx_src=np.arange(c.B, dtype=I32))
        extra = dict(pfx_ld=mc.pfx_tok.shape[1], pfx_sources=mc.pfx_tok.shape[0])
    bufs = B.upload({k: arrays[k] for k in names + (PFX if extra else [])}, DEV)
    kw = dict(V=c.V, ld=c.ld, width=c.width, B=c.B, beam=c.beam, K=c.K, pad=c.pad, eos=c.eos, pos=c.pos, seed=c.seed,
              inv_T=float(np.float32(1.0) / np.float32(c.temperature)), top_k=mc.top_k, top_p=mc.top_p, waves=waves, **extra)
    kw.update(over)
    native.debug_sbs_step_ex(**kw, **{k: B.dev(bufs[k]) for k in bufs})
    torch.cuda.synchronize()
    B.check_margins(bufs)
    B.check_inputs(bufs, arrays, IN + (PFX if extra else []))
    return B.download(bufs, OUT + (TRACE if trace else []))


def sub_mask_case(mc: M.MaskCase, b: int) -> M.MaskCase:
    pfx = {} if mc.pfx_tok is None else dict(pfx_tok=mc.pfx_tok[b:b + 1], pfx_len=mc.pfx_len[b:b + 1])
    return mc._replace(c=sub_case(mc.c, b), **pfx)


def check_against_float64(mc: M.MaskCase, got: dict, what: str) -> int:
    """The integers exactly given the selection, the selection and values through the checker.  Returns the excused count."""
    c = mc.c
    excused = n_fin = 0
    for b in range(c.B):
        cs, ks = slice(b * c.beam, (b + 1) * c.beam), slice(b * c.K, (b + 1) * c.K)
        par_c = got["parent"][ks]
        assert ((par_c >= b * c.beam) & (par_c < (b + 1) * c.beam)).all(), f"{what}: parent outside source {b}: {par_c}"
        tok = got["new_cand"][ks, c.width]
        dev = SimpleNamespace(parent=par_c - b * c.beam, token=tok, phi=got["new_phi"][ks], g=got["new_g"][ks], finished=got["new_finished"][ks])
        ref, flip = M.case_reference(mc, b, tol=TOL)
        bad, ex = M.check_step(dev, ref, flip, c.G[cs], c.phi[cs], c.finished[cs], c.K, c.pad, c.eos, M.MARGIN)
        assert not bad, f"{what}, source {b}: " + "; ".join(bad[:4])
        excused += ex
        want = np.full((c.K, c.ld), c.pad, dtype=I64)
        want[:, :c.width] = c.gen[par_c, :c.width]
        want[:, c.width] = tok
        B.same(got["new_cand"][ks], want, f"{what}: new_cand of source {b}")
        if np.isfinite(c.G[cs][0]) and not c.finished[cs].all():
            assert got["new_g"][ks][0].tobytes() == c.G[cs][0].tobytes(), f"{what}: gumbel of rank 0 is not the first parent's G"
        n_fin += int(got["new_finished"][ks].sum())
    n = c.B * c.K
    B.same(got["new_len"], np.full(n, c.width + 1, I32), f"{what}: new_len")
    B.same(got["parent_draft"], np.zeros(n, I32), f"{what}: parent_draft")
    B.same(got["summary"], np.array([SUMMARY0[0] + n_fin] + SUMMARY0[1:], I32), f"{what}: summary")
    assert set(np.unique(got["new_finished"]).tolist()) <= {0, 1}
    return excused


def alone_agrees(native, mc: M.MaskCase, got: dict, b: int = 1):
    c = mc.c
    alone = launch(native, sub_mask_case(mc, b))
    check_against_float64(sub_mask_case(mc, b), alone, "alone")
    ks = slice(b * c.K, (b + 1) * c.K)
    for name in ("new_cand", "new_phi", "new_g", "new_len", "new_finished", "parent_draft"):
        B.same(alone[name], got[name][ks], f"source {b} alone against among others: {name}")
    B.same(alone["parent"], got["parent"][ks] - b * c.beam, f"source {b} alone against among others: parent")


CASES = [(V, beam, K, tk, tp, t) for V in M.KERNEL_V for beam, K in M.KERNEL_BEAM_K for tk, tp in M.KERNEL_FILTER for t in M.KERNEL_T]


@pytest.mark.parametrize("V,beam,K,top_k,top_p,t", CASES, ids=[f"V{v}-beam{b}-K{k}-k{tk}-p{tp}-T{t}" for v, b, k, tk, tp, t in CASES])
def test_sbs_step_masked(native, V, beam, K, top_k, top_p, t):
    """B = 3 sources in one launch against float64, then source 1 alone (B = 1): the same bits."""
    assert M.KEPT_TOL == TOL
    mc = M.kernel_case(V, beam, K, t, top_k, top_p)
    assert beam == 1 or np.isneginf(mc.c.G).sum() == 3          # a -inf parent per source
    got = launch(native, mc)
    excused = check_against_float64(mc, got, "B = 3")
    print(f"{excused} of {mc.c.B * K} ranks excused")
    assert excused <= M.EXCUSED_CAP * mc.c.B * K, f"{excused} of {mc.c.B * K} ranks excused"
    alone_agrees(native, mc, got)


@pytest.mark.parametrize("beam,K", M.KERNEL_BEAM_K)
@pytest.mark.parametrize("t", M.KERNEL_T)
def test_a_full_mask_is_k_sbs_step_bit_for_bit(native, beam, K, t):
    """V = 7 <= 32 with top_k = 32, top_p = 1 keeps every token: every output of the masked kernel is k_sbs_step's."""
    mc = M.kernel_case(7, beam, K, t, 32, 1.0)
    masked, plain = launch(native, mc, trace=True), launch_plain(native, mc.c, trace=True)
    for name in OUT + TRACE:
        B.same(masked[name], plain[name], f"full mask against k_sbs_step: {name}")
    off = launch(native, mc._replace(top_k=0))                  # filter off: the same kernel, every token kept
    for name in OUT:
        B.same(off[name], plain[name], f"filter off against k_sbs_step: {name}")


@pytest.mark.parametrize("V", M.KERNEL_V)
def test_top_k_1_keeps_the_first_maximum_exactly(native, V):
    """Every unfinished parent has one finite child, its first maximum, with phi' == phi and G' == G on the bits."""
    mc = M.kernel_case(V, 5, 5, 3.0, 1, 1.0)
    c = mc.c
    got = launch(native, mc)
    check_against_float64(mc, got, "top_k 1")
    for b in range(c.B):
        ks = slice(b * c.K, (b + 1) * c.K)
        for r in range(c.K):
            p = int(got["parent"][ks][r])
            tok, g = int(got["new_cand"][ks][r, c.width]), got["new_g"][ks][r]
            if c.finished[p] or np.isneginf(g):
                continue
            x = c.logits[c.slot_of[p]]
            assert tok == int(np.nonzero(x == x.max())[0][0])
            assert g.tobytes() == c.G[p].tobytes() and got["new_phi"][ks][r].tobytes() == c.phi[p].tobytes()


def test_wave_counts_agree_and_the_trace_records_the_selection(native):
    mc = M.kernel_case(256, 32, 32, 3.0, 32, 0.9)
    c = mc.c
    first = launch(native, mc, trace=True)
    for waves in (4, 8, 16):
        other = launch(native, mc, waves=waves)
        for name in OUT:
            B.same(first[name], other[name], f"{waves} waves: {name}")
    B.same(first["tr_parent"], first["parent"] - (np.arange(c.B * c.K, dtype=I32) // c.K) * c.beam, "trace: parent rank")
    B.same(first["tr_token"], first["new_cand"][:, c.width].astype(I32), "trace: token")
    B.same(first["tr_phi"], first["new_phi"], "trace: phi")
    B.same(first["tr_g"], first["new_g"], "trace: g")


FORCED = [(65, 1, 5, (7, 70), 0, 1.0), (65, 5, 5, (2, -1), 5, 1.0), (7, 5, 5, (0, 7), 0, 1.0), (1024, 32, 32, (1000, 1 << 20), 32, 0.9),
          (256, 5, 5, (2, 2), 0, 1.0)]


@pytest.mark.parametrize("V,beam,K,toks,top_k,top_p", FORCED, ids=[f"V{v}-beam{b}-K{k}-tok{t[0]}-{t[1]}-k{tk}" for v, b, k, t, tk, _ in FORCED])
def test_forced_positions(native, V, beam, K, toks, top_k, top_p):
    """Source 0 forced (in range; 2 is EOS, 0 is PAD), source 1 free, source 2 forced with a token that may lie outside [0, V) (read as
    0).  The logits rows of the forced sources are NaN: a forced position reads none.  Forced children carry phi and G on the bits."""
    mc = M.forced_case(V, beam, K, toks, top_k, top_p)
    c = mc.c
    x = c.logits.copy()
    for b in (0, 2):
        live = c.slot_of[b * beam:(b + 1) * beam]
        x[live[live >= 0]] = np.nan
    mc = mc._replace(c=c._replace(logits=x))
    c = mc.c
    got = launch(native, mc)
    check_against_float64(mc, got, "forced")
    for b, tok in ((0, toks[0]), (2, toks[1] if 0 <= toks[1] < V else 0)):
        ks = slice(b * K, (b + 1) * K)
        par, t, g, ph = got["parent"][ks], got["new_cand"][ks, c.width], got["new_g"][ks], got["new_phi"][ks]
        live = (c.finished[par] == 0) & np.isfinite(g)
        assert live.any() and (t[live] == tok).all()
        assert g[live].tobytes() == c.G[par[live]].tobytes() and ph[live].tobytes() == c.phi[par[live]].tobytes()
        assert (got["new_finished"][ks][live] == (1 if tok in (c.eos, c.pad) else 0)).all()
        dead = (c.finished[par] == 0) & ~np.isfinite(g)
        assert np.isneginf(g[dead]).all() and np.isneginf(ph[dead]).all() and (got["new_finished"][ks][dead] == 1).all()
    alone_agrees(native, mc, got, b=2)


REFUSED = [dict(top_k=33), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(waves=2), dict(waves=32),
           dict(K=33), dict(V=1025), dict(pos=0), dict(inv_T=0.0)]


@pytest.mark.parametrize("over", REFUSED, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_refusals_write_nothing(native, over):
    import translation_transformer_amd as t
    mc = M.kernel_case(7, 5, 5, 3.0, 5, 1.0)
    c = mc.c
    arrays = arrays_of(c)
    bufs = B.upload(arrays, DEV)
    kw = dict(V=c.V, ld=c.ld, width=c.width, B=c.B, beam=c.beam, K=c.K, pad=c.pad, eos=c.eos, pos=c.pos, seed=c.seed, inv_T=1.0,
              top_k=5, top_p=1.0)
    kw.update(over)
    with pytest.raises(t.TtxError) as e:
        native.debug_sbs_step_ex(**kw, **{k: B.dev(bufs[k]) for k in arrays})
    assert e.value.code == -1
    torch.cuda.synchronize()
    B.check_margins(bufs)
    B.check_inputs(bufs, arrays, list(arrays))


def test_refuses_a_prefix_table_outside_its_bounds(native):
    import translation_transformer_amd as t
    mc = M.forced_case(65, 5, 5, (7, 70))
    c = mc.c
    for bad in (dict(pfx_len=np.array([c.pos, c.pos + 5, 0], I32)),                       # a length above ld
                dict(pfx_len=np.array([c.pos, -1, 0], I32)),                               # a negative length
                dict(pfx_src=np.array([0, 3, 1], I32))):                                   # a source outside the table
        arrays = arrays_of(c)
        arrays.update(pfx_tok=mc.pfx_tok, pfx_len=bad.get("pfx_len", mc.pfx_len), pfx_src=bad.get("pfx_src", np.arange(3, dtype=I32)))
        bufs = B.upload(arrays, DEV)
        kw = dict(V=c.V, ld=c.ld, width=c.width, B=c.B, beam=c.beam, K=c.K, pad=c.pad, eos=c.eos, pos=c.pos, seed=c.seed, inv_T=1.0,
                  pfx_ld=mc.pfx_tok.shape[1], pfx_sources=3)
        with pytest.raises(t.TtxError) as e:
            native.debug_sbs_step_ex(**kw, **{k: B.dev(bufs[k]) for k in arrays})
        assert e.value.code == -1
        torch.cuda.synchronize()
        B.check_margins(bufs)
        B.check_inputs(bufs, arrays, list(arrays))
