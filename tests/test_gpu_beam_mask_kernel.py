"""k_beam_step_masked (csrc/ttx_beam_mask.hip.h), one launch at a time through ttx_debug_beam_step_masked, against the restatement of
tests/util_beam_mask_checks.py (whose checker tests/test_beam_mask_checks_host.py shows to fail when it should).

  identity     finite logits, no table: every output equals ttx_debug_beam_step's on the same operands bit for bit
  restatement  the selection is the float64 order (the cases keep the finite totals a GAP apart, two orders of magnitude above the
               score bound of DESIGN §17, or equal by construction), every integer what that selection implies, finite scores inside
               the bound, a forced child's score its parent's on the bits, a dead row's -inf.  Kinds (util_beam_mask_checks.case): a
               tenth of the logits -inf with a finished parent, a dead parent and a live row without a finite logit beside live ones;
               sources with exactly K, K - 1, 1 and 0 finite children; forced positions with per-source prefix lengths (a forced source
               beside a free one, the table's rows permuted, an id outside the vocabulary); ties across identical parents
  shapes       V = 7, 64, 65, 256, 1 000 (the wave stride and the 256-thread stride); (beam, K) = (1, 3), (3, 3), (5, 5), and (32, 32)
               at V = 256; B = 3; width 1 and ld - 2
  memory       every output starts as sentinels and every array sits between guard margins (util_loop_checks.Buf); inputs are
               compared after the launch
  refusals     K > beam * V, width >= ld, a table outside its bounds
"""
import numpy as np
import pytest
import torch

import util_beam_checks as B
import util_beam_mask_checks as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
LD = 12


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def launch(fn, arrays: dict, c, extra=None):
    """Upload, launch ``fn`` on the case's operands, and hand back the outputs; margins and inputs are checked."""
    names = [k for k in M.STEP_IN + M.STEP_OUT + M.PFX_IN if k in arrays]
    bufs = B.upload({k: arrays[k] for k in names}, DEV)
    fn(V=c.V, ld=c.ld, width=c.width, B=c.B, beam=c.beam, K=c.K, pad=c.pad, eos=c.eos, **(extra or {}), **{k: B.dev(bufs[k]) for k in names})
    torch.cuda.synchronize()
    B.check_margins(bufs)
    B.check_inputs(bufs, arrays, [k for k in names if k not in M.STEP_OUT])
    return B.download(bufs, M.STEP_OUT)


def table_scalars(c) -> dict:
    return {} if c.pfx_len is None else dict(pfx_ld=c.pfx_ld, pfx_sources=len(c.pfx_tok))


SHAPES = [(beam, K, V) for V in (7, 64, 65, 256, 1000) for beam, K in ((1, 3), (3, 3), (5, 5))] + [(32, 32, 256)]
WIDTHS = [1, LD - 2]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("beam,K,V", SHAPES)
def test_identity_on_finite_logits(native, beam, K, V, width):
    c = M.case(beam=beam, K=K, V=V, kind="finite", width=width, ld=LD, seed=V + beam + width)
    a = M.arrays(c)
    got = launch(native.debug_beam_step_masked, a, c)
    ref = launch(native.debug_beam_step, a, c)
    for k in M.STEP_OUT:
        B.same(got[k], ref[k], f"{k} against k_beam_step")
    worst = M.check(got, c, f"finite beam {beam} K {K} V {V} width {width}")
    print(f"finite beam {beam} K {K} V {V} width {width}: error / bound {worst:.3f}")


def kinds_for(beam: int):
    return ["tenth", "few", "few0", "forced"] + (["tie"] if beam >= 5 else [])


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("beam,K,V,kind", [(b, K, V, kind) for b, K, V in SHAPES for kind in kinds_for(b)])
def test_against_the_restatement(native, beam, K, V, kind, width):
    c = M.case(beam=beam, K=K, V=V, kind=kind, width=width, ld=LD, seed=7 * V + beam + width)
    got = launch(native.debug_beam_step_masked, M.arrays(c), c, table_scalars(c))
    assert not np.isnan(got["new_score"]).any(), "a NaN score"
    worst = M.check(got, c, f"{kind} beam {beam} K {K} V {V} width {width}")
    print(f"{kind} beam {beam} K {K} V {V} width {width}: error / bound {worst:.3f}")


def test_an_empty_table_changes_nothing(native):
    """Prefix lengths below the width: the table is read for its lengths alone and the outputs are the free call's bits."""
    c = M.case(beam=5, K=5, V=65, kind="tenth", width=3, ld=LD, seed=3)
    free = launch(native.debug_beam_step_masked, M.arrays(c), c)
    c.pfx_ld, c.pfx_tok = 4, np.full((3, 4), 5, np.int32)
    c.pfx_len, c.pfx_src = np.array([2, 0, 1], np.int32), np.array([1, 2, 0], np.int32)
    got = launch(native.debug_beam_step_masked, M.arrays(c), c, table_scalars(c))
    for k in M.STEP_OUT:
        B.same(got[k], free[k], f"{k} under a table no source is inside")


def test_refused_arguments(native):
    import translation_transformer_amd as t
    c = M.case(beam=1, K=3, V=7, kind="forced", width=3, ld=LD, seed=1)
    a = M.arrays(c)

    def refused(extra=None, **change):
        d = M.NS(**{**vars(c), **change})
        with pytest.raises(t.TtxError):
            launch(native.debug_beam_step_masked, a, d, {**table_scalars(c), **(extra or {})})

    refused(K=8)                                                           # K > beam * V = 7
    refused(width=LD)
    refused(width=0)
    refused(dict(pfx_sources=2))                                           # a source row outside the table
    refused(dict(pfx_ld=3))                                                # lengths up to width + 1 = 4 beyond ld
    got = launch(native.debug_beam_step_masked, a, c, table_scalars(c))    # and the arguments as they are pass
    M.check(got, c, "forced")
