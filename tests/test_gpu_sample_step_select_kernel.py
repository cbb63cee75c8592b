"""k_sample_step (csrc/ttx_sample.hip.h) as a pass of the sampling slot pool runs it, one launch at a time through
ttx_debug_sample_step_select: rows stored compacted under a row map (the draft pass under draft select), the pass's own active list,
a caller-chosen output buffer, and the probe layout N = 1, D = 0.

Every compacted pred[row] must EQUAL the token the full-layout launch (ttx_debug_sample_step, held to k_sample and to float64 by
tests/test_gpu_sample_step_kernel.py) gives layout row row_map[row] from the same logits row; the probe's token must equal
ttx_debug_sample's at front + 1; temperature 0 must equal k_argmax.  Sentinels stand beyond the live count, guard margins hold.
The row maps are tests/util_sample_pool.select_row_map's (k_probe_split's order), over a single draft, every non-empty subset at
N = 3, and all drafts.
"""
import itertools

import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_sample_pool as P
import util_sample_spec as X
from test_gpu_sample_kernel import make_logits, planted
from test_gpu_sample_step_kernel import B, DEV, SETTINGS, StepOperands

pytestmark = pytest.mark.gpu
ND = [(1, 1), (3, 2), (2, 5)]


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def mask_sets(N: int) -> list:
    """Per-slot draft masks of the B slots of a pass: a single draft everywhere, all drafts everywhere, and mixtures that cover every
    non-empty subset of the N drafts."""
    subsets = [sum(1 << n for n in c) for k in range(1, N + 1) for c in itertools.combinations(range(N), k)]
    out = [[1 << (N - 1)] * B, [(1 << N) - 1] * B]
    for off in range(0, len(subsets), B):
        out.append([subsets[(off + i) % len(subsets)] for i in range(B)])
    return out


def launch_select(native, ops: StepOperands, N, D, n_active, row_map, live=None, **kw) -> np.ndarray:
    n_rows = len(row_map) if row_map is not None else n_active * U.rps(N, D)
    live = n_rows if live is None else live
    x = ops.x[:n_rows] if row_map is None else ops.x[row_map]
    logits = U.Buf(x.shape, torch.float32, DEV, x)
    pred = U.Buf((n_rows + 3,), torch.int32, DEV)                       # the pass's own buffer; three rows it must not touch
    rm = None if row_map is None else U.Buf((n_rows,), torch.int32, DEV, row_map)
    native.debug_sample_step_select(logits.v, ops.key.v, ops.smp.v, ops.act.v, ops.front.v, pred.v, B=B, n=N, d=D, n_active=n_active,
                                    n_rows=n_rows, row_map=None if rm is None else rm.v,
                                    m_live=torch.tensor([live], dtype=torch.int32, device=DEV), **kw)
    torch.cuda.synchronize()
    for b in (logits, pred, ops.key, ops.smp, ops.act, ops.front) + (() if rm is None else (rm,)):
        assert b.margins() is None, b.margins()
    got = pred.get()
    assert (got[live:] == U.SENTINEL[torch.int32]).all(), "a row at or beyond the live count was written"
    return got[:live]


@pytest.mark.parametrize("N,D", ND)
@pytest.mark.parametrize("V", [5, 65, 256, 1024])
def test_compacted_rows_equal_the_full_layout(native, V, N, D):
    R = U.rps(N, D)
    ops = StepOperands(make_logits(B * R, V, seed=V * 100 + N * 10 + D), N, D, seed=V + N + D)
    for n_active in (B, 3):
        for i, kw in enumerate(SETTINGS[:2] if V > 65 else SETTINGS):
            seed = 0x9E3779B97F4A7C15 ^ (i << 40)
            full = ops.launch(native, n_active, seed=seed, pad=-1, eos=-2, **kw)
            for masks in mask_sets(N):
                row_map = P.select_row_map(masks[:n_active], N, D)
                # the compacted launch reads logits row i for layout row row_map[i]: hand it those rows of the full layout
                got = launch_select(native, ops, N, D, n_active, row_map, seed=seed, pad=-1, eos=-2, **kw)
                d = U.first_difference(got, full[row_map])
                assert d is None, f"V {V} N {N} D {D} n_active {n_active} masks {masks} {kw}: {d}"
            ident = launch_select(native, ops, N, D, n_active, None, seed=seed, pad=-1, eos=-2, **kw)
            assert (ident == full[:n_active * R]).all(), "a null row map is the identity"
    row_map = P.select_row_map([1] * B, N, D)
    part = launch_select(native, ops, N, D, B, row_map, live=len(row_map) - 2, seed=7)
    assert (part == launch_select(native, ops, N, D, B, row_map, seed=7)[:len(row_map) - 2]).all()


@pytest.mark.parametrize("V", [5, 65, 256, 1024])
def test_probe_layout_equals_k_sample_at_the_next_position(native, V):
    ops = StepOperands(make_logits(B * 2, V, seed=V + 1), 1, 1, seed=V)
    ops.x = ops.x[:B]                                                   # the probe has one row per slot
    for n_active in (B, 2):
        for i, kw in enumerate(SETTINGS):
            seed = 0x51ED270B ^ (i << 33)
            got = launch_select(native, ops, 1, 0, n_active, None, seed=seed, pad=-1, eos=-2, **kw)
            b = ops.act_np[:n_active]
            want = np.full(n_active, -1, dtype=np.int32)
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
            for r in range(n_active):                                   # k_sample takes one front per launch
                one = torch.full((1,), -1, dtype=torch.int32, device=DEV)
                native.debug_sample(t(ops.x[r:r + 1], torch.float32), t(ops.key_np[b[r]:b[r] + 1], torch.int64),
                                    t(ops.smp_np[b[r]:b[r] + 1], torch.int32), torch.zeros(1, dtype=torch.int32, device=DEV),
                                    t(ops.front_np[b[r]:b[r] + 1], torch.int32), one, 1, pad=-1, eos=-2, seed=seed, **kw)
                want[r] = int(one.cpu()[0])
            assert (got == want).all(), f"V {V} n_active {n_active} {kw}: probe {got.tolist()} against k_sample {want.tolist()}"


@pytest.mark.parametrize("N,D", ND + [(1, 0)])
@pytest.mark.parametrize("V", [5, 65, 1024])
def test_greedy_settings_equal_k_argmax(native, V, N, D):
    R = U.rps(N, D)
    ops = StepOperands(planted(B * R, V, seed=V + N), N, max(D, 1), seed=3) if D else None
    if ops is None:
        ops = StepOperands(planted(B * 2, V, seed=V + N), 1, 1, seed=3)
        ops.x = ops.x[:B]
    masks = [1] * B if D else None
    row_map = P.select_row_map(masks, N, D) if D else None
    x = ops.x[row_map] if D else ops.x
    want = U.Buf((len(x),), torch.int32, DEV)
    lg = U.Buf(x.shape, torch.float32, DEV, x)
    native.debug_argmax(lg.v, want.v, len(x))
    torch.cuda.synchronize()
    for kw in (dict(temperature=0.0), dict(temperature=1.0, top_k=1)):
        got = launch_select(native, ops, N, D, B, row_map, seed=11, **kw)
        d = U.first_difference(got, want.get())
        assert d is None, f"V {V} N {N} D {D} {kw}: {d}"


def test_refused_arguments(native):
    from translation_transformer_amd._native import TtxError
    N, D = 3, 2
    ops = StepOperands(make_logits(B * U.rps(N, D), 5, seed=1), N, D, seed=2)
    pred = U.Buf((B * 7,), torch.int32, DEV)
    a = (ops.logits.v, ops.key.v, ops.smp.v, ops.act.v, ops.front.v, pred.v)
    rm = torch.from_numpy(P.select_row_map([1] * B, N, D)).to(DEV)
    ok = dict(B=B, n=N, d=D, n_active=B, n_rows=len(rm), row_map=rm)
    bad_map = rm.clone()
    bad_map[3] = B * 7
    neg_map = rm.clone()
    neg_map[0] = -1
    for kw in (dict(temperature=-1.0), dict(top_k=33), dict(n_active=B + 1), dict(n=0), dict(d=0), dict(n=2, d=0), dict(B=0),
               dict(n_rows=0), dict(n_rows=B * 7 + 1), dict(row_map=bad_map), dict(row_map=neg_map), dict(row_map=None),
               dict(m_live=torch.tensor([len(rm) + 1], dtype=torch.int32, device=DEV)),
               dict(m_live=torch.tensor([-1], dtype=torch.int32, device=DEV))):
        with pytest.raises(TtxError):
            native.debug_sample_step_select(*a, **{**ok, **kw})
    torch.cuda.synchronize()
    assert (pred.get() == U.SENTINEL[torch.int32]).all() and pred.margins() is None      # nothing was launched
