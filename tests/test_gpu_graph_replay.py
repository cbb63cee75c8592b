"""Graph replay of the four decoding loops (csrc/ttx_api.hip: graph_replay): a step or iteration runs eagerly the first time its
key is seen, is captured the second time and replayed from then on; a workspace that grows drops every captured graph; a session
created under TTX_NO_GRAPH=1 never captures.  None of this may show in a result.

Per loop, on ONE fresh session: the same call three times (eager warm-up, capture, replay), a call at a larger shape that grows
workspaces (the generation bump drops the cache), the first call again, and the call once more on a session created under
TTX_NO_GRAPH=1.  Outputs are equal element for element across all of them, and so are the counters the entry point returns
(the millisecond fields are timings).

  greedy speculative   ttx_greedy_speculative_generate        B = 3, N = 2, D = 3
  slot pool            ttx_greedy_speculative_generate_pool   capacity 4 over 6 rows, every step split (graph phases 1, 2 and 3)
  beam speculative     ttx_beam_speculative_generate          B = 2, n_best = 3, N = 2
  beam pool            ttx_beam_speculative_generate_pool     capacity 2 over 3 sources
"""
import ctypes as C

import numpy as np
import pytest
import torch

import util_two_phase as T
from util_models import BOS, EOS, PAD, fixture_tokens, tiny_state

pytestmark = pytest.mark.gpu
MAX_LEN = 150


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


def counters(st):
    return {name: int(getattr(st, name)) for name, _ in st._fields_ if not name.endswith("_ms")}


def trimmed(rows):
    """Fixture rows as one batch, as wide as its longest row."""
    src = fixture_tokens()[0][rows]
    return src[:, :int((src != PAD).sum(1).max())].contiguous()


def lengths_of(src):
    return ((src != PAD) * torch.arange(1, src.shape[1] + 1)).amax(dim=1).numpy().astype(np.int32)


# -- the four entry points: (model, shape) -> ([output arrays], counters) --------------------------------------------------------
def greedy_speculative(model, rows):
    from translation_transformer_amd import _native as NA
    src = trimmed(rows).to(model.device)
    B, Ls = src.shape
    out = torch.zeros((B, MAX_LEN), dtype=torch.int64, device=model.device)
    p, st = NA.GenParams(MAX_LEN, 3, 2, PAD, BOS, EOS, fixture_tokens()[2], 0), NA.GenStats()
    NA.check(model._lib.ttx_greedy_speculative_generate(model.session, src.data_ptr(), B, Ls, C.byref(p), out.data_ptr(), C.byref(st),
                                                        model._stream()))
    torch.cuda.synchronize()
    return [out.cpu().numpy()], counters(st)


def slot_pool(model, shape):
    from translation_transformer_amd import _native as NA
    rows, capacity = shape
    src_h = trimmed(rows)
    src = src_h.to(model.device)
    R, width = src.shape
    h_len = lengths_of(src_h)
    out = torch.zeros((R, MAX_LEN), dtype=torch.int64, device=model.device)
    traj = torch.zeros((R, MAX_LEN + 1), dtype=torch.int16, device=model.device)
    fin = torch.zeros((R,), dtype=torch.int32, device=model.device)
    sess = (C.c_void_p * 1)(model.session.value)
    p, st = NA.GenParams(MAX_LEN, 10, 3, PAD, BOS, EOS, fixture_tokens()[2], 0), NA.GenStats()
    NA.check(model._lib.ttx_greedy_speculative_generate_pool(sess, 1, src.data_ptr(), R, width, h_len.ctypes.data_as(C.POINTER(C.c_int32)),
                                                             capacity, C.byref(p), out.data_ptr(), traj.data_ptr(), fin.data_ptr(),
                                                             C.byref(st), model._stream()))
    torch.cuda.synchronize()
    return [out.cpu().numpy(), traj.cpu().numpy(), fin.cpu().numpy()], counters(st)


def beam_params(NA):
    return NA.BeamParams(MAX_LEN, 3, 5, 2, 0, PAD, BOS, EOS, fixture_tokens()[2], 300)


def beam_speculative(model, rows):
    from translation_transformer_amd import _native as NA
    src = trimmed(rows).to(model.device)
    B, Ls = src.shape
    out = torch.zeros((B, 3, MAX_LEN), dtype=torch.int64, device=model.device)
    p, st = beam_params(NA), NA.BeamStats()
    NA.check(model._lib.ttx_beam_speculative_generate(model.session, src.data_ptr(), B, Ls, C.byref(p), out.data_ptr(), C.byref(st),
                                                      model._stream()))
    torch.cuda.synchronize()
    return [out.cpu().numpy()], counters(st)


def beam_pool(model, shape):
    from translation_transformer_amd import _native as NA
    groups, capacity = shape
    rows = [r for g in groups for r in g]
    src_h = trimmed(rows)
    src = src_h.to(model.device)
    R, width = src.shape
    h_len = lengths_of(src_h)
    h_batch = np.repeat(np.arange(len(groups), dtype=np.int32), [len(g) for g in groups])
    h_given = np.array([h_len[h_batch == b].max() for b in range(len(groups))], dtype=np.int32)
    T_cap = MAX_LEN + 8
    out = torch.zeros((R, 3, MAX_LEN), dtype=torch.int64, device=model.device)
    tlen = torch.zeros((R, T_cap), dtype=torch.int16, device=model.device)
    summ = torch.zeros((R, 8), dtype=torch.int32, device=model.device)
    sess = (C.c_void_p * 1)(model.session.value)
    p, st = beam_params(NA), NA.BeamStats()
    i32 = C.POINTER(C.c_int32)
    NA.check(model._lib.ttx_beam_speculative_generate_pool(sess, 1, src.data_ptr(), R, width, h_len.ctypes.data_as(i32),
                                                           h_batch.ctypes.data_as(i32), len(groups), h_given.ctypes.data_as(i32), capacity,
                                                           C.byref(p), out.data_ptr(), tlen.data_ptr(), summ.data_ptr(), T_cap,
                                                           C.byref(st), model._stream()))
    torch.cuda.synchronize()
    return [out.cpu().numpy(), tlen.cpu().numpy(), summ.cpu().numpy()], counters(st)


LOOPS = {  # name: (call, the shape under test, a larger shape that grows workspaces)
    "greedy_speculative": (greedy_speculative, [0, 2, 3], [0, 2, 3, 4, 5, 6, 8]),
    "slot_pool": (slot_pool, ([0, 2, 3, 4, 5, 6], 4), ([0, 2, 3, 4, 5, 6, 8, 9, 0, 2], 8)),
    "beam_speculative": (beam_speculative, [2, 3], [0, 2, 3, 4]),
    "beam_pool": (beam_pool, ([[2, 3], [4]], 2), ([[0, 2, 3], [4, 5]], 4)),
}


@pytest.mark.parametrize("loop", list(LOOPS))
def test_eager_capture_replay_drop_and_no_graph_give_the_same_result(tta, monkeypatch, loop):
    call, shape, larger = LOOPS[loop]
    st, cfg = tiny_state()
    if loop == "slot_pool":                                  # as test_gpu_two_phase.py forces it: a probe graph for every step
        monkeypatch.setenv("TTX_TWO_PHASE", "1")
        monkeypatch.setenv("TTX_TWO_PHASE_MIN_ROWS", "0")
    monkeypatch.delenv("TTX_NO_GRAPH", raising=False)
    model = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    results = {name: call(model, shape) for name in ("eager warm-up", "capture", "replay")}
    call(model, larger)
    results["after the cache was dropped"] = call(model, shape)
    model.close()
    monkeypatch.setenv("TTX_NO_GRAPH", "1")
    eager = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    results["TTX_NO_GRAPH=1"] = call(eager, shape)
    eager.close()

    first, first_counters = results["eager warm-up"]
    assert first_counters["status"] == 0 and first_counters["model_calls"] > 0, first_counters
    assert any(a.any() for a in first), "the call wrote nothing"
    for name, (arrays, cnt) in results.items():
        for i, (a, b) in enumerate(zip(arrays, first)):
            assert a.shape == b.shape and np.array_equal(a, b), f"{loop}: output {i} of the {name} call differs from the first call"
        assert cnt == first_counters, f"{loop}: counters of the {name} call differ from the first call"
    if loop == "slot_pool":
        # graph phases 2 (draft pass + accept) and 3 (accept alone) both occurred, behind a probe (phase 1) each
        steps = T.pool_schedule(first[1], shape[1])
        assert len(steps) == first_counters["model_calls"]
        assert any(s[1] == 0 for s in steps) and any(s[1] > 0 for s in steps), steps
