"""The cases of tests/test_gpu_pool_schedule.py and tests/golden/make_golden_pool_schedule.py: pool calls on ONE session of the tiny
fixture model through the public C ABI (greedy, beam, stochastic-beam and sampling pool).  On one session a pool's schedule is deterministic (one step in flight, the host decides
after each publish), so everything recorded here is a pure function of the admission rule and the step policy: integer counters,
the seven words of ttx_pool_last_counters, the per-row traces, the output tokens.  Times are not recorded."""
import ctypes as C
import os

import numpy as np
import torch

from util_models import BOS, EOS, PAD, fixture_tokens, tiny_state

MAX_LEN = 150
# greedy pool: 40 fixture rows of mixed lengths, longest first, through 8 slots; a budget of 100 padded rows splits every admission
# of two rows or more (the shortest row has 28 tokens, the quarter-pool minimum is 2 rows, and most admissions are wider)
GREEDY_ROWS, GREEDY_CAPACITY, GREEDY_ADMIT_ROWS = 40, 8, 100
GREEDY_CASES = {                      # name -> environment of the call
    "one_pass": {"TTX_TWO_PHASE": "0"},
    "default": {},
    "split_every_step": {"TTX_TWO_PHASE_MIN_ROWS": "0"},      # 8 slots stay below the default threshold: this one runs the probe path
}
# beam pool: six batches of 1 to 4 sources through 4 source slots
BEAM_BATCHES, BEAM_CAPACITY = [[5, 0], [1], [3, 7, 2, 8], [4, 9, 6], [2], [6, 1]], 4
BEAM_CASES = {"all_drafts": 0, "smart_drafts": 1}             # name -> smart_drafts_mode
# the stochastic-beam source pool and the sampling slot pool (tests/golden/pool_schedule_more.npz): the ten fixture sources, longest
# first, through 4 slots, so both pools are filled, refilled as rows retire and drained
MORE_CAPACITY = 4
SBS_MAX_LEN, SBS_BEAM, SBS_SEED = 30, 3, 0x5EED0B5C0FFEE
SAMPLE_PER_SRC, SAMPLE_SEED = 2, 0x5A3B1E5EED          # 2 decoder rows per source: 4 slots hold two sources
MORE_KEYS = [7, 1 << 40, 3, 99, 12345678901, 0, 5, (1 << 62) + 1, 42, 8]
ENV_KEYS = ("TTX_ADMIT_ROWS", "TTX_TWO_PHASE", "TTX_TWO_PHASE_MIN_ROWS", "TTX_DRAFT_SELECT")


def lengths_of(src):
    return ((src != PAD) * torch.arange(1, src.shape[1] + 1)).amax(dim=1).numpy().astype(np.int32)


def int_fields(st):
    return np.array([int(getattr(st, name)) for name, _ in st._fields_ if not name.endswith("_ms")], dtype=np.int64)


class pool_env:
    """The call's environment: the pool switches unset except for `env` (the library reads them at the start of every pool call)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if self.saved[k] is not None:
                os.environ[k] = self.saved[k]


def make_model(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)


def greedy_pool(model, case):
    """-> {stats, counters, traj, fin_step} of ttx_greedy_speculative_generate_pool over the 40 rows."""
    from translation_transformer_amd import _native as NA
    fsrc, _, c_token, _ = fixture_tokens()
    idx = [i % fsrc.shape[0] for i in range(GREEDY_ROWS)]
    idx.sort(key=lambda r: -int(lengths_of(fsrc[r:r + 1])[0]))
    src_h = fsrc[idx].contiguous()
    src = src_h.to(model.device)
    R, width = src.shape
    h_len = lengths_of(src_h)
    out = torch.zeros((R, MAX_LEN), dtype=torch.int64, device=model.device)
    traj = torch.zeros((R, MAX_LEN + 1), dtype=torch.int16, device=model.device)
    fin = torch.zeros((R,), dtype=torch.int32, device=model.device)
    sess = (C.c_void_p * 1)(model.session_pool(1)[0].value)
    p, st = NA.GenParams(MAX_LEN, 10, 3, PAD, BOS, EOS, c_token, 0), NA.GenStats()
    words = (C.c_int64 * 7)()
    with pool_env({"TTX_ADMIT_ROWS": str(GREEDY_ADMIT_ROWS), **GREEDY_CASES[case]}):
        NA.check(model._lib.ttx_greedy_speculative_generate_pool(sess, 1, src.data_ptr(), R, width, h_len.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                 GREEDY_CAPACITY, C.byref(p), out.data_ptr(), traj.data_ptr(),
                                                                 fin.data_ptr(), C.byref(st), model._stream()))
    torch.cuda.synchronize()
    NA.check(model._lib.ttx_pool_last_counters(sess[0], words))
    return {"stats": int_fields(st), "counters": np.array(list(words), dtype=np.int64), "traj": traj.cpu().numpy(),
            "fin_step": fin.cpu().numpy()}


def beam_pool(model, case):
    """-> {stats, trace_len, summary} of ttx_beam_speculative_generate_pool over the six batches, the batch with the longest source
    first (as generate_many hands them over)."""
    from translation_transformer_amd import _native as NA
    fsrc, _, c_token, _ = fixture_tokens()
    all_len = lengths_of(fsrc)
    groups = sorted(BEAM_BATCHES, key=lambda g: -max(int(all_len[r]) for r in g))
    rows = [r for g in groups for r in g]
    h_len = np.ascontiguousarray(all_len[rows])
    src_h = fsrc[rows][:, :int(h_len.max())].contiguous()
    src = src_h.to(model.device)
    R, width = src.shape
    h_batch = np.repeat(np.arange(len(groups), dtype=np.int32), [len(g) for g in groups])
    h_given = np.array([h_len[h_batch == b].max() for b in range(len(groups))], dtype=np.int32)
    T_cap = MAX_LEN + 8
    out = torch.zeros((R, 3, MAX_LEN), dtype=torch.int64, device=model.device)
    tlen = torch.zeros((R, T_cap), dtype=torch.int16, device=model.device)
    summ = torch.zeros((R, 8), dtype=torch.int32, device=model.device)
    sess = (C.c_void_p * 1)(model.session_pool(1)[0].value)
    p, st = NA.BeamParams(MAX_LEN, 3, 5, 2, BEAM_CASES[case], PAD, BOS, EOS, c_token, 300), NA.BeamStats()
    i32 = C.POINTER(C.c_int32)
    with pool_env({}):
        NA.check(model._lib.ttx_beam_speculative_generate_pool(sess, 1, src.data_ptr(), R, width, h_len.ctypes.data_as(i32),
                                                               h_batch.ctypes.data_as(i32), len(groups), h_given.ctypes.data_as(i32),
                                                               BEAM_CAPACITY, C.byref(p), out.data_ptr(), tlen.data_ptr(), summ.data_ptr(),
                                                               T_cap, C.byref(st), model._stream()))
    torch.cuda.synchronize()
    return {"stats": int_fields(st), "trace_len": tlen.cpu().numpy(), "summary": summ.cpu().numpy()}


def sorted_sources(model):
    """The ten fixture sources, longest first: (device matrix, host lengths, device keys)."""
    fsrc, _, c_token, _ = fixture_tokens()
    all_len = lengths_of(fsrc)
    idx = sorted(range(fsrc.shape[0]), key=lambda r: -int(all_len[r]))
    h_len = np.ascontiguousarray(all_len[idx])
    src = fsrc[idx][:, :int(h_len.max())].contiguous().to(model.device)
    keys = torch.tensor(MORE_KEYS[:len(idx)], dtype=torch.int64, device=model.device)
    return src, h_len, keys, c_token


def sbs_pool(model):
    """-> {stats, src_running_rows, out} of ttx_sbs_generate_pool over the ten sources; stats holds model_calls, running_rows,
    src_tokens_padded, live_slots and status."""
    from translation_transformer_amd import _native as NA
    src, h_len, keys, _ = sorted_sources(model)
    S, width = src.shape
    out = torch.zeros((S, SBS_BEAM, SBS_MAX_LEN), dtype=torch.int64, device=model.device)
    logp = torch.zeros((S, SBS_BEAM), dtype=torch.float32, device=model.device)
    gum = torch.zeros((S, SBS_BEAM), dtype=torch.float32, device=model.device)
    per_src = torch.zeros((S,), dtype=torch.int32, device=model.device)
    sess = (C.c_void_p * 1)(model.session_pool(1)[0].value)
    p, st = NA.SbsParams(SBS_MAX_LEN, SBS_BEAM, 1.0, PAD, BOS, EOS, SBS_SEED), NA.SbsPoolStats()
    st.d_src_running_rows = per_src.data_ptr()
    with pool_env({}):
        NA.check(model._lib.ttx_sbs_generate_pool(sess, 1, src.data_ptr(), S, width, h_len.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  keys.data_ptr(), MORE_CAPACITY, C.byref(p), None, None, 0, None, out.data_ptr(),
                                                  logp.data_ptr(), gum.data_ptr(), C.byref(st), model._stream()))
    torch.cuda.synchronize()
    stats = np.array([st.model_calls, st.running_rows, st.src_tokens_padded, st.live_slots, st.status], dtype=np.int64)
    return {"stats": stats, "src_running_rows": per_src.cpu().numpy(), "out": out.cpu().numpy()}


def sampling_pool(model):
    """-> {stats, counters, out} of ttx_sample_speculative_generate_pool over the ten sources, two keyed samples each."""
    from translation_transformer_amd import _native as NA
    src, h_len, keys, c_token = sorted_sources(model)
    S, width = src.shape
    out = torch.zeros((S, SAMPLE_PER_SRC, MAX_LEN), dtype=torch.int64, device=model.device)
    sess = (C.c_void_p * 1)(model.session_pool(1)[0].value)
    p = NA.SampleSpecParams(NA.SampleParams(MAX_LEN, SAMPLE_PER_SRC, 1.0, 0, 1.0, PAD, BOS, EOS, SAMPLE_SEED), 10, 3, c_token, 0)
    st = NA.GenStats()
    words = (C.c_int64 * 7)()
    with pool_env({}):
        NA.check(model._lib.ttx_sample_speculative_generate_pool(sess, 1, src.data_ptr(), S, width, h_len.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                 keys.data_ptr(), MORE_CAPACITY, C.byref(p), out.data_ptr(), C.byref(st),
                                                                 model._stream()))
    torch.cuda.synchronize()
    NA.check(model._lib.ttx_pool_last_counters(sess[0], words))
    return {"stats": int_fields(st), "counters": np.array(list(words), dtype=np.int64), "out": out.cpu().numpy()}


def record_more(model):
    """The SBS-pool and the sampling-pool case, as the flat name -> array mapping of tests/golden/pool_schedule_more.npz."""
    rec = {f"sbs__{k}": v for k, v in sbs_pool(model).items()}
    rec.update({f"sampling__{k}": v for k, v in sampling_pool(model).items()})
    return rec


def record_all(model):
    """Every case, as the flat name -> array mapping of tests/golden/pool_schedule.npz."""
    rec = {}
    for case in GREEDY_CASES:
        rec.update({f"greedy__{case}__{k}": v for k, v in greedy_pool(model, case).items()})
    for case in BEAM_CASES:
        rec.update({f"beam__{case}__{k}": v for k, v in beam_pool(model, case).items()})
    return rec
