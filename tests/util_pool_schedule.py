"""The cases of tests/test_gpu_pool_schedule.py and tests/golden/make_golden_pool_schedule.py: pool calls on ONE session of the tiny
fixture model through the public C ABI.  On one session a pool's schedule is deterministic (one step in flight, the host decides
after each publish), so everything recorded here is a pure function of the admission rule and the step policy: integer counters,
the seven words of ttx_pool_last_counters, the per-row traces.  Times are not recorded."""
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


def record_all(model):
    """Every case, as the flat name -> array mapping of tests/golden/pool_schedule.npz."""
    rec = {}
    for case in GREEDY_CASES:
        rec.update({f"greedy__{case}__{k}": v for k, v in greedy_pool(model, case).items()})
    for case in BEAM_CASES:
        rec.update({f"beam__{case}__{k}": v for k, v in beam_pool(model, case).items()})
    return rec
