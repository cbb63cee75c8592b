#!/usr/bin/env python3
"""Generate tests/golden/pool_schedule.npz: the schedule of the greedy slot pool and of the beam-speculative batch pool on ONE
session of the tiny fixture model, recorded through the public C ABI alone (tests/util_pool_schedule.py holds the cases and says
what is recorded).  With `more` first, tests/golden/pool_schedule_more.npz instead: the stochastic-beam source pool and the sampling
slot pool, recorded the same way (a file of its own, so that pool_schedule.npz stays as it was recorded).  Needs an MI355X.  Run it
at the commit whose schedule is to be pinned: tests/test_gpu_pool_schedule.py then asserts exact equality with the file, so a change
to the admission rule or to the polling order of the pools shows up there.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pool_schedule.py [more] [OUT.npz]
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

import translation_transformer_amd as tta  # noqa: E402
import util_pool_schedule as U  # noqa: E402


def main():
    args = sys.argv[1:]
    more = bool(args) and args[0] == "more"
    record = U.record_more if more else U.record_all
    out = Path(args[more]) if len(args) > more else HERE / ("pool_schedule_more.npz" if more else "pool_schedule.npz")
    assert tta.lib().ttx_device_count() >= 1, "needs a gfx950 device"
    model = U.make_model(tta)
    rec = record(model)
    again = record(model)                      # the premise of the fixture: the schedule on one session is deterministic
    for k, v in rec.items():
        assert np.array_equal(v, again[k]), f"{k} differs between two runs: not a deterministic schedule"
    model.close()
    np.savez_compressed(out, **rec)
    for k, v in rec.items():
        print(k, v.shape, v.dtype, v.tolist() if v.size <= 16 else "")


if __name__ == "__main__":
    main()
