#!/usr/bin/env python3
"""What activation="gelu" costs over "relu" (not part of bench.py).  One JSON line.

1. The FFN1 launch (K = 256, N = 2048, bias) with activation 0 (none), 1 (ReLU) and 2 (exact GELU) through ttx_debug_gemm_act on
   random operands, at M = 64, 672 and 2048 rows: a tail step, a bs = 32 step and a pool-sized step.  Bulk launches (no live row
   count on the device: a step launch of this entry point reads the count back first, which would put a host round trip between
   the events): k_gemm24<4> in its 64x64 body — the loop and epilogue (g2_body<4>) that k_gemm2<4> runs for a small step.  Every
   launch sits between two events of its own; a long kernel queued ahead of each group keeps the stream busy while the host
   enqueues the group, so an event pair sees its launch and not the host.  The three activations alternate launch by launch.
   Reported: the median over all timed launches, in microseconds.
2. teacher_forced at bs = 32 over USPTO-MIT-shaped batches (tools/synth.py) on the full-size 4+4 seeded model of
   tools/bench_eval.py, built once as ReLU and once as GELU; the two alternate batch by batch.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

ACTS = {"none": 0, "relu": 1, "gelu": 2}


def bench_launches(native, M: int, N: int, K: int, groups: int, per_group: int) -> dict:
    gen = torch.Generator().manual_seed(M)
    x = (torch.rand((M, K), generator=gen) * 2 - 1).cuda()
    w = ((torch.rand((N, K), generator=gen) * 2 - 1) * 0.125).cuda()
    b = (torch.rand((N,), generator=gen) * 2 - 1).cuda()
    y = torch.empty((M, N), device="cuda")
    blocker = torch.empty((4096, 4096), device="cuda")
    run = lambda act: native.debug_gemm(x, w, b, y, N, K, M, variant=0, tiling=1, activation=act)     # noqa: E731
    kid = {name: run(a) for name, a in ACTS.items()}
    for _ in range(20):                                   # warmed shapes
        for a in ACTS.values():
            run(a)
    torch.cuda.synchronize()
    times = {name: [] for name in ACTS}
    for _ in range(groups):
        pairs = []
        blocker @ blocker                                 # a few milliseconds of work ahead of the group
        blocker @ blocker
        for _ in range(per_group):
            for name, a in ACTS.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(a)
                e1.record()
                pairs.append((name, e0, e1))
        torch.cuda.synchronize()
        for name, e0, e1 in pairs:
            times[name].append(e0.elapsed_time(e1) * 1e3)
    out = {"M": M, "N": N, "K": K, "kernel_id": kid["gelu"], "launches_each": groups * per_group}
    assert len(set(kid.values())) == 1
    for name, v in times.items():
        out[f"{name}_us"] = round(float(np.median(v)), 3)
    out["gelu_minus_relu_us"] = round(out["gelu_us"] - out["relu_us"], 3)
    out["gelu_over_relu"] = round(out["gelu_us"] / out["relu_us"], 4)
    return out


def bench_teacher_forced(bs: int, n_batches: int, warmup: int, passes: int) -> dict:
    import translation_transformer_amd as tta
    from tools.bench_eval import make_batches
    from tools.synth import V
    from util_models import full_state
    st = full_state(V, 20261016)
    models = {a: tta.NativeTransformer(st, 8, 0, device=0, activation=a) for a in ("relu", "gelu")}
    batches = make_batches(n_batches, bs)
    for _ in range(warmup):
        for s, t in batches:
            for m in models.values():
                m.teacher_forced(s, t)
    torch.cuda.synchronize()
    times = {a: [] for a in models}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(passes):
        for s, t in batches:
            ev[0].record()
            models["relu"].teacher_forced(s, t)
            ev[1].record()
            models["gelu"].teacher_forced(s, t)
            ev[2].record()
            ev[2].synchronize()
            times["relu"].append(ev[0].elapsed_time(ev[1]))
            times["gelu"].append(ev[1].elapsed_time(ev[2]))
    out = {"bs": bs, "batches": n_batches, "timed_calls_each": passes * n_batches,
           "mean_tgt_len": float(np.mean([t.shape[1] for _, t in batches])), "mean_src_len": float(np.mean([s.shape[1] for s, _ in batches]))}
    for a, v in times.items():
        out[a] = {"ms_per_batch": round(float(np.mean(v)), 4), "median_ms": round(float(np.median(v)), 4),
                  "sequences_per_s": round(bs * 1000.0 / float(np.mean(v)), 1)}
    out["gelu_over_relu"] = round(out["gelu"]["median_ms"] / out["relu"]["median_ms"], 4)
    out["gelu_minus_relu_ms"] = round(out["gelu"]["median_ms"] - out["relu"]["median_ms"], 4)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[64, 672, 2048])
    ap.add_argument("--groups", type=int, default=15)
    ap.add_argument("--per-group", type=int, default=20, help="launches of each activation per group (groups x per-group >= 200)")
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_activation.py measures on an MI355X; there is no CPU figure"
    import translation_transformer_amd as tta
    from util_models import tiny_state
    st, cfg = tiny_state()
    native = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session
    rec = {"tool": "bench_activation",
           "ffn1_launch": [bench_launches(native, M, 2048, 256, a.groups, a.per_group) for M in a.rows],
           "teacher_forced": bench_teacher_forced(a.bs, a.batches, a.warmup, a.passes)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
