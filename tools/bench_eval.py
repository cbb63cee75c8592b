#!/usr/bin/env python3
"""Teacher-forced evaluation throughput (validation_step / test_step's hot path, not part of bench.py).

Times ``NativeTransformer.teacher_forced`` (ttx_teacher_forced_eval: encoder + full-prefix decoder + classifier + the two metric
kernels) against ``__call__`` alone (ttx_forward, the same forward without the metric stage) on the synthetic 4+4 model
(d = 256, 8 heads, FFN 2048, V = 256; seeded weights: timing does not depend on their values) at bs = 32 over USPTO-MIT-shaped
batches (tools/synth.py), with warm-up and HIP events around each timed batch.  The two are timed alternately, batch by batch.
Prints one JSON line: sequences/s and ms per batch of both, and the overhead of teacher_forced over __call__.

The share of the two metric kernels in a ttx_teacher_forced_eval call comes from a separate run under
``rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_eval.py --trace-only``; ``--kernel-stats FILE`` then reads
rocprofv3's kernel_stats.csv and adds {kernel: total ns, launches} of k_token_metrics / k_batch_metrics and the share of all
kernel time of the traced teacher_forced calls to the line.
"""
from __future__ import annotations

import argparse
import csv
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def make_batches(n_batches: int, bs: int, seed: int = 123456):
    from tools.synth import SynthReactions, pad_batch
    src, tgt = SynthReactions(seed=seed).dataset(n_batches * bs)
    out = []
    for i in range(0, len(src), bs):
        out.append((torch.from_numpy(pad_batch(src[i:i + bs])).cuda(), torch.from_numpy(pad_batch(tgt[i:i + bs])).cuda()))
    return out


def model():
    import translation_transformer_amd as tta
    from util_models import full_state
    from tools.synth import V
    return tta.NativeTransformer(full_state(V, 20261016), 8, 0, device=0)


def kernel_share(stats_csv: str) -> dict:
    rows = list(csv.DictReader(open(stats_csv)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    mine = {}
    for r in rows:
        for k in ("k_token_metrics", "k_batch_metrics"):
            if k in r["Name"]:
                e = mine.setdefault(k, {"total_ns": 0.0, "launches": 0})
                e["total_ns"] += float(r["TotalDurationNs"])
                e["launches"] += int(r["Calls"])
    metric_ns = sum(e["total_ns"] for e in mine.values())
    return {"kernels": mine, "metric_kernels_share": metric_ns / total if total else None, "all_kernels_ns": total}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--batches", type=int, default=16, help="distinct batches, cycled")
    ap.add_argument("--warmup", type=int, default=2, help="passes over the batches before timing")
    ap.add_argument("--passes", type=int, default=5, help="timed passes over the batches")
    ap.add_argument("--trace-only", action="store_true", help="teacher_forced calls only (for the rocprofv3 run)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a --trace-only run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_eval.py measures on an MI355X; there is no CPU figure"
    native = model()
    batches = make_batches(a.batches, a.bs)
    if a.trace_only:
        for _ in range(a.warmup + a.passes):
            for s, t in batches:
                native.teacher_forced(s, t)
        torch.cuda.synchronize()
        print(json.dumps({"trace_only": True, "calls": (a.warmup + a.passes) * len(batches)}))
        return
    tf = lambda s, t: native.teacher_forced(s, t)                  # noqa: E731
    fw = lambda s, t: native(s, t[:, :-1])                         # noqa: E731   the slice is part of what a caller pays
    for _ in range(a.warmup):
        for s, t in batches:
            tf(s, t)
            fw(s, t)
    torch.cuda.synchronize()
    times = {"teacher_forced": [], "forward": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for _ in range(a.passes):
        for s, t in batches:
            ev[0].record()
            tf(s, t)
            ev[1].record()
            fw(s, t)
            ev[2].record()
            ev[2].synchronize()
            times["teacher_forced"].append(ev[0].elapsed_time(ev[1]))
            times["forward"].append(ev[1].elapsed_time(ev[2]))
    rec = {"tool": "bench_eval", "bs": a.bs, "batches": a.batches, "timed_calls": a.passes * a.batches,
           "mean_tgt_len": float(np.mean([t.shape[1] for _, t in batches])), "mean_src_len": float(np.mean([s.shape[1] for s, _ in batches]))}
    for k, v in times.items():
        ms = float(np.sum(v)) / len(v)
        rec[k] = {"ms_per_batch": round(ms, 4), "median_ms": round(float(np.median(v)), 4),
                  "sequences_per_s": round(a.bs * 1000.0 / ms, 1)}
    rec["overhead_vs_forward"] = round(rec["teacher_forced"]["ms_per_batch"] / rec["forward"]["ms_per_batch"] - 1.0, 4)
    if a.kernel_stats:
        rec["trace"] = kernel_share(a.kernel_stats)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
