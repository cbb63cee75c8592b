#!/usr/bin/env python3
"""Pooled stochastic beam search against the per-batch loop (not part of bench.py), written after tools/bench_sampling_pool.py and
tools/bench_sbs_mask.py: bench.py's 4+4 weights, 1 024 USPTO-MIT-shaped synthetic sources (tools/synth.py), max_len 200, temperature
1, K = 5 and 10, filter off and top_k = 32 with top_p = 0.9975, unprompted and prompted with the first half of each source's greedy
output.

Three contenders decode the same sources under the same keys (their rows are equal on the bits, which the tool checks once per case):
  pooled        generate_many over the whole list (ttx_sbs_generate_pool) at the default capacity
  per_batch_32  generate at 32 sources per call: the per-batch loop as it was before the pool existed
  per_batch_256 generate at 256 sources per call, length-sorted: the fair large-batch yardstick
One warm-up pass, then --repeats passes with the contenders alternated inside every pass (each takes every place), a host clock
around a device synchronise, medians.  Reported: sources/s, decoder passes (iterations), and for the pool the mean live slots and
mean running candidates per iteration.  Then a capacity sweep over {64, 128, 256, 512} source slots at K = 5, unfiltered, unprompted.

Writes one JSON line per case to --out (and prints them).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def half_greedy_prefixes(tta, native, srcs, max_len, PAD, BOS, EOS):
    """Per batch a Long[B, w]: the first half of every source's greedy output (BOS and EOS excluded), right-padded."""
    greedy = tta.TranslationInferenceGreedy(native, max_len, PAD, BOS, EOS)
    out = []
    for s in srcs:
        rows = greedy.generate(s)[:, 0].cpu().numpy()
        halves = []
        for r in rows:
            body = r[1:]
            stop = np.nonzero((body == EOS) | (body == PAD))[0]
            body = body[:int(stop[0])] if len(stop) else body
            halves.append(body[:len(body) // 2])
        w = max(1, max(len(h) for h in halves))
        p = np.full((len(halves), w), PAD, dtype=np.int64)
        for i, h in enumerate(halves):
            p[i, :len(h)] = h
        out.append(torch.from_numpy(p))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r24_bench_sbs_pool.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_sbs_pool.py measures on an MI355X; there is no CPU figure"
    assert a.repeats >= 5, "medians over at least five repeats"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    S = a.sources
    src_rows, _ = SynthReactions(123456, "mit").dataset(S)
    lengths = np.array([len(r) for r in src_rows])
    by_len = np.argsort(-lengths, kind="stable")

    def groups(order, size):
        """(batches on the device, their keys): the sources' indices are their keys, whatever the batching."""
        bs, ks = [], []
        for i in range(0, S, size):
            idx = order[i:i + size]
            bs.append(torch.from_numpy(next(iter(batches([src_rows[j] for j in idx], len(idx))))).cuda())
            ks.append(torch.from_numpy(np.asarray(idx, dtype=np.int64)))
        return bs, ks, [order[i:i + size] for i in range(0, S, size)]
    b32, k32, i32 = groups(np.arange(S), 32)                 # as a dataloader hands them out
    b256, k256, i256 = groups(by_len, 256)                   # length-sorted: the least padding a large batch can have
    pre32 = half_greedy_prefixes(tta, native, b32, a.max_len, PAD, BOS, EOS)
    pre_of = {}                                              # source index -> its prefix tokens
    for idx, p in zip(i32, pre32):
        for j, row in zip(idx, p.numpy()):
            pre_of[int(j)] = row[row != PAD]
    pre256 = []
    for idx in i256:
        w = max(1, max(len(pre_of[int(j)]) for j in idx))
        p = np.full((len(idx), w), PAD, dtype=np.int64)
        for r, j in enumerate(idx):
            p[r, :len(pre_of[int(j)])] = pre_of[int(j)]
        pre256.append(torch.from_numpy(p))

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def rows_by_source(outs, index_lists):
        full = [None] * S
        for o, idx in zip(outs, index_lists):
            o = o.cpu().numpy()
            for r, j in enumerate(idx):
                full[int(j)] = o[r]
        return np.stack(full)

    lines = []

    def case(name, K, prompted, capacity=None, contenders=("pooled", "per_batch_32", "per_batch_256"), **flt):
        def make():
            return tta.TranslationInferenceStochasticBeamSearch(native, K, a.max_len, PAD, BOS, EOS, temperature=1.0, seed=20260104, **flt)
        g = {c: make() for c in contenders}
        runs = {"pooled": lambda: g["pooled"].generate_many(b32, row_keys=k32, prefixes=pre32 if prompted else None, capacity=capacity),
                "per_batch_32": lambda: [g["per_batch_32"].generate(s, row_keys=k, prefix=p if prompted else None)
                                         for s, k, p in zip(b32, k32, pre32)],
                "per_batch_256": lambda: [g["per_batch_256"].generate(s, row_keys=k, prefix=p if prompted else None)
                                          for s, k, p in zip(b256, k256, pre256)]}
        outs = {c: runs[c]() for c in contenders}            # the warm-up pass; its rows are compared
        torch.cuda.synchronize()
        ref = rows_by_source(outs[contenders[0]], i32)
        equal = {c: bool(np.array_equal(rows_by_source(outs[c], i256 if c == "per_batch_256" else i32), ref)) for c in contenders[1:]}
        del outs
        secs = {c: [] for c in contenders}
        calls = {c: [] for c in contenders}
        rows = {c: [] for c in contenders}
        live = []
        names = list(contenders)
        for rep in range(a.repeats):
            order = names[rep % len(names):] + names[:rep % len(names)]          # alternated: every contender takes every place
            for c in order:
                before = (g[c].model_calls_num, g[c].b_sz)
                t, _ = timed(runs[c])
                secs[c].append(t)
                calls[c].append(g[c].model_calls_num - before[0])
                rows[c].append(g[c].b_sz - before[1])
                if c == "pooled":
                    live.append(int(g[c].last_stats.live_slots))
        for c in contenders:
            m = float(np.median(secs[c]))
            rec = {"tool": "bench_sbs_pool", "case": name, "contender": c, "sources": S, "K": K, "max_len": a.max_len, "vocab": V,
                   "prompted": bool(prompted), **{k: v for k, v in flt.items()}, "repeats": a.repeats, "seconds": round(m, 4),
                   "seconds_min": round(min(secs[c]), 4), "seconds_max": round(max(secs[c]), 4), "sources_per_s": round(S / m, 1),
                   "iterations": int(np.median(calls[c])), "running_rows": int(np.median(rows[c])),
                   "mean_running_rows_per_iteration": round(float(np.median(rows[c])) / max(1.0, float(np.median(calls[c]))), 1)}
            if c == "pooled":
                rec["capacity"] = int(g[c].last_group_size)
                rec["pools"] = int(g[c].last_pool_sessions)
                rec["mean_live_slots_per_iteration"] = round(float(np.median(live)) / max(1.0, float(np.median(calls[c]))), 1)
            else:
                rec["rows_equal_pooled"] = equal[c]
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        base = {r["contender"]: r for r in lines if r["case"] == name}
        for c in contenders[1:]:
            base["pooled"][f"speedup_over_{c}"] = round(base[c]["seconds"] / base["pooled"]["seconds"], 3)
        return base

    for K in (5, 10):
        for flt_name, flt in (("unfiltered", {}), ("top_k32_top_p0.9975", dict(top_k=32, top_p=0.9975))):
            for prompted in (False, True):
                case(f"K{K}_{flt_name}_{'prompted_half_greedy' if prompted else 'unprompted'}", K, prompted, **flt)
    if not a.skip_sweep:
        for cap in (64, 128, 256, 512):
            case(f"sweep_K5_capacity{cap}", 5, False, capacity=cap, contenders=("pooled",))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec), file=f)
    print("== summary ==")
    for rec in lines:
        if rec["contender"] == "pooled":
            print(json.dumps({k: rec[k] for k in rec if k in ("case", "capacity", "pools", "sources_per_s", "iterations",
                                                              "mean_running_rows_per_iteration", "mean_live_slots_per_iteration", "speedup_over_per_batch_32",
                                                              "speedup_over_per_batch_256")}))


if __name__ == "__main__":
    main()
