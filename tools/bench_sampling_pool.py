#!/usr/bin/env python3
"""Throughput of pooled speculative seeded sampling (TranslationInferenceSamplingSpeculative.generate_many, not part of bench.py) on
bench.py's 4+4 weights and 1 024 USPTO-MIT-shaped synthetic sources (tools/synth.py), max_len 200:

  num_samples 1 and 8, temperature 0.5 / 1 / 2, filters off and top_k = 32 with top_p = 0.9975, (n_drafts, draft_len) = (3, 10) and (1, 4),

beside three yardsticks of the same build on the same sources, keys and seed:
  (a) TranslationInferenceSampling.generate over batches of 32 sources (it emits the same rows),
  (b) the same sampler at 512 sources per call (the fair large-batch yardstick),
  (c) TranslationInferenceSamplingSpeculative.generate over batches of 32 sources.
The four are timed alternately, pass by pass, with HIP events around the whole list; the figures are medians over the passes after
warm-up.  Per case one JSON line: samples/s of each generator, device steps of the pool, accepted draft tokens per row and step, the
pool counters (split steps, matched slots, rows executed) and rows_equal_to_plain.  ``--sweep`` adds, at one case per num_samples
(temperature 1, filters off, (3, 10)), TTX_TWO_PHASE_MIN_ROWS in 0 / 800 / off (TTX_TWO_PHASE=0) and capacity in 256 / 512 / 1 024.
``--cases`` restricts the grid (``n:T:filter:N:D`` items, comma separated, ``*`` for any).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FILTERS = {"off": dict(), "top_k32_top_p0.9975": dict(top_k=32, top_p=0.9975)}
TEMPERATURES = (0.5, 1.0, 2.0)
DRAFTS = ((3, 10), (1, 4))
SEED = 20260104


def wanted(spec: str, case: tuple) -> bool:
    if not spec:
        return True
    for item in spec.split(","):
        parts = item.split(":")
        if all(p == "*" or p == str(c) for p, c in zip(parts, case)):
            return True
    return False


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2, help="untimed passes (a graph is captured the second time its key is seen)")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--cases", default="")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r19_bench_sampling_pool.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_sampling_pool.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.sources)
    small = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    large = [torch.from_numpy(b).cuda() for b in batches(src_rows, 512)]
    keys = lambda bs: [torch.arange(bs * i, min(bs * (i + 1), a.sources)) for i in range(-(-a.sources // bs))]
    k32, k512 = keys(32), keys(512)
    lines = []

    def measure(n, T, fname, N, D, env=None, capacity=None, yardsticks=True, tag=None):
        kw = dict(temperature=T, num_samples=n, seed=SEED, **FILTERS[fname])
        plain = tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, **kw)
        spec = tta.TranslationInferenceSamplingSpeculative(native, a.max_len, D, N, PAD, BOS, EOS, C_TOK, **kw)
        pool = tta.TranslationInferenceSamplingSpeculative(native, a.max_len, D, N, PAD, BOS, EOS, C_TOK, **kw)
        runs = {"pool": lambda: torch.cat(pool.generate_many(small, row_keys=k32, capacity=capacity), 0)}
        if yardsticks:
            runs["plain_bs32"] = lambda: torch.cat([plain.generate(s, row_keys=k) for s, k in zip(small, k32)], 0)
            runs["plain_bs512"] = lambda: torch.cat([plain.generate(s, row_keys=k) for s, k in zip(large, k512)], 0)
            runs["spec_bs32"] = lambda: torch.cat([spec.generate(s, row_keys=k) for s, k in zip(small, k32)], 0)
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            ms = {k: [] for k in runs}
            outs, stats, counters = {}, None, None
            for p in range(a.warmup + a.passes):
                for name, fn in runs.items():
                    if name == "pool":
                        before = (pool.model_calls_num, pool.accepted_tokens_num, pool.stats_total["produced_tokens"])
                    t, out = timed(fn)
                    if p >= a.warmup:
                        ms[name].append(t)
                    outs[name] = out
                    if name == "pool":
                        stats = (pool.model_calls_num - before[0], pool.accepted_tokens_num - before[1],
                                 pool.stats_total["produced_tokens"] - before[2])
                        counters = native.pool_last_counters()
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        samples = a.sources * n
        rec = {"tool": "bench_sampling_pool", "case": tag or f"n{n}_T{T}_{fname}_N{N}_D{D}", "n": n, "T": T, "filter": fname, "n_drafts": N,
               "draft_len": D, "sources": a.sources, "rows": samples, "max_len": a.max_len, "vocab": V, "passes": a.passes,
               "capacity_asked": pool.last_group_size, "env": env or {}}
        # what the call really ran (csrc/ttx_admit.h pool_shape): never more pools than sessions or than a share of 32 rows each, and
        # no pool wider than its share of the rows; above 256 slots the accept step runs in two launches
        per_pool = max(1, min(pool.last_group_size // 2, 32))
        pools = max(1, min(pool.last_pool_sessions, a.sources, -(-samples // per_pool)))
        rec["pools"] = pools
        rec["slots_per_pool"] = min(pool.last_group_size, max(n, -(-samples // pools)))
        rec["accept_in_two_launches"] = rec["slots_per_pool"] > 256 and os.environ.get("TTX_ACCEPT_SPREAD", "1") != "0"
        for name in runs:
            rec[f"{name}_samples_per_s"] = round(samples / (float(np.median(ms[name])) / 1e3), 1)
            rec[f"{name}_ms_spread"] = [round(min(ms[name]), 2), round(max(ms[name]), 2)]
        steps, accepted, produced = stats
        rec.update(device_steps=steps, accepted_per_row_step=round(accepted / max(1, produced - accepted), 4),
                   split_steps=counters["split_steps"], slot_steps_probed=counters["slot_steps_probed"], matched_slots=counters["slots_matched"],
                   rows_executed=counters["rows_executed"], draft_select=counters["draft_select"])
        if yardsticks:
            rec["rows_equal_to_plain"] = round(float((outs["pool"] == outs["plain_bs32"]).all(dim=2).float().mean()), 5)
            rec["rows_equal_to_spec"] = round(float((outs["pool"] == outs["spec_bs32"]).all(dim=2).float().mean()), 5)
            for y in ("plain_bs32", "plain_bs512", "spec_bs32"):
                rec[f"pool_over_{y}"] = round(rec["pool_samples_per_s"] / rec[f"{y}_samples_per_s"], 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for n in (1, 8):
        for T in TEMPERATURES:
            for fname in FILTERS:
                for N, D in DRAFTS:
                    if wanted(a.cases, (n, T, fname, N, D)):
                        measure(n, T, fname, N, D)
    if a.sweep:
        for n in (1, 8):
            for tag, env in (("min_rows_0", {"TTX_TWO_PHASE_MIN_ROWS": "0"}), ("min_rows_800", {"TTX_TWO_PHASE_MIN_ROWS": "800"}),
                             ("two_phase_off", {"TTX_TWO_PHASE": "0"})):
                measure(n, 1.0, "off", 3, 10, env=env, yardsticks=False, tag=f"sweep_n{n}_{tag}")
            for cap in (256, 512, 1024):
                measure(n, 1.0, "off", 3, 10, capacity=cap, yardsticks=False, tag=f"sweep_n{n}_capacity_{cap}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
