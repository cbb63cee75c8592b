#!/usr/bin/env python3
"""Cost of the sampling generator (TranslationInferenceSampling, not part of bench.py) on bench.py's 4+4 weights and
USPTO-MIT-shaped synthetic batches (tools/synth.py), bs = 32, max_len 200, temperature 1:

  n = 1 and n = 8 samples per source, filters off and top_k = 32 with top_p = 0.9975,

beside TranslationInferenceGreedy on the same batches (32 rows) and on the same batches with every source repeated 8 times (256
rows, the decoder rows of n = 8; greedy encodes each copy, the sampler each source once): existing code of the same build in the
same run, timed alternately batch by batch with HIP events around each call: the yardstick.  Sampled rows do not end where
the greedy row ends, so the figure to compare is ms per step (ms per call / decoder steps of the call), medians over the batches
and passes.  Writes one JSON line per case to --out (and prints them).

--trace-only: the greedy and the n = 1 sampling calls alone, once per batch, nothing timed: the command to put behind
``rocprofv3 --kernel-trace --stats --``, whose table then holds k_sample beside k_argmax.
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

FILTERS = {"off": dict(), "top_k32_top_p0.9975": dict(top_k=32, top_p=0.9975)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8, help="batches of 32 sources that are timed")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r15_bench_sampling.jsonl"))
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_sampling.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.batches * 32)
    srcs = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    keys = [torch.arange(32 * i, 32 * (i + 1)) for i in range(len(srcs))]

    gens = {"greedy_rows32": (tta.TranslationInferenceGreedy(native, a.max_len, PAD, BOS, EOS), 1, None)}
    for n in (1, 8):
        for fname, f in FILTERS.items():
            gens[f"sampling_n{n}_{fname}"] = (tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, temperature=1.0,
                                                                               num_samples=n, seed=20260103, **f), n, fname)
    gens["greedy_rows256"] = (tta.TranslationInferenceGreedy(native, a.max_len, PAD, BOS, EOS), 8, None)

    def call(name, i):
        g, n, fname = gens[name]
        if fname is None:
            return g.generate(srcs[i].repeat_interleave(n, 0) if n > 1 else srcs[i])
        return g.generate(srcs[i], row_keys=keys[i])

    if a.trace_only:
        for i in range(len(srcs)):
            for name in ("greedy_rows32", "sampling_n1_off", "sampling_n1_top_k32_top_p0.9975"):
                call(name, i)
        torch.cuda.synchronize()
        return

    for _ in range(a.warmup):
        for i in range(len(srcs)):
            for name in gens:
                call(name, i)
    torch.cuda.synchronize()
    ms = {k: [] for k in gens}
    steps = {k: [] for k in gens}
    distinct = {k: [] for k in gens}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(gens) + 1)]
    for p in range(a.passes):
        for i in range(len(srcs)):
            before = {k: g.model_calls_num for k, (g, _, _) in gens.items()}
            outs = {}
            ev[0].record()
            for j, name in enumerate(gens):
                outs[name] = call(name, i)
                ev[j + 1].record()
            ev[-1].synchronize()
            for j, name in enumerate(gens):
                ms[name].append(ev[j].elapsed_time(ev[j + 1]))
                steps[name].append(gens[name][0].model_calls_num - before[name])
                if p == 0 and gens[name][2] is not None and gens[name][1] > 1:
                    o = outs[name].cpu().numpy()
                    distinct[name].append(float(np.mean([len({tuple(r) for r in per.tolist()}) for per in o])))
    base = {}
    lines = []
    for name, (g, n, fname) in gens.items():
        per_step = np.array(ms[name]) / np.maximum(np.array(steps[name]), 1)
        rec = {"tool": "bench_sampling", "case": name, "sources": 32, "rows": 32 * n, "max_len": a.max_len, "vocab": V,
               "timed_batches": len(srcs), "passes": a.passes, "ms_per_call": round(float(np.median(ms[name])), 4),
               "steps_per_call": round(float(np.median(steps[name])), 1), "ms_per_step": round(float(np.median(per_step)), 5)}
        if fname is None:
            base[32 * n] = rec["ms_per_step"]
        else:
            rec["ms_per_step_over_greedy_same_rows"] = None                      # filled below: greedy_rows256 is timed last
            if distinct[name]:
                rec["distinct_samples_per_source"] = round(float(np.mean(distinct[name])), 2)
        lines.append(rec)
    for rec in lines:
        if "ms_per_step_over_greedy_same_rows" in rec:
            rec["ms_per_step_over_greedy_same_rows"] = round(rec["ms_per_step"] / base[rec["rows"]], 4)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec))
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
