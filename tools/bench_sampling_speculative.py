#!/usr/bin/env python3
"""Cost of speculative seeded sampling (TranslationInferenceSamplingSpeculative, not part of bench.py) on bench.py's 4+4 weights and
USPTO-MIT-shaped synthetic batches (tools/synth.py), bs = 32, max_len 200:

  num_samples 1 and 8, temperature 0.5 / 1 / 2, filters off and top_k = 32 with top_p = 0.9975, (n_drafts, draft_len) = (3, 10) and (1, 4),

beside TranslationInferenceSampling of the same build on the same sources, keys, seed and settings (the yardstick: it emits the same
rows one token per decoder pass).  The generators are timed alternately batch by batch with HIP events around each call; the
figures are medians over the batches and passes: ms per call, decoder steps per call and, for the speculative form, accepted draft
tokens per row and step (accepted / (produced - accepted): 0 means every step committed its bonus token alone).  Writes one JSON
line per case to --out (and prints them); ``speedup`` is the plain sampler's ms per call over the speculative form's.
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
TEMPERATURES = (0.5, 1.0, 2.0)
DRAFTS = ((3, 10), (1, 4))
SEED = 20260104


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4, help="batches of 32 sources that are timed")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r17_bench_sampling_spec.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_sampling_speculative.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.batches * 32)
    srcs = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    keys = [torch.arange(32 * i, 32 * (i + 1)) for i in range(len(srcs))]

    gens = {}                      # name -> (generator, settings, name of its yardstick or None)
    for n in (1, 8):
        for T in TEMPERATURES:
            for fname, f in FILTERS.items():
                kw = dict(temperature=T, num_samples=n, seed=SEED, **f)
                plain = f"plain_n{n}_T{T}_{fname}"
                gens[plain] = (tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, **kw), dict(n=n, T=T, filter=fname), None)
                for N, D in DRAFTS:
                    g = tta.TranslationInferenceSamplingSpeculative(native, a.max_len, D, N, PAD, BOS, EOS, C_TOK, **kw)
                    gens[f"spec_n{n}_T{T}_{fname}_N{N}_D{D}"] = (g, dict(n=n, T=T, filter=fname, n_drafts=N, draft_len=D), plain)

    for _ in range(a.warmup + 1):                                        # a graph is captured the second time its key is seen
        for i in range(len(srcs)):
            for g, _, _ in gens.values():
                g.generate(srcs[i], row_keys=keys[i])
    torch.cuda.synchronize()
    ms = {k: [] for k in gens}
    steps = {k: [] for k in gens}
    acc = {k: [] for k in gens}
    same = {k: [] for k in gens}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(gens) + 1)]
    for p in range(a.passes):
        for i in range(len(srcs)):
            before = {k: g.model_calls_num for k, (g, _, _) in gens.items()}
            outs = {}
            ev[0].record()
            for j, (name, (g, _, _)) in enumerate(gens.items()):
                outs[name] = g.generate(srcs[i], row_keys=keys[i])
                ev[j + 1].record()
            ev[-1].synchronize()
            for j, (name, (g, _, base)) in enumerate(gens.items()):
                ms[name].append(ev[j].elapsed_time(ev[j + 1]))
                steps[name].append(g.model_calls_num - before[name])
                if base is not None:
                    st = g.last_stats
                    acc[name].append(st.accepted_tokens / max(1, st.produced_tokens - st.accepted_tokens))
                    if p == 0:
                        same[name].append(float((outs[name] == outs[base]).all(dim=2).float().mean()))
    lines = []
    for name, (g, settings, base) in gens.items():
        rec = {"tool": "bench_sampling_speculative", "case": name, **settings, "sources": 32, "rows": 32 * settings["n"],
               "max_len": a.max_len, "vocab": V, "timed_batches": len(srcs), "passes": a.passes,
               "ms_per_call": round(float(np.median(ms[name])), 4), "steps_per_call": round(float(np.median(steps[name])), 1)}
        if base is not None:
            rec["accepted_per_row_step"] = round(float(np.median(acc[name])), 4)
            rec["plain_ms_per_call"] = round(float(np.median(ms[base])), 4)
            rec["speedup"] = round(rec["plain_ms_per_call"] / rec["ms_per_call"], 4)
            rec["rows_equal_to_plain"] = round(float(np.mean(same[name])), 4)
        lines.append(rec)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec))
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
