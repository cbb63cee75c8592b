#!/usr/bin/env python3
"""Cost of forced target prefixes (not part of bench.py) on bench.py's 4+4 weights and the 1 024 USPTO-MIT-shaped
synthetic sources of tools/bench_sampling_pool.py, max_len 200, temperature 1, filters off:

  (n_drafts, draft_len) = (1, 4) and (3, 10), num_samples 1 and 8,

four runs per case, on the same sources, keys and seed:
  pool_unprompted   TranslationInferenceSamplingSpeculative.generate_many(batches)
  pool_empty        the same call with all-empty prefixes (it must cost what the unprompted call costs: it is that call)
  pool_prompted     the pool prompted with the first half of each source's own temperature-0 output
  plain_prompted    TranslationInferenceSampling.generate prompted likewise, at 512 sources per call (one step per forced token)
The four are timed alternately, pass by pass, with HIP events around the whole list; per case one JSON line with the median and the
spread (min, max) of the passes after warm-up, samples/s, the pool's device steps and accepted draft tokens, and the number of
forced tokens.
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

DRAFTS = ((1, 4), (3, 10))
SEED = 20260104


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
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r20_bench_prefix.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_prefix.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.sources)
    small = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    large = [torch.from_numpy(b).cuda() for b in batches(src_rows, 512)]
    keys = lambda bs: [torch.arange(bs * i, min(bs * (i + 1), a.sources)) for i in range(-(-a.sources // bs))]
    k32, k512 = keys(32), keys(512)

    # the prompts: the first half of each source's own temperature-0 output (without BOS and without its EOS)
    greedy = tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, temperature=0.0)
    rows = torch.cat([greedy.generate(s)[:, 0] for s in large], 0).cpu().numpy()
    half = []
    for r in rows:
        body = r[1:]
        stop = np.nonzero((body == EOS) | (body == PAD))[0]
        n_tok = int(stop[0]) if len(stop) else len(body)
        half.append(body[:n_tok // 2])
    width = max(1, max(len(h) for h in half))
    pre = torch.full((a.sources, width), PAD, dtype=torch.int64)
    for i, h in enumerate(half):
        pre[i, :len(h)] = torch.from_numpy(np.ascontiguousarray(h))
    forced = int(sum(len(h) for h in half))
    split = lambda bs: [pre[bs * i:bs * (i + 1)] for i in range(-(-a.sources // bs))]
    p32, p512 = split(32), split(512)
    e32 = [torch.zeros((p.shape[0], 0), dtype=torch.int64) for p in p32]
    lines = []
    for N, D in DRAFTS:
        for n in (1, 8):
            kw = dict(temperature=1.0, num_samples=n, seed=SEED)
            plain = tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, **kw)
            pool = tta.TranslationInferenceSamplingSpeculative(native, a.max_len, D, N, PAD, BOS, EOS, C_TOK, **kw)
            runs = {"pool_unprompted": lambda: pool.generate_many(small, row_keys=k32),
                    "pool_empty": lambda: pool.generate_many(small, row_keys=k32, prefixes=e32),
                    "pool_prompted": lambda: pool.generate_many(small, row_keys=k32, prefixes=p32),
                    "plain_prompted": lambda: [plain.generate(s, row_keys=k, prefix=p) for s, k, p in zip(large, k512, p512)]}
            ms = {k: [] for k in runs}
            steps, accepted, outs = {}, {}, {}
            for p in range(a.warmup + a.passes):
                for name, fn in runs.items():
                    before = (pool.model_calls_num, pool.accepted_tokens_num)
                    t, out = timed(fn)
                    outs[name] = out
                    if p >= a.warmup:
                        ms[name].append(t)
                    if name.startswith("pool"):
                        steps[name], accepted[name] = pool.model_calls_num - before[0], pool.accepted_tokens_num - before[1]
            samples = a.sources * n
            rec = {"tool": "bench_prefix", "case": f"n{n}_N{N}_D{D}", "n": n, "n_drafts": N, "draft_len": D, "sources": a.sources,
                   "rows": samples, "max_len": a.max_len, "vocab": V, "temperature": 1.0, "passes": a.passes, "warmup": a.warmup,
                   "forced_tokens_per_source": round(forced / a.sources, 2)}
            for name in runs:
                med = float(np.median(ms[name]))
                rec[f"{name}_ms"] = round(med, 2)
                rec[f"{name}_ms_spread"] = [round(min(ms[name]), 2), round(max(ms[name]), 2)]
                rec[f"{name}_samples_per_s"] = round(samples / (med / 1e3), 1)
            for name in steps:
                rec[f"{name}_device_steps"], rec[f"{name}_accepted_tokens"] = steps[name], accepted[name]
            rec["empty_equals_unprompted"] = bool(torch.equal(torch.cat(outs["pool_empty"], 0), torch.cat(outs["pool_unprompted"], 0)))
            rec["empty_over_unprompted"] = round(rec["pool_empty_ms"] / rec["pool_unprompted_ms"], 4)
            rec["prompted_over_unprompted"] = round(rec["pool_prompted_ms"] / rec["pool_unprompted_ms"], 4)
            rec["plain_prompted_over_pool_prompted"] = round(rec["plain_prompted_ms"] / rec["pool_prompted_ms"], 4)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
