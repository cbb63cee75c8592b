#!/usr/bin/env python3
"""Cost of scoring a LIST of batches (not part of bench.py) on bench.py's 4+4 weights and USPTO-MIT-shaped synthetic batches
(tools/synth.py), three paths over the same rows:

  per_batch   ``score_hypotheses`` batch by batch: one trim synchronisation and one set of launches per batch;
  one_call    ONE ``score_hypotheses`` over the concatenated list (sources right-padded to the list's longest), trimmed at the
              longest row of the list and chunked through ``max_rows``;
  list        ``score_hypotheses_many``: the length-bucketed pass, one synchronisation.

Workloads: (i) ``--window`` batches of 32 greedy-speculative outputs at max_len 200 (DESIGN.md §10 row c); (ii) ``--sources``
sources x 8 samples of the pooled speculative sampler at temperature 1.  Per path: the median wall-clock ms of ``--passes`` passes
after ``--warmup`` (the paths alternate within a pass; the device is idle before and after each timed call), the fastest and
slowest pass (the run-to-run spread), and the decoder and source positions the path runs, counted from the shapes of its calls.
``list_beats_yardsticks``: the list's slowest pass is faster than the fastest pass of both other paths.  Both workloads also sweep
``max_rows`` of the list path (``list`` itself runs at the default).  ``scoring_share``: a path's ms / (generate_many ms + that ms).
One JSON line per workload, printed and written to ``--out``."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path
from timeit import default_timer as timer

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = timer()
    out = fn()
    torch.cuda.synchronize()
    return (timer() - t0) * 1e3, out


def extent(hyp: torch.Tensor, pad: int, eos: int) -> int:
    """The columns ``score_hypotheses(trim=True)`` keeps."""
    W = hyp.shape[-1]
    cols = torch.arange(1, W + 1, device=hyp.device)
    return min(W, max(2, int((((hyp != pad) | (hyp == eos)) * cols).amax())))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=256, help="batches of 32 of workload (i)")
    ap.add_argument("--sources", type=int, default=1024, help="sources of workload (ii)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--sweep", default="8192,16384,32768,65536", help="max_rows values of the list path, swept on both workloads")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r30_bench_score_many.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_score_many.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    sweep = [int(x) for x in a.sweep.split(",") if x]
    lines = []

    def measure(tag: str, srcs: list, preds: list, generate_ms: float, with_sweep: bool) -> None:
        Ls = max(s.shape[1] for s in srcs)
        src_all = torch.cat([torch.nn.functional.pad(s, (0, Ls - s.shape[1]), value=PAD) for s in srcs])
        hyp_all = torch.cat(preds)
        N = hyp_all.shape[1]
        paths = {"per_batch": lambda: [native.score_hypotheses(s, p, eos_token_idx=EOS) for s, p in zip(srcs, preds)],
                 "one_call": lambda: native.score_hypotheses(src_all, hyp_all, eos_token_idx=EOS),
                 "list": lambda: native.score_hypotheses_many(srcs, preds, eos_token_idx=EOS)}
        for m in (sweep if with_sweep else []):
            paths[f"list_max_rows_{m}"] = lambda m=m: native.score_hypotheses_many(srcs, preds, eos_token_idx=EOS, max_rows=m)
        ms = {k: [] for k in paths}
        outs, plans = {}, {}
        for p in range(a.warmup + a.passes):
            for name, fn in paths.items():
                t, outs[name] = wall_ms(fn)
                if name.startswith("list"):
                    plans[name] = native.last_score_plan
                if p >= a.warmup:
                    ms[name].append(t)
        cat = lambda rs, f: torch.cat([getattr(r, f) for r in rs])                                     # noqa: E731
        same = {f: bool(torch.equal(cat(outs["list"], f), cat(outs["per_batch"], f)) and
                        torch.equal(cat(outs["list"], f), getattr(outs["one_call"], f))) for f in ("score", "length", "finished")}
        ext = [extent(p, PAD, EOS) for p in preds]
        ext_all = extent(hyp_all, PAD, EOS)
        positions = {"per_batch": {"decoder": int(sum(p.shape[0] * N * (e - 1) for p, e in zip(preds, ext))),
                                   "source": int(sum(s.numel() for s in srcs)), "calls": len(srcs)},
                     "one_call": {"decoder": int(hyp_all.shape[0] * N * (ext_all - 1)), "source": int(src_all.numel()),
                                  "calls": -(-hyp_all.shape[0] // max(1, native.SCORE_MAX_ROWS // (N * (ext_all - 1))))}}
        for name, plan in plans.items():
            positions[name] = {"decoder": int(sum(c.positions for c in plan)), "source": int(sum(len(c.sources) * c.Ls for c in plan)),
                               "calls": len(plan)}
        rec = {"tool": "bench_score_many", "workload": tag, "batches": len(srcs), "rows": int(hyp_all.shape[0] * N), "N": int(N),
               "hyp_width": int(hyp_all.shape[2]), "longest_row_columns": ext_all - 1, "mean_batch_columns": round(float(np.mean(ext)) - 1, 2),
               "passes": a.passes, "max_rows": native.SCORE_MAX_ROWS,
               "median_ms": {k: round(float(np.median(v)), 2) for k, v in ms.items()},
               "spread_ms": {k: [round(min(v), 2), round(max(v), 2)] for k, v in ms.items()},
               "positions": positions, "bit_identical_to_both": same}
        med = rec["median_ms"]
        rec["list_over_per_batch"] = round(med["list"] / med["per_batch"], 4)
        rec["list_over_one_call"] = round(med["list"] / med["one_call"], 4)
        rec["list_beats_yardsticks"] = bool(max(ms["list"]) < min(min(ms["per_batch"]), min(ms["one_call"])))
        rec["generate_many_ms"] = round(generate_ms, 2)
        rec["scoring_share"] = {k: round(med[k] / (generate_ms + med[k]), 4) for k in ("per_batch", "one_call", "list")}
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    # (i) the greedy-speculative outputs of a window of batches of 32
    src_rows, _ = SynthReactions(123456, "mit").dataset(max(a.window * 32, a.sources))
    src32 = [torch.from_numpy(b).cuda() for b in batches(src_rows[:a.window * 32], 32)]
    greedy = tta.TranslationInferenceGreedySpeculative(native, 200, 10, 3, PAD, BOS, EOS, C_TOK)
    many = lambda: greedy.generate_many(src32, in_flight=8, reorder=True, on_error="skip")             # noqa: E731
    many()
    gen_ms, preds = wall_ms(many)
    keep = [i for i, p in enumerate(preds) if p is not None]
    measure("i_greedy_speculative_256x32", [src32[i] for i in keep], [preds[i] for i in keep], gen_ms, True)

    # (ii) 8 samples per source from the pooled speculative sampler, temperature 1
    small = [torch.from_numpy(b).cuda() for b in batches(src_rows[:a.sources], 32)]
    keys = [torch.arange(32 * i, min(32 * (i + 1), a.sources)) for i in range(len(small))]
    pool = tta.TranslationInferenceSamplingSpeculative(native, 200, 10, 3, PAD, BOS, EOS, C_TOK, temperature=1.0, num_samples=8, seed=1234)
    sample = lambda: pool.generate_many(small, row_keys=keys)                                          # noqa: E731
    sample()
    gen_ms, preds = wall_ms(sample)
    measure("ii_pooled_sampler_1024x8", small, preds, gen_ms, True)

    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
