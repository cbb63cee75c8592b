#!/usr/bin/env python3
"""What folding sampled hypotheses costs on the device and on the host (not part of bench.py): ``fold`` (ttx_fold_hypotheses,
order="score", gather on) beside ``scoring.unique_samples`` on the same tensors, and beside the two calls that come before it: the
``generate_many`` / ``generate`` call that produced the rows and the ``score`` pass.  bench.py's 4+4 weights, USPTO-MIT-shaped
synthetic sources (tools/synth.py), max_len 200, temperature 1:

  pool_1024_n8 / pool_1024_n64   TranslationInferenceSamplingSpeculative.generate_many over 1 024 sources at num_samples 8 and 64
                                 ((n_drafts, draft_len) = (3, 10)), the rows of all sources folded in one call
  batch_32_n8                    one batch of 32 sources from TranslationInferenceSampling.generate at num_samples 8

Timing: the device fold with HIP events around ``--reps`` back-to-back calls after warm-up; ``unique_samples`` on the host clock,
ending in a synchronise (it copies the rows to the host itself); generation and scoring with HIP events around one call.  The
four are timed alternately, pass by pass; figures are medians over the passes.  Then the kernel alone at N = 1 024, W = 200,
B = 64: all rows distinct (the worst case of phases 2 and 3) and all rows equal.  One JSON line per case, written to ``--out``.
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
SEED = 20260128


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=1024, help="sources of the pool's list")
    ap.add_argument("--warmup", type=int, default=1, help="untimed passes")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back fold calls inside one timed window")
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r28_bench_fold.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_fold.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.sources)
    small = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def host_fold(pred, sc):
        t0 = time.perf_counter()
        out = tta.scoring.unique_samples(pred, sc, eos=EOS)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def measure(name, g, generate, score_chunks):
        """``generate()`` -> Long[B, n, L]; the score pass runs over ``score_chunks`` sources at a time."""
        def score(pred, srcs):
            parts = [g.score(s, p).score for s, p in zip(srcs, pred.split([int(s.shape[0]) for s in srcs], 0))]
            return torch.cat(parts, 0)
        ms = {k: [] for k in ("generate", "score", "fold", "unique_samples")}
        for p in range(a.warmup + a.passes):
            t_gen, pred = timed(generate)
            t_sc, sc = timed(lambda: score(pred, score_chunks))
            f = native.fold_hypotheses(pred, sc, order="score", eos=EOS)            # warm
            t_fold, f = timed(lambda: [native.fold_hypotheses(pred, sc, order="score", eos=EOS) for _ in range(a.reps)][-1])
            t_host, u = host_fold(pred, sc)
            if p >= a.warmup:
                for k, v in (("generate", t_gen), ("score", t_sc), ("fold", t_fold / a.reps), ("unique_samples", t_host)):
                    ms[k].append(v)
        nu = f.n_unique.cpu()
        assert [len(x) for x in u] == nu.tolist(), "the device fold and unique_samples disagree on the distinct hypotheses"
        B, n, L = pred.shape
        rec = {"tool": "bench_fold", "case": name, "sources": B, "num_samples": n, "max_len": L, "passes": a.passes, "fold_reps": a.reps,
               "order": "score", "gather": True, "mean_n_unique": round(float(nu.float().mean()), 3)}
        for k, v in ms.items():
            rec[f"{k}_ms"] = round(float(np.median(v)), 4)
            rec[f"{k}_ms_spread"] = [round(min(v), 4), round(max(v), 4)]
        rec["unique_samples_over_fold"] = round(rec["unique_samples_ms"] / rec["fold_ms"], 1)
        rec["fold_share_of_generate_plus_score"] = round(rec["fold_ms"] / (rec["generate_ms"] + rec["score_ms"]), 6)
        rec["note"] = ("fold: HIP events around back-to-back calls (output allocation and launch included); unique_samples: host clock "
                       "ending in a synchronise, device-to-host copy included; generate / score: HIP events around one call")
        emit(rec)

    kw = dict(temperature=1.0, seed=SEED)
    for n in (8, 64):
        g = tta.TranslationInferenceSamplingSpeculative(native, a.max_len, 10, 3, PAD, BOS, EOS, C_TOK, num_samples=n, **kw)
        measure(f"pool_{a.sources}_n{n}", g, lambda g=g: torch.cat(g.generate_many(small), 0), small)
    g = tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, num_samples=8, **kw)
    measure("batch_32_n8", g, lambda: g.generate(small[0]), small[:1])

    # the kernel alone: N = 1 024, W = 200, B = 64
    B, N, W = 64, 1024, 200
    base = torch.randint(4, 200, (B, 1, W), device="cuda")
    base[:, :, W - 1] = EOS
    equal = base.expand(B, N, W).contiguous()
    distinct = equal.clone()
    distinct[:, :, 5] = 1000 + torch.arange(N, device="cuda")
    sc = -torch.rand((B, N), device="cuda") * 30
    for name, rows in (("kernel_all_distinct", distinct), ("kernel_all_equal", equal)):
        for _ in range(3):
            f = native.fold_hypotheses(rows, sc, order="score", eos=EOS)
        per = []
        for _ in range(a.passes):
            t, f = timed(lambda: [native.fold_hypotheses(rows, sc, order="score", eos=EOS) for _ in range(10)][-1])
            per.append(t / 10)
        emit({"tool": "bench_fold", "case": name, "sources": B, "rows_per_source": N, "width": W, "order": "score", "gather": True,
              "mean_n_unique": float(f.n_unique.float().mean()), "ms_per_call": round(float(np.median(per)), 4),
              "ms_spread": [round(min(per), 4), round(max(per), 4)],
              "input_GB": round(B * N * W * 8 / 1e9, 4),
              "note": "back-to-back calls on one stream, output allocation and launch included; one workgroup per source, so 64 of the "
                      "256 CUs are busy"})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
