#!/usr/bin/env python3
"""Cost of cross-attention maps (NativeTransformer.attention_maps, not part of bench.py) on bench.py's 4+4 weights and
USPTO-MIT-shaped synthetic batches (tools/synth.py):

  a  bs = 32, N = 1: the greedy-speculative outputs at max_len 200;
  b  bs = 4, n_best = 5: the beam-speculative outputs (bench.py's c3 generator settings).

Per case: ms per call (median over the batches and passes, HIP events around each call, the functions timed alternately) of
``attention_maps`` with heads="mean" and heads="all" (last layer) and of ``score_hypotheses`` on the same inputs — code the parent
commit has, the yardstick: the maps' pass ends at the last layer's cross attention, the scores' pass runs on through the
classifier.  ``fill_all_GBps``: the rate at which a plain fp32 fill (torch's ``fill_``) streams a buffer of the size of the
heads="all" maps of a batch, timed the same way: what stores alone reach on this part.  Prints one JSON line.

The kernel's own time comes from runs of their own under
``rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_attn_maps.py --trace-only --heads all --hyp FILE``
(attention_maps calls only, on hypotheses a plain run saved with ``--hyp FILE``; one run per ``--heads``); ``--kernel-stats FILE
--heads H --line JSON`` then reads rocprofv3's kernel_stats.csv and adds, under trace_H, the total ns and launches of k_attn_probs /
k_hyp_length, the map bytes those launches wrote (computed from the saved shapes) and the kernel's output bytes per second.
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
from tools.bench_score import extent, median_ms  # noqa: E402

KERNELS = ("k_attn_probs", "k_hyp_length")
HEADS = 8


def map_bytes(cases: dict, heads: str, pad: int, eos: int) -> int:
    """Bytes of maps and alignments one pass over the saved cases writes (trimmed widths, as attention_maps runs them)."""
    total = 0
    for name in ("a", "b"):
        for s, h in cases[name]:
            B, N, _ = h.shape
            T = extent(h, pad, eos) - 1
            total += B * N * T * (s.shape[1] * 4 * (HEADS if heads == "all" else 1) + 4)
    return total


def kernel_trace(stats_csv: str, out_bytes: int) -> dict:
    rows = list(csv.DictReader(open(stats_csv)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    mine = {}
    for r in rows:
        for k in KERNELS:
            if k in r["Name"]:
                e = mine.setdefault(k, {"total_ns": 0.0, "launches": 0})
                e["total_ns"] += float(r["TotalDurationNs"])
                e["launches"] += int(r["Calls"])
    ns = mine.get("k_attn_probs", {}).get("total_ns", 0.0)
    return {"kernels": mine, "all_kernels_ns": total, "attn_probs_share": ns / total if total else None,
            "output_bytes": out_bytes, "attn_probs_output_GBps": round(out_bytes / ns, 2) if ns else None}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16, help="batches of each case that are timed")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--heads", default="all", choices=("mean", "all"), help="--trace-only / --kernel-stats: which maps")
    ap.add_argument("--hyp", default=None, help="plain run: save the hypotheses here (.pt); --trace-only / --kernel-stats: read them")
    ap.add_argument("--trace-only", action="store_true", help="attention_maps calls only (for the rocprofv3 run)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a --trace-only run")
    ap.add_argument("--line", default=None, help="with --kernel-stats: add the trace to this earlier JSON line, measure nothing")
    a = ap.parse_args()
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK, V
    if a.line:
        rec = json.loads(Path(a.line).read_text().strip().split("\n")[-1])
        cases = torch.load(a.hyp, weights_only=True)
        calls = rec["trace_calls_per_case_pass"]
        rec[f"trace_{a.heads}"] = kernel_trace(a.kernel_stats, map_bytes(cases, a.heads, PAD, EOS) * calls)
        print(json.dumps(rec))
        return
    assert torch.cuda.is_available(), "tools/bench_attn_maps.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), HEADS, PAD, device=0)
    maps = lambda c, heads: native.attention_maps(c[0], c[1], eos_token_idx=EOS, heads=heads)     # noqa: E731

    if a.trace_only:
        cases = torch.load(a.hyp, weights_only=True)
        calls = 0
        for _ in range(a.warmup + a.passes):
            for name in ("a", "b"):
                for s, h in cases[name]:
                    maps((s.cuda(), h.cuda()), a.heads)
                    calls += 1
        torch.cuda.synchronize()
        print(json.dumps({"trace_only": True, "heads": a.heads, "calls": calls}))
        return

    c3 = bench.BEAM_CONFIGS["c3"]
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.batches * 32)
    src32 = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    src4 = [torch.from_numpy(b).cuda() for b in batches(src_rows[:a.batches * c3["bs"]], c3["bs"])]
    greedy = tta.TranslationInferenceGreedySpeculative(native, 200, 10, 3, PAD, BOS, EOS, C_TOK)
    beam = tta.TranslationInferenceBeamSearchSpeculative(native, 200, c3["n_best"], 10, c3["N"], V, False, PAD, BOS, EOS, C_TOK,
                                                         max_steps=800)
    rec = {"tool": "bench_attn_maps", "timed_batches": a.batches, "passes": a.passes, "layer": -1,
           "trace_calls_per_case_pass": a.warmup + a.passes}
    saved = {}
    for name, gen, srcs in (("a", greedy, src32), ("b", beam, src4)):
        cases = []
        for s in srcs:                              # a batch on which the reference raises has no hypotheses
            try:
                cases.append((s, gen.generate(s)))
            except (tta.ReferenceError_, RuntimeError):
                pass
        saved[name] = [(s.cpu(), h.cpu()) for s, h in cases]
        ext = [extent(h, PAD, EOS) for _, h in cases]
        all_floats = int(np.median([h.shape[0] * h.shape[1] * HEADS * (e - 1) * s.shape[1] for (s, h), e in zip(cases, ext)]))
        fill_buf = torch.empty(all_floats, dtype=torch.float32, device="cuda")
        fns = {"maps_mean": lambda c: maps(c, "mean"), "maps_all": lambda c: maps(c, "all"),
               "score": lambda c: native.score_hypotheses(c[0], c[1], eos_token_idx=EOS),
               "fill_all": lambda c: fill_buf.fill_(1.0)}
        ms = median_ms(fns, cases, a.warmup, a.passes)
        m = [maps(c, "mean") for c in cases]
        sc = [native.score_hypotheses(c[0], c[1], eos_token_idx=EOS) for c in cases]
        assert all(torch.equal(x.length, y.length) for x, y in zip(m, sc))
        rec[name] = {"shape": list(cases[0][1].shape), "mean_columns": float(np.mean(ext)) - 1,
                     "mean_source_columns": float(np.mean([s.shape[1] for s, _ in cases])), "ms": ms,
                     "maps_mean_over_score": round(ms["maps_mean"] / ms["score"], 4),
                     "maps_all_over_score": round(ms["maps_all"] / ms["score"], 4),
                     "median_all_map_bytes": all_floats * 4,
                     "fill_all_GBps": round(all_floats * 4 / (ms["fill_all"] * 1e6), 2),
                     "maps_all_call_GBps": round(all_floats * 4 / (ms["maps_all"] * 1e6), 2)}
    # k: ONE k_attn_probs launch (ttx_debug_attn_probs) at the size of a 32 x 5 beam batch, R = 160, H = 8, T = Ls = 200, every
    # position live, beside a plain fill of its 205 MB: events around a single launch, so launch overhead is included in both
    R, T, Ls, dh = 160, 200, 200, 32
    gen = torch.Generator(device="cuda").manual_seed(7)
    q = torch.randn((R * T, HEADS * dh), device="cuda", generator=gen)
    k = torch.randn((32 * Ls, 2 * HEADS * dh), device="cuda", generator=gen)
    key_pad = torch.zeros(32 * Ls, dtype=torch.uint8, device="cuda")
    mem_row = (torch.arange(R, device="cuda") // 5).to(torch.int32)
    length = torch.full((R,), T, dtype=torch.int32, device="cuda")
    heads = torch.empty((R, HEADS, T, Ls), device="cuda")
    mean = torch.empty((R, T, Ls), device="cuda")
    probs = lambda **kw: native.debug_attn_probs(q, k, key_pad, length, HEADS, dh, T, Ls, dh ** -0.5, mem_row=mem_row, **kw)  # noqa: E731
    ms = median_ms({"probs_heads": lambda c: probs(out_heads=heads), "probs_mean": lambda c: probs(out_mean=mean),
                    "fill_heads": lambda c: heads.fill_(1.0), "fill_mean": lambda c: mean.fill_(1.0)}, [None], 3, 20)
    rec["k"] = {"R": R, "H": HEADS, "T": T, "Ls": Ls, "head_dim": dh, "ms": ms, "heads_bytes": heads.numel() * 4,
                "probs_heads_GBps": round(heads.numel() * 4 / (ms["probs_heads"] * 1e6), 1),
                "fill_heads_GBps": round(heads.numel() * 4 / (ms["fill_heads"] * 1e6), 1),
                "probs_mean_GBps": round(mean.numel() * 4 / (ms["probs_mean"] * 1e6), 1),
                "fill_mean_GBps": round(mean.numel() * 4 / (ms["fill_mean"] * 1e6), 1),
                "gflop": round(2.0 * R * HEADS * T * Ls * dh / 1e9, 2)}
    if a.hyp:
        torch.save(saved, a.hyp)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
