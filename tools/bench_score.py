#!/usr/bin/env python3
"""Cost of hypothesis scores (NativeTransformer.score_hypotheses, not part of bench.py) on bench.py's 4+4 weights and
USPTO-MIT-shaped synthetic batches (tools/synth.py):

  a  bs = 32, N = 1: the greedy-speculative outputs at max_len 200 (PAD-filled to 200 columns), with and without ``trim``;
  b  bs = 4, n_best = 5: the beam-speculative outputs (bench.py's c3 generator settings);
  c  a window of ``--window`` batches of (a) in ONE call, chunked through ``max_rows`` (sources right-padded to the window's
     longest), beside the same batches scored one call each.

Per case: ms per call of ``score_hypotheses`` (median over the batches and passes, HIP events around each call), of the same
forward alone on the same rows and columns — ``encode_src`` + ``decode_tgt`` with a row map, existing code of the same build in
the same run, timed alternately: the yardstick — and of ``decode_tgt`` alone, and scoring time as a fraction of the time the
generator took to decode the same batches (``generate`` per batch for a / b, ``generate_many(reorder=True)`` for the window).
Prints one JSON line.

The scoring kernels' share of kernel time comes from a run of its own under
``rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_score.py --trace-only --hyp FILE`` (score_hypotheses calls
only, on hypotheses a plain run saved with ``--hyp FILE``); ``--kernel-stats FILE`` then reads rocprofv3's kernel_stats.csv and adds
{kernel: total ns, launches} of k_hyp_score / k_score_src_of and their share of all kernel time to the line.
"""
from __future__ import annotations

import argparse
import csv
import json
import sys
from pathlib import Path
from timeit import default_timer as timer

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

KERNELS = ("k_hyp_score", "k_score_src_of")


def kernel_share(stats_csv: str) -> dict:
    rows = list(csv.DictReader(open(stats_csv)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    mine = {}
    for r in rows:
        for k in KERNELS:
            if k in r["Name"]:
                e = mine.setdefault(k, {"total_ns": 0.0, "launches": 0})
                e["total_ns"] += float(r["TotalDurationNs"])
                e["launches"] += int(r["Calls"])
    ns = sum(e["total_ns"] for e in mine.values())
    return {"kernels": mine, "score_kernels_share": ns / total if total else None, "all_kernels_ns": total}


def median_ms(fns: dict, cases: list, warmup: int, passes: int) -> dict:
    """{name: median ms per call} of every fn(case), the functions timed alternately case by case."""
    for _ in range(warmup):
        for c in cases:
            for f in fns.values():
                f(c)
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
    for _ in range(passes):
        for c in cases:
            ev[0].record()
            for i, f in enumerate(fns.values()):
                f(c)
                ev[i + 1].record()
            ev[-1].synchronize()
            for i, k in enumerate(fns):
                times[k].append(ev[i].elapsed_time(ev[i + 1]))
    return {k: round(float(np.median(v)), 4) for k, v in times.items()}


def extent(hyp: torch.Tensor, pad: int, eos: int) -> int:
    """The columns ``trim`` keeps."""
    W = hyp.shape[-1]
    cols = torch.arange(1, W + 1, device=hyp.device)
    return min(W, max(2, int((((hyp != pad) | (hyp == eos)) * cols).amax())))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16, help="batches of case a / b that are timed")
    ap.add_argument("--window", type=int, default=256, help="batches of case c")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hyp", default=None, help="plain run: save the hypotheses here (.pt); --trace-only: read them")
    ap.add_argument("--trace-only", action="store_true", help="score_hypotheses calls only (for the rocprofv3 run)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a --trace-only run")
    ap.add_argument("--line", default=None, help="with --kernel-stats: add the trace to this earlier JSON line, measure nothing")
    a = ap.parse_args()
    if a.line:
        rec = json.loads(Path(a.line).read_text().strip().split("\n")[-1])
        rec["trace"] = kernel_share(a.kernel_stats)
        print(json.dumps(rec))
        return
    assert torch.cuda.is_available(), "tools/bench_score.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    score = lambda c, **kw: native.score_hypotheses(c[0], c[1], eos_token_idx=EOS, **kw)     # noqa: E731

    if a.trace_only:
        cases = torch.load(a.hyp, weights_only=True)
        calls = 0
        for _ in range(a.warmup + a.passes):
            for name in ("a", "b"):
                for s, h in cases[name]:
                    score((s.cuda(), h.cuda()))
                    calls += 1
        torch.cuda.synchronize()
        print(json.dumps({"trace_only": True, "calls": calls}))
        return

    c3 = bench.BEAM_CONFIGS["c3"]
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.window * 32)
    src32 = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    src4 = [torch.from_numpy(b).cuda() for b in batches(src_rows[:a.batches * c3["bs"]], c3["bs"])]
    greedy = tta.TranslationInferenceGreedySpeculative(native, 200, 10, 3, PAD, BOS, EOS, C_TOK)
    beam = tta.TranslationInferenceBeamSearchSpeculative(native, 200, c3["n_best"], 10, c3["N"], V, False, PAD, BOS, EOS, C_TOK,
                                                         max_steps=800)

    def forward(c, cols=None):                      # the yardstick: the same encoder + decoder pass through the existing entry points
        s, h = c
        B, N, W = h.shape
        Wt = cols or W
        rows = torch.arange(B * N, device=s.device, dtype=torch.int32) // N
        return native.decode_tgt(h.reshape(B * N, W)[:, :Wt - 1], native.encode_src(s), s == PAD, memory_row=rows)

    rec = {"tool": "bench_score", "timed_batches": a.batches, "passes": a.passes, "max_rows": native.SCORE_MAX_ROWS}
    saved = {}
    for name, gen, srcs in (("a", greedy, src32[:a.batches]), ("b", beam, src4)):
        cases = []
        for s in srcs:                              # a batch on which the reference raises has no hypotheses to score
            try:
                cases.append((s, gen.generate(s)))
            except (tta.ReferenceError_, RuntimeError):
                pass
        decode_ms = median_ms({"generate": gen.generate}, [s for s, _ in cases], 1, 2)["generate"]
        saved[name] = [(s.cpu(), h.cpu()) for s, h in cases]
        ext = [extent(h, PAD, EOS) for _, h in cases]
        mem = [native.encode_src(s) for s, _ in cases]
        idx = {id(c): i for i, c in enumerate(cases)}

        def decode_only(c, trimmed):
            s, h = c
            B, N, W = h.shape
            Wt = ext[idx[id(c)]] if trimmed else W
            rows = torch.arange(B * N, device=s.device, dtype=torch.int32) // N
            return native.decode_tgt(h.reshape(B * N, W)[:, :Wt - 1], mem[idx[id(c)]], s == PAD, memory_row=rows)

        fns = {"score_trim": lambda c: score(c),
               "forward_trim": lambda c: forward(c, ext[idx[id(c)]]),
               "decode_tgt_trim": lambda c: decode_only(c, True)}
        if name == "a":
            fns.update({"score_full": lambda c: score(c, trim=False), "forward_full": lambda c: forward(c),
                        "decode_tgt_full": lambda c: decode_only(c, False)})
        ms = median_ms(fns, cases, a.warmup, a.passes)
        sc = [score(c) for c in cases]
        rec[name] = {"shape": list(cases[0][1].shape), "mean_columns_scored": float(np.mean(ext)) - 1, "ms": ms,
                     "generate_ms": decode_ms, "score_over_generate": round(ms["score_trim"] / decode_ms, 4),
                     "score_over_forward": round(ms["score_trim"] / ms["forward_trim"], 4),
                     "unfinished": int(sum((~r.finished).sum() for r in sc)), "hypotheses": int(sum(r.score.numel() for r in sc)),
                     "mean_top1_logprob": round(float(torch.cat([r.score[:, 0] for r in sc]).double().mean()), 4)}
        if name == "a":
            rec[name]["score_full_over_forward_full"] = round(ms["score_full"] / ms["forward_full"], 4)
    if a.hyp:
        torch.save(saved, a.hyp)

    # c: one call over the whole window (sources right-padded to the window's longest, hypotheses [window * 32, 1, 200])
    many = lambda: greedy.generate_many(src32, in_flight=8, reorder=True, on_error="skip")      # noqa: E731
    many()
    torch.cuda.synchronize()
    t0 = timer()
    preds = many()
    torch.cuda.synchronize()
    window_decode_ms = (timer() - t0) * 1e3
    src32 = [s for s, p in zip(src32, preds) if p is not None]
    preds = [p for p in preds if p is not None]
    Ls = max(s.shape[1] for s in src32)
    src_all = torch.cat([torch.nn.functional.pad(s, (0, Ls - s.shape[1]), value=PAD) for s in src32])
    hyp_all = torch.cat(preds)
    case = (src_all, hyp_all)
    ms = median_ms({"score_window": lambda c: score(c), "score_per_batch": lambda c: [score(p) for p in zip(src32, preds)]},
                   [case], 1, 3)
    rec["c"] = {"shape": list(hyp_all.shape), "columns_scored": extent(hyp_all, PAD, EOS) - 1, "ms": ms,
                "generate_many_ms": round(window_decode_ms, 2),
                "score_over_generate": round(ms["score_window"] / window_decode_ms, 4),
                "ms_per_batch_of_32": round(ms["score_window"] / len(src32), 4)}
    if a.kernel_stats:
        rec["trace"] = kernel_share(a.kernel_stats)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
