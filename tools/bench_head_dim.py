#!/usr/bin/env python3
"""Cost of head dimension 64 beside head dimension 32 (not part of bench.py): two seeded 4+4-layer models of bench.py's width
(d = 256, F = 2048) that differ only in the head count, 8 heads (head dimension 32: verify steps on k_attn3 / k_attn3s) and 4
heads (head dimension 64: verify steps on k_attn2), on the same USPTO-MIT-shaped synthetic sources (tools/synth.py):

  a  greedy-speculative ``generate`` at bs = 32, N = 3, D = 10, max_len 200, per batch;
  b  ``generate_many(reorder=True)`` over 640 rows (20 batches of 32) through the slot pool.

Same build, same run, the two models alternated batch by batch, medians over the batches and passes (HIP events around each
call).  The weights are seeded, not trained, so the two models do not decode the same tokens: beside the ms per call the line
gives the decoder calls of each model and the ms per decoder call, which is the figure to compare.  Prints one JSON line.

Attention's share of kernel time comes from runs of their own under
``rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_head_dim.py --trace-only --heads H`` (case a only);
``--kernel-stats-8 FILE --kernel-stats-4 FILE --line FILE`` then adds {kernel: total ns, launches} of the attention kernels and
their share of all kernel time to an earlier line.
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
sys.path.insert(0, str(ROOT / "tests"))

D_MODEL, FFN, LAYERS, SEED = 256, 2048, 4, 20250725
N_DRAFTS, DRAFT_LEN, MAX_LEN, BS = 3, 10, 200, 32


def kernel_share(stats_csv: str) -> dict:
    rows = list(csv.DictReader(open(stats_csv)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    mine = {}
    for r in rows:
        name = r["Name"]
        if "k_attn" in name:
            key = name[name.index("k_attn"):].split("(")[0]
            e = mine.setdefault(key, {"total_ns": 0.0, "launches": 0})
            e["total_ns"] += float(r["TotalDurationNs"])
            e["launches"] += int(r["Calls"])
    ns = sum(e["total_ns"] for e in mine.values())
    return {"kernels": mine, "attention_share": ns / total if total else None, "all_kernels_ns": total}


def model(tta, heads: int, V: int, pad: int):
    from util_models import seeded_weights, state_shapes
    st = seeded_weights(state_shapes(V, D_MODEL, FFN, LAYERS, LAYERS), SEED)
    st["tgt_token_featurizer.embedding.weight"] = st["src_token_featurizer.embedding.weight"]
    return tta.NativeTransformer(st, heads, pad, device=0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20, help="batches of 32 rows (case b decodes all of them in one call)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true", help="case a of one model only (for the rocprofv3 run)")
    ap.add_argument("--heads", type=int, default=4, help="--trace-only: the model's head count (8 or 4)")
    ap.add_argument("--kernel-stats-8", default=None, help="rocprofv3 kernel_stats.csv of a --trace-only --heads 8 run")
    ap.add_argument("--kernel-stats-4", default=None, help="the same for --heads 4")
    ap.add_argument("--line", default=None, help="with --kernel-stats-*: add the traces to this earlier JSON line, measure nothing")
    a = ap.parse_args()
    if a.line:
        rec = json.loads(Path(a.line).read_text().strip().split("\n")[-1])
        rec["trace"] = {h: kernel_share(f) for h, f in (("heads8", a.kernel_stats_8), ("heads4", a.kernel_stats_4)) if f}
        print(json.dumps(rec))
        return
    assert torch.cuda.is_available(), "tools/bench_head_dim.py measures on an MI355X; there is no CPU figure"
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK, V
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.batches * BS)
    srcs = [torch.from_numpy(b).cuda() for b in batches(src_rows, BS)]
    gen = lambda m: tta.TranslationInferenceGreedySpeculative(m, MAX_LEN, DRAFT_LEN, N_DRAFTS, PAD, BOS, EOS, C_TOK)   # noqa: E731

    def decodable(g):                                 # a batch on which the reference raises is left out for both models
        ok = set()
        for i, s in enumerate(srcs):
            try:
                g.generate(s)
                ok.add(i)
            except (tta.ReferenceError_, RuntimeError):
                pass
        return ok

    if a.trace_only:
        g = gen(model(tta, a.heads, V, PAD))
        ok = decodable(g)
        for _ in range(a.passes):
            for i in sorted(ok):
                g.generate(srcs[i])
        torch.cuda.synchronize()
        print(json.dumps({"trace_only": True, "heads": a.heads, "batches": len(ok), "passes": a.passes}))
        return

    gens = {"heads8": gen(model(tta, 8, V, PAD)), "heads4": gen(model(tta, 4, V, PAD))}
    keep = sorted(set.intersection(*(decodable(g) for g in gens.values())))
    srcs = [srcs[i] for i in keep]
    rec = {"tool": "bench_head_dim", "d": D_MODEL, "ffn": FFN, "layers": LAYERS, "bs": BS, "n_drafts": N_DRAFTS, "draft_len": DRAFT_LEN,
           "max_len": MAX_LEN, "batches": len(srcs), "passes": a.passes}

    # a: per-batch generate, the two models alternated batch by batch
    times = {k: [] for k in gens}
    calls = {k: 0 for k in gens}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for p in range(a.warmup + a.passes):
        for s in srcs:
            ev[0].record()
            for i, (k, g) in enumerate(gens.items()):
                c0 = g.model_calls_num
                g.generate(s)
                ev[i + 1].record()
                if p >= a.warmup:
                    calls[k] += g.model_calls_num - c0
            ev[-1].synchronize()
            if p >= a.warmup:
                for i, k in enumerate(gens):
                    times[k].append(ev[i].elapsed_time(ev[i + 1]))
    rec["a_generate"] = {k: {"ms_per_batch_median": round(float(np.median(times[k])), 3),
                             "decoder_calls_per_batch": round(calls[k] / len(times[k]), 2),
                             "ms_per_decoder_call": round(float(np.sum(times[k])) / calls[k], 4)} for k in gens}
    rec["a_generate"]["ms_per_decoder_call_ratio_4_over_8"] = round(
        rec["a_generate"]["heads4"]["ms_per_decoder_call"] / rec["a_generate"]["heads8"]["ms_per_decoder_call"], 4)

    # b: the rows of all batches through the slot pool, the two models alternated call by call
    many = {k: [] for k in gens}
    mcalls = {}
    for p in range(a.warmup + a.passes):
        for k, g in gens.items():
            c0 = g.model_calls_num
            torch.cuda.synchronize()
            t0 = timer()
            g.generate_many(srcs, in_flight=8, reorder=True, on_error="skip")
            torch.cuda.synchronize()
            if p >= a.warmup:
                many[k].append((timer() - t0) * 1e3)
                mcalls[k] = g.model_calls_num - c0
    rec["b_generate_many"] = {k: {"rows": len(srcs) * BS, "ms_median": round(float(np.median(many[k])), 2),
                                  "decoder_calls": mcalls[k], "ms_per_decoder_call": round(float(np.median(many[k])) / mcalls[k], 4)}
                              for k in gens}
    rec["b_generate_many"]["ms_per_decoder_call_ratio_4_over_8"] = round(
        rec["b_generate_many"]["heads4"]["ms_per_decoder_call"] / rec["b_generate_many"]["heads8"]["ms_per_decoder_call"], 4)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
