#!/usr/bin/env python3
"""Cost of stochastic beam search (TranslationInferenceStochasticBeamSearch, not part of bench.py) on bench.py's 4+4 weights and
USPTO-MIT-shaped synthetic batches (tools/synth.py), bs = 32, max_len 200, temperature 1, K = 5 and 10:

  per generate call, beside TranslationInferenceBeamSearch of the same K on the same rows (the same loop with k_beam_step: the
  yardstick) and beside TranslationInferenceSampling with num_samples = K followed by scoring.unique_samples' folding (distinct
  candidates per source and per millisecond).  HIP events around each call, the generators alternated batch by batch, warm-up
  first, medians over the batches and passes.  The loops do not run the same number of steps, so ms per step is given too.

  k_sbs_step alone against k_beam_step alone at (beam, V) = (5, 256) and (32, 1 024), 32 sources: one ttx_debug_* launch each
  (launch, kernel and the entry's stream synchronisation, the same for both) between two events, alternated, median of 5 rounds of
  20 launches.

Writes one JSON line per case to --out (and prints them).
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
sys.path.insert(0, str(ROOT / "tests"))


def kernel_alone(native, beam: int, V: int, B: int = 32, rounds: int = 5, launches: int = 20) -> dict:
    import util_sbs_checks as S
    c = S._draw_case(V, beam, beam, 1.0, B, 0)
    n = B * beam
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    common = dict(logits=dev(c.logits), slot_of=dev(c.slot_of), finished=dev(c.finished.astype(np.uint8)), gen=dev(c.gen),
                  new_cand=torch.zeros((n, c.ld), dtype=torch.int64, device="cuda"), parent=torch.zeros(n, dtype=torch.int32, device="cuda"),
                  new_len=torch.zeros(n, dtype=torch.int32, device="cuda"), new_finished=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                  parent_draft=torch.zeros(n, dtype=torch.int32, device="cuda"), summary=torch.zeros(5, dtype=torch.int32, device="cuda"))
    phi, G, key = dev(c.phi), dev(c.G), dev(c.keys)
    new_a, new_b = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shape = dict(V=V, ld=c.ld, width=c.width, B=B, beam=beam, K=beam, pad=c.pad, eos=c.eos)

    def sbs():
        native.debug_sbs_step(**shape, pos=c.pos, seed=c.seed, inv_T=1.0, phi=phi, g=G, key=key, new_phi=new_a, new_g=new_b, **common)

    def beam_step():
        native.debug_beam_step(**shape, score=phi, new_score=new_a, **common)
    for f in (sbs, beam_step):
        for _ in range(5):
            f()
    times = {"k_sbs_step": [], "k_beam_step": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for name, f in (("k_sbs_step", sbs), ("k_beam_step", beam_step)):
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000.0 / launches)
    rec = {"tool": "bench_sbs", "case": f"step_kernel_beam{beam}_V{V}", "sources": B,
           "us_per_launch_k_sbs_step": round(float(np.median(times["k_sbs_step"])), 2),
           "us_per_launch_k_beam_step": round(float(np.median(times["k_beam_step"])), 2)}
    rec["difference_us"] = round(rec["us_per_launch_k_sbs_step"] - rec["us_per_launch_k_beam_step"], 2)
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5, help="batches of 32 sources that are timed")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r21_bench_sbs.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_sbs.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.batches * 32)
    srcs = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    keys = [torch.arange(32 * i, 32 * (i + 1)) for i in range(len(srcs))]

    lines = []
    for K in (5, 10):
        gens = {"stochastic_beam_search": tta.TranslationInferenceStochasticBeamSearch(native, K, a.max_len, PAD, BOS, EOS, temperature=1.0,
                                                                                       seed=20260104),
                "beam_search": tta.TranslationInferenceBeamSearch(native, K, a.max_len, PAD, BOS, EOS),
                "sampling": tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, temperature=1.0, num_samples=K, seed=20260104)}

        def call(name, i):
            return gens[name].generate(srcs[i]) if name == "beam_search" else gens[name].generate(srcs[i], row_keys=keys[i])
        for _ in range(a.warmup):
            for i in range(len(srcs)):
                for name in gens:
                    call(name, i)
        torch.cuda.synchronize()
        ms, steps, distinct = ({k: [] for k in gens} for _ in range(3))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(gens) + 1)]
        for p in range(a.passes):
            for i in range(len(srcs)):
                before = {k: g.model_calls_num for k, g in gens.items()}
                order = list(gens)[i % 3:] + list(gens)[:i % 3]                  # alternated: every generator takes every place
                outs = {}
                ev[0].record()
                for j, name in enumerate(order):
                    outs[name] = call(name, i)
                    ev[j + 1].record()
                ev[-1].synchronize()
                for j, name in enumerate(order):
                    ms[name].append(ev[j].elapsed_time(ev[j + 1]))
                    steps[name].append(gens[name].model_calls_num - before[name])
                    if p == 0:
                        o = outs[name]
                        folded = tta.scoring.unique_samples(o, torch.zeros(o.shape[:2]), eos=EOS)
                        distinct[name].append(float(np.mean([len(f) for f in folded])))
        for name in gens:
            m = float(np.median(ms[name]))
            rec = {"tool": "bench_sbs", "case": f"{name}_K{K}", "sources": 32, "K": K, "max_len": a.max_len, "vocab": V,
                   "timed_batches": len(srcs), "passes": a.passes, "ms_per_call": round(m, 3),
                   "steps_per_call": round(float(np.median(steps[name])), 1),
                   "ms_per_step": round(float(np.median(np.array(ms[name]) / np.maximum(np.array(steps[name]), 1))), 4),
                   "distinct_candidates_per_source": round(float(np.mean(distinct[name])), 2)}
            rec["distinct_candidates_per_ms"] = round(32 * rec["distinct_candidates_per_source"] / m, 2)
            lines.append(rec)
        base = next(r for r in lines if r["case"] == f"beam_search_K{K}")
        for r in lines:
            if r["K"] == K:
                r["ms_per_call_over_beam_search"] = round(r["ms_per_call"] / base["ms_per_call"], 4)
                r["ms_per_step_over_beam_search"] = round(r["ms_per_step"] / base["ms_per_step"], 4)
    for beam, v in ((5, 256), (32, 1024)):
        lines.append(kernel_alone(native, beam, v))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec))
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
