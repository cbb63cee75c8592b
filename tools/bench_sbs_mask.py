#!/usr/bin/env python3
"""Cost of stochastic beam search under a top-k / top-p filter and under forced prefixes (not part of bench.py), written after
tools/bench_sbs.py: bench.py's 4+4 weights, USPTO-MIT-shaped synthetic batches (tools/synth.py), bs = 32, max_len 200, temperature
1, K = 5 and 10.

  per generate call and per decoder step: the unfiltered search (k_sbs_step), the filtered search with top_k = 32 and
  top_p = 0.9975 / 0.9 (k_sbs_step_masked), and a prompted call whose prefix is the first half of each source's greedy output
  (k_sbs_step_masked at every step, forced or free).  HIP events around each call, the generators alternated batch by batch, one
  warm-up pass, medians over 5 batches.  Steps per call are given: the filter shortens the rows.

  --unfiltered-only measures the unfiltered search alone, in a process of its own; with --tree DIR the package is imported from
  another checkout, so the parent commit's ttx_sbs_generate is measured by the same code (processes alternated by the caller).

  k_sbs_step_masked alone against k_sbs_step alone at (beam, V) = (5, 256) and (32, 1 024), 32 sources, top_k = 32 and
  top_p = 0.9: one ttx_debug_* launch each (launch, kernel and the entry's stream synchronisation, the same for all) between two
  events, alternated, median of 5 rounds of 20 launches; the masked kernel with production's waves per source and with 4.

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
    ops = dict(logits=dev(c.logits), slot_of=dev(c.slot_of), finished=dev(c.finished.astype(np.uint8)), gen=dev(c.gen),
               new_cand=torch.zeros((n, c.ld), dtype=torch.int64, device="cuda"), parent=torch.zeros(n, dtype=torch.int32, device="cuda"),
               new_len=torch.zeros(n, dtype=torch.int32, device="cuda"), new_finished=torch.zeros(n, dtype=torch.uint8, device="cuda"),
               parent_draft=torch.zeros(n, dtype=torch.int32, device="cuda"), summary=torch.zeros(5, dtype=torch.int32, device="cuda"),
               phi=dev(c.phi), g=dev(c.G), key=dev(c.keys), new_phi=torch.zeros(n, device="cuda"), new_g=torch.zeros(n, device="cuda"))
    shape = dict(V=V, ld=c.ld, width=c.width, B=B, beam=beam, K=beam, pad=c.pad, eos=c.eos, pos=c.pos, seed=c.seed, inv_T=1.0)
    runs = {"k_sbs_step": lambda: native.debug_sbs_step(**shape, **ops),
            "k_sbs_step_masked": lambda: native.debug_sbs_step_ex(**shape, top_k=32, top_p=0.9, **ops),
            "k_sbs_step_masked_4_waves": lambda: native.debug_sbs_step_ex(**shape, top_k=32, top_p=0.9, waves=4, **ops),
            "k_sbs_step_masked_filter_off": lambda: native.debug_sbs_step_ex(**shape, **ops)}
    for f in runs.values():
        for _ in range(5):
            f()
    times = {k: [] for k in runs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for name, f in runs.items():
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000.0 / launches)
    rec = {"tool": "bench_sbs_mask", "case": f"step_kernel_beam{beam}_V{V}", "sources": B, "top_k": 32, "top_p": 0.9}
    for name in runs:
        rec[f"us_per_launch_{name}"] = round(float(np.median(times[name])), 2)
    rec["masked_minus_plain_us"] = round(rec["us_per_launch_k_sbs_step_masked"] - rec["us_per_launch_k_sbs_step"], 2)
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5, help="batches of 32 sources that are timed")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--unfiltered-only", action="store_true")
    ap.add_argument("--tree", default=None, help="with --unfiltered-only: import the package from this checkout (a parent commit's build)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r23_bench_sbs_mask.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_sbs_mask.py measures on an MI355X; there is no CPU figure"
    if a.tree:
        assert a.unfiltered_only, "--tree measures another build's unfiltered search only"
        sys.path[:2] = [str(Path(a.tree).resolve()), str(Path(a.tree).resolve() / "tests")]
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.batches * 32)
    srcs = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    keys = [torch.arange(32 * i, 32 * (i + 1)) for i in range(len(srcs))]
    # the prefixes: the first half of every source's greedy output (BOS and EOS excluded), right-padded
    greedy = tta.TranslationInferenceGreedy(native, a.max_len, PAD, BOS, EOS)
    prefixes = []
    for s in srcs:
        rows = greedy.generate(s)[:, 0].cpu().numpy()
        halves = []
        for r in rows:
            body = r[1:]
            stop = np.nonzero((body == EOS) | (body == PAD))[0]
            body = body[:int(stop[0])] if len(stop) else body
            halves.append(body[:len(body) // 2])
        w = max(1, max(len(h) for h in halves))
        p = np.full((len(halves), w), PAD, dtype=np.int64)
        for i, h in enumerate(halves):
            p[i, :len(h)] = h
        prefixes.append(torch.from_numpy(p))

    lines = []
    for K in (5, 10):
        def make(**kw):
            return tta.TranslationInferenceStochasticBeamSearch(native, K, a.max_len, PAD, BOS, EOS, temperature=1.0, seed=20260104, **kw)
        gens = {"unfiltered": make()}
        if not a.unfiltered_only:
            gens.update({"top_k32_top_p0.9975": make(top_k=32, top_p=0.9975), "top_k32_top_p0.9": make(top_k=32, top_p=0.9),
                         "prompted_half_greedy": make()})

        def call(name, i):
            more = {"prefix": prefixes[i]} if name.startswith("prompted") else {}
            return gens[name].generate(srcs[i], row_keys=keys[i], **more)
        for _ in range(a.warmup):
            for i in range(len(srcs)):
                for name in gens:
                    call(name, i)
        torch.cuda.synchronize()
        ms, steps = ({k: [] for k in gens} for _ in range(2))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(gens) + 1)]
        names = list(gens)
        for i in range(len(srcs)):
            before = {k: g.model_calls_num for k, g in gens.items()}
            order = names[i % len(names):] + names[:i % len(names)]            # alternated: every generator takes every place
            ev[0].record()
            for j, name in enumerate(order):
                call(name, i)
                ev[j + 1].record()
            ev[-1].synchronize()
            for j, name in enumerate(order):
                ms[name].append(ev[j].elapsed_time(ev[j + 1]))
                steps[name].append(gens[name].model_calls_num - before[name])
        for name in gens:
            m = float(np.median(ms[name]))
            rec = {"tool": "bench_sbs_mask", "case": f"{name}_K{K}", "sources": 32, "K": K, "max_len": a.max_len, "vocab": V,
                   "timed_batches": len(srcs), "ms_per_call": round(m, 3), "steps_per_call": round(float(np.median(steps[name])), 1),
                   "ms_per_step": round(float(np.median(np.array(ms[name]) / np.maximum(np.array(steps[name]), 1))), 4)}
            if name.startswith("prompted"):
                rec["prefix_tokens_per_source"] = round(float(np.mean([(p != PAD).sum(1).float().mean().item() for p in prefixes])), 1)
            lines.append(rec)
        base = next(r for r in lines if r["case"] == f"unfiltered_K{K}")
        for r in lines:
            if r["K"] == K:
                r["ms_per_call_over_unfiltered"] = round(r["ms_per_call"] / base["ms_per_call"], 4)
                r["ms_per_step_over_unfiltered"] = round(r["ms_per_step"] / base["ms_per_step"], 4)
    if not a.unfiltered_only:
        for beam, v in ((5, 256), (32, 1024)):
            lines.append(kernel_alone(native, beam, v))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec))
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
