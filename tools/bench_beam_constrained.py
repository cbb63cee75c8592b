#!/usr/bin/env python3
"""Cost of constrained beam search (TranslationInferenceBeamSearchConstrained, not part of bench.py) on bench.py's 4+4 weights and
USPTO-MIT-shaped synthetic batches (tools/synth.py), bs = 32, max_len 200, K = 5 and 10:

  per generate call and per decoder step, beside TranslationInferenceBeamSearch of the same build on the same sources, under
    zero_bias       an all-zero logit bias: the rows and the step counts are the plain generator's, so the difference is k_logit_bias
                    and k_beam_step_masked in k_beam_step's place
    neutral_syntax  an all-neutral syntax table under a max_len no row reaches: the same rows again, k_syntax_mask and the kernel
    source_tokens   the "tokens of the source" allow-list (scoring.allowlist_from_source with EOS): other rows, a second figure
  Where the plain generator fills a rank with a continuation of a finished hypothesis (a token other than PAD after the EOS, 35
  below its parent: the constrained class gives a finished hypothesis the PAD child alone), the rows of that source differ by design;
  the records count those sources and say whether every differing source is one of them.
  HIP events around each call, the generators alternated batch by batch (every one takes every place), warm-up first, medians
  over the batches and passes.

  k_beam_step_masked alone against k_beam_step alone on the same operands at (beam, V) = (5, 256) and (32, 1 024), 32 sources: one
  ttx_debug_* launch each (launch, kernel and the entry's stream synchronisation, the same for both) between two events, alternated,
  median of 5 rounds of 20 launches.

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
    import util_beam_checks as S
    c = S.step_case(B=B, beam=beam, K=beam, V=V, kind="random", width=3, ld=12, seed=1)         # finite logits, finished parents
    a = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in S.step_arrays(c).items()}
    shape = dict(V=V, ld=c.ld, width=c.width, B=B, beam=beam, K=beam, pad=c.pad, eos=c.eos)
    fns = {"k_beam_step_masked": lambda: native.debug_beam_step_masked(**shape, **a), "k_beam_step": lambda: native.debug_beam_step(**shape, **a)}
    for f in fns.values():
        for _ in range(5):
            f()
    times = {k: [] for k in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for name, f in fns.items():
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000.0 / launches)
    rec = {"tool": "bench_beam_constrained", "case": f"step_kernel_beam{beam}_V{V}", "sources": B,
           "us_per_launch_k_beam_step_masked": round(float(np.median(times["k_beam_step_masked"])), 2),
           "us_per_launch_k_beam_step": round(float(np.median(times["k_beam_step"])), 2)}
    rec["difference_us"] = round(rec["us_per_launch_k_beam_step_masked"] - rec["us_per_launch_k_beam_step"], 2)
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5, help="batches of 32 sources that are timed")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r29_bench_beam_constrained.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_beam_constrained.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.batches * 32)
    srcs = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    zero = torch.zeros(32, V, device="cuda")
    neutral = torch.zeros(V, dtype=torch.int8)
    allow = [tta.scoring.allowlist_from_source(s, [EOS], V, PAD) for s in srcs]

    lines = []
    for K in (5, 10):
        plain = tta.TranslationInferenceBeamSearch(native, K, a.max_len, PAD, BOS, EOS)
        con = {k: tta.TranslationInferenceBeamSearchConstrained(native, K, a.max_len, PAD, BOS, EOS)
               for k in ("zero_bias", "neutral_syntax", "source_tokens")}
        gens = dict(con, beam_search=plain)
        calls = {"beam_search": lambda i: plain.generate(srcs[i]),
                 "zero_bias": lambda i: con["zero_bias"].generate(srcs[i], logit_bias=zero[:srcs[i].shape[0]]),
                 "neutral_syntax": lambda i: con["neutral_syntax"].generate(srcs[i], syntax=neutral),
                 "source_tokens": lambda i: con["source_tokens"].generate(srcs[i], allowed=allow[i])}
        names = list(calls)
        same = {k: True for k in ("zero_bias", "neutral_syntax")}
        differ, goes_on, explained = {k: 0 for k in same}, 0, {k: True for k in same}
        reached = False                   # a row in the last column: there the neutral table binds and the rows may differ
        for _ in range(a.warmup):
            for i in range(len(srcs)):
                outs = {name: calls[name](i) for name in names}
                ref = outs["beam_search"]
                after = (ref[:, :, :-1] == EOS).cumsum(-1) > 0                    # columns after a row's first EOS
                on = ((ref[:, :, 1:] != PAD) & after).any(-1).any(-1)             # sources with a row that goes on after its EOS
                goes_on += int(on.sum())
                for k in same:
                    w = max(outs[k].shape[-1], ref.shape[-1])                     # the batch's width follows its longest live row
                    x, y = (torch.nn.functional.pad(t, (0, w - t.shape[-1]), value=PAD) for t in (outs[k], ref))
                    d = (x != y).any(-1).any(-1)
                    same[k] &= not bool(d.any())
                    differ[k] += int(d.sum())
                    explained[k] &= bool((on | ~d).all())
                reached |= outs["beam_search"].shape[-1] >= a.max_len
        torch.cuda.synchronize()
        ms, steps = ({k: [] for k in names} for _ in range(2))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        for p in range(a.passes):
            for i in range(len(srcs)):
                before = {k: g.model_calls_num for k, g in gens.items()}
                order = names[i % len(names):] + names[:i % len(names)]            # alternated: every generator takes every place
                ev[0].record()
                for j, name in enumerate(order):
                    calls[name](i)
                    ev[j + 1].record()
                ev[-1].synchronize()
                for j, name in enumerate(order):
                    ms[name].append(ev[j].elapsed_time(ev[j + 1]))
                    steps[name].append(gens[name].model_calls_num - before[name])
        for name in names:
            m = float(np.median(ms[name]))
            rec = {"tool": "bench_beam_constrained", "case": f"{name}_K{K}", "sources": 32, "K": K, "max_len": a.max_len, "vocab": V,
                   "timed_batches": len(srcs), "passes": a.passes, "ms_per_call": round(m, 3),
                   "steps_per_call": round(float(np.median(steps[name])), 1),
                   "ms_per_step": round(float(np.median(np.array(ms[name]) / np.maximum(np.array(steps[name]), 1))), 4)}
            if name in same:
                rec["rows_equal_beam_search"] = same[name]
                rec["a_row_reaches_max_len"] = bool(reached)
                rec["sources_that_differ"] = differ[name]
                rec["sources_where_beam_search_goes_on_after_eos"] = goes_on
                rec["every_differing_source_is_one_of_them"] = explained[name]
            lines.append(rec)
        base = next(r for r in lines if r["case"] == f"beam_search_K{K}")
        for r in lines:
            if r.get("K") == K:
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
