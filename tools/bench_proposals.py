#!/usr/bin/env python3
"""What caller-supplied proposal drafts buy and cost (not part of bench.py) on bench.py's 4+4 weights and the 1 024
USPTO-MIT-shaped synthetic sources and settings of tools/bench_prefix.py: max_len 200, filters off, batches of 32 sources through
TranslationInferenceSamplingSpeculative.generate_many, (n_drafts, draft_len) = (1, 4) and (3, 10).

  edits    temperature 1, num_samples 1.  The unproposed pool against the pool proposed with: the call's own output (perfect); that
           output with one substitution, one insertion, one deletion in the middle of every row, each at CTX 2, 4 and 8
           (TTX_PROPOSAL_CTX); random tokens of the same lengths (what giving up source draft 0 costs).
  cascade  num_samples 8 at temperature 0.5 and 1, proposed with the source's own temperature-0 output; the pool call that produces
           that output (temperature 0, num_samples 1) is timed too, so the figure is given with and without its cost.

All runs of a case are timed alternately, pass by pass, with HIP events around the whole list; per case one JSON line with the median
and the spread (min, max) of the passes after warm-up, the pool's device steps and accepted draft tokens per run, and whether every
proposed run returned the unproposed run's rows, with the number of rows that differ and, for the edits, the number that differ from
the plain sampler's rows (the speculative sampler's one caveat: a uniform within fp32 rounding of a CDF boundary).
"""
from __future__ import annotations

import argparse
import json
import os
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


def row_tokens(row, pad, eos) -> list:
    out = []
    for t in row[1:]:
        if t == pad:
            break
        out.append(int(t))
        if t == eos:
            break
    return out


def edited(t: list, kind: str, other: int) -> list:
    t = list(t)
    at = len(t) // 2
    if not t:
        return t
    if kind == "sub":
        t[at] = other
    elif kind == "ins":
        t.insert(at, other)
    elif kind == "del":
        del t[at]
    return t


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2, help="untimed passes (a graph is captured the second time its key is seen)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r22_bench_proposals.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_proposals.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.sources)
    small = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    k32 = [torch.arange(32 * i, min(32 * (i + 1), a.sources)) for i in range(-(-a.sources // 32))]
    rng = np.random.default_rng(SEED)

    def table(rows: list) -> list:
        """Per batch of 32 a right-padded Long matrix of the sources' proposals."""
        rows = [r[:a.max_len - 1] for r in rows]
        width = max(1, max(len(r) for r in rows))
        m = torch.full((a.sources, width), PAD, dtype=torch.int64)
        for i, r in enumerate(rows):
            m[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
        return [m[32 * i:32 * (i + 1)] for i in range(-(-a.sources // 32))]

    def spec(N, D, **kw):
        return tta.TranslationInferenceSamplingSpeculative(native, a.max_len, D, N, PAD, BOS, EOS, C_TOK, seed=SEED, **kw)

    def measure(runs: dict) -> tuple:
        """runs: name -> (generator, proposals or None, CTX or None).  Alternating passes; (ms, steps, accepted, outputs) by name."""
        ms = {k: [] for k in runs}
        steps, accepted, outs = {}, {}, {}
        for p in range(a.warmup + a.passes):
            for name, (g, props, ctx) in runs.items():
                if ctx is None:
                    os.environ.pop("TTX_PROPOSAL_CTX", None)
                else:
                    os.environ["TTX_PROPOSAL_CTX"] = str(ctx)
                before = (g.model_calls_num, g.accepted_tokens_num)
                t, out = timed(lambda: g.generate_many(small, row_keys=k32, proposals=props))
                outs[name] = torch.cat(out, 0)
                if p >= a.warmup:
                    ms[name].append(t)
                steps[name], accepted[name] = g.model_calls_num - before[0], g.accepted_tokens_num - before[1]
        os.environ.pop("TTX_PROPOSAL_CTX", None)
        return ms, steps, accepted, outs

    def record(case: str, N, D, n, T, runs, ms, steps, accepted, outs, base: str, same_as_base) -> dict:
        rec = {"tool": "bench_proposals", "case": case, "n": n, "n_drafts": N, "draft_len": D, "sources": a.sources, "rows": a.sources * n,
               "max_len": a.max_len, "vocab": V, "temperature": T, "passes": a.passes, "warmup": a.warmup}
        for name in runs:
            med = float(np.median(ms[name]))
            rec[f"{name}_ms"] = round(med, 2)
            rec[f"{name}_ms_spread"] = [round(min(ms[name]), 2), round(max(ms[name]), 2)]
            rec[f"{name}_device_steps"], rec[f"{name}_accepted_tokens"] = steps[name], accepted[name]
            if name != base:
                rec[f"{name}_over_{base}"] = round(med / float(np.median(ms[base])), 4)
        rec["rows_equal_unproposed"] = bool(all(torch.equal(outs[k], outs[base]) for k in same_as_base))
        for k in same_as_base:                         # rows (of sources * n) in which a run and the unproposed run differ somewhere
            if k != base:
                rec[f"{k}_rows_differing"] = int((outs[k] != outs[base]).any(-1).sum())
        return rec

    lines = []
    for N, D in DRAFTS:
        # -- edits: temperature 1, one sample ------------------------------------------------------------------------------------
        g = spec(N, D, temperature=1.0, num_samples=1)
        own = torch.cat(g.generate_many(small, row_keys=k32), 0)[:, 0].cpu().numpy()
        toks = [row_tokens(r, PAD, EOS) for r in own]
        runs = {"unproposed": (g, None, None), "perfect": (g, table(toks), None),
                "random": (g, table([[int(x) for x in rng.integers(3, V, size=len(t))] for t in toks]), None)}
        for kind in ("sub", "ins", "del"):
            props = table([edited(t, kind, int(rng.integers(3, V))) for t in toks])
            for ctx in (2, 4, 8):
                runs[f"{kind}_ctx{ctx}"] = (g, props, ctx)
        ms, steps, accepted, outs = measure(runs)
        rec = record(f"edits_N{N}_D{D}", N, D, 1, 1.0, runs, ms, steps, accepted, outs, "unproposed", [k for k in runs])
        rec["emitted_tokens_per_row"] = round(float(np.mean([len(t) for t in toks])), 2)
        # the plain sampler's rows: where a run departs from the unproposed one, which of the two departs from these
        plain = tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, temperature=1.0, num_samples=1, seed=SEED)
        ref = torch.cat([plain.generate(s, row_keys=k) for s, k in zip(small, k32)], 0)
        for k in runs:
            rec[f"{k}_rows_differing_from_plain_sampler"] = int((outs[k] != ref).any(-1).sum())
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        # -- cascade: the temperature-0 output as the proposal of eight samples ------------------------------------------------------
        g0 = spec(N, D, temperature=0.0, num_samples=1)
        greedy = torch.cat(g0.generate_many(small, row_keys=k32), 0)[:, 0].cpu().numpy()
        props = table([row_tokens(r, PAD, EOS) for r in greedy])
        for T in (0.5, 1.0):
            g8 = spec(N, D, temperature=T, num_samples=8)
            runs = {"unproposed": (g8, None, None), "proposed": (g8, props, None), "greedy_n1": (g0, None, None)}
            ms, steps, accepted, outs = measure(runs)
            rec = record(f"cascade_T{T}_N{N}_D{D}", N, D, 8, T, runs, ms, steps, accepted, outs, "unproposed", ["proposed"])
            both = float(np.median(ms["proposed"])) + float(np.median(ms["greedy_n1"]))
            rec["proposed_plus_greedy_ms"] = round(both, 2)
            rec["proposed_plus_greedy_over_unproposed"] = round(both / float(np.median(ms["unproposed"])), 4)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
