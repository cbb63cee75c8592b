#!/usr/bin/env python3
"""What a per-source logit bias costs (not part of bench.py): the biased call beside the unbiased call of the same build, on
bench.py's 4+4 weights and USPTO-MIT-shaped synthetic sources (tools/synth.py), max_len 200, temperature 1, for

  plain     TranslationInferenceSampling.generate over batches of 32 sources,
  pool      TranslationInferenceSamplingSpeculative.generate_many over 1 024 sources ((n_drafts, draft_len) = (3, 10)),
  sbs       TranslationInferenceStochasticBeamSearch.generate, K = 5, over batches of 32 sources,

each under two biases: ``zero`` (an all-zero table: the tokens, and so the step counts, are the unbiased call's, which isolates the
extra launch per step and the table's copy per call) and ``allowlist`` (every source may emit its own tokens plus the structure
tokens and EOS: scoring.allowlist_from_source, the "product tokens come from the reactants" constraint; rows and step counts
differ from the unbiased call's, so the per-step figure is the comparable one).  The three variants of a generator are timed
alternately, pass by pass, with HIP events around the whole list; figures are medians over the passes after warm-up: ms per call
(a call: one batch; the whole list for the pool) and ms per decoder step.  Then the kernel alone (ttx_debug_logit_bias) at 10 000
rows for V = 256 and 1 024, plain mapping and step layout.  One JSON line per case, written to ``--out``.
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
SEED = 20260126


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
    ap.add_argument("--batches", type=int, default=8, help="batches of 32 sources for the per-batch generators")
    ap.add_argument("--warmup", type=int, default=2, help="untimed passes (a graph is captured the second time its key is seen)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r26_bench_logit_bias.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_logit_bias.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from translation_transformer_amd.scoring import allowlist_from_source, bias_from_allowed
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK, DOT, BRANCH, BOND, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.sources)
    small = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    keys = [torch.arange(32 * i, 32 * i + int(s.shape[0])) for i, s in enumerate(small)]
    always = [EOS, C_TOK, DOT, BRANCH, BOND]
    tables = {"none": [None] * len(small), "zero": [torch.zeros((int(s.shape[0]), V), device="cuda") for s in small],
              "allowlist": [bias_from_allowed(allowlist_from_source(s, always, V, PAD)) for s in small]}
    share = float(np.mean([float(torch.isfinite(b).float().mean()) for b in tables["allowlist"]]))
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def measure(name, make, run, n_calls, rows_per_call):
        """``run(generator, variant)`` decodes the list once; three generators (one per variant) so that counters stay apart."""
        gens = {v: make() for v in tables}
        ms, steps, outs = {v: [] for v in tables}, {}, {}
        for p in range(a.warmup + a.passes):
            for v, g in gens.items():
                before = g.model_calls_num
                t, out = timed(lambda: run(g, v))
                steps[v], outs[v] = g.model_calls_num - before, out
                if p >= a.warmup:
                    ms[v].append(t)
        rec = {"tool": "bench_logit_bias", "case": name, "max_len": a.max_len, "vocab": V, "calls": n_calls, "rows_per_call": rows_per_call,
               "passes": a.passes, "allowlist_share_of_vocab": round(share, 4)}
        for v in tables:
            med = float(np.median(ms[v]))
            rec[f"{v}_ms_per_call"] = round(med / n_calls, 4)
            rec[f"{v}_ms_per_step"] = round(med / max(1, steps[v]), 5)
            rec[f"{v}_steps"] = int(steps[v])
            rec[f"{v}_ms_spread"] = [round(min(ms[v]), 2), round(max(ms[v]), 2)]
        for v in ("zero", "allowlist"):
            rec[f"{v}_over_none_per_step"] = round(rec[f"{v}_ms_per_step"] / rec["none_ms_per_step"], 4)
            rec[f"{v}_over_none_per_call"] = round(rec[f"{v}_ms_per_call"] / rec["none_ms_per_call"], 4)
        rec["zero_rows_equal_to_none"] = bool(torch.equal(outs["zero"], outs["none"]))
        emit(rec)

    nb = min(a.batches, len(small))
    kw = dict(temperature=1.0, seed=SEED)
    measure("plain_bs32", lambda: tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, num_samples=1, **kw),
            lambda g, v: torch.cat([g.generate(s, row_keys=k, logit_bias=b) for s, k, b in zip(small[:nb], keys[:nb], tables[v][:nb])], 0), nb, 32)
    measure("pool_1024_N3_D10", lambda: tta.TranslationInferenceSamplingSpeculative(native, a.max_len, 10, 3, PAD, BOS, EOS, C_TOK, num_samples=1, **kw),
            lambda g, v: torch.cat(g.generate_many(small, row_keys=keys, logit_biases=None if v == "none" else tables[v]), 0), 1, a.sources)
    measure("sbs_bs32_K5", lambda: tta.TranslationInferenceStochasticBeamSearch(native, 5, a.max_len, PAD, BOS, EOS, **kw),
            lambda g, v: torch.cat([g.generate(s, row_keys=k, logit_bias=b) for s, k, b in zip(small[:nb], keys[:nb], tables[v][:nb])], 0), nb, 32)

    # the kernel alone: 10 000 logits rows, 32 sources; plain mapping (row -> source) and the step layout (N = 3, D = 10: 31 rows a slot)
    M = 10000
    for Vk in (256, 1024):
        logits = torch.randn((M, Vk), device="cuda")
        table = torch.where(torch.rand((32, Vk), device="cuda") < 0.5, torch.zeros((), device="cuda"), torch.full((), float("-inf"), device="cuda"))
        src_row = torch.randint(0, 32, (M,), dtype=torch.int32, device="cuda")
        slots = -(-M // 31)
        act, src_slot = torch.randperm(slots, device="cuda").to(torch.int32), torch.randint(0, 32, (slots,), dtype=torch.int32, device="cuda")
        for mapping, call in (("plain", lambda: native.debug_logit_bias(logits, table, src=src_row)),
                              ("step_N3_D10", lambda: native.debug_logit_bias(logits, table, src=src_slot, act_idx=act, n=3, d=10))):
            for _ in range(10):
                call()
            t, _ = timed(lambda: [call() for _ in range(a.kernel_reps)])
            us = 1e3 * t / a.kernel_reps
            emit({"tool": "bench_logit_bias", "case": f"kernel_{mapping}_V{Vk}", "rows": M, "vocab": Vk, "reps": a.kernel_reps,
                  "us_per_launch": round(us, 3), "GBs_logits_read_and_written": round(2 * M * Vk * 4 / (us * 1e-6) / 1e9, 1),
                  "note": "back-to-back launches on one stream, launch overhead included"})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
