#!/usr/bin/env python3
"""What the syntax constraint costs and what it buys (not part of bench.py): the constrained call beside the unconstrained call of the
same build, on bench.py's 4+4 weights and USPTO-MIT-shaped synthetic sources (tools/synth.py), max_len 200, temperature 1, for

  plain     TranslationInferenceSampling.generate over batches of 32 sources,
  pool      TranslationInferenceSamplingSpeculative.generate_many over 1 024 sources ((n_drafts, draft_len) = (3, 10)),

each under two tables: ``neutral`` (every class 0: a row that ends before the last column is the unconstrained call's, token for
token, which isolates the extra launch per step and the table's copy per call) and ``smiles`` (the table of tools/synth.py's token
strings: "(" opens, ")" closes, the digits and %10 .. %63 are ring labels, PAD / BOS / "?" and the labels above 63 are forbidden;
rows and step counts differ from the unconstrained call's, so the per-step figure is the comparable one).  The three variants of a
generator are timed alternately, pass by pass, with HIP events around the whole list; figures are medians over the passes after
warm-up: ms per call (a call: one batch; the whole list for the pool) and ms per decoder step.  Then the kernel alone
(ttx_debug_syntax_mask) at 10 000 rows for V = 256 and 1 024, plain mapping and step layout, over committed prefixes of 60 tokens.
Then the share of rows that are finished and balanced (SmilesSyntax.check) with and without the ``smiles`` table at temperature 0.5,
1 and 2.  One JSON line per case, written to ``--out``.
"""
from __future__ import annotations

import argparse
import json
import re
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SEED = 20260127


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def synth_table(vocab: dict, V: int) -> torch.Tensor:
    """The int8 classes of tools/synth.py's vocabulary: ring numbers 0 .. 63 are labels, the %nn above them are forbidden (the rule
    tracks 64 labels, and a label it does not track could not be held to an even count)."""
    cls = np.zeros(V, dtype=np.int8)
    for tok, i in vocab.items():
        m = re.match(r"^(?:([0-9])|%([0-9]{2}))$", tok)
        if tok in ("<PAD>", "<BOS>", "?"):
            cls[i] = -1
        elif tok == "(":
            cls[i] = 1
        elif tok == ")":
            cls[i] = 2
        elif m:
            n = int(m.group(1) if m.group(1) is not None else m.group(2))
            cls[i] = 3 + n if n < 64 else -1
    return torch.from_numpy(cls)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=1024, help="sources of the pool's list")
    ap.add_argument("--batches", type=int, default=8, help="batches of 32 sources for the per-batch generator")
    ap.add_argument("--warmup", type=int, default=2, help="untimed passes (a graph is captured the second time its key is seen)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r27_bench_syntax.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_syntax.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.synth import SynthReactions, batches, smiles_vocabulary, PAD, BOS, EOS, C_TOK, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.sources)
    small = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    keys = [torch.arange(32 * i, 32 * i + int(s.shape[0])) for i, s in enumerate(small)]
    smiles = tta.SmilesSyntax(synth_table(smiles_vocabulary(), V))
    tables = {"none": None, "neutral": tta.SmilesSyntax(torch.zeros(V, dtype=torch.int8)), "smiles": smiles}
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def measure(name, make, run, n_calls, rows_per_call):
        """``run(generator, table)`` decodes the list once; three generators (one per variant) so that counters stay apart."""
        gens = {v: make() for v in tables}
        ms, steps, outs = {v: [] for v in tables}, {}, {}
        for p in range(a.warmup + a.passes):
            for v, g in gens.items():
                before = g.model_calls_num
                t, out = timed(lambda: run(g, tables[v]))
                steps[v], outs[v] = g.model_calls_num - before, out
                if p >= a.warmup:
                    ms[v].append(t)
        rec = {"tool": "bench_syntax", "case": name, "max_len": a.max_len, "vocab": V, "calls": n_calls, "rows_per_call": rows_per_call,
               "passes": a.passes}
        for v in tables:
            med = float(np.median(ms[v]))
            rec[f"{v}_ms_per_call"] = round(med / n_calls, 4)
            rec[f"{v}_ms_per_step"] = round(med / max(1, steps[v]), 5)
            rec[f"{v}_steps"] = int(steps[v])
            rec[f"{v}_ms_spread"] = [round(min(ms[v]), 2), round(max(ms[v]), 2)]
        for v in ("neutral", "smiles"):
            rec[f"{v}_over_none_per_step"] = round(rec[f"{v}_ms_per_step"] / rec["none_ms_per_step"], 4)
            rec[f"{v}_over_none_per_call"] = round(rec[f"{v}_ms_per_call"] / rec["none_ms_per_call"], 4)
        same = (outs["neutral"] == outs["none"]).all(-1)
        rec["neutral_rows_equal_to_none"] = f"{int(same.sum())} of {same.numel()}"
        rec["none_rows_that_reach_the_last_column"] = int(((outs["none"][..., -1] != PAD)).sum())
        emit(rec)

    nb = min(a.batches, len(small))
    kw = dict(temperature=1.0, seed=SEED)
    measure("plain_bs32", lambda: tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, num_samples=1, **kw),
            lambda g, t: torch.cat([g.generate(s, row_keys=k, syntax=t) for s, k in zip(small[:nb], keys[:nb])], 0), nb, 32)
    measure("pool_1024_N3_D10", lambda: tta.TranslationInferenceSamplingSpeculative(native, a.max_len, 10, 3, PAD, BOS, EOS, C_TOK, num_samples=1, **kw),
            lambda g, t: torch.cat(g.generate_many(small, row_keys=keys, syntax=t), 0), 1, a.sources)

    # the kernel alone: 10 000 logits rows over committed prefixes of 60 tokens; plain mapping and the step layout (N = 3, D = 10)
    M, F = 10000, 60
    for Vk in (256, 1024):
        logits = torch.randn((M, Vk), device="cuda")
        cls = torch.zeros(Vk, dtype=torch.int8)
        cls[:4], cls[6], cls[7] = torch.tensor([-1, -1, 0, -1], dtype=torch.int8), 1, 2
        cls[8:72] = torch.arange(3, 67, dtype=torch.int8)
        cls = cls.cuda()
        slots = -(-M // 31)
        gen = torch.randint(4, Vk, (M, F + 14), dtype=torch.int32, device="cuda")
        front1 = torch.full((1,), F, dtype=torch.int32, device="cuda")
        front = torch.full((slots,), F, dtype=torch.int32, device="cuda")
        act = torch.randperm(slots, device="cuda").to(torch.int32)
        drafts = torch.randint(4, Vk, (slots, 3, 10), dtype=torch.int32, device="cuda")
        for mapping, call in (("plain", lambda: native.debug_syntax_mask(logits, cls, 200, EOS, gen, front=front1)),
                              ("step_N3_D10", lambda: native.debug_syntax_mask(logits, cls, 200, EOS, gen, front=front, act_idx=act, drafts=drafts,
                                                                               n=3, d=10))):
            for _ in range(10):
                call()
            t, _ = timed(lambda: [call() for _ in range(a.kernel_reps)])
            us = 1e3 * t / a.kernel_reps
            emit({"tool": "bench_syntax", "case": f"kernel_{mapping}_V{Vk}", "rows": M, "vocab": Vk, "prefix_tokens": F, "reps": a.kernel_reps,
                  "us_per_launch": round(us, 3), "masked_share_of_logits": round(float(torch.isinf(logits).float().mean()), 4),
                  "note": "back-to-back launches on one stream, launch overhead included; the logits are only written where masked"})

    # what it buys: finished-and-balanced rows with and without the table
    for temp in (0.5, 1.0, 2.0):
        rec = {"tool": "bench_syntax", "case": f"balanced_share_T{temp}", "max_len": a.max_len, "rows": 32 * nb}
        for v in ("none", "smiles"):
            g = tta.TranslationInferenceSampling(native, a.max_len, PAD, BOS, EOS, num_samples=1, temperature=temp, seed=SEED)
            out = torch.cat([g.generate(s, row_keys=k, syntax=tables[v]) for s, k in zip(small[:nb], keys[:nb])], 0)
            rep = smiles.check(out, EOS)
            ok = rep.balanced & rep.finished & (rep.first_offending == -1)
            rec[f"{v}_finished_and_balanced"] = round(float(ok.mean()), 4)
            rec[f"{v}_finished"] = round(float(rep.finished.mean()), 4)
        emit(rec)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec), file=f)


if __name__ == "__main__":
    main()
