#!/usr/bin/env python3
"""Cost of scoring hypotheses under the sampling distribution (NativeTransformer.proposal_scores, not part of bench.py) on
bench.py's 4+4 weights and USPTO-MIT-shaped synthetic batches (tools/synth.py):

  a  bs = 32, N = 1: the greedy-speculative outputs at max_len 200;
  b  bs = 4, n_best = 5: the beam-speculative outputs (bench.py's c3 generator settings);

each at three settings: unfiltered T = 0.5; top_k = 8; top_k = 32 with top_p = 0.9975.  Per case: ms per call of
``proposal_scores`` (median over the batches and passes, HIP events around each call), of ``proposal_scores(with_scores=True)``,
of the two separate calls it replaces (``score_hypotheses`` then ``proposal_scores``) and of ``score_hypotheses`` on the same
inputs — existing code of the same build in the same run, timed alternately: the yardstick — and the overhead over it.

The kernel alone (ttx_hypothesis_logq beside ttx_hypothesis_logprobs on the same logits, timed alternately) at R = 160, T = 200
with every position live (32 000 positions), V = 256 and V = 1 024, the same three settings.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SETTINGS = {"T0.5": dict(temperature=0.5), "k8": dict(top_k=8), "k32_p0.9975": dict(top_k=32, top_p=0.9975)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16, help="batches of case a / b that are timed")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_logq.py measures on an MI355X; there is no CPU figure"
    import bench
    import translation_transformer_amd as tta
    from tools.bench_score import median_ms
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK, V
    native = tta.NativeTransformer(bench.get_weights(bench.TRAIN_STEPS, "cuda"), 8, PAD, device=0)
    c3 = bench.BEAM_CONFIGS["c3"]
    src_rows, _ = SynthReactions(123456, "mit").dataset(a.batches * 32)
    src32 = [torch.from_numpy(b).cuda() for b in batches(src_rows, 32)]
    src4 = [torch.from_numpy(b).cuda() for b in batches(src_rows[:a.batches * c3["bs"]], c3["bs"])]
    greedy = tta.TranslationInferenceGreedySpeculative(native, 200, 10, 3, PAD, BOS, EOS, C_TOK)
    beam = tta.TranslationInferenceBeamSearchSpeculative(native, 200, c3["n_best"], 10, c3["N"], V, False, PAD, BOS, EOS, C_TOK,
                                                         max_steps=800)
    rec = {"tool": "bench_logq", "timed_batches": a.batches, "passes": a.passes, "vocab": V}
    for name, gen, srcs in (("a", greedy, src32), ("b", beam, src4)):
        cases = []
        for s in srcs:                              # a batch on which the reference raises has no hypotheses
            try:
                cases.append((s, gen.generate(s)))
            except (tta.ReferenceError_, RuntimeError):
                pass
        fns = {"score_hypotheses": lambda c: native.score_hypotheses(c[0], c[1], eos_token_idx=EOS)}
        for tag, d in SETTINGS.items():
            fns[f"proposal_scores_{tag}"] = lambda c, d=d: native.proposal_scores(c[0], c[1], eos_token_idx=EOS, **d)
            fns[f"proposal_scores_with_scores_{tag}"] = lambda c, d=d: native.proposal_scores(c[0], c[1], eos_token_idx=EOS,
                                                                                              with_scores=True, **d)
            fns[f"two_calls_{tag}"] = lambda c, d=d: (native.score_hypotheses(c[0], c[1], eos_token_idx=EOS, return_token_logp=True),
                                                      native.proposal_scores(c[0], c[1], eos_token_idx=EOS, **d))
        ms = median_ms(fns, cases, a.warmup, a.passes)
        rec[name] = {"shape": list(cases[0][1].shape), "ms": ms,
                     "over_score_hypotheses": {n: round(v / ms["score_hypotheses"], 4) for n, v in ms.items() if n != "score_hypotheses"}}

    # the kernel alone, every position live
    R, T = 160, 200
    gen = torch.Generator(device="cuda").manual_seed(7)
    rec["stage"] = {"rows": R, "positions_per_row": T}
    for vocab in (256, 1024):
        logits = torch.randn((R, T, vocab), generator=gen, device="cuda") * 3.0
        hyp = torch.randint(3, vocab, (R, T + 1), generator=gen, device="cuda")
        # the C entry points on preallocated outputs: no allocation and no token check on the clock
        lib, sess, stream = native._lib, native._scoring_session(), native._stream()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")       # noqa: E731
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")         # noqa: E731
        tok, score, length, fin = f32(R, T), f32(R), i32(R), torch.empty(R, dtype=torch.uint8, device="cuda")
        first, rank, kept = i32(R), i32(R, T), i32(R, T)
        fns = {"hypothesis_logprobs": lambda c: tta._native.check(lib.ttx_hypothesis_logprobs(
            sess, c[0].data_ptr(), c[1].data_ptr(), R, T + 1, vocab, PAD, EOS, tok.data_ptr(), score.data_ptr(), length.data_ptr(),
            fin.data_ptr(), stream))}
        for tag, d in SETTINGS.items():
            dist = tta._native.Dist(d.get("temperature", 1.0), d.get("top_k", 0), d.get("top_p", 1.0))
            for with_rank in (False, True):
                fns[f"hypothesis_logq_{tag}" + ("_rank" if with_rank else "")] = lambda c, dist=dist, wr=with_rank: tta._native.check(
                    lib.ttx_hypothesis_logq(sess, c[0].data_ptr(), c[1].data_ptr(), R, T + 1, vocab, PAD, EOS, C.byref(dist), None,
                                            tok.data_ptr(), score.data_ptr(), first.data_ptr(), rank.data_ptr() if wr else None,
                                            kept.data_ptr() if wr else None, length.data_ptr(), fin.data_ptr(), stream))
        ms = median_ms(fns, [(logits, hyp)], a.warmup, 4 * a.passes)
        rec["stage"][f"V{vocab}"] = {"ms": ms, "over_hypothesis_logprobs": {n: round(v / ms["hypothesis_logprobs"], 3)
                                                                             for n, v in ms.items() if n != "hypothesis_logprobs"}}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
