#!/usr/bin/env python3
"""Generate tests/golden/hyp_scores.npz: log-likelihood scores of hypotheses under the REFERENCE model (the tiny 2+2 model of
tiny_weights.npz), by the definition of include/ttx.h (ttx_score_hypotheses).

Runs ONLY in the build container, where the reference is mounted read-only: like make_golden.py it imports the reference's
modules (stub parent packages, so no Lightning-importing __init__ runs) and stores nothing but inputs and results.

  beam__*     the 10 fixture sources; hyp = the reference's own standard beam search (beam 5, max_len 150) -> [10, 5, W]
  targets__*  the 10 fixture pairs; hyp = the fixture targets as an N = 1 case -> [10, 1, Lt]
  rule__*     hand-made rows for the length rule: EOS at column 1, no EOS with trailing PAD, no EOS filling the row, all-PAD,
              a PAD before the EOS, two EOS -> [3, 2, 12]
Each case stores src, hyp, tok_logp (float64 log_softmax of the reference's fp32 logits VanillaTransformer.forward(src[b],
hyp[b, k, :-1]), gathered at hyp[b, k, 1:], zero past the length), score (their float64 sum), length, finished; the beam case
also min_gap [10]: the smallest difference between consecutive scores of each source (what an ordering test may rely on).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_scores.py
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF_SRC = Path("/root/reference") / "src"

sys.dont_write_bytecode = True
sys.path.insert(0, str(REF_SRC))
for _name in ("model", "utils", "decoding"):
    _m = types.ModuleType(_name)
    _m.__path__ = [str(REF_SRC / _name)]
    sys.modules[_name] = _m

from model.modules import VanillaTransformer  # noqa: E402
from decoding.standard_decoding import TranslationInferenceBeamSearch  # noqa: E402

PAD, BOS, EOS = 0, 1, 2


def length_rule(row: np.ndarray) -> tuple:
    """(n, finished) of one hypothesis row: the first EOS at a column >= 1, else the last non-PAD column >= 1, else 0."""
    for t in range(1, len(row)):
        if row[t] == EOS:
            return t, True
    for t in range(len(row) - 1, 0, -1):
        if row[t] != PAD:
            return t, False
    return 0, False


def score_case(m, src: torch.Tensor, hyp: torch.Tensor) -> dict:
    B, N, W = hyp.shape
    rows = hyp.reshape(B * N, W)
    with torch.inference_mode():
        logits = m(src.repeat_interleave(N, dim=0), rows[:, :-1])                 # fp32 [B*N, W-1, V]
    logp = torch.log_softmax(logits.double(), dim=-1).numpy()
    tok = np.zeros((B * N, W - 1), np.float64)
    length = np.zeros(B * N, np.int32)
    fin = np.zeros(B * N, bool)
    for r, row in enumerate(rows.numpy()):
        n, f = length_rule(row)
        length[r], fin[r] = n, f
        for t in range(1, n + 1):
            tok[r, t - 1] = logp[r, t - 1, row[t]]
    assert np.isfinite(tok).all()
    return dict(src=src.numpy(), hyp=hyp.numpy(), tok_logp=tok.reshape(B, N, W - 1), score=tok.sum(1).reshape(B, N),
                length=length.reshape(B, N), finished=fin.reshape(B, N))


def main() -> None:
    torch.set_num_threads(8)
    z = np.load(HERE / "fixture_tokens.npz")
    src, tgt, V = torch.from_numpy(z["src"]), torch.from_numpy(z["tgt"]), int(z["vocab_size"])
    m = VanillaTransformer(V, V, 2, 2, 64, 2, 128, 0.0, "relu", True, PAD, PAD)
    w = np.load(HERE / "tiny_weights.npz")
    m.load_state_dict({k: torch.from_numpy(w[k]) for k in w.files})
    m.eval()
    cases = {}
    with torch.inference_mode():
        beam = TranslationInferenceBeamSearch(m, 5, 150, PAD, BOS, EOS).generate(src)
    cases["beam"] = score_case(m, src, beam.long())
    sc = cases["beam"]["score"]
    cases["beam"]["min_gap"] = (sc[:, :-1] - sc[:, 1:]).min(axis=1)
    cases["targets"] = score_case(m, src, tgt[:, None, :].long())
    a, b, c, d, e, f, g = 5, 6, 7, 8, 9, 10, 11
    rule = np.array([[[BOS, EOS, a, b, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD],        # EOS at column 1 (tokens after it ignored)
                      [BOS, a, b, c, d, PAD, PAD, PAD, PAD, PAD, PAD, PAD]],           # no EOS, trailing PAD
                     [[BOS, a, b, c, d, e, f, g, a, b, c, d],                          # no EOS, the row is full
                      [PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD]],   # all-PAD
                     [[BOS, a, b, PAD, c, d, EOS, PAD, PAD, PAD, PAD, PAD],            # a PAD before the EOS is a target
                      [BOS, a, b, EOS, c, EOS, PAD, PAD, PAD, PAD, PAD, PAD]]],        # two EOS: the first counts
                    dtype=np.int64)
    assert rule.max() < V
    cases["rule"] = score_case(m, src[:3], torch.from_numpy(rule))
    out = {"case_names": np.array(list(cases))}
    for name, cse in cases.items():
        out.update({f"{name}__{k}": v for k, v in cse.items()})
        print(name, "hyp", cse["hyp"].shape, "finished", int(cse["finished"].sum()), "/", cse["finished"].size,
              "score range", float(cse["score"].min()), float(cse["score"].max()))
    print("beam min gaps", cases["beam"]["min_gap"])
    print("rule lengths", cases["rule"]["length"].ravel(), "finished", cases["rule"]["finished"].ravel())
    np.savez_compressed(HERE / "hyp_scores.npz", **out)
    print("wrote", HERE / "hyp_scores.npz", (HERE / "hyp_scores.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
