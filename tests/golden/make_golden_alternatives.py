#!/usr/bin/env python3
"""Generate tests/golden/alternatives.npz: the per-position alternatives of hypotheses under the REFERENCE model (the tiny 2+2
model of tiny_weights.npz), by the definition of include/ttx.h (ttx_score_alternatives).

Runs ONLY in the build container, where the reference is mounted read-only: like make_golden_scores.py it imports the reference's
modules (stub parent packages, so no Lightning-importing __init__ runs) and stores nothing but inputs and results.

Input: the three cases of hyp_scores.npz (beam, targets, rule) with their own src and hyp.  Stored per case, from the float64
log_softmax of the reference's fp32 logits VanillaTransformer.forward(src[b], hyp[b, k, :-1]):
  top_logp [B, N, W-1, 9]  the 9 largest values per live position, largest first (K = 8 plus one more, so that the gap below
                           rank 7 is known); 0 where not live
  top_id   [B, N, W-1, 9]  their ids (equal fp32 logits: the lower id first); -1 where not live
  entropy  [B, N, W-1]     -sum q log q in float64; 0 where not live
  rank     [B, N, W-1]     ids the fp32 logits order before the emitted token hyp[b, k, p+1]; -1 where not live
  length   [B, N]
No logits are stored.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_alternatives.py
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

PAD, BOS, EOS = 0, 1, 2
KEEP = 9


def length_rule(row: np.ndarray) -> int:
    for t in range(1, len(row)):
        if row[t] == EOS:
            return t
    for t in range(len(row) - 1, 0, -1):
        if row[t] != PAD:
            return t
    return 0


def alternatives_case(m, src: torch.Tensor, hyp: torch.Tensor) -> dict:
    B, N, W = hyp.shape
    rows = hyp.reshape(B * N, W)
    with torch.inference_mode():
        logits = m(src.repeat_interleave(N, dim=0), rows[:, :-1])                 # fp32 [B*N, W-1, V]
    x = logits.numpy()
    logp = torch.log_softmax(logits.double(), dim=-1).numpy()
    R, T = B * N, W - 1
    top_logp = np.zeros((R, T, KEEP), np.float64)
    top_id = np.full((R, T, KEEP), -1, np.int32)
    entropy = np.zeros((R, T), np.float64)
    rank = np.full((R, T), -1, np.int32)
    length = np.zeros(R, np.int32)
    for r, row in enumerate(rows.numpy()):
        length[r] = n = length_rule(row)
        for p in range(n):
            order = np.argsort(-x[r, p], kind="stable")                           # descending, equal logits by ascending id
            top_id[r, p] = order[:KEEP]
            top_logp[r, p] = logp[r, p, order[:KEEP]]
            entropy[r, p] = -(np.exp(logp[r, p]) * logp[r, p]).sum()
            rank[r, p] = int(np.nonzero(order == row[p + 1])[0][0])
    assert np.isfinite(top_logp).all() and np.isfinite(entropy).all()
    return dict(src=src.numpy(), hyp=hyp.numpy(), top_logp=top_logp.reshape(B, N, T, KEEP), top_id=top_id.reshape(B, N, T, KEEP),
                entropy=entropy.reshape(B, N, T), rank=rank.reshape(B, N, T), length=length.reshape(B, N))


def main() -> None:
    torch.set_num_threads(8)
    V = int(np.load(HERE / "fixture_tokens.npz")["vocab_size"])
    assert V >= KEEP
    m = VanillaTransformer(V, V, 2, 2, 64, 2, 128, 0.0, "relu", True, PAD, PAD)
    w = np.load(HERE / "tiny_weights.npz")
    m.load_state_dict({k: torch.from_numpy(w[k]) for k in w.files})
    m.eval()
    z = np.load(HERE / "hyp_scores.npz")
    names = [str(n) for n in z["case_names"]]
    out = {"case_names": np.array(names)}
    for name in names:
        cse = alternatives_case(m, torch.from_numpy(z[f"{name}__src"]), torch.from_numpy(z[f"{name}__hyp"]).long())
        assert np.array_equal(cse["length"], z[f"{name}__length"])
        out.update({f"{name}__{k}": v for k, v in cse.items()})
        live = cse["rank"] >= 0
        print(name, "hyp", cse["hyp"].shape, "live positions", int(live.sum()), "rank 0 at", int((cse["rank"][live] == 0).sum()),
              "max entropy", float(cse["entropy"].max()))
    np.savez_compressed(HERE / "alternatives.npz", **out)
    print("wrote", HERE / "alternatives.npz", (HERE / "alternatives.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
