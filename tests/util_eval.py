"""Helpers of the teacher-forced evaluation tests: a torch restatement of the reference's validation metrics
(src/model/lightning_model.py:174-189, src/utils/metrics.py) and the golden cases of tests/golden/eval_metrics.npz."""
from __future__ import annotations

import numpy as np
import torch

from util_models import load_npz


def reference_metrics(logits: torch.Tensor, tgt: torch.Tensor, eos: int, pred: torch.Tensor | None = None) -> dict:
    """loss / token_acc / seq_acc as validation_step computes them, on the CPU.  `pred` replaces the argmax (to score a
    prediction that differs from it at a proven near-tie)."""
    logits, tgt = logits.detach().float().cpu(), tgt.detach().cpu()
    target_future = tgt[:, 1:]
    V = logits.shape[-1]
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, V), target_future.reshape(-1))
    if pred is None:
        pred = torch.argmax(logits, dim=2)
    pred = pred.detach().cpu()
    token_acc = (pred == target_future).float().mean()
    hit = (pred == target_future).long()
    is_eos = target_future == eos
    seq_acc = (hit.cumsum(dim=-1)[is_eos.roll(-1, dims=-1)] == is_eos.nonzero(as_tuple=True)[1]).float().mean()
    return {"loss": float(loss), "token_acc": float(token_acc), "seq_acc": float(seq_acc), "pred": pred}


def golden_cases() -> dict:
    """name -> {tgt, logits, eos, pred, loss, token_acc, seq_acc, n_pairs} (the tiny model's fixture run is 'tiny')."""
    z = load_npz("eval_metrics.npz")
    names = ["tiny"] + [str(n) for n in z["case_names"]]
    keys = ("tgt", "logits", "eos", "pred", "loss", "token_acc", "seq_acc", "n_pairs")
    return {n: {k: z[f"{n}__{k}"] for k in keys} for n in names}


def same_float(a: float, b: float) -> bool:
    """Bit-for-bit equality of two fp32 values, NaN equal to NaN."""
    a, b = np.float32(a), np.float32(b)
    return bool((np.isnan(a) and np.isnan(b)) or a == b)
