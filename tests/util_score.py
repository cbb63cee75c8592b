"""Helpers of the hypothesis-score tests: a plain torch restatement of the definition (include/ttx.h, ttx_score_hypotheses) and
the golden cases of tests/golden/hyp_scores.npz."""
from __future__ import annotations

import torch

from util_models import load_npz


def length_rule(hyp: torch.Tensor, pad: int, eos: int):
    """hyp Long[..., W] -> (length int64 [...], finished bool [...]): the column of the first EOS at a column >= 1, else the last
    column >= 1 holding a non-PAD token, else 0.  Column 0 (the BOS) never counts."""
    hyp = hyp.detach().cpu()
    W = hyp.shape[-1]
    cols = torch.arange(W).expand_as(hyp)
    body = cols >= 1
    is_eos = (hyp == eos) & body
    finished = is_eos.any(-1)
    first_eos = torch.where(is_eos, cols, torch.full_like(cols, W)).amin(-1)
    last_tok = torch.where((hyp != pad) & body, cols, torch.zeros_like(cols)).amax(-1)
    return torch.where(finished, first_eos, last_tok), finished


def scores_from_token_logp(tok_logp: torch.Tensor, hyp: torch.Tensor, pad: int, eos: int) -> dict:
    """tok_logp [..., W-1] (any values past the length) -> masked tok_logp (float64, exactly 0 past the length), score, length,
    finished."""
    length, finished = length_rule(hyp, pad, eos)
    tok = tok_logp.detach().cpu().double()
    keep = torch.arange(tok.shape[-1]).expand_as(tok) < length.unsqueeze(-1)
    tok = torch.where(keep, tok, torch.zeros_like(tok))
    return {"tok_logp": tok, "score": tok.sum(-1), "length": length, "finished": finished}


def reference_scores(logits: torch.Tensor, hyp: torch.Tensor, pad: int, eos: int) -> dict:
    """The definition in float64 from logits [..., W-1, V] (fp32 as a model gave them) and hyp Long[..., W]."""
    hyp = hyp.detach().cpu()
    logp = torch.log_softmax(logits.detach().cpu().double(), dim=-1)
    tok = logp.gather(-1, hyp[..., 1:].unsqueeze(-1)).squeeze(-1)
    return scores_from_token_logp(tok, hyp, pad, eos)


def golden_cases() -> dict:
    """name -> {src, hyp, tok_logp, score, length, finished[, min_gap]} as torch tensors."""
    z = load_npz("hyp_scores.npz")
    out = {}
    for n in (str(x) for x in z["case_names"]):
        out[n] = {k[len(n) + 2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(n + "__")}
    return out
