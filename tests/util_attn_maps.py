"""Helpers of the attention-map tests: the definition of include/ttx.h (ttx_attention_maps) restated in float64 on the oracle, the
plain NumPy softmax-of-QK^T for kernel-level operands (fp32 and float64, with switchable defects for the checkers' own test), and
the checkers both GPU and host tests use."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle.model import OracleTransformer, config_from_state
from util_models import load_npz
from util_score import length_rule

EPS32 = 2.0 ** -23


def lengths_of(hyp, pad: int, eos: int) -> np.ndarray:
    """hyp Long[..., W] -> int32 [...]: n of the scoring rule."""
    return length_rule(torch.as_tensor(np.asarray(hyp)), pad, eos)[0].numpy().astype(np.int32)


def live_mask(length: np.ndarray, T: int) -> np.ndarray:
    """bool [R, T]: query position t is live iff t + 1 <= n."""
    return np.arange(T)[None, :] < np.asarray(length).reshape(-1)[:, None]


def golden_cases() -> dict:
    """name -> {src, hyp, length, heads_l0, heads_l1, f64_dist} of tests/golden/attn_maps.npz."""
    z = load_npz("attn_maps.npz")
    return {n: {k[len(n) + 2:]: v for k, v in z.items() if k.startswith(n + "__")} for n in (str(x) for x in z["case_names"])}


def oracle_maps(state: dict, num_heads: int, src, hyp, layer: int, pad: int = 0, eos: int = 2, dtype=torch.float64) -> np.ndarray:
    """The definition in float64 (or, with ``dtype=torch.float32``, what plain fp32 tensor algebra makes of it): per-head maps
    [B*N, H, W-1, Ls] of decoder layer ``layer`` for src [B, Ls], hyp [B, N, W]; zeros at PAD keys and at positions that are not
    live.  Q from the stream behind the layer's self-attention LayerNorm, K from the encoder memory, both through the layer's
    cross-attention in_proj slices."""
    src, hyp = torch.as_tensor(np.asarray(src)).long(), torch.as_tensor(np.asarray(hyp)).long()
    B, N, W = hyp.shape
    cfg = config_from_state(state, num_heads, pad)
    if layer < 0:
        layer += cfg.num_decoder_layers
    o = OracleTransformer(cfg, state, dtype=dtype)
    o.trace = {}
    rows, src_rows = hyp.reshape(B * N, W), src.repeat_interleave(N, dim=0)
    key_pad = src_rows == pad
    memory = o.encode_src(src_rows, key_pad)
    o.decode_hidden(rows[:, :-1], memory, key_pad)
    x = o.trace[f"dec.layer{layer}.sa"]
    E, H = cfg.embedding_dim, cfg.num_heads
    dh = E // H
    p = f"transformer.decoder.layers.{layer}.multihead_attn"
    w_in, b_in = o.w[p + ".in_proj_weight"], o.w[p + ".in_proj_bias"]
    q = (x @ w_in[:E].T + b_in[:E]).view(B * N, W - 1, H, dh).transpose(1, 2)
    k = (memory @ w_in[E:2 * E].T + b_in[E:2 * E]).view(B * N, -1, H, dh).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    s = s.masked_fill(key_pad[:, None, None, :], float("-inf"))
    prob = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0).numpy()      # a source that is all PAD: zeros
    live = live_mask(lengths_of(rows, pad, eos), W - 1)
    return np.where(live[:, None, :, None], prob, prob.dtype.type(0))


def head_mean(heads: np.ndarray) -> np.ndarray:
    """[R, H, T, Ls] fp32 -> [R, T, Ls] fp32: heads added in ascending order in fp32, divided by (float)H."""
    heads = np.asarray(heads, np.float32)
    acc = heads[:, 0].copy()
    for h in range(1, heads.shape[1]):
        acc = acc + heads[:, h]
    return acc / np.float32(heads.shape[1])


def first_argmax(mean: np.ndarray, live: np.ndarray) -> np.ndarray:
    """[R, T, Ls], live bool [R, T] -> int32 [R, T]: the smallest j holding the row maximum, -1 where not live."""
    return np.where(live, np.argmax(mean, axis=-1), -1).astype(np.int32)


def np_attn_probs(q, k, key_pad, mem_row, length, H: int, dh: int, T: int, Ls: int, scale: float, dtype=np.float32,
                  defect: str | None = None, n_per_src: int = 1) -> dict:
    """softmax_j(scale * q . k) in plain NumPy at ``dtype`` on kernel-level operands: q [R*T, >= H*dh], k [Rm*Ls, >= H*dh], key_pad
    [Rm*Ls] (non-zero = PAD), mem_row [R] or None, length [R] -> {heads [R,H,T,Ls], mean [R,T,Ls], align [R,T]}.  ``defect`` names
    ONE deliberate mistake (the checkers' own test): no_scale, pad_leak, unnormalised, boundary, row_map (r % n_per_src for the
    r / n_per_src the caller's mem_row holds), nonlive_nonzero, descending_heads, last_max, align_zero."""
    q, k = np.asarray(q, dtype), np.asarray(k, dtype)
    length = np.asarray(length).reshape(-1)
    R = length.size
    pad = np.asarray(key_pad).reshape(-1, Ls) != 0
    q = q[:, :H * dh].reshape(R, T, H, dh)
    k = k[:, :H * dh].reshape(-1, Ls, H, dh)
    heads = np.zeros((R, H, T, Ls), dtype)
    sc = dtype(1.0 if defect == "no_scale" else scale)
    for r in range(R):
        b = r if mem_row is None else int(np.asarray(mem_row)[r])
        if defect == "row_map":
            b = r % n_per_src
        n = min(int(length[r]) + (1 if defect == "boundary" else 0), T)
        ok = ~pad[b]
        for h in range(H):
            if n == 0 and defect != "nonlive_nonzero":
                continue
            rows = T if defect == "nonlive_nonzero" else n
            s = (q[r, :rows, h] @ k[b, :, h].T) * sc
            if ok.any():
                s = np.where(ok[None, :], s, -np.inf)
                e = np.where(ok[None, :], np.exp(s - s.max(axis=1, keepdims=True)), dtype(0))
                p = e if defect == "unnormalised" else e / e.sum(axis=1, keepdims=True, dtype=dtype)
                if defect == "pad_leak":
                    p = np.where(ok[None, :], p, dtype(1e-9))
                heads[r, h, :rows] = p
    live = live_mask(length, T)
    hs = heads[:, ::-1] if defect == "descending_heads" else heads
    mean = head_mean(hs) if dtype == np.float32 else hs.mean(axis=1)
    if defect == "last_max":
        align = np.where(live, Ls - 1 - np.argmax(mean[..., ::-1], axis=-1), -1).astype(np.int32)
    else:
        align = first_argmax(mean, live)
    if defect == "align_zero":
        align = np.where(live, align, 0).astype(np.int32)
    return {"heads": heads, "mean": mean, "align": align}


def check_result(got: dict, ref64: np.ndarray, key_pad_rows: np.ndarray, length: np.ndarray, tol: float) -> list:
    """The checks of one result {heads [R,H,T,Ls], mean [R,T,Ls], align [R,T]} (missing keys are skipped) against the float64 per-head
    maps ``ref64``; key_pad_rows bool [R, Ls]: the PAD keys of the memory row each query row reads.  Returns the names of the checks
    that fail (empty: all hold): tolerance, pad_zero, nonlive_zero, row_sum, mean_bits, align_first_max, align_nonlive."""
    bad = []
    R, H, T, Ls = ref64.shape
    live = live_mask(length, T)
    pad = np.asarray(key_pad_rows, bool)
    heads, mean, align = got.get("heads"), got.get("mean"), got.get("align")
    if heads is not None:
        heads = np.asarray(heads)
        assert heads.dtype == np.float32 and heads.shape == ref64.shape
        if not np.isfinite(heads).all() or np.abs(heads.astype(np.float64) - ref64).max() > tol:
            bad.append("tolerance")
        if (heads[np.broadcast_to(pad[:, None, None, :], heads.shape)] != 0).any():
            bad.append("pad_zero")
        if (heads[np.broadcast_to(~live[:, None, :, None], heads.shape)] != 0).any():
            bad.append("nonlive_zero")
        sums = heads.astype(np.float64).sum(-1)
        want = np.broadcast_to((live & ~pad.all(-1)[:, None])[:, None, :], sums.shape)
        if (np.abs(sums - 1.0)[want] > Ls * EPS32).any():
            bad.append("row_sum")
    if mean is not None:
        mean = np.asarray(mean)
        assert mean.dtype == np.float32 and mean.shape == (R, T, Ls)
        if heads is not None:
            if not np.array_equal(mean.view(np.uint32), head_mean(heads).view(np.uint32)):
                bad.append("mean_bits")
        else:
            if not np.isfinite(mean).all() or np.abs(mean.astype(np.float64) - ref64.mean(1)).max() > tol:
                bad.append("tolerance")
            if (mean[np.broadcast_to(pad[:, None, :], mean.shape)] != 0).any():
                bad.append("pad_zero")
            if (mean[np.broadcast_to(~live[:, :, None], mean.shape)] != 0).any():
                bad.append("nonlive_zero")
    if align is not None:
        align = np.asarray(align)
        assert align.dtype == np.int32 and align.shape == (R, T)
        if (align[~live] != -1).any():
            bad.append("align_nonlive")
        if mean is not None and not np.array_equal(align[live], first_argmax(mean, live)[live]):
            bad.append("align_first_max")
    return bad


def align_agreement(align: np.ndarray, ref_heads32: np.ndarray, length: np.ndarray, gap: float) -> tuple:
    """(mismatches, compared, live): ``align`` against the first argmax of the reference's head mean, only at live positions whose
    two largest reference values are more than ``gap`` apart."""
    ref_mean = head_mean(ref_heads32).astype(np.float64)
    live = live_mask(length, ref_mean.shape[1])
    top2 = np.sort(ref_mean, axis=-1)[..., -2:]
    clear = live & ((top2[..., 1] - top2[..., 0]) > gap)
    return int((np.asarray(align)[clear] != np.argmax(ref_mean, -1)[clear]).sum()), int(clear.sum()), int(live.sum())
