#!/usr/bin/env python3
"""Generate tests/golden/attn_maps.npz: per-head cross-attention maps of hypotheses under the REFERENCE model (the tiny 2+2 model
of tiny_weights.npz), by the definition of include/ttx.h (ttx_attention_maps).

Runs ONLY in the build container, where the reference is mounted read-only: like make_golden_scores.py it imports the reference's
modules (stub parent packages, so no Lightning-importing __init__ runs) and stores nothing but inputs and results.

The reference's decoder layers call their cross attention with need_weights=False, so the maps are taken without patching it: a
forward pre-hook (with_kwargs=True) on every decoder layer's ``multihead_attn`` records the arguments of the call inside
``m(src, hyp[:, :-1])`` (eval mode), and the module is called again on them with need_weights=True, average_attn_weights=False.

  targets__*  fixture pairs SOURCES (source 5 is the only one without a PAD column); hyp = the fixture targets as an N = 1 case
  rule__*     the hand-made rows of hyp_scores.npz (EOS at column 1, no EOS, all-PAD row, PAD before EOS, two EOS) -> [3, 2, 12]
Each case stores src, hyp, length, heads_l0 / heads_l1 (fp32 [B*N, H, W-1, Ls]: the reference's maps with the positions that are
not live set to zero, as the definition has them) and f64_dist [2]: per layer the largest distance of those fp32 maps from the
same recipe on the reference cast to float64 — how far the reference's own fp32 is from the exact result.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attn.py
"""
import copy
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
SOURCES = [2, 5, 7]


def length_rule(row: np.ndarray) -> int:
    for t in range(1, len(row)):
        if row[t] == EOS:
            return t
    for t in range(len(row) - 1, 0, -1):
        if row[t] != PAD:
            return t
    return 0


def maps_of(m, src: torch.Tensor, rows: torch.Tensor, two_stage: bool = False) -> list:
    """Per decoder layer the per-head cross-attention weights [R, H, W-1, Ls] of m(src, rows[:, :-1]); ``two_stage``: of
    m.decode_tgt(rows[:, :-1], m.encode_src(src)) with boolean masks (the float64 copy: its forward() mixes fp32 masks in)."""
    calls = []
    layers = list(m.transformer.decoder.layers)
    hooks = [layer.multihead_attn.register_forward_pre_hook(lambda mod, a, kw: calls.append((mod, a, dict(kw))), with_kwargs=True)
             for layer in layers]
    with torch.inference_mode():
        if two_stage:
            m.decode_tgt(rows[:, :-1], m.encode_src(src, src == PAD), src == PAD)
        else:
            m(src, rows[:, :-1])
        for h in hooks:
            h.remove()
        assert len(calls) == len(layers)
        out = []
        for mod, a, kw in calls:
            kw.update(need_weights=True, average_attn_weights=False)
            # the reference builds its additive masks in fp32: a no-op for the fp32 model, a cast for the float64 one
            kw = {k: v.to(a[0].dtype) if torch.is_tensor(v) and v.is_floating_point() else v for k, v in kw.items()}
            _, w = mod(*a, **kw)
            mean = mod(*a, **{**kw, "average_attn_weights": True})[1]
            assert torch.equal(mean, w.sum(1) / w.shape[1]) or torch.allclose(mean, w.mean(1), rtol=0, atol=1e-7)
            out.append(w)
    return out


def attn_case(m, m64, src: torch.Tensor, hyp: torch.Tensor) -> dict:
    B, N, W = hyp.shape
    rows = hyp.reshape(B * N, W)
    src_rows = src.repeat_interleave(N, dim=0)
    length = np.array([length_rule(r) for r in rows.numpy()], np.int32)
    live = (np.arange(W - 1)[None, :] < length[:, None])[:, None, :, None]
    case = dict(src=src.numpy(), hyp=hyp.numpy(), length=length.reshape(B, N))
    dist = []
    for l, (w32, w64) in enumerate(zip(maps_of(m, src_rows, rows), maps_of(m64, src_rows, rows, two_stage=True))):
        a32 = np.where(live, w32.numpy(), np.float32(0))
        a64 = np.where(live, w64.numpy(), 0.0)
        assert a32.dtype == np.float32 and np.isfinite(a32).all()
        assert (a32[np.broadcast_to((src_rows.numpy() == PAD)[:, None, None, :], a32.shape)] == 0).all()
        case[f"heads_l{l}"] = a32
        dist.append(np.abs(a32.astype(np.float64) - a64).max())
    case["f64_dist"] = np.array(dist, np.float64)
    return case


def main() -> None:
    torch.set_num_threads(8)
    z = np.load(HERE / "fixture_tokens.npz")
    src, tgt, V = torch.from_numpy(z["src"]), torch.from_numpy(z["tgt"]), int(z["vocab_size"])
    m = VanillaTransformer(V, V, 2, 2, 64, 2, 128, 0.0, "relu", True, PAD, PAD)
    w = np.load(HERE / "tiny_weights.npz")
    m.load_state_dict({k: torch.from_numpy(w[k]) for k in w.files})
    m.eval()
    m64 = copy.deepcopy(m).double().eval()
    assert not (src[5] == PAD).any()
    rule = torch.from_numpy(np.load(HERE / "hyp_scores.npz")["rule__hyp"])
    cases = {"targets": attn_case(m, m64, src[SOURCES], tgt[SOURCES][:, None, :].long()),
             "rule": attn_case(m, m64, src[:3], rule.long())}
    out = {"case_names": np.array(list(cases)), "targets__sources": np.array(SOURCES)}
    for name, cse in cases.items():
        out.update({f"{name}__{k}": v for k, v in cse.items()})
        print(name, "heads", cse["heads_l0"].shape, "length", cse["length"].ravel(), "f64_dist", cse["f64_dist"])
    np.savez_compressed(HERE / "attn_maps.npz", **out)
    print("wrote", HERE / "attn_maps.npz", (HERE / "attn_maps.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
