#!/usr/bin/env python3
"""Generate the four-head fixtures under tests/golden/ from the REFERENCE implementation: a 2+2-layer model with d = 128 and 4
heads (head dimension 32, a head count that is a multiple of 4: the verify step's attention runs on k_attn3 / k_attn3s, which the
draft-select mode of the slot pool needs), F = 128, trained here on the ten fixture pairs, and the tokens of the reference's
greedy-speculative generator on it.

Runs ONLY in the build container, where the reference is mounted read-only; like make_golden_hd64.py, and like it importing
make_golden.py for its loaders and its reference imports, it stores nothing but weights trained by this script and output arrays:

  h4_config.json            the model's hyper-parameters
  h4_weights_{0,1,2}.npz    the state dict, split by tensor so that every file stays below 1 MiB (tests/util_draft_select.py joins them)
  h4_gen.npz                spec_greedy__b1_n3_d10_tokens / _calls: the reference's greedy-speculative generator, one fixture row
                            at a time, N = 3, D = 10, max_len 150

Before it writes, the script asserts what tests/test_gpu_draft_select.py relies on: the float32 and float64 oracles reproduce
every reference token and counter, and a decode of the ten rows has slot-steps with one, with two and with no draft starting
with the predicted token (tests/util_draft_select.py: executed_rows on the oracle's own fronts).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_h4.py
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

import make_golden as MG  # noqa: E402  (puts the reference's src/ on sys.path)
from make_golden import PAD, BOS, EOS, TranslationInferenceGreedy, TranslationInferenceGreedySpeculative, trim_np  # noqa: E402

H4 = dict(num_encoder_layers=2, num_decoder_layers=2, embedding_dim=128, num_heads=4, feedforward_dim=128)
PART_BYTES = 900 * 1024


def train():
    src, tgt, _, V = MG.fixture_tokens()
    torch.manual_seed(123456)
    model = MG.build_ref_model(V, H4)
    opt = torch.optim.Adam(model.parameters(), lr=2e-3)
    crit = torch.nn.CrossEntropyLoss(reduction="mean")
    model.train()
    for step in range(4000):
        logits = model(src, tgt[:, :-1])
        loss = crit(logits.reshape(-1, V), tgt[:, 1:].reshape(-1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        if float(loss) < 2e-3:
            break
    model.eval()
    with torch.inference_mode():
        g = TranslationInferenceGreedy(model, 150, PAD, BOS, EOS).generate(src)
    ok = sum(int(torch.equal(g[i, 0, :int((tgt[i] != PAD).sum())], tgt[i, :int((tgt[i] != PAD).sum())])) for i in range(src.size(0)))
    print("h4: final loss", float(loss), "steps", step, "greedy exact", ok, "/ 10", flush=True)
    assert ok == 10
    return model, V


def write_weights(model, V):
    sd = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in model.state_dict().items()}
    parts, size = [{}], 0
    for k, v in sd.items():
        if size + v.nbytes > PART_BYTES and parts[-1]:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    for old in HERE.glob("h4_weights_*.npz"):
        old.unlink()
    for i, p in enumerate(parts):
        np.savez_compressed(HERE / f"h4_weights_{i}.npz", **p)
        assert (HERE / f"h4_weights_{i}.npz").stat().st_size < 1024 * 1024
    (HERE / "h4_config.json").write_text(json.dumps(dict(H4, vocab_size=V, share_embeddings=True, weight_parts=len(parts))))
    return sd


def main():
    from oracle.decoding import GreedySpeculativeOracle
    from oracle.model import OracleTransformer, config_from_state
    import util_draft_select as S
    model, V = train()
    sd = write_weights(model, V)
    cfg = config_from_state(sd, H4["num_heads"])
    src, _, c_tok, _ = MG.fixture_tokens()
    N, D = 3, 10
    with torch.inference_mode():
        g = TranslationInferenceGreedySpeculative(model, 150, D, N, PAD, BOS, EOS, c_tok)
        toks = np.concatenate([trim_np(g.generate(src[i:i + 1])) for i in range(10)])
        for dtype in (torch.float32, torch.float64):
            o = GreedySpeculativeOracle(OracleTransformer(cfg, sd, dtype=dtype), 150, D, N, PAD, BOS, EOS, c_tok)
            assert np.array_equal(np.concatenate([o.generate(src[i:i + 1]).numpy() for i in range(10)]), toks), dtype
            assert o.model_calls_num == g.model_calls_num
    # the fronts of a greedy-speculative decode follow from its tokens and drafts: a step accepts the longest draft prefix that
    # agrees with the tokens behind the front
    drafts = np.load(HERE / "drafts.npz")["nobos_d10_n3"]
    traj = np.full((10, 151), -1, dtype=np.int16)
    for r in range(10):
        row = [int(t) for t in toks[r, 0]]
        end = row.index(EOS)
        f, it = 0, 0
        traj[r, 0] = 0
        while f < end:
            acc = max(next((j for j in range(D) if f + 1 + j > end or drafts[r, n, j] != row[f + 1 + j]), D) for n in range(N))
            f, it = f + acc + 1, it + 1
            traj[r, it] = f
    rows, fewer, several, matched = S.executed_rows(traj, toks[:, 0], drafts)
    print(f"h4: {int((traj[:, 1:] >= 0).sum())} slot-steps, {rows} rows under draft select, {fewer} slot-steps with 1 or 2 drafts present, "
          f"{several} with more than one, {matched} drafts matched", flush=True)
    assert fewer > 0 and several > 0
    np.savez_compressed(HERE / "h4_gen.npz", spec_greedy__b1_n3_d10_tokens=toks, spec_greedy__b1_n3_d10_calls=np.int64(g.model_calls_num))


if __name__ == "__main__":
    main()
