#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics.npz: the teacher-forced evaluation of the REFERENCE (validation_step / test_step,
src/model/lightning_model.py:174-207, with the metrics of src/utils/metrics.py).

Runs ONLY in the build container, where the reference is mounted read-only: like make_golden.py it imports the reference's
modules (stub parent packages, so no Lightning-importing __init__ runs) and stores nothing but inputs and results.

  tiny__*      the tiny 2+2 model (tiny_weights.npz) on the 10 fixture pairs: VanillaTransformer.forward(src, tgt[:, :-1])
               logits, the CrossEntropyLoss mean, calc_token_acc and calc_sequence_acc of the argmax;
  <case>__*    hand-built logits / targets for every quirk of the metrics: the argmax is placed on a chosen prediction, with
               exact ties resolved both ways against the target, rows without EOS, several EOS in a row, EOS at position 0,
               a batch without any EOS (NaN), PAD targets, V not a multiple of 4 and V = 1024.
Each case stores tgt (int64 [B, Lt], read at column 1 like target_future), logits (fp32 [B, Lt-1, V]), eos, and the
reference's pred (argmax), loss, token_acc, seq_acc and n_pairs (EOS count of the targets).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py
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
for _name in ("model", "utils"):
    _m = types.ModuleType(_name)
    _m.__path__ = [str(REF_SRC / _name)]
    sys.modules[_name] = _m

from model.modules import VanillaTransformer  # noqa: E402
from utils.metrics import calc_token_acc, calc_sequence_acc  # noqa: E402

PAD, BOS, EOS = 0, 1, 2


def reference_metrics(logits: torch.Tensor, tgt: torch.Tensor, eos: int) -> dict:
    """What validation_step computes from the logits (lightning_model.py:174-189)."""
    target_future = tgt[:, 1:]
    V = logits.shape[-1]
    loss = torch.nn.CrossEntropyLoss(reduction="mean")(logits.reshape(-1, V), target_future.reshape(-1))
    pred = torch.argmax(logits, dim=2)
    return dict(pred=pred.numpy(), loss=np.float32(loss.item()), token_acc=np.float32(calc_token_acc(pred, target_future).item()),
                seq_acc=np.float32(calc_sequence_acc(pred, target_future, eos).item()),
                n_pairs=np.int64(int((target_future == eos).sum())))


def section_tiny(out: dict) -> None:
    z = np.load(HERE / "fixture_tokens.npz")
    src, tgt, V = torch.from_numpy(z["src"]), torch.from_numpy(z["tgt"]), int(z["vocab_size"])
    m = VanillaTransformer(V, V, 2, 2, 64, 2, 128, 0.0, "relu", True, PAD, PAD)
    w = np.load(HERE / "tiny_weights.npz")
    m.load_state_dict({k: torch.from_numpy(w[k]) for k in w.files})
    m.eval()
    with torch.inference_mode():
        logits = m(src, tgt[:, :-1])
    r = reference_metrics(logits, tgt, EOS)
    out.update({"tiny__tgt": tgt.numpy(), "tiny__logits": logits.numpy(), "tiny__eos": np.int64(EOS)})
    out.update({"tiny__" + k: v for k, v in r.items()})
    print("tiny: loss", r["loss"], "token_acc", r["token_acc"], "seq_acc", r["seq_acc"], "pairs", r["n_pairs"])


def build_logits(rng, pred: np.ndarray, V: int, ties=()) -> np.ndarray:
    """Random logits whose argmax (first maximum) is `pred`; ties: (b, p, j) puts a second, later maximum at column j > pred."""
    B, T = pred.shape
    x = (rng.standard_normal((B, T, V)) * 3.0).astype(np.float32)
    for b in range(B):
        for p in range(T):
            x[b, p, pred[b, p]] = np.float32(x[b, p].max() + 1.0 + rng.random())
    for b, p, j in ties:
        assert j > pred[b, p]
        x[b, p, j] = x[b, p, pred[b, p]]
    return x


def with_bos(target_future) -> np.ndarray:
    t = np.asarray(target_future, dtype=np.int64)
    return np.concatenate([np.full((t.shape[0], 1), BOS, np.int64), t], axis=1)


def noisy_pred(rng, tf: np.ndarray, V: int, p_wrong: float) -> np.ndarray:
    wrong = rng.random(tf.shape) < p_wrong
    other = (tf + 1 + rng.integers(0, V - 1, tf.shape)) % V
    return np.where(wrong, other, tf).astype(np.int64)


def cases(rng) -> dict:
    c = {}
    # the example of the metric's quirks: one pair per row with a single EOS, the EOS-at-0 row pairs with the last position
    # (a hit exactly when nothing of the row is predicted right), two pairs in the row with two EOS; 3 hits of 4 pairs
    tf = np.array([[5, 6, 2, 0, 0], [2, 0, 0, 0, 0], [5, 2, 7, 2, 0], [5, 6, 7, 8, 9]])
    pr = np.array([[5, 6, 2, 1, 1], [3, 3, 3, 3, 3], [5, 2, 4, 2, 0], [5, 6, 7, 8, 8]])
    for name, V in (("example_v12", 12), ("example_v13", 13)):
        c[name] = (with_bos(tf), build_logits(rng, pr, V), EOS)
    # several EOS per row, EOS at position 0 together with later ones, EOS at the last position, rows without EOS
    tf = np.array([[2, 5, 2, 6, 7, 2, 0, 0, 0],
                   [2, 2, 5, 9, 2, 0, 0, 0, 0],
                   [5, 6, 7, 8, 9, 10, 11, 12, 2],
                   [5, 2, 6, 2, 7, 2, 8, 2, 0],
                   [5, 6, 7, 8, 9, 10, 11, 12, 13],
                   [2, 0, 0, 0, 0, 0, 0, 0, 0],
                   [2, 5, 6, 7, 8, 9, 10, 11, 2]])
    for name, V, pw in (("multi_eos_v30", 30, 0.2), ("multi_eos_v32", 32, 0.1), ("multi_eos_exact_v30", 30, 0.0)):
        pr = noisy_pred(rng, tf, V, pw)
        c[name] = (with_bos(tf), build_logits(rng, pr, V), EOS)
    # EOS at 0 in a row predicted entirely wrong, and one predicted right up to a late miss
    tf = np.array([[2, 5, 6, 2, 0, 0], [2, 5, 6, 7, 8, 2]])
    pr = np.array([[4, 4, 4, 4, 4, 4], [2, 5, 6, 7, 8, 9]])
    c["eos0_v20"] = (with_bos(tf), build_logits(rng, pr, 20), EOS)
    # no EOS anywhere: calc_sequence_acc is the mean of an empty tensor (NaN)
    tf = rng.integers(3, 16, (3, 7))
    c["no_eos_v16"] = (with_bos(tf), build_logits(rng, noisy_pred(rng, tf, 16, 0.3), 16), EOS)
    # PAD-heavy targets (PADs count in the loss and the token accuracy: no ignore_index), some PADs predicted wrong
    tf = np.zeros((5, 12), np.int64)
    for b, n in enumerate((3, 1, 6, 11, 0)):
        tf[b, :n] = rng.integers(3, 20, n)
        if n < 12:
            tf[b, n] = EOS
    c["pad_heavy_v21"] = (with_bos(tf), build_logits(rng, noisy_pred(rng, tf, 21, 0.25), 21), EOS)
    # exact ties, the first maximum wins: resolved to the target (hit) and away from it (miss), inside one float4, across lanes,
    # across 64-column strides; another EOS id (the metrics take it as an argument)
    for name, V in (("ties_v64", 64), ("ties_v67", 67)):
        tf = np.array([[10, 11, 12, 7, 0, 0], [20, 21, 7, 0, 0, 0]])
        pr = tf.copy()
        ties = [(0, 0, 11), (0, 1, 60), (0, 2, V - 1), (1, 0, 23), (1, 1, 22)]
        pr[1, 0], pr[1, 1] = 20, 21              # target = first index: hits
        pr[0, 3] = 3
        ties.append((0, 3, 7))                   # target = the later index: the first wins, a miss
        pr[1, 3] = 1
        ties.append((1, 3, 4))                   # a PAD target next to a tie away from it
        c[name] = (with_bos(tf), build_logits(rng, pr, V, ties), 7)
    # the library's largest vocabulary
    tf = np.array([[100, 900, 1023, 2, 0, 0], [2, 5, 1000, 64, 63, 2]])
    pr = tf.copy()
    pr[0, 1] = 899
    ties = [(0, 0, 1000), (1, 3, 1023), (1, 4, 64)]
    c["v1024"] = (with_bos(tf), build_logits(rng, pr, 1024, ties), EOS)
    return c


def main() -> None:
    torch.set_num_threads(8)
    out = {}
    section_tiny(out)
    rng = np.random.default_rng(20261016)
    names = []
    for name, (tgt, logits, eos) in cases(rng).items():
        r = reference_metrics(torch.from_numpy(logits), torch.from_numpy(tgt), eos)
        out.update({f"{name}__tgt": tgt, f"{name}__logits": logits, f"{name}__eos": np.int64(eos)})
        out.update({f"{name}__{k}": v for k, v in r.items()})
        names.append(name)
        print(f"{name}: B,T,V = {logits.shape}  loss {r['loss']:.6f}  token_acc {r['token_acc']}  seq_acc {r['seq_acc']}"
              f"  pairs {r['n_pairs']}")
    out["case_names"] = np.array(names)
    np.savez_compressed(HERE / "eval_metrics.npz", **out)
    print("wrote", HERE / "eval_metrics.npz", (HERE / "eval_metrics.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
