"""A float64 constrained beam search over the oracle model's logits (tests/test_gpu_beam_constrained.py): the rule of include/ttx.h
"Constrained beam search" with the restated masks (tests/util_syntax.py) and no fp32 anywhere, one source at a time.

search() returns, per source, the K rows best first, their totals, and ``close``: the smallest margin the search itself had to decide
on, as (gap, level) pairs reduced to one flag.  At level l (the column being predicted) the fp32 library may order two totals
otherwise than float64 does only if they are closer than the error of l accumulated log-probabilities; with logits within LOGIT_TOL
of the oracle's a log-softmax value moves by at most 2 * LOGIT_TOL, so a source counts as CLOSE when, at some level, the K-th and the
(K + 1)-th total or two adjacent selected totals (finite ones) lie closer than 2 * LOGIT_TOL * level.  Only such a source may differ
from the library's rows.
"""
from __future__ import annotations

import numpy as np
import torch

import util_syntax as Y

NEG = -np.inf


def log_softmax64(x: np.ndarray) -> np.ndarray:
    """log softmax over the finite entries of a float64 row; -inf stays -inf; no finite entry: all -inf."""
    ok = np.isfinite(x)
    out = np.full(len(x), NEG)
    if ok.any():
        a = x[ok] - x[ok].max()
        out[ok] = a - np.log(np.exp(a).sum())
    return out


def search(o64, src_row: torch.Tensor, K: int, max_len: int, pad: int, bos: int, eos: int, tol: float, *, bias=None, cls=None,
           prefix=None, levels: int | None = None):
    """One source.  ``bias`` float [V] (0 / -inf / values), ``cls`` int8 [V] (the syntax table), ``prefix`` a list of forced tokens.
    ``levels``: the number of steps the library's batch ran (its out_width - 1; None: until every row is finished or max_len - 1).
    Returns (rows int64 [K, width], totals float64 [K], close)."""
    prefix = [] if prefix is None else [int(t) for t in prefix]
    cands = [([bos], 0.0, False)]
    close = False
    steps = max_len - 1 if levels is None else levels
    for level in range(1, steps + 1):
        live = [i for i, (_, s, f) in enumerate(cands) if not f]
        forced = level <= len(prefix)
        lg = None
        if live and not forced:
            with torch.no_grad():
                tok = torch.tensor([cands[i][0] for i in live], dtype=torch.int64)
                lg = o64(src_row[None].expand(len(live), -1), tok)[:, -1].numpy().astype(np.float64)
        V = None if lg is None else lg.shape[1]
        tot = []
        for i, (toks, s, f) in enumerate(cands):
            if f:
                t = {pad: s} if s != NEG else {}            # a finished parent's one child (the artificial row costs log z = 3e-14)
            elif forced:
                t = {prefix[level - 1]: s}
            else:
                x = lg[live.index(i)].copy()
                if bias is not None:
                    x = x + np.asarray(bias, np.float64)
                if cls is not None:
                    x[~Y.allowed(cls, *Y.state(cls, toks[1:]), level, max_len, eos)] = NEG
                lp = log_softmax64(x)
                t = {v: s + lp[v] for v in range(V) if lp[v] != NEG}
            tot.append(t)
        flat = sorted(((-val, i, v) for i, t in enumerate(tot) for v, val in t.items()))
        vals = [-a for a, _, _ in flat[:K + 1]]
        for hi, lo in zip(vals[:-1], vals[1:]):
            if hi - lo < 2 * tol * level:
                close = True
        new = []
        for a, i, v in flat[:K]:
            toks, s, f = cands[i]
            new.append((toks + [v], -a, f or v == eos))
        while len(new) < K:                                   # dead rows: the first parent's tokens and PAD (blanked by the caller)
            new.append((cands[0][0] + [pad], NEG, True))
        cands = new
        if levels is None and all(f for _, _, f in cands) and level > 1:
            break
    rows = np.array([t for t, _, _ in cands], dtype=np.int64)
    totals = np.array([s for _, s, _ in cands])
    dead = totals == NEG
    rows[dead, 1:] = pad
    return rows, totals, close
