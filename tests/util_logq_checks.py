"""The quantity of ttx_hypothesis_logq / ttx_score_proposal (include/ttx.h) restated in NumPy float64 on top of
tests/util_sample_checks.py, the checker ``check_row`` that compares an implementation's outputs with it, and an enumerable toy
model.  No tests here.

``row_logq`` is the definition: the log of the probability that the sampler's rule (util_sample_checks.sample64) emits each token
of a hypothesis, forced positions free, summed over the scored positions of the row.
"""
from __future__ import annotations

import itertools
import math
from typing import NamedTuple

import numpy as np

import util_sample_checks as S

NEG_INF = -math.inf


def length_rule(h, pad: int, eos: int) -> tuple:
    """(n, finished) of a hypothesis row h[0..W-1]: the column of the first EOS at a column >= 1, else the last column >= 1 holding
    a non-PAD token, else 0."""
    h = np.asarray(h)
    for c in range(1, len(h)):
        if h[c] == eos:
            return c, True
    live = [c for c in range(1, len(h)) if h[c] != pad]
    return (live[-1] if live else 0), False


def rank_of(y: np.ndarray, t: int) -> int:
    """The number of v with y_v > y_t, or y_v == y_t and v < t."""
    return int((y > y[t]).sum() + ((y == y[t]) & (np.arange(len(y)) < t)).sum())


def token_logq(x: np.ndarray, t: int, p: S.Params, n_kept: int | None = None) -> tuple:
    """(log q, rank, kept-set size) of token ``t`` under logits row ``x`` (fp32: scaled as the kernel scales; float64: an oracle's).
    ``n_kept``: the kept-set size to use under a filter instead of the nominal one (an implementation's own, for the value check)."""
    x = np.asarray(x)
    V = len(x)
    if p.temperature == 0:
        return (0.0 if t == S.argmax_first(x) else NEG_INF), rank_of(x.astype(np.float64), t), 1
    y = S.scaled(x, p.temperature)
    rk = rank_of(y, t)
    if not p.filtered:
        m = y.max()
        with np.errstate(divide="ignore"):
            return float(y[t] - m - np.log(np.exp(y - m).sum())), rk, V
    order, _, n, _ = S.kept_counts(y, p, 0.0)
    n = n if n_kept is None else int(n_kept)
    kept = order[:n]
    if t not in kept.tolist() or not np.isfinite(y[t]):
        return NEG_INF, rk, n
    m = y[kept].max()
    return float(y[t] - m - np.log(np.exp(y[kept] - m).sum())), rk, n


class RowLogq(NamedTuple):
    tok: np.ndarray            # float64 [T]
    logq: float
    first_outside: int
    rank: np.ndarray           # int [T]
    n_kept: np.ndarray         # int [T]
    length: int
    finished: bool


def row_logq(logits: np.ndarray, h, p: S.Params, forced: int = 0, n_kept=None) -> RowLogq:
    """The definition for one hypothesis: ``logits`` [T, V], ``h`` [T + 1] (a token id outside [0, V) is read as 0), ``forced``
    leading positions forced (clamped to [0, n]).  ``n_kept`` [T]: an implementation's kept-set sizes to evaluate with."""
    logits, h = np.asarray(logits), np.asarray(h)
    T, V = logits.shape
    n, fin = length_rule(h, p.pad, p.eos)
    forced = min(max(int(forced), 0), n)
    tok, rank, kept = np.zeros(T), np.full(T, -1), np.zeros(T, dtype=np.int64)
    for pos in range(forced, n):
        t = int(h[pos + 1])
        t = t if 0 <= t < V else 0
        tok[pos], rank[pos], kept[pos] = token_logq(logits[pos], t, p, None if n_kept is None else n_kept[pos])
    outside = [pos for pos in range(n) if tok[pos] == NEG_INF]
    return RowLogq(tok, float(tok[:n].sum()) if n else 0.0, outside[0] if outside else -1, rank, kept, n, fin)


def check_row(got: dict, logits: np.ndarray, h, p: S.Params, forced: int = 0, tol: float = 1e-9) -> list:
    """Compare an implementation's outputs for one row with the definition.  ``got``: tok [T], logq, first_outside, and optionally
    rank [T], n_kept [T], length, finished.  Returns the list of complaints (empty: consistent).  Finite values within ``tol`` per
    token (``tol`` * max(1, n) for the sum), -inf and exact zeros exactly."""
    ref = row_logq(logits, h, p, forced)
    bad = []
    tok = np.asarray(got["tok"], dtype=np.float64)
    T = len(ref.tok)
    for pos in range(T):
        a, b = tok[pos], ref.tok[pos]
        if pos >= ref.length or pos < min(max(forced, 0), ref.length):
            if a != 0.0:
                bad.append(f"position {pos} is forced or not live and holds {a!r}, not exactly 0")
        elif (a == NEG_INF) != (b == NEG_INF):
            bad.append(f"position {pos}: support membership differs ({a!r} against {b!r})")
        elif b != NEG_INF and not abs(a - b) <= tol:
            bad.append(f"position {pos}: {a!r} against {b!r}")
    lq = float(got["logq"])
    if (lq == NEG_INF) != (ref.logq == NEG_INF):
        bad.append(f"logq {lq!r} against {ref.logq!r}")
    elif ref.logq != NEG_INF and not abs(lq - ref.logq) <= tol * max(1, ref.length):
        bad.append(f"logq {lq!r} against {ref.logq!r}")
    if int(got["first_outside"]) != ref.first_outside:
        bad.append(f"first_outside {int(got['first_outside'])} against {ref.first_outside}")
    for name, want in (("rank", ref.rank), ("n_kept", ref.n_kept)):
        if got.get(name) is not None and np.asarray(got[name]).tolist() != want.tolist():
            bad.append(f"{name} {np.asarray(got[name]).tolist()} against {want.tolist()}")
    if got.get("length") is not None and int(got["length"]) != ref.length:
        bad.append(f"length {int(got['length'])} against {ref.length}")
    if got.get("finished") is not None and bool(got["finished"]) != ref.finished:
        bad.append(f"finished {bool(got['finished'])} against {ref.finished}")
    return bad


def as_got(r: RowLogq) -> dict:
    return {"tok": r.tok.copy(), "logq": r.logq, "first_outside": r.first_outside, "rank": r.rank.copy(), "n_kept": r.n_kept.copy(),
            "length": r.length, "finished": r.finished}


# an enumerable toy model ---------------------------------------------------------------------------------------------------
class Toy:
    """An autoregressive model over V = 5 tokens (PAD 0, BOS 1, EOS 2, two letters) whose float64 logits are a fixed function of
    the last two tokens and the position; the PAD logit is -inf, as good as it is in a trained model, so a row ends at its EOS or
    at the width.  ``max_len`` = 4: rows are BOS plus up to three tokens."""
    V, W, PAD, BOS, EOS = 5, 4, 0, 1, 2

    def __init__(self, seed: int = 7):
        self.table = np.random.default_rng(seed).normal(0.0, 1.5, size=(self.W, self.V, self.V, self.V))
        self.table[..., self.PAD] = NEG_INF

    def logits(self, prefix) -> np.ndarray:
        """The logits row for the token after ``prefix`` (BOS first), float64 [V]."""
        a = prefix[-2] if len(prefix) > 1 else 0
        return self.table[len(prefix) - 1, a, prefix[-1]]

    def row_logits(self, h) -> np.ndarray:
        """Teacher-forced logits [W - 1, V] of row ``h`` (positions behind a PAD reuse the PAD's table entry: never scored)."""
        return np.stack([self.logits(list(h[:c + 1])) for c in range(self.W - 1)])

    def complete_rows(self) -> list:
        """Every row a sampler can return: non-PAD tokens up to the first EOS (PAD after it) or up to the width."""
        rows = []
        for body in itertools.product(range(1, self.V), repeat=self.W - 1):
            cut = next((i for i, t in enumerate(body) if t == self.EOS), None)
            if cut is not None:                  # an ended row is PAD behind its EOS (the set removes the repeats)
                body = body[:cut + 1] + (self.PAD,) * (len(body) - cut - 1)
            rows.append((self.BOS,) + tuple(body))
        return sorted(set(rows))

    def logq(self, h, p: S.Params, forced: int = 0) -> float:
        return row_logq(self.row_logits(h), h, p, forced).logq

    def sample(self, us, p: S.Params) -> tuple:
        """The row sample64 emits for the uniforms ``us`` (one per position)."""
        h = [self.BOS]
        for u in us:
            t = S.sample64(self.logits(h), u, p)
            h.append(t)
            if t in (self.EOS, self.PAD):
                break
        return tuple(h + [self.PAD] * (self.W - len(h)))
