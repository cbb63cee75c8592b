"""The rule of k_sample (csrc/ttx_sample.hip.h, include/ttx.h: ttx_sample_generate) restated for the tests: Philox4x32-10 in NumPy
integers, the kept set, its order and the CDF in float64, a float64 sampler, and the checker ``consistent``.  No tests here.

A sampler's token for a row is right when the row's uniform falls into the token's own interval of the CDF, taken in the
kernel's order.  The kernel forms the CDF in fp32 and this file in float64, so the checker takes the interval widened by ``tol``
on either side; where the nucleus boundary itself lies within ``tol`` of ``top_p`` both kept sets are admissible.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MAX_KEEP = 32
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 on integer arrays: ``counter`` [..., 4] and ``key`` [..., 2] of 32-bit words (broadcast against each other)
    -> uint32 [..., 4].  Integer arithmetic only: the 32 x 32 products are taken in uint64."""
    c = np.asarray(counter, dtype=np.uint64) & MASK32
    k = np.asarray(key, dtype=np.uint64) & MASK32
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead).copy() for i in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform(seed, key, sample, pos) -> np.ndarray:
    """u = (x0 >> 8) * 2^-24 as float64 (exact: 24 bits), x0 = word 0 of Philox with key (seed_lo, seed_hi) and counter
    (key_lo, key_hi, sample, pos).  Every argument is an integer or an integer array; 64-bit ones are taken modulo 2^64."""
    def u64(v):
        if isinstance(v, int):
            return np.asarray(v % (1 << 64), dtype=np.uint64)
        a = np.asarray(v)
        return a if a.dtype == np.uint64 else a.astype(np.int64).astype(np.uint64)      # an int64's bits

    def words64(v):
        v = u64(v)
        return v & MASK32, v >> np.uint64(32)
    slo, shi = words64(seed)
    klo, khi = words64(key)
    smp, p = u64(sample) & MASK32, u64(pos) & MASK32
    lead = np.broadcast_shapes(slo.shape, klo.shape, smp.shape, p.shape)
    ctr = np.stack([np.broadcast_to(a, lead) for a in (klo, khi, smp, p)], axis=-1)
    ky = np.stack([np.broadcast_to(a, lead) for a in (slo, shi)], axis=-1)
    x0 = philox4x32_10(ctr, ky)[..., 0]
    return (x0 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


class Params(NamedTuple):
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    pad: int = 0
    eos: int = 2

    @property
    def filtered(self) -> bool:
        return self.top_k != 0 or self.top_p < 1.0

    @property
    def keep_cap(self) -> int:
        """The top_k the kernel runs with: a call that gives only top_p < 1 runs with 32."""
        return self.top_k if self.top_k != 0 else MAX_KEEP


def scaled(logits: np.ndarray, temperature: float) -> np.ndarray:
    """y = x * inv_T with inv_T = 1.0f / T in fp32, as float64.  fp32 logits are scaled in fp32 (the kernel's own product, bit
    for bit); float64 logits (an oracle's) in float64."""
    inv_t = np.float32(1.0) / np.float32(temperature)
    x = np.asarray(logits)
    if x.dtype == np.float32:
        with np.errstate(over="ignore"):
            return (x * inv_t).astype(np.float64)
    return x.astype(np.float64) * np.float64(inv_t)


def argmax_first(x: np.ndarray) -> int:
    return int(np.nonzero(x == x.max())[0][0])


def rank_order(y: np.ndarray) -> np.ndarray:
    """Token ids best first; equal values: the lower id first."""
    return np.lexsort((np.arange(len(y)), -y))


def kept_counts(y: np.ndarray, p: Params, tol: float) -> tuple:
    """(order, n_lo, n, n_hi): the rank order and how many leading ranks are kept with the boundary moved down by ``tol``, as it
    is, and moved up by ``tol``.  Rank i is kept while i < top_k, y is finite and the softmax mass ranked above it is < top_p;
    rank 0 always."""
    order = rank_order(y)
    ys = y[order]
    e = np.exp(ys - ys[0])
    above = np.concatenate([[0.0], np.cumsum(e)[:-1]]) / e.sum()
    cap = min(p.keep_cap, int(np.isfinite(ys).sum()), len(y))

    def count(bound):
        n = 1
        while n < cap and above[n] < bound:
            n += 1
        return n
    return order, count(p.top_p - tol), count(p.top_p), count(p.top_p + tol)


def cdf_orders(y: np.ndarray, p: Params, tol: float = 0.0) -> list:
    """The admissible kept sets as arrays of token ids in the kernel's CDF order: ascending id without a filter, rank order with
    one (several where the nucleus boundary is within ``tol`` of top_p; the nominal one first)."""
    if not p.filtered:
        return [np.arange(len(y))]
    order, lo, n, hi = kept_counts(y, p, tol)
    return [order[:n]] + [order[:m] for m in range(lo, hi + 1) if m != n]


def cdf(y: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """Inclusive float64 CDF over ``ids`` in their order, normalised to end at 1."""
    e = np.exp(y[ids] - y[ids].max())
    c = np.cumsum(e)
    return c / c[-1]


def sample64(logits: np.ndarray, u: float, p: Params) -> int:
    """The rule in float64: the first kept token whose inclusive CDF exceeds u; the last one with a positive share otherwise."""
    x = np.asarray(logits)
    if p.temperature == 0:
        return argmax_first(x)
    y = scaled(x, p.temperature)
    ids = cdf_orders(y, p)[0]
    c = cdf(y, ids)
    hit = np.nonzero((c > u) & np.isfinite(y[ids]))[0]
    if len(hit):
        return int(ids[hit[0]])
    return int(ids[np.nonzero(np.isfinite(y[ids]))[0][-1]])


def excess(token: int, logits: np.ndarray, u: float, p: Params, tol: float = 0.0) -> float:
    """How far u lies outside the token's CDF interval (0: inside), the smallest over the admissible kept sets; inf for a token
    that is not kept or whose logit is -inf.  temperature 0: 0 for the first maximum, inf otherwise."""
    x = np.asarray(logits)
    if p.temperature == 0:
        return 0.0 if token == argmax_first(x) else math.inf
    y = scaled(x, p.temperature)
    if not (0 <= token < len(y)) or not np.isfinite(y[token]):
        return math.inf
    best = math.inf
    for ids in cdf_orders(y, p, tol):
        at = np.nonzero(ids == token)[0]
        if len(at) == 0:
            continue
        i = int(at[0])
        c = cdf(y, ids)
        prev = c[i - 1] if i else 0.0
        best = min(best, max(prev - u, u - c[i], 0.0))
    return best


def consistent(token: int, logits: np.ndarray, u: float, p: Params, tol: float) -> bool:
    """True iff ``token`` is kept and C(prev) - tol <= u <= C(token) + tol, C the float64 CDF in the kernel's order."""
    return excess(int(token), logits, float(u), p, tol) <= tol


def ends(rows: np.ndarray, pad: int, eos: int) -> np.ndarray:
    """Per row of generated tokens [R, W] (BOS in column 0): the column of the first EOS or PAD after BOS, or W - 1."""
    rows = np.asarray(rows)
    stop = (rows[:, 1:] == eos) | (rows[:, 1:] == pad)
    return np.where(stop.any(1), stop.argmax(1) + 1, rows.shape[1] - 1)


# chi-square ---------------------------------------------------------------------------------------------------------------
CHI2_11_Q1E6 = 48.8656          # the chi-square quantile at 1 - 1e-6 for 11 degrees of freedom (chi2_sf below gives 1e-6 there)


def chi2_sf(x: float, k: int) -> float:
    """P[chi2_k > x] for odd k, by the closed form erfc(sqrt(x/2)) + sqrt(2x/pi) e^(-x/2) sum_{j<(k-1)/2} x^j / (1*3*..*(2j+1))."""
    assert k % 2 == 1
    s, term = 0.0, 1.0
    for j in range((k - 1) // 2):
        if j:
            term *= x / (2 * j + 1)
        s += term
    return math.erfc(math.sqrt(x / 2)) + math.sqrt(2 * x / math.pi) * math.exp(-x / 2) * s
