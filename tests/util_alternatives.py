"""Helpers of the alternatives tests: a plain NumPy restatement of the definition (include/ttx.h, ttx_score_alternatives), the
checkers the GPU test runs on a result, and the golden cases of tests/golden/alternatives.npz."""
from __future__ import annotations

import numpy as np

from util_models import load_npz

TOK_TOL = 1e-5          # relative to max(1, max|ref|): the bound test_gpu_score.py holds token_logp to
FIELDS = ("top_id", "top_logp", "chosen_logp", "rank", "entropy", "length")


def lengths(hyp: np.ndarray, pad: int, eos: int) -> np.ndarray:
    """hyp [R, W] -> int32 [R]: the column of the first EOS at a column >= 1, else the last non-PAD column >= 1, else 0."""
    out = np.zeros(hyp.shape[0], np.int32)
    for r, row in enumerate(hyp):
        hit = np.nonzero(row[1:] == eos)[0]
        if hit.size:
            out[r] = hit[0] + 1
        else:
            tok = np.nonzero(row[1:] != pad)[0]
            out[r] = tok[-1] + 1 if tok.size else 0
    return out


def order_of(x: np.ndarray) -> np.ndarray:
    """ids by descending logit, equal logits (-0.0 == 0.0) by ascending id, -inf last: a stable sort of the negated row."""
    return np.argsort(-x, axis=-1, kind="stable")


def restate(logits: np.ndarray, hyp: np.ndarray, pad: int, eos: int, k: int, dtype=np.float64) -> dict:
    """The definition from fp32 logits [R, T, V] and hyp [R, T+1], every value computed in ``dtype``; the not-live values where a
    position is not live."""
    x = np.asarray(logits, np.float32)
    R, T, V = x.shape
    n = lengths(hyp, pad, eos)
    live = np.arange(T)[None, :] < n[:, None]
    xd = x.astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = xd.max(-1, keepdims=True)
        logp = (xd - m) - np.log(np.exp(xd - m).sum(-1, keepdims=True, dtype=dtype))
        q = np.exp(logp)
        entropy = -np.where(q > 0, q * logp, 0).sum(-1, dtype=dtype)
    order = order_of(x)
    t = hyp[:, 1:].astype(np.int64)
    rank = (order == t[..., None]).argmax(-1).astype(np.int32)
    top_id = order[..., :k].astype(np.int32)
    out = {
        "top_id": np.where(live[..., None], top_id, -1).astype(np.int32),
        "top_logp": np.where(live[..., None], np.take_along_axis(logp, order[..., :k], -1), 0).astype(dtype),
        "chosen_logp": np.where(live, np.take_along_axis(logp, t[..., None], -1)[..., 0], 0).astype(dtype),
        "rank": np.where(live, rank, -1).astype(np.int32),
        "entropy": np.where(live, entropy, 0).astype(dtype),
        "length": n,
    }
    return out


def first_k(ref: dict, k: int) -> dict:
    """The restatement at a smaller k: the first k columns of the top lists."""
    return {**ref, "top_id": ref["top_id"][..., :k], "top_logp": ref["top_logp"][..., :k]}


def _close(got: np.ndarray, ref: np.ndarray, tol: float) -> np.ndarray:
    """|got - ref| <= tol where ref is finite, got == ref where it is not (a -inf logit has log-probability -inf)."""
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        return np.where(fin, np.abs(got.astype(np.float64) - np.where(fin, ref, 0)) <= tol, got == ref)


def value_tolerance(ref: dict) -> float:
    """TOK_TOL * max(1, max|ref|) over the finite reference log-probabilities; the entropy is held to the same bound."""
    v = np.concatenate([ref["top_logp"].ravel(), ref["chosen_logp"].ravel()])
    v = v[np.isfinite(v)]
    return TOK_TOL * max(1.0, float(np.abs(v).max()) if v.size else 0.0)


def check_result(got: dict, logits: np.ndarray, hyp: np.ndarray, pad: int, eos: int, range_only: np.ndarray | None = None,
                 ref: dict | None = None) -> list:
    """Every defect of a result ``got`` (FIELDS -> arrays [R, T(, k)] / [R]) against the float64 restatement on the same fp32
    logits, as a list of strings (empty: none).  ids, rank and length are compared exactly, the values within
    TOK_TOL * max(1, max|ref|); positions of ``range_only`` (bool [R, T]: rows outside the contract) only for ids and ranks in
    [0, V).  ``ref``: the float64 restatement at this or a larger k, when the caller has it already."""
    x = np.asarray(logits, np.float32)
    R, T, V = x.shape
    k = got["top_id"].shape[-1]
    ref = first_k(ref, k) if ref is not None else restate(x, hyp, pad, eos, k)
    bad = []
    if not np.array_equal(got["length"], ref["length"]):
        return ["length"]
    live = np.arange(T)[None, :] < ref["length"][:, None]
    if range_only is None:
        range_only = np.zeros((R, T), bool)
    if ((got["top_id"][range_only] < 0) | (got["top_id"][range_only] >= V)).any() or \
            ((got["rank"][range_only] < 0) | (got["rank"][range_only] >= V)).any():
        bad.append("id or rank outside [0, V)")
    dead = ~live
    if (got["top_id"][dead] != -1).any() or (got["rank"][dead] != -1).any() or (got["top_logp"][dead] != 0).any() or \
            (got["chosen_logp"][dead] != 0).any() or (got["entropy"][dead] != 0).any():
        bad.append("a value past the length")
    c = live & ~range_only                                   # the positions under the contract
    ids, lp = got["top_id"][c], got["top_logp"][c]
    if k > 1 and (np.sort(ids, -1)[:, 1:] == np.sort(ids, -1)[:, :-1]).any():
        bad.append("duplicated id")
    with np.errstate(invalid="ignore"):
        if k > 1 and (lp[:, 1:] > lp[:, :-1]).any():
            bad.append("top_logp not sorted")
    safe = np.clip(ids, 0, V - 1)
    xs = np.take_along_axis(x[c], safe, -1)
    if k > 1 and ((xs[:, 1:] == xs[:, :-1]) & (ids[:, 1:] < ids[:, :-1])).any():
        bad.append("a tie broken towards the higher id")
    if not np.array_equal(ids, ref["top_id"][c]):
        bad.append("top_id")
    rk, t = got["rank"][c], hyp[:, 1:][c]
    if not np.array_equal(rk, ref["rank"][c]):
        bad.append("rank")
    inside = (rk >= 0) & (rk < k)
    if (np.take_along_axis(ids, np.clip(rk, 0, k - 1)[:, None], -1)[:, 0][inside] != t[inside]).any():
        bad.append("top_id[rank] != chosen")
    tol = value_tolerance({f: ref[f][c] for f in ("top_logp", "chosen_logp")})
    for f in ("top_logp", "chosen_logp", "entropy"):
        if not _close(got[f][c], ref[f][c], tol).all():
            bad.append(f)
    return bad


def value_errors(got: dict, ref: dict, live: np.ndarray) -> dict:
    """max |got - ref| over the live positions where the reference value is finite, per value field."""
    out = {}
    for f in ("top_logp", "chosen_logp", "entropy"):
        g, r = got[f][live].astype(np.float64), ref[f][live].astype(np.float64)
        fin = np.isfinite(r)
        out[f] = float(np.abs(g[fin] - r[fin]).max()) if fin.any() else 0.0
    return out


def golden_cases() -> dict:
    """name -> {src, hyp, top_logp, top_id, entropy, rank, length} as NumPy arrays."""
    z = load_npz("alternatives.npz")
    return {n: {key[len(n) + 2:]: v for key, v in z.items() if key.startswith(n + "__")} for n in (str(x) for x in z["case_names"])}


def compare_with_golden(got: dict, case: dict, k: int) -> dict:
    """A result at ``k`` against a golden case (which stores k + 1 ranks).  Returns what the test asserts on: the largest errors
    of length-masked sorted top_logp and entropy, the bound, the (position, rank) pairs whose reference value is more than
    4 * bound away from both neighbours in rank, the pairs among them whose id differs, and the live positions whose emitted
    token's own pair is compared but whose rank differs."""
    lead = case["length"].shape
    T = case["rank"].shape[-1]
    live = np.arange(T) < case["length"][..., None]
    ref_lp, ref_id = case["top_logp"][live], case["top_id"][live]            # [P, k + 1]
    assert ref_lp.shape[-1] == k + 1
    bound = TOK_TOL * max(1.0, float(np.abs(ref_lp[:, :k]).max()))           # the entropy is held to the same bound
    lp, ids = got["top_logp"].reshape(lead + (T, k))[live], got["top_id"].reshape(lead + (T, k))[live]
    gap_below = ref_lp[:, :k] - ref_lp[:, 1:k + 1]
    gap_above = np.concatenate([np.full((ref_lp.shape[0], 1), np.inf), gap_below[:, :-1]], axis=1)
    clear = (gap_below > 4 * bound) & (gap_above > 4 * bound)
    rk, ref_rk = got["rank"].reshape(lead + (T,))[live], case["rank"][live]
    own = (ref_rk < k) & np.take_along_axis(clear, np.clip(ref_rk, 0, k - 1)[:, None], -1)[:, 0]
    return {"bound": bound, "length_equal": np.array_equal(got["length"].reshape(lead), case["length"]),
            "top_logp_err": float(np.abs(lp - ref_lp[:, :k]).max()),
            "entropy_err": float(np.abs(got["entropy"].reshape(lead + (T,))[live] - case["entropy"][live]).max()),
            "pairs": int(clear.size), "left_out": int((~clear).sum()), "id_mismatches": int((ids != ref_id[:, :k])[clear].sum()),
            "rank_mismatches": int((rk != ref_rk)[own].sum())}
