"""The rule of k_sbs_step_masked (csrc/ttx_sbs.hip.h, include/ttx.h: ttx_sbs_generate_ex) restated for the tests: the per-parent token
mask of a top-k / top-p filter or a forced prefix put in front of util_sbs_checks.step / search, in float64 (or float32, to measure
what fp32 costs), operands for the kernel test, and the checker.  No tests here.

Free position, filter on: the kept set of a parent's row is util_sample_checks.kept_counts on y = x * inv_T (the sampler's own
restatement); every other logit becomes -inf and util_sbs_checks.step runs on that row as it is: m, z and lp over the kept set,
Philox keyed by the token id.  Forced position: the child `tok` of every unfinished parent carries phi and G of the parent, every
other child is -inf, no logit is read and no uniform formed.

The checker is util_sbs_checks.check_step with one more excuse: a rank whose float64-selected or device-selected token changes
between kept and not kept when top_p moves by ``tol`` (KEPT_TOL, the tolerance tests/test_gpu_sample_kernel.py holds the sampler's
kept set to).  Where fp32 and float64 do disagree on such a token, the boundary lies within fp32 rounding of top_p, the token's mass
at most that, and its siblings' lp move by as little: inside the margin.  kernel_case draws its inputs so that float64 alone, this
excuse included, excuses at most half of EXCUSED_CAP.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import util_sample_checks as P
import util_sbs_checks as S
from util_sbs_checks import EXCUSED_CAP, ILL, Step

KEPT_TOL = 1e-4            # tests/test_gpu_sample_kernel.py: TOL (the tests assert the two are equal)
# max |G'_fp32 - G'_float64| over the selected, well-conditioned children of the masked kernel test's own inputs (kernel_cases()),
# NumPy restatement in float32 against float64 (tests/test_sbs_mask_checks_host.py re-measures and asserts it); ten times that for
# the device's own expf / logf / log1pf.  Measured: 1.07e-5, on (V 65, beam 5, K 5, T 0.5, top_k 32, top_p 0.9); every other parametrisation
# stays below 3.8e-6, where util_sbs_checks' unmasked cases stay (3.9e-6)
FP32_GAP = 1.1e-5
MARGIN = 10 * FP32_GAP

DEFECTS = ("kept_off_by_one", "noise_by_kept_rank", "lp_not_renormalised", "prefix_lp_added", "forced_noise", "masked_child_emitted")


def params(temperature: float, top_k: int, top_p: float) -> P.Params:
    return P.Params(temperature, top_k, top_p)


def kept(y: np.ndarray, p: P.Params, tol: float = 0.0, defect: str | None = None):
    """(keep, flip) bool [V] of one scaled row: the kept set, and the tokens whose status changes when top_p moves by ``tol``."""
    if not p.filtered:
        return np.ones(len(y), bool), np.zeros(len(y), bool)
    order, lo, n, hi = P.kept_counts(y, p, tol)
    if defect == "kept_off_by_one":
        n = n + 1 if n < min(len(y), int(np.isfinite(y).sum())) else n - 1
    keep, flip = np.zeros(len(y), bool), np.zeros(len(y), bool)
    keep[order[:n]] = True
    flip[order[lo:hi]] = True
    return keep, flip


def masked_logits(logits, finished, p: P.Params, tol: float = 0.0, defect: str | None = None):
    """(logits with -inf outside every unfinished parent's kept set, flip [beam, V])."""
    x = np.array(logits, copy=True)
    flip = np.zeros(x.shape, bool)
    for k in range(x.shape[0]):
        if not finished[k]:
            keep, flip[k] = kept(P.scaled(x[k], p.temperature), p, tol, defect)
            x[k, ~keep] = -np.inf
    return x, flip


def _select(img_g, img_phi, ill, finished, K: int, pad: int, eos: int, defect: str | None = None) -> Step:
    """Steps 6-7 of the rule on the images (util_sbs_checks.step's own tail)."""
    V = img_g.shape[1]
    flat = img_g.reshape(-1)
    exists = np.nonzero(~np.isnan(flat))[0]
    order = exists[np.lexsort((exists, -flat[exists]))]
    sel = order[:K].copy()
    if defect == "masked_child_emitted":
        low = order[np.isneginf(flat[order])]
        low = low[~finished[low // V]]
        if len(low) and np.isfinite(flat[sel[-1]]):
            sel[-1] = low[0]
    par, tok = sel // V, sel % V
    g_sel = flat[sel]
    fin = finished[par] | (tok == eos) | (tok == pad) | np.isneginf(g_sel)
    return Step(par, tok, img_phi.reshape(-1)[sel], g_sel, fin, order, img_g, img_phi, ill)


def _rows(x, xm, phi, G, finished, key, pos, seed, temperature, pad, dtype, defect):
    """The images of a free step written out, for the planted defects only (the rule itself goes through util_sbs_checks.step)."""
    beam, V = x.shape
    inv_t = np.float32(1.0) / np.float32(temperature)
    img_g = np.full((beam, V), np.nan, dtype=dtype)
    img_phi = np.full((beam, V), np.nan, dtype=dtype)
    ill = np.zeros((beam, V), dtype=bool)
    u_all = S.uniforms(seed, key, np.arange(beam), V, pos).astype(dtype)
    with np.errstate(all="ignore"):
        for k in range(beam):
            if finished[k]:
                img_g[k, pad], img_phi[k, pad] = G[k], phi[k]
                continue
            y, yf = (xm[k] * inv_t).astype(dtype), (x[k] * inv_t).astype(dtype)
            u = u_all[k]
            if defect == "noise_by_kept_rank":            # the r-th best kept token takes the uniform of id r
                order = P.rank_order(y.astype(np.float64))
                u = u.copy()
                u[order] = u_all[k][np.arange(V)]
            src = yf if defect == "lp_not_renormalised" else y
            m = src.max()
            lp = np.where(np.isneginf(y), -np.inf, (src - m) - np.log(np.exp(src - m).sum(dtype=dtype)))
            ph = phi[k] + lp
            g = ph - np.log(-np.log(u))
            Z = g.max()
            t = (G[k] - g) + np.log1p(-np.exp(g - Z))
            Gc = G[k] - np.maximum(t, 0) - np.log1p(np.exp(-np.abs(t)))
            Gc = np.where(g == Z, G[k], Gc)
            Gc = np.where(np.isneginf(y), -np.inf, Gc)
            img_g[k], img_phi[k] = Gc.astype(dtype), ph
            ill[k] = (Z - g > 0) & (Z - g < ILL)
    return img_g, img_phi, ill


def step(logits, phi, G, finished, key: int, pos: int, seed: int, temperature: float, K: int, pad: int, eos: int,
         top_k: int = 0, top_p: float = 1.0, forced: int | None = None, dtype=np.float64, defect: str | None = None,
         tol: float = 0.0):
    """One step of the masked rule for one source: (Step, flip [beam, V]).  ``forced``: the prefix token of a forced position (an id
    outside [0, V) is read as 0), or None for a free position.  ``defect`` plants one deviation (DEFECTS)."""
    x = np.asarray(logits)
    if x.dtype != np.float64:
        x = x.astype(np.float32)
    beam, V = x.shape
    finished = np.asarray(finished, dtype=bool)
    if forced is not None:
        tok = int(forced) if 0 <= int(forced) < V else 0
        phi_d, G_d = np.asarray(phi, dtype=dtype), np.asarray(G, dtype=dtype)
        img_g = np.full((beam, V), -np.inf, dtype=dtype)
        img_phi = np.full((beam, V), -np.inf, dtype=dtype)
        if defect in ("prefix_lp_added", "forced_noise"):
            # the defect treats the forced token as a sampled one: lp over the full row, noise over the full row
            full, _, _ = _rows(x, x, phi_d, G_d, finished, key, pos, seed, temperature, pad, dtype, None)
            st = S.step(x, phi_d, G_d, finished, key, pos, seed, temperature, K, pad, eos, dtype)
        for k in range(beam):
            if finished[k]:
                img_g[k], img_phi[k] = np.nan, np.nan
                img_g[k, pad], img_phi[k, pad] = G_d[k], phi_d[k]
                continue
            img_g[k, tok], img_phi[k, tok] = G_d[k], phi_d[k]
            if defect == "prefix_lp_added":
                img_phi[k, tok] = st.img_phi[k, tok]
            if defect == "forced_noise":
                img_g[k, tok] = full[k, tok]
        return _select(img_g, img_phi, np.zeros((beam, V), bool), finished, K, pad, eos, defect), np.zeros((beam, V), bool)
    p = params(temperature, top_k, top_p)
    xm, flip = masked_logits(x, finished, p, tol, defect)
    if defect in ("noise_by_kept_rank", "lp_not_renormalised"):
        img = _rows(x, xm, np.asarray(phi, dtype=dtype), np.asarray(G, dtype=dtype), finished, key, pos, seed, temperature, pad, dtype, defect)
        return _select(*img, finished, K, pad, eos), flip
    st = S.step(xm, phi, G, finished, key, pos, seed, temperature, K, pad, eos, dtype)
    if defect == "masked_child_emitted":
        st = _select(st.img_g, st.img_phi, st.ill, finished, K, pad, eos, defect)
    return st, flip


def search(model, key: int, seed: int, temperature: float, K: int, max_len: int, pad: int, bos: int, eos: int, top_k: int = 0,
           top_p: float = 1.0, prefix=(), dtype=np.float64):
    """util_sbs_checks.search under the mask: ``prefix`` the forced tokens of positions 1 .. len(prefix).  Returns
    (rows [K, max_len], phi [K], g [K], finished [K], levels)."""
    rows = np.array([[bos]], dtype=np.int64)
    phi, G, fin = np.zeros(1, dtype=dtype), np.zeros(1, dtype=dtype), np.zeros(1, dtype=bool)
    levels = []
    for pos in range(1, max_len):
        forced = int(prefix[pos - 1]) if pos <= len(prefix) else None
        logits = np.asarray(model(rows))
        st, _ = step(logits, phi, G, fin, key, pos, seed, temperature, K, pad, eos, top_k, top_p, forced, dtype)
        rows = np.concatenate([rows[st.parent], st.token[:, None]], axis=1)
        phi, G, fin = st.phi, st.g, st.finished
        levels.append(st)
        if fin.all():
            break
    out = np.full((K, max_len), pad, dtype=np.int64)
    out[:, :rows.shape[1]] = rows
    return out, phi, G, fin, levels


# operands for the kernel test ---------------------------------------------------------------------------------------------------
class MaskCase(NamedTuple):
    """util_sbs_checks.Case plus the filter and, for forced cases, the prefix table by source."""
    c: S.Case
    top_k: int
    top_p: float
    pfx_tok: np.ndarray | None = None    # int32 [B, ld]
    pfx_len: np.ndarray | None = None    # int32 [B]

    def forced(self, b: int):
        if self.pfx_len is None or self.c.pos > int(self.pfx_len[b]):
            return None
        return int(self.pfx_tok[b, self.c.pos - 1])


KERNEL_V = (7, 65, 256, 1024)
KERNEL_BEAM_K = ((1, 5), (5, 5), (32, 32))
KERNEL_FILTER = ((1, 1.0), (5, 1.0), (32, 0.9), (0, 0.5))
KERNEL_T = (0.5, 3.0)


def _with_dead_parent(c: S.Case) -> S.Case:
    """The last parent of every source of a wider beam becomes a finished -inf candidate (a masked child an earlier level emitted):
    phi = G = -inf.  Its logits row stays in the matrix, unused."""
    if c.beam == 1:
        return c
    phi, G, fin, slot_of = c.phi.copy(), c.G.copy(), c.finished.copy(), c.slot_of.copy()
    last = np.arange(c.B) * c.beam + c.beam - 1
    phi[last], G[last], fin[last], slot_of[last] = -np.inf, -np.inf, 1, -1
    return c._replace(phi=phi, G=G, finished=fin, slot_of=slot_of)


def case_reference(mc: MaskCase, b: int, dtype=np.float64, defect: str | None = None, tol: float = 0.0):
    """(Step, flip) of the restatement for source b of a case."""
    c = mc.c
    cs = slice(b * c.beam, (b + 1) * c.beam)
    rows = np.where(c.slot_of[cs] >= 0, c.slot_of[cs], 0)
    return step(c.logits[rows], c.phi[cs], c.G[cs], c.finished[cs] != 0, int(c.keys[b]), c.pos, c.seed, c.temperature, c.K, c.pad,
                c.eos, mc.top_k, mc.top_p, mc.forced(b), dtype, defect, tol)


def float64_excused(mc: MaskCase) -> int:
    """Ranks of a case that the float64 restatement alone excuses (near-ties, ill-conditioned children, kept-set boundaries)."""
    n = 0
    for b in range(mc.c.B):
        ref, flip = case_reference(mc, b, tol=KEPT_TOL)
        n += int((S.excused_ranks(ref, mc.c.K, MARGIN) | flip.reshape(-1)[ref.order[:mc.c.K]]).sum())
    return n


def kernel_case(V: int, beam: int, K: int, temperature: float, top_k: int, top_p: float, B: int = 3) -> MaskCase:
    """The deterministic operands of one parametrisation: util_sbs_checks' draw (with a -inf parent per source of a wider beam), the
    first salt on which float64 alone (near-ties, ill-conditioned children, kept-set boundaries) excuses at most half of EXCUSED_CAP."""
    for salt in range(100):
        mc = MaskCase(_with_dead_parent(S._draw_case(V, beam, K, temperature, B, salt)), top_k, top_p)
        if 2 * float64_excused(mc) <= EXCUSED_CAP * B * K:
            return mc
    raise AssertionError("no draw without near-ties")


def kernel_cases():
    return [kernel_case(V, beam, K, t, tk, tp) for V in KERNEL_V for beam, K in KERNEL_BEAM_K for tk, tp in KERNEL_FILTER
            for t in KERNEL_T]


def forced_case(V: int, beam: int, K: int, toks, top_k: int = 0, top_p: float = 1.0) -> MaskCase:
    """Three sources at one position: source 0 forced to toks[0], source 1 free (its prefix ended one position earlier), source 2
    forced to toks[1] (which may lie outside [0, V)), with a prefix that goes on."""
    mc = kernel_case(V, beam, K, 1.0, top_k, top_p)
    pos = mc.c.pos
    tab = np.full((3, pos + 1), 3, dtype=np.int32)
    tab[0, pos - 1], tab[2, pos - 1] = toks
    return mc._replace(pfx_tok=tab, pfx_len=np.array([pos, pos - 1, pos + 1], dtype=np.int32))


# the checker ----------------------------------------------------------------------------------------------------------------------
def check_step(dev, ref: Step, flip, parent_G, parent_phi, parent_finished, K: int, pad: int, eos: int, margin: float):
    """util_sbs_checks.check_step, and a rank is also excused where the float64-selected or the device-selected token lies on a
    kept-set boundary (``flip`` from step(.., tol=KEPT_TOL)).  Returns (problems, excused)."""
    bad, _ = S.check_step(dev, ref, parent_G, parent_phi, parent_finished, K, pad, eos, margin)
    beam, V = ref.img_g.shape
    par, tok = np.asarray(dev.parent).astype(np.int64), np.asarray(dev.token).astype(np.int64)
    if ((par < 0) | (par >= beam) | (tok < 0) | (tok >= V)).any():
        return bad, 0
    mine = par * V + tok
    fl = np.asarray(flip).reshape(-1)
    boundary = fl[ref.order[:K]] | fl[mine]
    excused = S.excused_ranks(ref, K, margin) | ref.ill.reshape(-1)[mine] | boundary
    bad = [m for m in bad if not any(boundary[r] and m.startswith(f"rank {r}:") for r in range(K))]
    return bad, int(excused.sum())


def measure_fp32_gap(cases) -> float:
    """util_sbs_checks.measure_fp32_gap on masked cases: the restatement in float32 against itself in float64, same kept sets."""
    worst = 0.0
    for mc in cases:
        for b in range(mc.c.B):
            r64, r32 = case_reference(mc, b)[0], case_reference(mc, b, np.float32)[0]
            sel = r64.order[:mc.c.K]
            sel = sel[~r64.ill.reshape(-1)[sel]]
            a, d = r64.img_g.reshape(-1)[sel], r32.img_g.reshape(-1)[sel].astype(np.float64)
            both = np.isfinite(a) & np.isfinite(d)
            assert (a[~both] == d[~both]).all()
            if both.any():
                worst = max(worst, float(np.abs(a[both] - d[both]).max()))
    return worst
