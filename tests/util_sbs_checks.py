"""The rule of k_sbs_step (csrc/ttx_sbs.hip.h, include/ttx.h: ttx_sbs_generate) restated for the tests: the uniforms from Philox in
NumPy integers (util_sample_checks.philox4x32_10), one step of stochastic beam search in float64 (or, to measure what fp32 costs,
in float32) taking fp32 logits as given, a whole search over a callable model, consistent states for the kernel test, and the
checker ``check_step``.  No tests here.

The checker.  A device step is compared with the float64 step of the same operands.  Exact whatever the rounding: new_g is
non-increasing, no child is selected twice, a child of a finished parent is PAD with phi and G carried on the bits, G' never exceeds
its parent's G, the finished flag follows the rule, and ties between -inf children go to the lower flat index.  Against float64:
rank r must name the float64 step's (parent, token) and carry its phi' and G' within ``margin``.  A rank is excused from that where
the float64 G' of its child lies within ``margin`` of a neighbouring rank's (the (K+1)-th included): fp32 may order the two either
way, and a swap moves both ranks, so the rank below a near-tie is excused with the rank above it.  A rank is also excused where the
float64-selected or the device-selected child is ill-conditioned, 0 < Z - g < ILL (log1p(-exp(g - Z)) loses its digits there); the
G' of such a child is not checked.  What the device selected instead is still checked against ITS float64 phi' (and G' unless
ill-conditioned), so an excused rank cannot carry arbitrary values.  ``check_step`` returns the problems and the excused count;
the caller holds the count against EXCUSED_CAP.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from util_sample_checks import philox4x32_10

ILL = 1e-2                 # children with 0 < Z - g < ILL are ill-conditioned
EXCUSED_CAP = 0.05         # at most this share of the ranks of a parametrisation may be excused
# max |G'_fp32 - G'_float64| over the selected, well-conditioned children of the kernel test's own inputs (kernel_cases below), from
# the NumPy restatement run in float32 against itself in float64 (tests/test_sbs_checks_host.py re-measures and asserts it), and
# ten times that for the device's own expf / logf / log1pf
FP32_GAP = 4.0e-6
MARGIN = 10 * FP32_GAP


def uniforms(seed: int, key: int, k, V: int, pos: int, half: float = 0.5) -> np.ndarray:
    """u_{k,v} for v < V as float64 (exact: 24 bits): word v & 3 of the Philox block with key (seed_lo, seed_hi) and counter
    (key_lo, key_hi, 0x80000000 | k << 8 | v >> 2, pos), mapped by ((w >> 9) + 0.5) * 2^-23.  ``k`` an integer: [V]; an array of
    parent ranks: [len(k), V]."""
    seed, key = seed % (1 << 64), key % (1 << 64)
    ks = np.atleast_1d(np.asarray(k)).astype(np.uint64)
    blk = np.broadcast_to(np.arange((V + 3) // 4, dtype=np.uint64), (len(ks), (V + 3) // 4))
    ctr = np.stack([np.full_like(blk, key & 0xFFFFFFFF), np.full_like(blk, key >> 32),
                    np.uint64(0x80000000) | (ks[:, None] << np.uint64(8)) | blk, np.full_like(blk, pos)], axis=-1)
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).reshape(len(ks), -1)[:, :V]
    u = ((w >> np.uint32(9)).astype(np.float64) + half) * 2.0 ** -23
    return u[0] if np.ndim(k) == 0 else u


class Step(NamedTuple):
    parent: np.ndarray       # [K] rank of the parent
    token: np.ndarray        # [K]
    phi: np.ndarray          # [K]
    g: np.ndarray            # [K]
    finished: np.ndarray     # [K] bool
    order: np.ndarray        # every existing child's flat index k * V + v, ranked
    img_g: np.ndarray        # [beam, V] G' (NaN: no such child)
    img_phi: np.ndarray      # [beam, V] phi'
    ill: np.ndarray          # [beam, V] bool


def step(logits, phi, G, finished, key: int, pos: int, seed: int, temperature: float, K: int, pad: int, eos: int,
         dtype=np.float64, defect: str | None = None) -> Step:
    """One step of the rule for one source.  ``logits`` fp32 [beam, V] (rows of finished parents are not read), ``phi`` / ``G`` /
    ``finished`` [beam].  The arithmetic after the fp32 product y = x * inv_T runs in ``dtype``.  ``defect`` plants one deviation
    from the rule (the checker's sensitivity test): 'tie_high', 'noise_by_token', 'no_clamp', 'u_reaches_1', 'finished_expanded',
    'pad_not_end', 'phi_wrong_parent', 'order_ascending'."""
    x = np.asarray(logits)
    if x.dtype != np.float64:                  # fp32 logits are scaled in fp32 (the kernel's own product), an oracle's in float64
        x = x.astype(np.float32)
    beam, V = x.shape
    phi, G = np.asarray(phi, dtype=dtype), np.asarray(G, dtype=dtype)
    finished = np.asarray(finished, dtype=bool)
    inv_t = np.float32(1.0) / np.float32(temperature)
    img_g = np.full((beam, V), np.nan, dtype=dtype)
    img_phi = np.full((beam, V), np.nan, dtype=dtype)
    ill = np.zeros((beam, V), dtype=bool)
    u_all = uniforms(seed, key, np.zeros(beam, np.int64) if defect == "noise_by_token" else np.arange(beam), V, pos,
                     1.0 if defect == "u_reaches_1" else 0.5).astype(dtype)
    with np.errstate(all="ignore"):
        for k in range(beam):
            if finished[k] and defect != "finished_expanded":
                img_g[k, pad], img_phi[k, pad] = G[k], phi[k]
                continue
            y = (x[k] * (inv_t if x.dtype == np.float32 else np.float64(inv_t))).astype(dtype)
            m = y.max()
            lp = (y - m) - np.log(np.exp(y - m).sum(dtype=dtype))
            src = (k + 1) % beam if defect == "phi_wrong_parent" else k
            ph = phi[src] + lp
            g = ph - np.log(-np.log(u_all[k]))
            Z = g.max()
            t = (G[k] - g) + np.log1p(-np.exp(g - Z))
            Gc = G[k] - np.maximum(t, 0) - np.log1p(np.exp(-np.abs(t)))
            Gc = np.where(g == Z, G[k], Gc)
            Gc = np.where(np.isneginf(y), -np.inf, Gc)
            if defect == "no_clamp":
                Gc = g
            img_g[k], img_phi[k] = Gc.astype(dtype), ph
            ill[k] = (Z - g > 0) & (Z - g < ILL)
    flat_g = img_g.reshape(-1)
    exists = np.nonzero(~np.isnan(flat_g))[0]
    tie = -exists if defect == "tie_high" else exists
    order = exists[np.lexsort((tie, -flat_g[exists]))]
    sel = order[:K]
    if defect == "order_ascending":
        sel = sel[::-1]
    par, tok = sel // V, sel % V
    g_sel = flat_g[sel]
    ends = (tok == eos) | (tok == pad) if defect != "pad_not_end" else (tok == eos)
    fin = finished[par] | ends | np.isneginf(g_sel)
    return Step(par, tok, img_phi.reshape(-1)[sel], g_sel, fin, order, img_g, img_phi, ill)


def search(model, key: int, seed: int, temperature: float, K: int, max_len: int, pad: int, bos: int, eos: int, dtype=np.float64):
    """The whole rule for one source: ``model(prefixes)`` -> logits [n, V] (fp32, or an oracle's float64) of the next token for the integer rows
    ``prefixes`` [n, width].  Returns (rows [K, max_len], phi [K], g [K], finished [K], levels)."""
    rows = np.array([[bos]], dtype=np.int64)
    phi, G, fin = np.zeros(1, dtype=dtype), np.zeros(1, dtype=dtype), np.zeros(1, dtype=bool)
    levels = []
    for pos in range(1, max_len):
        logits = np.asarray(model(rows))
        st = step(logits, phi, G, fin, key, pos, seed, temperature, K, pad, eos, dtype)
        rows = np.concatenate([rows[st.parent], st.token[:, None]], axis=1)
        phi, G, fin = st.phi, st.g, st.finished
        levels.append(st)
        if fin.all():
            break
    out = np.full((K, max_len), pad, dtype=np.int64)
    out[:, :rows.shape[1]] = rows
    return out, phi, G, fin, levels


# consistent operands for the kernel test --------------------------------------------------------------------------------------
def make_logits(rng, rows: int, V: int) -> np.ndarray:
    """fp32 logits with about a tenth of the entries -inf (never a whole row), as the sampler's kernel test makes them."""
    x = (2.0 * rng.standard_normal((rows, V))).astype(np.float32)
    if V > 1:
        hole = rng.random((rows, V)) < 0.1
        hole[np.arange(rows), rng.integers(0, V, rows)] = False
        x[hole] = -np.inf
    return x


def make_state(rng, beam: int, width: int, V: int, pad: int, eos: int):
    """(phi, G, finished, gen [beam, width]) of one source: G = phi + a Gumbel draw, sorted jointly by G descending, which is how the
    candidates of a running search are distributed (a parent's G and its children's maximum Z are draws of the same law).  A single
    candidate is the root (phi = G = 0).  About a fifth of the candidates of a wider beam are finished."""
    gen = rng.integers(3, max(V, 4), (beam, width)).astype(np.int32) % V
    gen[:, 0] = 1
    if beam == 1:
        return np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.uint8), gen
    phi = -rng.gamma(2.0, 1.5, beam)
    G = phi - np.log(-np.log(rng.random(beam)))
    o = np.argsort(-G)
    phi, G = phi[o].astype(np.float32), (G[o] - G[o][0]).astype(np.float32)
    fin = (rng.random(beam) < 0.2).astype(np.uint8)
    for k in np.nonzero(fin)[0]:
        gen[k, width - 1] = eos if (k & 1 or width < 3) else pad
        if width >= 3 and not (k & 1):
            gen[k, width - 2] = eos
    return phi, G, fin, gen


class Case(NamedTuple):
    """The operands of one k_sbs_step launch over B sources (beam parents each) and what identifies it."""
    V: int
    beam: int
    K: int
    B: int
    temperature: float
    logits: np.ndarray       # [B * beam, V], the row of candidate c at slot_of[c] (finished candidates have none)
    slot_of: np.ndarray      # [B * beam]
    phi: np.ndarray
    G: np.ndarray
    finished: np.ndarray
    gen: np.ndarray          # [B * beam, ld]
    keys: np.ndarray         # [B] int64
    width: int
    ld: int
    pos: int
    seed: int
    pad: int = 0
    eos: int = 2


KERNEL_V = (7, 64, 65, 256, 1024)
KERNEL_BEAM_K = ((1, 1), (1, 5), (2, 2), (5, 5), (32, 32))
KERNEL_T = (0.5, 1.0, 3.0)


def kernel_case(V: int, beam: int, K: int, temperature: float, B: int = 3) -> Case:
    """The deterministic operands of one parametrisation of the kernel test (the CPU test measures FP32_GAP on these very cases):
    the first draw on which the float64 restatement alone excuses at most half of EXCUSED_CAP of the B * K ranks (none, where
    B * K < 40), so that near-ties of the inputs do not use up what the cap leaves the device."""
    for salt in range(100):
        c = _draw_case(V, beam, K, temperature, B, salt)
        if 2 * sum(int(excused_ranks(case_reference(c, b), K, MARGIN).sum()) for b in range(B)) <= EXCUSED_CAP * B * K:
            return c
    raise AssertionError("no draw without near-ties")


def _draw_case(V: int, beam: int, K: int, temperature: float, B: int, salt: int) -> Case:
    rng = np.random.default_rng([V, beam, K, int(temperature * 10), 2019, salt])
    width = 1 if beam == 1 else 4
    ld, pad, eos = width + 3, 0, 2
    phi, G, fin, gen = [], [], [], []
    for _ in range(B):
        p, g, f, rows = make_state(rng, beam, width, V, pad, eos)
        full = np.full((beam, ld), pad, dtype=np.int32)
        full[:, :width] = rows
        phi.append(p); G.append(g); fin.append(f); gen.append(full)
    phi, G, fin, gen = np.concatenate(phi), np.concatenate(G), np.concatenate(fin), np.concatenate(gen)
    live = np.nonzero(fin == 0)[0]
    slot_of = np.full(B * beam, -1, dtype=np.int32)
    slot_of[live] = rng.permutation(len(live)).astype(np.int32)          # compact rows, in an order of their own
    logits = np.zeros((max(len(live), 1), V), dtype=np.float32)
    logits[slot_of[live]] = make_logits(rng, len(live), V)
    keys = rng.integers(-2 ** 62, 2 ** 62, B).astype(np.int64)
    return Case(V, beam, K, B, temperature, logits, slot_of, phi, G, fin, gen, keys, width, ld, width,
                int(rng.integers(0, 2 ** 63)), pad, eos)


def case_reference(c: Case, b: int, dtype=np.float64, defect: str | None = None) -> Step:
    """The restatement's step for source b of a case."""
    cs = slice(b * c.beam, (b + 1) * c.beam)
    rows = np.where(c.slot_of[cs] >= 0, c.slot_of[cs], 0)
    return step(c.logits[rows], c.phi[cs], c.G[cs], c.finished[cs] != 0, int(c.keys[b]), c.pos, c.seed, c.temperature, c.K,
                c.pad, c.eos, dtype, defect)


# the checker ----------------------------------------------------------------------------------------------------------------
def _gap(a: float, b: float) -> float:
    """|a - b| between two ranked G' values; two -inf are an exact tie that the index rule decides: never a near-tie."""
    if np.isneginf(a) and np.isneginf(b):
        return np.inf
    return abs(a - b)


def excused_ranks(ref: Step, K: int, margin: float) -> np.ndarray:
    """bool [K]: ranks the float64 step alone excuses (a neighbouring rank within ``margin``, or an ill-conditioned child)."""
    flat = ref.img_g.reshape(-1)
    ranked = flat[ref.order[:K + 1]]
    out = np.zeros(K, dtype=bool)
    for r in range(K):
        if r + 1 < len(ranked) and _gap(ranked[r], ranked[r + 1]) < margin:
            out[r] = True
            if r + 1 < K:
                out[r + 1] = True
    return out | ref.ill.reshape(-1)[ref.order[:K]]


def check_step(dev, ref: Step, parent_G, parent_phi, parent_finished, K: int, pad: int, eos: int, margin: float):
    """``dev``: anything with parent / token / phi / g / finished [K] (a device launch's outputs for one source, or a Step).
    Returns (problems, excused): the list of what is wrong and how many of the K ranks were excused (see the module docstring)."""
    V = ref.img_g.shape[1]
    par, tok = np.asarray(dev.parent).astype(np.int64), np.asarray(dev.token).astype(np.int64)
    phi, g, fin = np.asarray(dev.phi), np.asarray(dev.g), np.asarray(dev.finished).astype(bool)
    parent_G, parent_phi, parent_finished = np.asarray(parent_G), np.asarray(parent_phi), np.asarray(parent_finished).astype(bool)
    bad = []
    beam = ref.img_g.shape[0]
    if ((par < 0) | (par >= beam) | (tok < 0) | (tok >= V)).any():
        return [f"parent or token out of range: {par.tolist()} {tok.tolist()}"], 0
    flat = par * V + tok
    if len(set(flat.tolist())) != K:
        bad.append(f"a child was selected twice: {flat.tolist()}")
    if np.isnan(g).any() or np.isnan(phi).any():
        bad.append("NaN in new_phi / new_g")
    if (g[1:] > g[:-1]).any():
        bad.append(f"new_g is not non-increasing: {g.tolist()}")
    excused = excused_ranks(ref, K, margin)
    ref_flat_g, ref_flat_phi, ref_ill = ref.img_g.reshape(-1), ref.img_phi.reshape(-1), ref.ill.reshape(-1)
    for r in range(K):
        k, v = int(par[r]), int(tok[r])
        if g[r] > parent_G[k]:
            bad.append(f"rank {r}: G' {g[r]!r} exceeds its parent's G {parent_G[k]!r}")
        if parent_finished[k]:
            if v != pad:
                bad.append(f"rank {r}: finished parent {k} expanded with token {v}")
            elif np.float32(g[r]).tobytes() != np.float32(parent_G[k]).tobytes() or \
                    np.float32(phi[r]).tobytes() != np.float32(parent_phi[k]).tobytes():
                bad.append(f"rank {r}: finished parent {k} not carried bit for bit")
        want_fin = bool(parent_finished[k] or v == eos or v == pad or np.isneginf(g[r]))
        if bool(fin[r]) != want_fin:
            bad.append(f"rank {r}: finished flag {bool(fin[r])}, the rule says {want_fin}")
        # the child the device selected, against its own float64 values
        if np.isnan(ref_flat_g[flat[r]]):
            if not parent_finished[k]:
                bad.append(f"rank {r}: child ({k}, {v}) does not exist")
            continue
        if ref_ill[flat[r]]:
            excused[r] = True
        for name, got, want, skip in (("phi'", phi[r], ref_flat_phi[flat[r]], False), ("G'", g[r], ref_flat_g[flat[r]], ref_ill[flat[r]])):
            if skip:
                continue
            if np.isinf(want) or np.isinf(got):
                if got != want:
                    bad.append(f"rank {r}: {name} {got!r}, float64 {want!r}")
            elif abs(float(got) - float(want)) > margin:
                bad.append(f"rank {r}: {name} {got!r} is {abs(float(got) - float(want)):.3g} from float64 {want!r} (margin {margin:g})")
        if not excused[r] and flat[r] != ref.order[r]:
            bad.append(f"rank {r}: selected (parent {k}, token {v}), float64 selects (parent {int(ref.order[r]) // V}, "
                       f"token {int(ref.order[r]) % V})")
    return bad, int(excused.sum())


def measure_fp32_gap(cases) -> float:
    """max |G'_fp32 - G'_float64| over the float64-selected, well-conditioned children of ``cases``: the NumPy restatement in
    float32 against itself in float64, independent of any kernel."""
    worst = 0.0
    for c in cases:
        for b in range(c.B):
            r64, r32 = case_reference(c, b), case_reference(c, b, np.float32)
            sel = r64.order[:c.K]
            sel = sel[~r64.ill.reshape(-1)[sel]]
            a, d = r64.img_g.reshape(-1)[sel], r32.img_g.reshape(-1)[sel].astype(np.float64)
            both = np.isfinite(a) & np.isfinite(d)
            assert (a[~both] == d[~both]).all()
            if both.any():
                worst = max(worst, float(np.abs(a[both] - d[both]).max()))
    return worst


# chi-square ---------------------------------------------------------------------------------------------------------------
LEVEL = 1e-4               # the level of the frequency checks (seeds are fixed: the outcome is deterministic)


def gammaincc(a: float, x: float) -> float:
    """Regularised upper incomplete gamma Q(a, x): the series below a + 1, Lentz's continued fraction above."""
    if x <= 0:
        return 1.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1:
        term = total = 1.0 / a
        n = a
        while abs(term) > abs(total) * 1e-16:
            n += 1
            term *= x / n
            total += term
        return 1.0 - lead * total
    tiny = 1e-300
    b = x + 1 - a
    c, d = 1 / tiny, 1 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        delta = d * c
        h *= delta
        if abs(delta - 1) < 1e-16:
            break
    return lead * h


def chi2_sf(x: float, dof: int) -> float:
    return gammaincc(dof / 2, x / 2)


def chi2_p(counts: np.ndarray, probs: np.ndarray) -> float:
    """p-value of the counts against the cell probabilities; cells expecting fewer than 5 are pooled into one."""
    n = counts.sum()
    small = probs * n < 5
    if small.sum() > 1:
        counts = np.concatenate([counts[~small], [counts[small].sum()]])
        probs = np.concatenate([probs[~small], [probs[small].sum()]])
    e = probs * n
    return chi2_sf(float(((counts - e) ** 2 / e).sum()), len(e) - 1)
