"""CPU checks of the stochastic-beam-search test tools (tests/util_sbs_checks.py) and of scoring.sbs_weights: the float64
restatement samples without replacement from an enumerable model, nests, feeds an unbiased estimator; the checker flags planted
defects; the Philox layout and the uniform mapping match hand-computed values; the kernel test's inputs keep the float64
restatement under the excused cap and reproduce the recorded fp32 gap."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import util_sbs_checks as S
from util_sbs_checks import LEVEL, chi2_p
from translation_transformer_amd import scoring

V, DEPTH, BOS = 3, 3, 0
NONE = -1                     # pad / eos of the toy model: no token ends a row, so every sequence has DEPTH tokens
N_KEYS = 20000
SEED = 20190611


@pytest.fixture(scope="module")
def toy():
    """Fixed conditional tables over V = 3 tokens for every prefix of fewer than DEPTH tokens, the sequence probabilities, and the
    restatement's K = 4 search for N_KEYS keys (shared by the tests; never modified)."""
    rng = np.random.default_rng(7)
    tables = {}
    for d in range(DEPTH):
        for idx in np.ndindex(*(V,) * d):
            tables[idx] = rng.uniform(-1.0, 1.0, V).astype(np.float32)

    def model(rows):
        return np.stack([tables[tuple(int(t) for t in r[1:])] for r in rows])
    seqs = list(np.ndindex(*(V,) * DEPTH))
    p = np.ones(len(seqs))
    for i, s in enumerate(seqs):
        for d in range(DEPTH):
            t = tables[s[:d]].astype(np.float64)
            p[i] *= np.exp(t[s[d]]) / np.exp(t).sum()
    assert abs(p.sum() - 1) < 1e-12
    index = {s: i for i, s in enumerate(seqs)}
    K = 4
    ids = np.zeros((N_KEYS, K), dtype=np.int64)
    logp, gum = np.zeros((N_KEYS, K)), np.zeros((N_KEYS, K))
    for key in range(N_KEYS):
        rows, ph, g, _, _ = S.search(model, key, SEED, 1.0, K, DEPTH + 1, NONE, BOS, NONE)
        ids[key] = [index[tuple(int(t) for t in r[1:])] for r in rows]
        logp[key], gum[key] = ph, g
    return SimpleNamespace(model=model, p=p, ids=ids, logp=logp, gumbel=gum, K=K)


def test_first_row_is_distributed_as_the_model(toy):
    counts = np.bincount(toy.ids[:, 0], minlength=len(toy.p)).astype(np.float64)
    assert chi2_p(counts, toy.p) > LEVEL
    assert np.allclose(toy.logp[:, 0], np.log(toy.p[toy.ids[:, 0]]), atol=1e-9)
    assert (toy.gumbel[:, 0] == 0).all()


def test_first_two_rows_are_a_sample_without_replacement(toy):
    n = len(toy.p)
    a, b = toy.ids[:, 0], toy.ids[:, 1]
    assert (a != b).all()
    counts = np.bincount(a * n + b, minlength=n * n).astype(np.float64).reshape(n, n)
    probs = toy.p[:, None] * toy.p[None, :] / (1 - toy.p[:, None])
    off = ~np.eye(n, dtype=bool)
    assert abs(probs[off].sum() - 1) < 1e-12
    assert chi2_p(counts[off], probs[off]) > LEVEL


def test_rows_are_distinct_and_gumbel_descends(toy):
    assert all(len(set(r)) == toy.K for r in toy.ids[:500].tolist())
    assert (np.diff(toy.gumbel, axis=1) <= 0).all()


def test_k_is_the_first_k_of_k_plus_2(toy):
    for key in range(40):
        rows, ph, g, fin, _ = S.search(toy.model, key, SEED, 1.0, toy.K - 2, DEPTH + 1, NONE, BOS, NONE)
        big = S.search(toy.model, key, SEED, 1.0, toy.K, DEPTH + 1, NONE, BOS, NONE)
        assert np.array_equal(rows, big[0][:toy.K - 2])
        assert ph.tobytes() == big[1][:toy.K - 2].tobytes() and g.tobytes() == big[2][:toy.K - 2].tobytes()


def test_sbs_weights_estimate_of_total_mass_averages_to_one(toy):
    """sum_i w_i estimates 1 and sum_i w_i 1[y_i == y*] the mass of y*: the means over the keys lie within 4 standard errors of the
    restatement's own spread."""
    w = scoring.sbs_weights(toy.logp, toy.gumbel)               # the K = 4 call feeds a sample of 3
    assert w.shape == (N_KEYS, toy.K - 1) and w.dtype == np.float64
    total = w.sum(1)
    assert abs(total.mean() - 1) <= 4 * total.std(ddof=1) / math.sqrt(N_KEYS)
    star = int(np.argmax(toy.p))
    mass = (w * (toy.ids[:, :-1] == star)).sum(1)
    assert abs(mass.mean() - toy.p[star]) <= 4 * mass.std(ddof=1) / math.sqrt(N_KEYS)
    # the formula itself (the paper's weight averaged over the root's Gumbel draw, by brute-force quadrature), kappa near 0 and
    # far below, and the threshold at -inf
    e = np.linspace(0, 60, 6_000_001)
    for kappa in (-0.05, -2.0, -30.0):
        lp, g = np.log([0.5, 0.25, 1e-7, 0.125]), np.array([0.0, kappa / 3, kappa / 2, kappa])
        a = np.expm1(-kappa)
        f = [np.exp(-e) / -np.expm1(-p * (a + e)) for p in np.exp(lp[:3])]
        want = [p * float(((y[1:] + y[:-1]) / 2).sum() * (e[1] - e[0])) for p, y in zip(np.exp(lp[:3]), f)]
        assert np.allclose(scoring.sbs_weights(lp, g), want, rtol=1e-6), kappa
    lp, g = np.log([0.5, 0.25, 0.125]), np.array([0.0, -1.0, -2.0])
    assert np.allclose(scoring.sbs_weights(lp, np.array([0.0, -1.0, -np.inf])), [0.5, 0.25])
    with pytest.raises(ValueError):
        scoring.sbs_weights(lp, g[:2])


# the checker -------------------------------------------------------------------------------------------------------------------
def _checked(c: S.Case, b: int, defect):
    ref = S.case_reference(c, b)
    dev = S.case_reference(c, b, defect=defect)
    cs = slice(b * c.beam, (b + 1) * c.beam)
    return S.check_step(dev, ref, c.G[cs], c.phi[cs], c.finished[cs], c.K, c.pad, c.eos, S.MARGIN)


def _u1_case() -> S.Case:
    """A root step whose first uniform word has its 23 leading bits set (seed found by search): a mapping that can reach 1 does."""
    c = S.kernel_case(64, 1, 5, 1.0, B=1)
    x = c.logits.copy()
    x[0, 0] = x[0, 1:].max() - 30.0          # a token that only an infinite perturbation brings into the selection
    c = c._replace(keys=np.zeros(1, np.int64), seed=18802194, pos=1, logits=x)
    assert S.uniforms(c.seed, 0, 0, 4, 1)[0] == 1 - 2.0 ** -24
    return c


def _few_finite_case() -> S.Case:
    """A root step with fewer finite children than K: the -inf children tie and the index rule alone orders them."""
    c = S.kernel_case(7, 1, 5, 1.0, B=1)
    x = c.logits.copy()
    x[0, [1, 3, 4, 6]] = -np.inf
    x[0, [0, 2, 5]] = [0.5, -0.25, 1.0]
    return c._replace(logits=x)


DEFECTS = {
    "tie_high": _few_finite_case,
    "noise_by_token": lambda: S.kernel_case(64, 5, 5, 1.0, B=1),
    "no_clamp": lambda: S.kernel_case(64, 5, 5, 1.0, B=1),
    "u_reaches_1": _u1_case,
    "finished_expanded": lambda: S.kernel_case(65, 32, 32, 1.0, B=1),
    "pad_not_end": lambda: S.kernel_case(7, 5, 5, 3.0, B=1),
    "phi_wrong_parent": lambda: S.kernel_case(64, 5, 5, 1.0, B=1),
    "order_ascending": lambda: S.kernel_case(64, 5, 5, 1.0, B=1),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_checker_flags_a_planted_defect(defect):
    c = DEFECTS[defect]()
    clean, _ = _checked(c, 0, None)
    assert clean == []
    if defect == "finished_expanded":
        assert c.finished.any()
    if defect == "pad_not_end":
        assert (S.case_reference(c, 0).token[c.finished[S.case_reference(c, 0).parent] == 0] == c.pad).any()
    bad, _ = _checked(c, 0, defect)
    assert bad, f"the checker accepts a step with the defect {defect!r}"


def test_checker_accepts_the_fp32_restatement():
    for c in (S.kernel_case(65, 5, 5, 0.5), S.kernel_case(7, 32, 32, 3.0), S.kernel_case(1024, 2, 2, 1.0)):
        for b in range(c.B):
            cs = slice(b * c.beam, (b + 1) * c.beam)
            bad, _ = S.check_step(S.case_reference(c, b, np.float32), S.case_reference(c, b), c.G[cs], c.phi[cs], c.finished[cs],
                                  c.K, c.pad, c.eos, S.MARGIN)
            assert bad == []


# Philox ------------------------------------------------------------------------------------------------------------------------
def _philox_by_hand(ctr, key):
    """Philox4x32-10 in plain Python integers, written out from the definition (Salmon et al., SC'11)."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [c0, c1, c2, c3]


def test_philox_words_and_uniform_mapping():
    # the known-answer vectors of the Random123 distribution for Philox4x32-10
    assert _philox_by_hand([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert _philox_by_hand([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # two counters of the layout: (key_lo, key_hi, 0x80000000 | k << 8 | v >> 2, pos), key (seed_lo, seed_hi); word v & 3
    seed, key = 0x0123456789ABCDEF, -5
    for k, pos, V in ((0, 1, 7), (31, 23, 1024)):
        u = S.uniforms(seed, key, k, V, pos)
        assert u.shape == (V,) and (u > 0).all() and (u < 1).all()
        for v in (0, 5, V - 1):
            w = _philox_by_hand([(key % 2 ** 64) & 0xFFFFFFFF, (key % 2 ** 64) >> 32, 0x80000000 | (k << 8) | (v >> 2), pos],
                                [seed & 0xFFFFFFFF, seed >> 32])[v & 3]
            assert u[v] == ((w >> 9) + 0.5) * 2.0 ** -23
            assert np.float32(u[v]) == u[v]                      # exact in fp32
    assert ((0 >> 9) + 0.5) * 2.0 ** -23 == 2.0 ** -24 and ((0xFFFFFFFF >> 9) + 0.5) * 2.0 ** -23 == 1 - 2.0 ** -24


# the kernel test's inputs ---------------------------------------------------------------------------------------------------------
def test_kernel_cases_keep_float64_under_the_cap_and_reproduce_the_fp32_gap():
    """Measured on these cases: max |G'_fp32 - G'_float64| over the selected well-conditioned children is below FP32_GAP = 4.0e-6
    (MARGIN = 4.0e-5), and the float64 restatement alone excuses at most EXCUSED_CAP of the ranks of any parametrisation."""
    cases = [S.kernel_case(v, beam, K, t) for v in S.KERNEL_V for beam, K in S.KERNEL_BEAM_K for t in S.KERNEL_T]
    gap = S.measure_fp32_gap(cases)
    print(f"max |G'_fp32 - G'_float64| = {gap:.3g}")
    assert gap <= S.FP32_GAP and S.MARGIN == 10 * S.FP32_GAP
    worst = 0.0
    for c in cases:
        n = sum(int(S.excused_ranks(S.case_reference(c, b), c.K, S.MARGIN).sum()) for b in range(c.B))
        worst = max(worst, n / (c.B * c.K))
        assert n <= S.EXCUSED_CAP * c.B * c.K, (c.V, c.beam, c.K, c.temperature, n)
    print(f"largest excused share of a parametrisation, float64 alone: {worst:.3f}")
