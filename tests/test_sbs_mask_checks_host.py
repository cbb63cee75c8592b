"""CPU checks of the masked stochastic-beam-search test tools (tests/util_sbs_mask_checks.py): under a top-k filter, and under a
filter and a forced prefix, the float64 restatement samples without replacement from the filtered / conditional distribution of an
enumerable model; a full mask is the unmasked restatement; K nests; top_k = 1 is the argmax path; the checker flags planted defects;
the kernel test's inputs keep float64 alone under half the excused cap and reproduce the recorded fp32 gap."""
from types import SimpleNamespace

import numpy as np
import pytest

import util_sample_checks as P
import util_sbs_checks as S
import util_sbs_mask_checks as M
from util_sbs_checks import LEVEL, chi2_p

V, DEPTH, BOS = 5, 3, 0
NONE = -1                     # pad / eos of the toy model: no token ends a row, so every sequence has DEPTH tokens
N_KEYS = 20000
SEED = 20190611
TOP_K = 3
PREFIX = (3,)


@pytest.fixture(scope="module")
def toy():
    """test_sbs_checks_host.py's toy model widened to V = 5, its sequence probabilities under top_k = 3 (kept sets renormalised), and
    the restatement's K = 2 searches for N_KEYS keys, free and under the one-token prefix (shared by the tests; never modified)."""
    rng = np.random.default_rng(7)
    tables = {}
    for d in range(DEPTH):
        for idx in np.ndindex(*(V,) * d):
            tables[idx] = rng.uniform(-1.0, 1.0, V).astype(np.float32)

    def model(rows):
        return np.stack([tables[tuple(int(t) for t in r[1:])] for r in rows])
    seqs = list(np.ndindex(*(V,) * DEPTH))
    prm = P.Params(1.0, TOP_K, 1.0)
    p, p_cond = np.ones(len(seqs)), np.ones(len(seqs))
    for i, s in enumerate(seqs):
        for d in range(DEPTH):
            t = tables[s[:d]].astype(np.float64)
            keep, _ = M.kept(t, prm)
            q = np.exp(t[s[d]]) / np.exp(t[keep]).sum() if keep[s[d]] else 0.0
            p[i] *= q
            # a forced token costs nothing and need not be kept by the filter (PREFIX[0] is not, in this model)
            p_cond[i] *= (1.0 if s[0] == PREFIX[0] else 0.0) if d == 0 else q
    assert abs(p.sum() - 1) < 1e-12 and (p > 0).sum() == TOP_K ** DEPTH
    assert abs(p_cond.sum() - 1) < 1e-12 and (p_cond > 0).sum() == TOP_K ** (DEPTH - 1)
    index = {s: i for i, s in enumerate(seqs)}

    def run(prefix):
        ids = np.zeros((N_KEYS, 2), dtype=np.int64)
        logp, gum = np.zeros((N_KEYS, 2)), np.zeros((N_KEYS, 2))
        for key in range(N_KEYS):
            rows, ph, g, _, _ = M.search(model, key, SEED, 1.0, 2, DEPTH + 1, NONE, BOS, NONE, TOP_K, 1.0, prefix)
            ids[key] = [index[tuple(int(t) for t in r[1:])] for r in rows]
            logp[key], gum[key] = ph, g
        return SimpleNamespace(ids=ids, logp=logp, gumbel=gum)
    return SimpleNamespace(model=model, p=p, p_cond=p_cond, free=run(()), prompted=run(PREFIX))


def _first_row(run, p):
    counts = np.bincount(run.ids[:, 0], minlength=len(p)).astype(np.float64)
    assert (counts[p == 0] == 0).all(), "a masked sequence was drawn"
    assert chi2_p(counts[p > 0], p[p > 0]) > LEVEL
    assert np.allclose(run.logp[:, 0], np.log(p[run.ids[:, 0]]), atol=1e-9)
    assert (run.gumbel[:, 0] == 0).all()


def _first_two_rows(run, p):
    n = len(p)
    a, b = run.ids[:, 0], run.ids[:, 1]
    assert (a != b).all()
    counts = np.bincount(a * n + b, minlength=n * n).astype(np.float64).reshape(n, n)
    probs = p[:, None] * p[None, :] / (1 - p[:, None])
    off = ~np.eye(n, dtype=bool) & (probs > 0)
    assert abs(probs[off].sum() - 1) < 1e-12 and counts[~off].sum() == 0
    assert chi2_p(counts[off], probs[off]) > LEVEL


def test_first_row_is_distributed_as_the_filtered_model(toy):
    _first_row(toy.free, toy.p)


def test_first_two_rows_are_a_sample_without_replacement_from_the_filtered_model(toy):
    _first_two_rows(toy.free, toy.p)


def test_under_a_prefix_both_hold_for_the_conditional_distribution(toy):
    _first_row(toy.prompted, toy.p_cond)
    _first_two_rows(toy.prompted, toy.p_cond)


def test_a_full_mask_is_the_unmasked_restatement(toy):
    """top_k = 32 >= V with top_p = 1 keeps every token: rows, phi and G of the masked search are the unmasked search's, bit for
    bit; so is one step of a kernel case with V = 7."""
    for key in range(40):
        a = M.search(toy.model, key, SEED, 1.0, 4, DEPTH + 1, NONE, BOS, NONE, 32, 1.0)
        b = S.search(toy.model, key, SEED, 1.0, 4, DEPTH + 1, NONE, BOS, NONE)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    mc = M.kernel_case(7, 5, 5, 3.0, 32, 1.0)
    for b in range(mc.c.B):
        m, s = M.case_reference(mc, b)[0], S.case_reference(mc.c, b)
        assert np.array_equal(m.order, s.order) and m.img_g.tobytes() == s.img_g.tobytes() and m.img_phi.tobytes() == s.img_phi.tobytes()


def test_k_is_the_first_k_of_k_plus_2(toy):
    for prefix in ((), PREFIX):
        for key in range(40):
            rows, ph, g, fin, _ = M.search(toy.model, key, SEED, 1.0, 2, DEPTH + 1, NONE, BOS, NONE, TOP_K, 1.0, prefix)
            big = M.search(toy.model, key, SEED, 1.0, 4, DEPTH + 1, NONE, BOS, NONE, TOP_K, 1.0, prefix)
            assert np.array_equal(rows, big[0][:2])
            assert ph.tobytes() == big[1][:2].tobytes() and g.tobytes() == big[2][:2].tobytes()
            if prefix:
                assert (big[0][:, 1] == prefix[0]).all() and len({tuple(r) for r in big[0].tolist()}) == 4


def test_top_k_1_is_the_argmax_path(toy):
    want = [BOS]
    for _ in range(DEPTH):
        want.append(int(np.argmax(toy.model(np.array([want]))[0])))
    for key in range(10):
        rows, ph, g, fin, _ = M.search(toy.model, key, SEED, 1.0, 3, DEPTH + 1, NONE, BOS, NONE, 1, 1.0)
        assert rows[0].tolist() == want and ph[0] == 0.0 and g[0] == 0.0
        assert np.isneginf(ph[1:]).all() and np.isneginf(g[1:]).all() and fin[1:].all()


# the checker -------------------------------------------------------------------------------------------------------------------
def _checked(mc: M.MaskCase, b: int, defect):
    c = mc.c
    ref, flip = M.case_reference(mc, b, tol=M.KEPT_TOL)
    dev, _ = M.case_reference(mc, b, defect=defect)
    cs = slice(b * c.beam, (b + 1) * c.beam)
    return M.check_step(dev, ref, flip, c.G[cs], c.phi[cs], c.finished[cs], c.K, c.pad, c.eos, M.MARGIN)


DEFECT_CASES = {
    "kept_off_by_one": lambda: (M.kernel_case(65, 5, 5, 3.0, 5, 1.0), 0),
    "noise_by_kept_rank": lambda: (M.kernel_case(65, 5, 5, 3.0, 5, 1.0), 0),
    "lp_not_renormalised": lambda: (M.kernel_case(65, 5, 5, 3.0, 5, 1.0), 0),
    "prefix_lp_added": lambda: (M.forced_case(65, 5, 5, (7, 70)), 0),
    "forced_noise": lambda: (M.forced_case(65, 5, 5, (7, 70)), 2),
    "masked_child_emitted": lambda: (M.kernel_case(65, 1, 5, 3.0, 32, 0.9), 0),
}


def test_every_defect_has_a_case():
    assert sorted(DEFECT_CASES) == sorted(M.DEFECTS)


@pytest.mark.parametrize("defect", sorted(DEFECT_CASES))
def test_checker_flags_a_planted_defect(defect):
    mc, b = DEFECT_CASES[defect]()
    clean, _ = _checked(mc, b, None)
    assert clean == []
    bad, _ = _checked(mc, b, defect)
    assert bad, f"the checker accepts a step with the defect {defect!r}"


def test_checker_accepts_the_fp32_restatement():
    for mc in (M.kernel_case(65, 5, 5, 0.5, 5, 1.0), M.kernel_case(7, 32, 32, 3.0, 32, 0.9), M.kernel_case(1024, 5, 5, 3.0, 0, 0.5),
               M.forced_case(256, 5, 5, (2, -1), 5, 1.0)):
        c = mc.c
        for b in range(c.B):
            cs = slice(b * c.beam, (b + 1) * c.beam)
            ref, flip = M.case_reference(mc, b, tol=M.KEPT_TOL)
            bad, _ = M.check_step(M.case_reference(mc, b, np.float32)[0], ref, flip, c.G[cs], c.phi[cs], c.finished[cs], c.K, c.pad,
                                  c.eos, M.MARGIN)
            assert bad == []


def test_forced_steps_carry_phi_and_g_and_spend_no_noise():
    mc = M.forced_case(65, 5, 5, (2, 70))                       # 2 is EOS; 70 lies outside [0, 65) and is read as 0
    c = mc.c
    for b, tok in ((0, 2), (2, 0)):
        st, _ = M.case_reference(mc, b)
        cs = slice(b * c.beam, (b + 1) * c.beam)
        live = np.nonzero(c.finished[cs] == 0)[0]
        finite = np.isfinite(st.g)
        mine = finite & np.isin(st.parent, live)
        assert sorted(st.parent[mine].tolist()) == live.tolist() and (st.token[mine] == tok).all()
        assert (st.g[mine] == c.G[cs][st.parent[mine]]).all() and (st.phi[mine] == c.phi[cs][st.parent[mine]]).all()
        assert st.finished[mine].all() == (tok in (c.eos, c.pad))
        assert not finite.all() and st.finished[~finite].all() and np.isneginf(st.phi[~finite]).all()
        other = M.step(np.full((c.beam, c.V), np.nan, np.float32), c.phi[cs], c.G[cs], c.finished[cs] != 0, 99, c.pos, 1, 7.0, c.K,
                       c.pad, c.eos, forced=mc.forced(b))[0]                              # no logit, key, seed or temperature is read
        assert np.array_equal(other.order, st.order) and other.g.tobytes() == st.g.tobytes()
    assert mc.forced(1) is None


# the kernel test's inputs ---------------------------------------------------------------------------------------------------------
def test_kernel_cases_keep_float64_under_half_the_cap_and_reproduce_the_fp32_gap():
    """Measured on these cases: max |G'_fp32 - G'_float64| over the selected well-conditioned children stays below FP32_GAP
    (MARGIN ten times it), and the float64 restatement alone (kept-set boundaries within KEPT_TOL included) excuses at most half of
    EXCUSED_CAP of the ranks of any parametrisation."""
    from test_gpu_sample_kernel import TOL
    assert M.KEPT_TOL == TOL
    cases = M.kernel_cases()
    gap = M.measure_fp32_gap(cases)
    print(f"max |G'_fp32 - G'_float64| = {gap:.3g}")
    assert gap <= M.FP32_GAP and M.MARGIN == 10 * M.FP32_GAP
    worst = 0.0
    for mc in cases:
        n = M.float64_excused(mc)
        worst = max(worst, n / (mc.c.B * mc.c.K))
        assert 2 * n <= M.EXCUSED_CAP * mc.c.B * mc.c.K, (mc.c.V, mc.c.beam, mc.c.K, mc.c.temperature, mc.top_k, mc.top_p, n)
    print(f"largest excused share of a parametrisation, float64 alone: {worst:.4f}")
