"""CPU checks of what the sampling tests stand on (tests/util_sample_checks.py): Philox4x32-10 against known answers, the
uniform's range, the checker against a float64 sampler and against stand-ins that break the rule one way each,
scoring.unique_samples on hand-made rows, and the header / binding / library agreeing on the two new entry points."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import util_sample_checks as S

ROOT = Path(__file__).resolve().parent.parent


# -- Philox ------------------------------------------------------------------------------------------------------------------
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(w) for w in S.philox4x32_10(ctr, key)) == want


def test_philox_is_elementwise():
    ctr = np.array([k[0] for k in KNOWN], dtype=np.uint64)
    key = np.array([k[1] for k in KNOWN], dtype=np.uint64)
    assert S.philox4x32_10(ctr, key).tolist() == [list(k[2]) for k in KNOWN]


def test_uniform_range_and_words():
    u = S.uniform(7, np.arange(5000), 3, 11)
    assert u.shape == (5000,) and (u >= 0).all() and (u < 1).all()
    assert (u * 2.0 ** 24 == np.floor(u * 2.0 ** 24)).all() and (u.astype(np.float32).astype(np.float64) == u).all()
    assert 0.45 < u.mean() < 0.55
    # the words go where the rule puts them: key (seed_lo, seed_hi), counter (key_lo, key_hi, sample, pos)
    seed, key = 0x299f31d0a4093822, 0x85a308d3243f6a88
    assert S.uniform(seed, key, 0x13198a2e, 0x03707344) == (0xd16cfe09 >> 8) * 2.0 ** -24
    assert S.uniform(seed, key - (1 << 64), 0x13198a2e, 0x03707344) == (0xd16cfe09 >> 8) * 2.0 ** -24     # an int64 key's bits
    # the largest word gives the largest u, still below 1, and fp32 holds it
    top = (0xffffffff >> 8) * 2.0 ** -24
    assert top < 1.0 and float(np.float32(top)) == top


# -- the checker -------------------------------------------------------------------------------------------------------------
V, ROWS, TOL = 97, 2000, 1e-4


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(20260101)
    x = (2.0 * rng.standard_normal((ROWS, V))).astype(np.float32)
    x[:, 5] = -np.inf                                  # a column that may never be emitted
    x[np.arange(ROWS), rng.integers(6, V, ROWS)] = -np.inf
    u = S.uniform(1234, np.arange(ROWS), 0, 9)
    return x, u


CASES = [S.Params(1.0), S.Params(0.5), S.Params(3.0), S.Params(1.0, top_k=1), S.Params(1.0, top_k=2), S.Params(0.5, top_k=32),
         S.Params(1.0, top_p=0.5), S.Params(3.0, top_p=0.9975), S.Params(0.0), S.Params(2.0, top_k=5, top_p=0.8)]


def failures(tokens, x, u, p):
    return sum(not S.consistent(t, x[r], u[r], p, TOL) for r, t in enumerate(tokens))


@pytest.mark.parametrize("p", CASES)
def test_checker_accepts_float64_sampler(rows, p):
    x, u = rows
    tokens = [S.sample64(x[r], u[r], p) for r in range(ROWS)]
    assert failures(tokens, x, u, p) == 0
    assert all(np.isfinite(x[r, t]) for r, t in enumerate(tokens))
    if p.temperature and not p.filtered:
        assert len(set(tokens)) > V // 2               # it does sample


def test_kept_set_is_the_nucleus_rule(rows):
    """The restated kept set against mask_with_num_logits_according_nucleus written out with a full sort."""
    x, _ = rows
    for r in range(50):
        for p in (S.Params(1.0, top_p=0.5), S.Params(3.0, top_p=0.9975), S.Params(1.0, top_k=7, top_p=0.9)):
            y = torch.from_numpy(S.scaled(x[r], p.temperature))
            sy, si = torch.sort(y, descending=True, stable=True)
            cum = torch.roll(torch.cumsum(sy.softmax(-1), -1), 1)
            cum[0] = p.top_p - 1
            keep = cum < p.top_p
            keep[p.keep_cap:] = False
            assert S.cdf_orders(y.numpy(), p)[0].tolist() == si[keep].tolist()


def stand_ins(x, u, p):
    """name -> (tokens, the parameters the checker holds them to)."""
    other_pos = S.uniform(1234, np.arange(ROWS), 0, 10)
    other_smp = S.uniform(1234, np.arange(ROWS), 1, 9)
    flt = S.Params(1.0, top_k=2)
    out = {
        "always argmax": ([S.argmax_first(x[r]) for r in range(ROWS)], p),
        "u of the wrong position": ([S.sample64(x[r], other_pos[r], p) for r in range(ROWS)], p),
        "u of the wrong sample id": ([S.sample64(x[r], other_smp[r], p) for r in range(ROWS)], p),
        "descending-id CDF": ([V - 1 - S.sample64(x[r, ::-1], u[r], p) for r in range(ROWS)], p),
        "temperature ignored": ([S.sample64(x[r], u[r], p) for r in range(ROWS)], S.Params(0.25)),
        "filter ignored": ([S.sample64(x[r], u[r], p) for r in range(ROWS)], flt),
        "a -inf token emitted": ([5] * ROWS, p),
    }
    return out


@pytest.mark.parametrize("name", ["always argmax", "u of the wrong position", "u of the wrong sample id", "descending-id CDF",
                                  "temperature ignored", "filter ignored", "a -inf token emitted"])
def test_checker_flags_stand_in(rows, name):
    x, u = rows
    tokens, held_to = stand_ins(x, u, S.Params(1.0))[name]
    bad = failures(tokens, x, u, held_to)
    print(f"{name}: {bad} of {ROWS} rows flagged")
    assert bad > ROWS // 2, f"{name}: only {bad} of {ROWS} rows flagged"


def test_boundary_within_tol_admits_both_sets():
    x = np.log(np.array([0.5, 0.3, 0.2])).astype(np.float64)
    p = S.Params(1.0, top_p=0.5)                       # the mass above rank 1 is 0.5 up to rounding: the boundary itself
    assert sorted(len(o) for o in S.cdf_orders(x, p, 1e-4)) == [1, 2]
    assert S.consistent(0, x, 0.9, p, 1e-4) and S.consistent(1, x, 0.9, p, 1e-4) and not S.consistent(2, x, 0.9, p, 1e-4)
    q = S.Params(1.0, top_p=0.6)
    assert [len(o) for o in S.cdf_orders(x, q, 1e-4)] == [2]
    assert not S.consistent(0, x, 0.9, q, 1e-4) and S.consistent(1, x, 0.9, q, 1e-4)


def test_chi_square_bar():
    assert abs(S.chi2_sf(S.CHI2_11_Q1E6, 11) / 1e-6 - 1) < 1e-3
    assert abs(S.chi2_sf(19.675, 11) - 0.05) < 1e-4   # a textbook value of the same function


def test_ends():
    rows = np.array([[1, 5, 2, 0, 0], [1, 5, 0, 7, 2], [1, 5, 6, 7, 8], [1, 2, 2, 2, 2]])
    assert S.ends(rows, 0, 2).tolist() == [2, 2, 4, 1]


# -- unique_samples ----------------------------------------------------------------------------------------------------------
def test_unique_samples():
    from translation_transformer_amd.scoring import unique_samples
    s = torch.tensor([[[1, 5, 6, 2, 0], [1, 5, 7, 2, 0], [1, 5, 6, 2, 9], [1, 5, 6, 6, 2], [1, 5, 7, 2, 0]],
                      [[1, 2, 0, 0, 0], [1, 2, 0, 0, 0], [1, 2, 0, 0, 0], [1, 4, 0, 0, 0], [1, 4, 0, 0, 0]]])
    sc = torch.tensor([[-1.0, -0.5, -1.0, -3.0, -0.5], [-0.1, -0.1, -0.1, -9.0, -9.0]])
    out = unique_samples(s, sc)
    assert [[(t.tolist(), c, v) for t, c, v in per] for per in out] == [
        [([1, 5, 7, 2, 0], 2, -0.5), ([1, 5, 6, 2, 0], 2, -1.0), ([1, 5, 6, 6, 2], 1, -3.0)],
        [([1, 2, 0, 0, 0], 3, pytest.approx(-0.1)), ([1, 4, 0, 0, 0], 2, -9.0)]]
    assert sum(c for _, c, _ in out[0]) == 5
    # anything with a .score works, and the EOS id is the caller's
    class Sc:
        score = sc
    assert [c for _, c, _ in unique_samples(s, Sc)[0]] == [2, 2, 1]
    assert [c for _, c, _ in unique_samples(s[:1], sc[:1], eos=7)[0]] == [2, 1, 1, 1]   # ending at 7, rows 0 and 2 differ in column 4
    with pytest.raises(ValueError):
        unique_samples(s, sc[:, :4])


# -- the ABI -----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_sampling():
    import ctypes as C
    import translation_transformer_amd as tta
    from translation_transformer_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ttx.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(ttx_[a-z_]+)\s*\(", text))
    lib = tta.lib()
    for name in ("ttx_sample_generate", "ttx_debug_sample"):
        assert name in declared and name in N.SYMBOLS and hasattr(lib, name), name
    assert len(N.SYMBOLS["ttx_sample_generate"][1]) == 9 and len(N.SYMBOLS["ttx_debug_sample"][1]) == 12
    assert C.sizeof(N.SampleParams) == 8 * 4 + 8 and N.SampleParams.seed.offset == 32
    assert C.sizeof(N.GenParams) == 8 * 4 and lib.ttx_abi_version() == 4             # additive: nothing else moved
    assert (N.CSRC / "ttx_sample.hip.h") in N.HEADERS
    assert tta.TranslationInferenceSampling is not None
