"""The checks of tests/test_gpu_gemm_kernels.py and tests/test_gpu_finish_ln.py can fail: each comparison helper of
util_gemm_checks is fed a correct fp32 result computed on the CPU, and then the same result with one defect a GEMM kernel or
the finisher could have, and must pass the first and flag the second under the check that claims to catch it.  No GPU."""
import pytest
import torch

import util_gemm_checks as G

K, N, M, M_MAX, LDY = 256, 37, 45, 48, 40


def cpu_gemm(x, w, bias, relu, y: G.Arena, live, defect=None, slice_k=64):
    """A stand-in for a kernel: the canonical slice sum in fp32 on the CPU, written into the live rows of ``y``; ``defect``
    names the one thing it gets wrong.  ``x`` is the arena view [m_max, K] whose rows >= live are NaN."""
    k_of = torch.arange(K)
    if defect == "last k pair dropped":
        k_of = k_of[:K - 2]
    elif defect == "one k used twice":
        k_of[101] = 100
    xs, ws = x[:live][:, k_of], w[:, k_of]
    if defect == "NaN leaked from a row >= M":
        xs = xs.clone()
        xs[live - 1, 7] = x[live, 7]
    tot = None
    for k0 in range(0, xs.shape[1], slice_k):
        part = xs[:, k0:k0 + slice_k] @ ws[:, k0:k0 + slice_k].T
        tot = part if tot is None else tot + part
    if bias is not None:
        tot = tot + (bias[torch.clamp(torch.arange(N) + 1, max=N - 1)] if defect == "bias of column n + 1" else bias)
    if relu:
        tot = torch.relu(tot)
    y.reset()
    y.m[:live] = tot
    if defect == "row written beyond M":
        y.m[live] = tot[live - 1]
    elif defect == "guard element overwritten":
        y.buf[G.GUARD - 1] = 0.0
    elif defect == "column written beyond N":
        y.buf[G.GUARD + N] = 1.0
    return y.m[:live].clone()


def arenas(x):
    xa = G.Arena(M_MAX, K, K + 4)
    xa.m[:M] = x[:M]
    return xa, G.Arena(M_MAX, N, LDY, fill=G.OUT_FILL)


def run_checks(kind, defect):
    """The checks of the GPU module on one stand-in launch; returns the names of the checks that flagged it."""
    gen = torch.Generator().manual_seed(5)
    flagged = []
    if kind in ("integers", "floats"):
        x, w, b = (G.int_operands if kind == "integers" else G.float_operands)(gen, M_MAX, N, K)
        xa, y = arenas(x)
        got = cpu_gemm(xa.m, w, b, True, y, M, defect)
        ref = G.gemm_ref64(x[:M], w, b, True)
        checks = [("untouched", lambda: G.check_untouched(y, M, "host"))]
        if kind == "integers":
            checks.append(("a", lambda: G.check_exact(got, ref, "host")))
        else:
            checks.append(("c", lambda: G.check_bound(got, ref, G.gemm_bound(x[:M], w, b, K), "host")))
            clean = cpu_gemm(xa.m, w, b, True, G.Arena(M_MAX, N, LDY, fill=G.OUT_FILL), M, None)
            checks.append(("d", lambda: G.check_same(got, clean, "host")))
    else:                                             # selector: X the identity, M = K rows
        w = G.scaled_normals(gen, N, K)
        xa = G.Arena(K + 3, K, K + 4)
        xa.m[:K] = torch.eye(K)
        y = G.Arena(K + 3, N, LDY, fill=G.OUT_FILL)
        got = cpu_gemm(xa.m, w, None, False, y, K, defect)
        checks = [("untouched", lambda: G.check_untouched(y, K, "host")),
                  ("b", lambda: G.check_exact(got, w.T.contiguous(), "host", bits=True))]
    for name, fn in checks:
        try:
            fn()
        except AssertionError as e:
            assert "host" in str(e)
            flagged.append(name)
    return flagged


@pytest.mark.parametrize("kind", ["integers", "floats", "selector"])
def test_a_correct_result_passes_every_check(kind):
    assert run_checks(kind, None) == []


# defect -> the checks that claim to catch it
CLAIMS = {"last k pair dropped": [("integers", "a"), ("selector", "b")],
          "one k used twice": [("integers", "a"), ("selector", "b")],
          "bias of column n + 1": [("integers", "a")],
          "row written beyond M": [("integers", "untouched"), ("floats", "untouched")],
          "guard element overwritten": [("integers", "untouched")],
          "column written beyond N": [("integers", "untouched")],
          "NaN leaked from a row >= M": [("integers", "a"), ("floats", "c"), ("floats", "d")]}


@pytest.mark.parametrize("defect", list(CLAIMS))
def test_every_defect_is_flagged_by_the_check_that_claims_it(defect):
    for kind, check in CLAIMS[defect]:
        assert check in run_checks(kind, defect), (defect, kind, check)


def test_a_dropped_k_pair_exceeds_the_float_bound_somewhere():
    """(c) is the backstop for float handling, not the indexing test — but at K = 256 a dropped pair is outside it on most elements."""
    assert "c" in run_checks("floats", "last k pair dropped")


def test_reordered_slices_break_bit_identity_only():
    """A slice sum in another order stays inside (c) and exact on integers; (d) is the check that sees it."""
    gen = torch.Generator().manual_seed(9)
    x, w, b = G.float_operands(gen, M_MAX, N, K)
    xa, y = arenas(x)
    a = cpu_gemm(xa.m, w, b, False, y, M)
    parts = [x[:M, k:k + 64] @ w[:, k:k + 64].T for k in range(0, K, 64)]
    other = ((parts[0] + parts[2]) + parts[1]) + parts[3] + b
    G.check_bound(other, G.gemm_ref64(x[:M], w, b, False), G.gemm_bound(x[:M], w, b, K), "host")
    with pytest.raises(AssertionError):
        G.check_same(other, a, "host")


# ---- finisher -----------------------------------------------------------------------------------------------------
def cpu_finish(slabs, resid, bias, g1, b1, row_valid, y: G.Arena, live, defect=None):
    order = list(range(slabs.shape[0]))
    if defect == "slabs 0 and 1 swapped":
        order[0], order[1] = 1, 0
    elif defect == "slabs 1 and 2 swapped":
        order[1], order[2] = 2, 1
    elif defect == "loop starts at slab 2":
        order.pop(1)
    pre = G.finish_pre32_in_order(slabs[order], bias, resid)
    out = G.finish_torch32(pre, g1, b1, None, None, 1e-5)
    if row_valid is not None:
        out = torch.where(row_valid[:, None] != 0, out, torch.zeros_like(out))
        if defect == "masked row not zeroed":
            out[0] = 1e-30
    y.reset()
    y.m[:live] = out
    if defect == "row written beyond M":
        y.m[live] = out[0]
    return y


def finish_case(n_slabs=9, rows=4, d=64):
    gen = torch.Generator().manual_seed(3)
    u = lambda *s: torch.rand(s, generator=gen) * 2 - 1
    return dict(slabs=G.magnitude_slabs(gen, n_slabs, rows, d), resid=u(rows, d), bias=u(d), g1=1 + 0.1 * u(d), b1=0.1 * u(d))


def finish_checks(defect, row_valid=None):
    o = finish_case()
    rows, d = o["resid"].shape
    y = cpu_finish(o["slabs"], o["resid"], o["bias"], o["g1"], o["b1"], row_valid, G.Arena(rows + 3, d, fill=G.OUT_FILL), rows, defect)
    pre32 = G.finish_pre32_in_order(o["slabs"], o["bias"], o["resid"])
    ref = G.finish_ref64(pre32, o["g1"], o["b1"], None, None, 1e-5)
    _, tol = G.finish_tolerance(G.finish_torch32(pre32, o["g1"], o["b1"], None, None, 1e-5), ref)
    keep = torch.ones(rows, dtype=torch.bool) if row_valid is None else row_valid != 0
    G.check_finish_structure(y, rows, row_valid, "host")
    G.check_finish_values(y.m[:rows][keep], ref[keep], tol, "host")
    # the case tells the slab order from the exact sum
    exact = G.finish_ref64(G.finish_pre64(o["slabs"], o["bias"], o["resid"]), o["g1"], o["b1"], None, None, 1e-5)
    assert float((y.m[:rows].to(torch.float64) - exact)[keep].abs().max()) > tol


def test_finisher_checks_pass_a_correct_result():
    finish_checks(None)
    finish_checks(None, torch.tensor([0, 1, 1, 0], dtype=torch.uint8))


@pytest.mark.parametrize("defect", ["slabs 1 and 2 swapped", "loop starts at slab 2", "row written beyond M"])
def test_finisher_defects_are_flagged(defect):
    with pytest.raises(AssertionError, match="host"):
        finish_checks(defect)


def test_masked_row_must_be_exactly_zero():
    with pytest.raises(AssertionError, match="host"):
        finish_checks("masked row not zeroed", torch.tensor([0, 1, 1, 0], dtype=torch.uint8))


def test_swapping_the_first_two_slabs_is_not_a_defect():
    """fp32 addition commutes: (s0 + s1) + s2 + ... and (s1 + s0) + s2 + ... are the same number, so no check can (or needs to)
    see slabs 0 and 1 change places; the smallest reordering that changes the sum is slabs 1 and 2 (flagged above)."""
    o = finish_case()
    a = G.finish_pre32_in_order(o["slabs"], o["bias"], o["resid"])
    b = G.finish_pre32_in_order(o["slabs"][[1, 0] + list(range(2, 9))], o["bias"], o["resid"])
    assert torch.equal(a, b)
    finish_checks("slabs 0 and 1 swapped")
