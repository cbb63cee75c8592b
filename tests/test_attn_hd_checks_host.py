"""The checks of tests/test_gpu_attn_hd64.py can fail (no GPU): a CPU stand-in that evaluates each case in fp32 passes them,
and the same stand-in with ONE defect of the kind a head-dimension port can have fails them:

  first_32_dims          the q k^T contraction stops after the first 32 dims of a head
  upper_half_unwritten   dims 32 .. 63 of every head of the output are never stored
  upper_half_copied      dims 32 .. 63 of the output repeat dims 0 .. 31
  head_offset_32         head h is read at column 32 h instead of 64 h
  next_head_v            the values come from the next head

Also here: util_attn_hd at head dimension 32 is util_attn_checks (same operands from the same seeds, same reference), the
step visibility rules agree at the grid's shapes, and the ``upper`` distribution is what it says."""
import pytest
import torch

import util_attn_checks as A
import util_attn_hd as AH

DH = 64


def _cases():
    slots = [dict(f=33, src=33), dict(f=0, src=1, front_pad=True), dict(f=65, src=70, prefix_pads=True)]
    out = []
    for i, dist in enumerate(AH.DISTS):
        out.append(AH.full_case(DH, AH.ENC, 33, 0, 3, H=2, dist=dist, seed=i))
        out.append(AH.full_case(DH, AH.FULL_SELF, 17, 0, 1, H=4, dist=dist, seed=10 + i))
        out.append(AH.full_case(DH, AH.FULL_CROSS, 3, 65, 3, H=2, dist=dist, seed=20 + i, shared_mem=bool(i % 2)))
        out.append(AH.step_case(DH, AH.STEP_SELF, 3, 10, slots, H=2, dist=dist, seed=30 + i, extra_groups=1, cache_slot=bool(i % 2)))
        out.append(AH.step_case(DH, AH.STEP_CROSS, 4, 3, slots, H=2, dist=dist, seed=40 + i, src_of=bool(i % 2), src_len=not i % 2))
    return out


CASES = _cases()


def checks(out, case, what):
    AH.check_structure(out, case, what)
    AH.check_values(out.m[:case.live_rows], case, what)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_a_correct_standin_passes(case):
    checks(AH.standin(case), case, case.name)


@pytest.mark.parametrize("defect", AH.DEFECTS)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_each_defect_is_caught(case, defect):
    with pytest.raises(AssertionError):
        checks(AH.standin(case, defect), case, f"{case.name} with {defect}")


def test_upper_distribution_uses_only_the_upper_dims():
    for case in [c for c in CASES if c.dist == "upper"]:
        low = (torch.arange(case.d) % DH) < 32
        for t in (case.q, case.k, case.kcache):
            if t is not None:
                v = t[..., low]
                assert bool(((v == 0) | torch.isnan(v)).all()) and bool((t[..., ~low][~torch.isnan(t[..., ~low])] != 0).any())
        half, _, _ = AH.evaluate(case, torch.float64, defect="first_32_dims")
        ref = AH.reference(case)["ref"]
        assert float((half - ref).abs().max()) > 1e3 * AH.reference(case)["tol"]


def test_head_dimension_32_is_util_attn_checks():
    """The restated builders and rule at dh = 32 give util_attn_checks' operands and reference bit for bit."""
    slots = A.grid_slots(3, 4)
    pairs = [(AH.full_case(32, A.ENC, 33, 0, 3, H=4, dist="ascending", seed=5), A.full_case(A.ENC, 33, 0, 3, H=4, dist="ascending", seed=5)),
             (AH.full_case(32, A.FULL_CROSS, 3, 65, 3, H=4, dist="offset", seed=6, shared_mem=True),
              A.full_case(A.FULL_CROSS, 3, 65, 3, H=4, dist="offset", seed=6, shared_mem=True)),
             (AH.step_case(32, A.STEP_SELF, 3, 10, slots, H=4, dist="descending", seed=7, cache_slot=True),
              A.step_case(A.STEP_SELF, 3, 10, slots, H=4, dist="descending", seed=7, cache_slot=True)),
             (AH.step_case(32, A.STEP_CROSS, 7, 10, slots, H=4, dist="peaked", seed=8, src_len=True),
              A.step_case(A.STEP_CROSS, 7, 10, slots, H=4, dist="peaked", seed=8, src_len=True))]
    for mine, theirs in pairs:
        for name in ("q", "k", "v", "kcache", "vcache", "tok", "key_pad"):
            a, b = getattr(mine, name), getattr(theirs, name)
            assert (a is None) == (b is None)
            if a is not None:
                assert torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0)), (mine.name, name)
        ra, rb = AH.reference(mine), A.reference(theirs)
        assert torch.equal(ra["ref"], rb["ref"]) and ra["tol"] == rb["tol"] and ra["e32"] == rb["e32"]


def test_step_rules_agree():
    real = torch.ones(300, dtype=torch.bool)
    real[3] = False
    for N, D in [(1, 0), (1, 1), (3, 10), (7, 10), (64, 1), (4, 3)]:
        for f in (0, 1, 33):
            assert torch.equal(AH.step_visibility_direct(N, D, f, real, True), AH.step_visibility_expanded(N, D, f, real, True))
