"""CPU-side checks of the per-source logit bias: the NumPy restatement (tests/util_logit_bias.py) on hand-made cases, its checker
against planted defects of a stand-in for the kernel, the pure argument check and the two allow-list helpers of scoring.py.
No device is needed."""
import numpy as np
import pytest
import torch

import util_logit_bias as L
from util_models import fixture_tokens, PAD, EOS

INF = np.inf


# -- the restatement on hand-made cases ---------------------------------------------------------------------------------------------
def test_rule_by_hand():
    x = np.array([[1.0, -0.0, 2.5, -INF, 0.0], [3.0, 3.0, 3.0, 3.0, 3.0]], dtype=np.float32)
    b = np.array([[0.5, 0.0, -INF, 8.0, -0.0], [-8.0, 1.0, 0.0, -0.0, 2.0]], dtype=np.float32)
    out = L.apply(x, b, [1, 0])
    assert L.first_difference(out, np.array([[-7.0, 1.0, 2.5, -INF, 2.0], [3.5, 3.0, -INF, 11.0, 3.0]], dtype=np.float32)) is None
    # a zero entry (either sign) leaves the BITS: the -0.0 logit under a +0.0 bias keeps its sign, where an add would give +0.0
    out = L.apply(x, b, [0, 1])
    assert np.signbit(out[0, 1]) and not np.signbit(out[0, 4]) and out[0, 3] == -INF and out[0, 2] == -INF
    assert np.signbit(np.float32(-0.0) + np.float32(-0.0)) and not np.signbit(np.float32(-0.0) + np.float32(0.0))     # what the skip avoids
    # one rounded fp32 add: 2^24 + 1 is not representable
    big = L.apply(np.array([[16777216.0]], dtype=np.float32), np.array([[1.0]], dtype=np.float32), [0])
    assert big[0, 0] == np.float32(16777216.0)
    # a denormal entry is not zero: it is added (and is absorbed by a normal logit, kept by a zero one)
    tiny = L.apply(np.array([[1.0, -0.0]], dtype=np.float32), np.array([[1e-40, 1e-40]], dtype=np.float32), [0])
    assert tiny[0, 0] == np.float32(1.0) and tiny[0, 1] == np.float32(1e-40) and tiny[0, 1] != 0
    # dead rows keep their bits; the input is not written
    keep = x.copy()
    out = L.apply(x, b, [0, 0], m_live=1)
    assert L.first_difference(out[1:], x[1:]) is None and L.first_difference(x, keep) is None


def test_row_mappings_by_hand():
    assert L.step_rps(2, 3) == 7 and L.step_rps(1, 0) == 1
    assert L.rows_plain([2, 2, 0, 1], 4).tolist() == [2, 2, 0, 1]
    assert L.rows_plain(None, 6, 3).tolist() == [0, 0, 0, 1, 1, 1]
    act, src = np.array([2, 0, 1]), np.array([5, 6, 5])                      # slot -> decoder row -> bias row
    assert L.rows_step(act, src, 21, 2, 3).tolist() == [5] * 7 + [5] * 7 + [6] * 7
    assert L.rows_step(act, src, 3, 1, 0).tolist() == [5, 5, 6]              # the probe layout: one row per slot
    row_map = np.array([0, 1, 2, 3, 14, 18, 19, 20])                          # a compacted pass: slot 0's row 0 and draft 0, slot 2's row 0 and draft 1
    assert L.rows_step(act, src, 8, 2, 3, row_map).tolist() == [5, 5, 5, 5, 6, 6, 6, 6]
    assert L.rows_step(act, src, 8, 2, 3).tolist() == [5] * 7 + [5]          # the same eight rows read without the map: slots 0 and 1


# -- the checker against planted defects ----------------------------------------------------------------------------------------------
DEFECTS = ["neighbour_source", "applied_twice", "dead_row_written", "zero_entries_added", "tail_skipped", "row_map_ignored"]


def stand_in(x, b, act, src, N, D, row_map, m_live, defect=None):
    """What a kernel with the planted defect would leave in the logits."""
    M, V = x.shape
    rows = L.rows_step(act, src, M, N, D, None if defect == "row_map_ignored" else row_map)
    if defect == "neighbour_source":
        rows = (rows + 1) % b.shape[0]
    live = M if defect == "dead_row_written" else m_live
    out = L.apply(x, b, rows, live)
    if defect == "applied_twice":
        out = L.apply(out, b, rows, live)
    if defect == "zero_entries_added":
        with np.errstate(invalid="ignore"):
            out[:m_live] = x[:m_live] + b[rows[:m_live], :V]
    if defect == "tail_skipped":
        out[:, V - V % 4:] = x[:, V - V % 4:]
    return out


def defect_case():
    rng = np.random.default_rng(5)
    N, D, V = 2, 3, 250                                       # V % 4 == 2: a tail of two
    act, src = np.array([2, 0, 1]), np.array([0, 1, 2])
    row_map = np.array([0, 1, 2, 3, 7, 11, 12, 13, 14, 15, 16, 17], dtype=np.int64)       # 12 compacted rows of the 21 layout rows
    x, b = L.make_logits(rng, 12, V), L.make_bias(rng, 3, V)
    x[0, 1], b[0, 1], b[1, 1], b[2, 1] = -0.0, 0.0, 0.0, 0.0  # a -0.0 logit under a +0.0 bias in every source
    x[:, V - 1] = 1.0
    b[:, V - 1] = 3.0                                         # a finite pair in the tail of every row
    return x, b, act, src, N, D, row_map, 9


def test_checker_passes_the_rule_and_flags_every_defect():
    x, b, act, src, N, D, row_map, m_live = defect_case()
    rows = L.rows_step(act, src, x.shape[0], N, D, row_map)
    L.check(stand_in(x, b, act, src, N, D, row_map, m_live), x, b, rows, m_live, "the rule itself")
    for d in DEFECTS:
        with pytest.raises(AssertionError, match=r"row \d+ \((live|dead)\) token \d+"):
            L.check(stand_in(x, b, act, src, N, D, row_map, m_live, d), x, b, rows, m_live, d)


def test_checker_names_the_first_differing_entry():
    x, b, act, src, N, D, row_map, m_live = defect_case()
    rows = L.rows_step(act, src, x.shape[0], N, D, row_map)
    out = stand_in(x, b, act, src, N, D, row_map, m_live)
    out[4, 17] = np.float32(out[4, 17] + 1.0) if np.isfinite(out[4, 17]) else np.float32(0.0)
    out[6, 3] = np.float32(123.0)
    with pytest.raises(AssertionError, match=r"row 4 \(live\) token 17"):
        L.check(out, x, b, rows, m_live, "planted")
    dead = stand_in(x, b, act, src, N, D, row_map, m_live, "dead_row_written")
    with pytest.raises(AssertionError, match=r"row (9|10|11) \(dead\)"):
        L.check(dead, x, b, rows, m_live, "dead")


# -- the pure argument check ------------------------------------------------------------------------------------------------------------
def test_check_logit_bias():
    from translation_transformer_amd.scoring import check_logit_bias, combine_bias
    B, V = 3, 30
    ok = torch.zeros(B, V)
    ok[1, 4], ok[2, 7] = float("-inf"), -8.0
    out = check_logit_bias(ok, B, V)
    assert out.dtype == torch.float32 and torch.equal(out, ok) and check_logit_bias(None, B, V) is None
    assert check_logit_bias(ok.double(), B, V).dtype == torch.float32
    assert check_logit_bias(ok.numpy(), B, V).shape == (B, V)
    for bad in (torch.zeros(B, V + 1), torch.zeros(B + 1, V), torch.zeros(V), torch.zeros(B, V, 1)):
        with pytest.raises(ValueError, match="shape"):
            check_logit_bias(bad, B, V)
    for bad in (torch.zeros(B, V, dtype=torch.int64), torch.zeros(B, V, dtype=torch.bool)):
        with pytest.raises(ValueError, match="floating"):
            check_logit_bias(bad, B, V)
    for value in (float("nan"), float("inf")):
        bad = ok.clone()
        bad[2, 5] = value
        with pytest.raises(ValueError, match="source 2"):
            check_logit_bias(bad, B, V)
    # both keywords: the allow-list is added as -inf onto the bias
    allowed = torch.ones(B, V, dtype=torch.bool)
    allowed[0, 9] = False
    both = combine_bias(ok, allowed, B, V)
    assert both[0, 9] == float("-inf") and both[1, 4] == float("-inf") and both[2, 7] == -8.0 and float(both[0, 0]) == 0.0
    assert combine_bias(None, None, B, V) is None and torch.equal(combine_bias(ok, None, B, V), ok)
    with pytest.raises(ValueError):
        combine_bias(None, torch.ones(B, V + 2, dtype=torch.bool), B, V)


# -- the allow-list helpers on the fixture tokens ----------------------------------------------------------------------------------------
def test_allowlist_from_source_and_bias_from_allowed():
    from translation_transformer_amd.scoring import allowlist_from_source, bias_from_allowed
    src, _, _, V = fixture_tokens()
    always = [EOS, 4, 6, 7]
    allowed = allowlist_from_source(src, always, V, PAD)
    assert allowed.shape == (src.shape[0], V) and allowed.dtype == torch.bool
    for b in range(src.shape[0]):
        want = set(int(t) for t in src[b].tolist() if t != PAD) | set(always)
        assert set(torch.nonzero(allowed[b]).reshape(-1).tolist()) == want, f"source {b}"
    assert not bool(allowed[:, PAD].any()) and bool(allowed[:, EOS].all())
    assert bool((~allowed).any()), "every fixture source uses the whole vocabulary: the check is empty"
    bias = bias_from_allowed(allowed)
    assert bias.dtype == torch.float32 and bias.shape == allowed.shape
    assert bool((bias[allowed] == 0).all()) and bool((bias[~allowed] == float("-inf")).all())
    # ids outside the vocabulary in the source are ignored, in `always` refused
    wide = src.clone()
    wide[0, 3] = V + 5
    assert torch.equal(allowlist_from_source(wide, always, V, PAD)[1:], allowed[1:])
    with pytest.raises(ValueError):
        allowlist_from_source(src, [V], V, PAD)
    with pytest.raises(ValueError):
        bias_from_allowed(torch.zeros(3, V))
    with pytest.raises(ValueError):
        allowlist_from_source(src.float(), always, V, PAD)
