"""CPU checks of forced target prefixes (include/ttx.h: "Forced target prefixes") and of tests/util_prefix.py, the restatement the
prefix kernels are held to.

1  The interface: the six new entry points in the header and the binding, ``prefix`` / ``prefixes`` on the three Python calls.
2  Driven through util_sample_spec.run_loop and util_sample_pool.run_pool with a float64 sampler on a host model, the restated
   k_prefix_drafts and forced position return util_sample_spec.sequential's rows with the same positions forced, exactly, for
   prefixes of length 0, 1, D, D + 1, D + 2, max_len - 1 and one with an EOS inside.
3  With every row prompted over max_len - 1 tokens the loop takes ceil((max_len - 1) / (D + 1)) steps: every step commits D + 1
   columns until the front reaches max_len - 1.
4  A stand-in written as the kernels are (a wave's passes of 64 lanes over a slot's D tokens; one wave-uniform branch per step row)
   agrees with the restatement, and the checker flags each single defect planted in it.
5  What the Python layer refuses without a device.
"""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_prefix as F
import util_sample_checks as S
import util_sample_spec as X
from test_sample_spec_host import SEED, V, host_model, planted_drafts

import translation_transformer_amd as tta
from translation_transformer_amd import _native as N
from translation_transformer_amd import decoding as D_

PAD, BOS, EOS = X.PAD, X.BOS, X.EOS
ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["ttx_sample_generate_prefix", "ttx_sample_speculative_generate_prefix", "ttx_sample_speculative_generate_pool_prefix",
               "ttx_debug_prefix_drafts", "ttx_debug_sample_prefix", "ttx_debug_sample_step_prefix"]


# -- 1 ----------------------------------------------------------------------------------------------------------------------------
def test_interface_is_present():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ttx.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert "prefix" in inspect.signature(tta.TranslationInferenceSampling.generate).parameters
    assert "prefix" in inspect.signature(tta.TranslationInferenceSamplingSpeculative.generate).parameters
    assert "prefixes" in inspect.signature(tta.TranslationInferenceSamplingSpeculative.generate_many).parameters
    for cls in (tta.TranslationInferenceGreedy, tta.TranslationInferenceGreedySpeculative, tta.TranslationInferenceBeamSearch,
                tta.TranslationInferenceBeamSearchSpeculative):
        assert "prefix" not in inspect.signature(cls.generate).parameters, cls.__name__


# -- 2 ----------------------------------------------------------------------------------------------------------------------------
N_D = (3, 4)
MAX_LEN = 14
PARAMS = [S.Params(1.0), S.Params(0.7, top_k=5, top_p=0.9), S.Params(0.0)]


def prefix_rows(D: int, max_len: int, rng) -> list:
    """Prefixes of length 0, 1, D, D + 1, D + 2, max_len - 1, and one of D + 3 tokens with an EOS at its third place; tokens that
    a host model row would not need to emit by itself (they are forced)."""
    rows = [list(rng.integers(3, V, size=n)) for n in (0, 1, D, D + 1, D + 2, max_len - 1)]
    inside = list(rng.integers(3, V, size=D + 3))
    inside[2] = EOS
    return [[int(t) for t in r] for r in rows + [inside]]


def setting(n: int = 1, seed: int = 1):
    rng = np.random.default_rng(seed)
    rows = prefix_rows(N_D[1], MAX_LEN, rng)
    S_total = len(rows)
    pre = F.Prefixes.of_rows(rows, ld=MAX_LEN)
    model = host_model((["eos", "pad", "long"] * S_total)[:S_total])
    keys = rng.integers(-2 ** 63, 2 ** 63, S_total, dtype=np.int64)
    return rng, rows, pre, model, keys


@pytest.mark.parametrize("params", PARAMS)
def test_prompted_loop_returns_sequential_with_the_positions_forced(params):
    rng, rows, pre, model, keys = setting()
    B = len(rows)
    sample = rng.integers(0, 9, B)
    want = F.sequential(B, MAX_LEN, model, keys, sample, SEED, params, pre)
    for b, r in enumerate(rows):                     # the forced part is there, and a forced EOS ended its row
        cut = r.index(EOS) + 1 if EOS in r else len(r)
        assert want[b, 1:1 + cut].tolist() == r[:cut]
        if EOS in r:
            assert (want[b, 1 + cut:] == PAD).all()
    free = X.sequential(B, MAX_LEN, model, keys, sample, SEED, params)
    assert np.array_equal(want[0], free[0]) and not np.array_equal(want[2], free[2])       # length 0: the unprompted row
    s = F.run_loop(planted_drafts(want, N_D[0], N_D[1], rng), MAX_LEN, model, keys, sample, SEED, params, pre)
    d = U.first_difference(s.out, want)
    assert d is None, f"{params}: {d}"
    assert s.words["accepted"] > 0 and s.words["error"] == 0 and s.words["n_active"] == 0


@pytest.mark.parametrize("n", [1, 2])
def test_prompted_pool_returns_sequential_with_the_positions_forced(n):
    rng, rows, pre, model, keys = setting(seed=2)
    S_total, params = len(rows), S.Params(1.0)
    want = F.sequential(S_total * n, MAX_LEN, lambda r, prefix: model(r // n, prefix), np.repeat(keys, n),
                        np.tile(np.arange(n), S_total), SEED, params, pre, src_of_row=lambda r: r // n)
    drafts = planted_drafts(want[::n], N_D[0], N_D[1], rng)
    for C_ in (n, 2 * n + 1, S_total * n):
        for sub in (0, 2):
            out = F.run_pool(drafts, keys, n, C_, MAX_LEN, model, SEED, params, pre, sub_chunk=sub)
            d = U.first_difference(out, want)
            assert d is None, f"n {n} capacity {C_} sub-chunk {sub}: {d}"
    if n > 1:                                        # the samples of a source share its prefix and differ behind it
        assert np.array_equal(want[2 * n, :2], want[2 * n + 1, :2]) and len({tuple(r) for r in want[:n].tolist()}) > 1


# -- 3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_,D,max_len", [(1, 1, 12), (3, 4, 14), (2, 5, 21), (1, 3, 17), (2, 4, 16)])
def test_full_length_prefixes_take_the_fewest_steps(N_, D, max_len):
    rng = np.random.default_rng(D)
    B = 5
    rows = [[int(t) for t in rng.integers(3, V, size=max_len - 1)] for _ in range(B)]
    pre = F.Prefixes.of_rows(rows)
    model = host_model(["long"] * B)
    key, sample = rng.integers(0, 2 ** 40, B), np.zeros(B, dtype=np.int64)
    steps = []
    s = F.run_loop(rng.integers(3, V, size=(B, N_, D)), max_len, model, key, sample, SEED, S.Params(1.0), pre, steps=steps)
    assert s.out[:, 1:].tolist() == rows and (s.out[:, 0] == BOS).all()
    assert len(steps) == s.words["steps"] == -(-(max_len - 1) // (D + 1))
    assert s.words["accepted"] >= B * ((max_len - 1) // (D + 1)) * D


# -- 4 ----------------------------------------------------------------------------------------------------------------------------
DEFECTS = ["not-restored", "off-by-one", "eos-in-draft", "drawn-from-logits", "by-slot"]


def standin_drafts(defect=None):
    """k_prefix_drafts as it is written: one wave per slot, lane l of every pass of 64 owns token j = pass * 64 + l."""
    def fn(drafts, draft0, act_idx, n_active, front, pre, src_of, eos=EOS, pad=PAD, repl=F.REPL):
        out = np.array(drafts, copy=True)
        D = out.shape[2]
        for slot in range(n_active):
            b = int(act_idx[slot])
            f = int(front[b])
            s = int(src_of[slot if defect == "by-slot" else b])
            plen = int(pre.length[s]) - (1 if defect == "off-by-one" else 0)
            for base in range(0, D, 64):
                for lane in range(64):
                    j = base + lane
                    if j >= D:
                        continue
                    c = f + 1 + j
                    if c <= plen:
                        t = int(pre.table[s, c - 1])
                        if t in (eos, pad) and defect != "eos-in-draft":
                            t = repl
                    elif defect == "not-restored":
                        t = int(out[b, 0, j])
                    else:
                        t = int(draft0[b, j])
                    out[b, 0, j] = t
        return out
    return fn


def standin_force(defect=None):
    """The forced position as k_sample_step has it: one wave-uniform branch per step row."""
    def fn(pred, b, pos, pre, src_of, V_=None):
        out = np.array(pred, copy=True)
        for i in range(len(b)):
            s = int(src_of[int(b[i])])
            plen = int(pre.length[s]) - (1 if defect == "off-by-one" else 0)
            if pos[i] <= plen and defect != "drawn-from-logits":
                out[i] = pre.token(s, int(pos[i]), V_)
        return out
    return fn


def single_step_cases():
    """Constructed states of one k_prefix_drafts launch: fronts and lengths that put the window wholly inside the prefix, across
    its end, at it and beyond it; no prefix; EOS and PAD inside; two rows of one source; a compacted active list."""
    out = []
    for N_, D in [(1, 1), (3, 4), (2, 70)]:
        rng = np.random.default_rng(N_ * 7 + D)
        B, n_sources, ld = 6, 4, 3 * D + 8
        length = np.array([2 * D + 3, 0, D + 1, ld])
        table = rng.integers(3, 40, size=(n_sources, ld))
        table[0, 1], table[0, D + 1], table[2, 0] = EOS, PAD, EOS
        src_of = np.array([0, 1, 2, 0, 3, 2])
        front = np.array([0, 0, D + 1, D + 4, 2, 1])         # inside, none, f == plen, straddling, inside (long), straddling
        drafts = rng.integers(3, 40, size=(B, N_, D))
        draft0 = rng.integers(3, 40, size=(B, D))
        act = np.array([4, 0, 3, 2, 5, 1])
        out.append((f"N{N_}-D{D}", drafts, draft0, act, 5, front, F.Prefixes(table, length), src_of))
    return out


def checker(drafts_fn, force_fn) -> list:
    """What a prompted implementation is held to, on the host: its draft rewrite against the restatement on the constructed
    single-step cases, and the loop it drives against position-by-position sampling.  Returns the findings (empty: passes)."""
    found = []
    for name, drafts, draft0, act, n_active, front, pre, src_of in single_step_cases():
        got = drafts_fn(drafts, draft0, act, n_active, front, pre, src_of)
        want = F.prefix_drafts(drafts, draft0, act, n_active, front, pre, src_of)
        d = U.first_difference(got, want)
        if d is not None:
            found.append(f"drafts {name}: {d}")
        if np.isin(got[act[:n_active], 0], (EOS, PAD)).any():
            found.append(f"drafts {name}: EOS or PAD inside a draft")
    rng, rows, pre, model, keys = setting(seed=5)
    B = len(rows)
    sample = np.zeros(B, dtype=np.int64)
    want = F.sequential(B, MAX_LEN, model, keys, sample, SEED, S.Params(1.0), pre)
    s = F.run_loop(planted_drafts(want, N_D[0], N_D[1], rng), MAX_LEN, model, keys, sample, SEED, S.Params(1.0), pre,
                   drafts_fn=drafts_fn, force_fn=force_fn)
    d = U.first_difference(s.out, want)
    if d is not None:
        found.append(f"loop: {d}")
    return found


def test_standin_agrees_with_the_restatement():
    assert checker(standin_drafts(), standin_force()) == []
    assert checker(F.prefix_drafts, F.force_pred) == []


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_defect_is_flagged(defect):
    found = checker(standin_drafts(defect), standin_force(defect))
    assert found, f"{defect}: not flagged"


def test_prefix_by_slot_is_flagged_in_the_pool():
    rng, rows, pre, model, keys = setting(seed=6)
    S_total = len(rows)
    want = F.sequential(S_total, MAX_LEN, model, keys, np.zeros(S_total, dtype=np.int64), SEED, S.Params(1.0), pre)
    drafts = planted_drafts(want, N_D[0], N_D[1], rng)
    assert U.first_difference(F.run_pool(drafts, keys, 1, 3, MAX_LEN, model, SEED, S.Params(1.0), pre), want) is None
    assert U.first_difference(F.run_pool(drafts, keys, 1, 3, MAX_LEN, model, SEED, S.Params(1.0), pre, by_slot=True), want) is not None


# -- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_check_prefix_lengths_and_refusals():
    p, lens = D_.check_prefix(torch.tensor([[5, 6, 0, 0], [0, 0, 0, 0], [7, 8, 9, 4]]), 3, 10, 0, 30)
    assert lens == [2, 0, 4] and p.dtype == torch.int64 and p.device.type == "cpu"
    assert D_.check_prefix(None, 3, 10, 0, 30) == (None, None)
    assert D_.check_prefix(torch.zeros((2, 0), dtype=torch.int64), 2, 10, 0, 30)[1] == [0, 0]
    assert D_.check_prefix(torch.full((1, 9), 3), 1, 10, 0, 30)[1] == [9]                  # max_len - 1 fits
    for bad, B in [(torch.tensor([[5, 0, 6]]), 1),                                        # a token after a PAD
                   (torch.tensor([[30, 0, 0]]), 1), (torch.tensor([[-1, 0, 0]]), 1),      # outside the vocabulary
                   (torch.full((1, 10), 3), 1),                                           # longer than max_len - 1
                   (torch.tensor([[5, 6]]), 2),                                           # one row for two sources
                   (torch.tensor([5, 6]), 2), (torch.tensor([[0.5, 1.0]]), 1)]:           # not an integer matrix
        with pytest.raises(ValueError):
            D_.check_prefix(bad, B, 10, 0, 30)
