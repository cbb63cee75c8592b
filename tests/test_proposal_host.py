"""CPU checks of proposal drafts (include/ttx.h: "Proposal drafts") and of tests/util_proposal.py, the restatement k_proposal_drafts
is held to.

1  The interface: the three new entry points in the header and the binding, ``proposal`` / ``proposals`` on the speculative sampling
   generator and on nothing else.
2  Driven through util_sample_spec.run_loop and util_sample_pool.run_pool with a float64 sampler on a deterministic host model, the
   restated rule returns position-by-position sampling's rows, exactly, for perfect, shifted, edited, garbage and empty proposals:
   nothing is forced.
3  With the rows themselves as proposals the loop takes at most max_b ceil(L_b / (D + 1)) steps (L_b: the tokens row b emits, the
   ending one included), and fewer than without proposals.
4  A stand-in written as the kernel is (64 lanes, one packed integer per lane, a butterfly maximum, passes of 64 lanes over the D
   tokens) agrees with the restatement, and the checker flags each single defect planted in it.
5  What the Python layer refuses without a device.
"""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_proposal as Q
import util_sample_checks as S
import util_sample_spec as X
from test_sample_spec_host import SEED, V, host_model

import translation_transformer_amd as tta
from translation_transformer_amd import _native as N

PAD, BOS, EOS = X.PAD, X.BOS, X.EOS
ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["ttx_sample_speculative_generate_proposal", "ttx_sample_speculative_generate_pool_proposal", "ttx_debug_proposal_drafts"]


# -- 1 ----------------------------------------------------------------------------------------------------------------------------
def test_interface_is_present():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ttx.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert (N.CSRC / "ttx_proposal.hip.h") in N.HEADERS
    assert "proposal" in inspect.signature(tta.TranslationInferenceSamplingSpeculative.generate).parameters
    assert "proposals" in inspect.signature(tta.TranslationInferenceSamplingSpeculative.generate_many).parameters
    for cls in (tta.TranslationInferenceSampling, tta.TranslationInferenceGreedy, tta.TranslationInferenceGreedySpeculative,
                tta.TranslationInferenceBeamSearch, tta.TranslationInferenceBeamSearchSpeculative):
        assert "proposal" not in inspect.signature(cls.generate).parameters, cls.__name__
    assert "ttx_abi_version" in N.SYMBOLS


# -- 2 ----------------------------------------------------------------------------------------------------------------------------
N_D = (3, 4)
MAX_LEN = 24
PARAMS = [S.Params(1.0), S.Params(0.7, top_k=5, top_p=0.9), S.Params(0.0)]
KINDS = ["perfect", "shift+1", "shift-2", "sub", "ins", "del", "garbage", "empty"]


def proposals_of(want: np.ndarray, kind: str, rng) -> list:
    """One proposal (token list) per row of ``want`` [B, max_len]."""
    rows = []
    for b in range(want.shape[0]):
        t = Q.row_tokens(want[b])
        other = int(rng.integers(3, V))
        if kind == "shift+1":
            t = [other] + t
        elif kind == "shift-2":
            t = t[2:]
        elif kind in ("sub", "ins", "del"):
            t = Q.perturbed(t, kind, len(t) // 2, other)
        elif kind == "garbage":
            t = [int(x) for x in rng.integers(3, V, size=len(t))]
        elif kind == "empty":
            t = []
        rows.append(t[:MAX_LEN - 1])
    return rows


def setting(seed: int = 1, n_rows: int = 6):
    rng = np.random.default_rng(seed)
    model = host_model((["eos", "pad", "long"] * n_rows)[:n_rows])
    keys = rng.integers(-2 ** 63, 2 ** 63, n_rows, dtype=np.int64)
    return rng, model, keys


@pytest.mark.parametrize("params", PARAMS)
def test_proposed_loop_returns_sequential(params):
    rng, model, keys = setting()
    B = len(keys)
    sample = rng.integers(0, 9, B)
    want = X.sequential(B, MAX_LEN, model, keys, sample, SEED, params)
    drafts = rng.integers(3, V, size=(B, N_D[0], N_D[1]))
    for kind in KINDS:
        prop = Q.Proposals.of_rows(proposals_of(want, kind, rng), ld=MAX_LEN)
        s = Q.run_loop(drafts, MAX_LEN, model, keys, sample, SEED, params, prop)
        d = U.first_difference(s.out, want)
        assert d is None, f"{params} {kind}: {d}"
        assert s.words["error"] == 0 and s.words["n_active"] == 0
        if kind != "empty" and kind != "garbage":
            assert s.words["accepted"] > 0, kind


@pytest.mark.parametrize("n", [1, 2])
def test_proposed_pool_returns_sequential(n):
    rng, model, keys = setting(seed=2)
    S_total, params = len(keys), S.Params(1.0)
    want = X.sequential(S_total * n, MAX_LEN, lambda r, prefix: model(r // n, prefix), np.repeat(keys, n),
                        np.tile(np.arange(n), S_total), SEED, params)
    drafts = rng.integers(3, V, size=(S_total, N_D[0], N_D[1]))
    for kind in ("perfect", "ins", "garbage", "empty"):
        prop = Q.Proposals.of_rows(proposals_of(want[::n], kind, rng), ld=MAX_LEN)       # sample 0's row: shared by the source's samples
        for C_ in (n, 2 * n + 1, S_total * n):
            out = Q.run_pool(drafts, keys, n, C_, MAX_LEN, model, SEED, params, prop, sub_chunk=2 if C_ > n else 0)
            d = U.first_difference(out, want)
            assert d is None, f"n {n} {kind} capacity {C_}: {d}"


# -- 3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_,D,ctx", [(1, 1, 4), (3, 4, 4), (2, 5, 2), (1, 3, 8), (2, 7, 4)])
def test_perfect_proposals_meet_the_step_bound(N_, D, ctx):
    rng, model, keys = setting(seed=D)
    B = len(keys)
    sample = np.zeros(B, dtype=np.int64)
    want = X.sequential(B, MAX_LEN, model, keys, sample, SEED, S.Params(1.0))
    emitted = S.ends(want, PAD, EOS)                    # column of the last token a row emits = the tokens it emits
    bound = int(max(-(-int(L) // (D + 1)) for L in emitted))
    drafts = rng.integers(3, V, size=(B, N_, D))
    steps, plain = [], []
    prop = Q.Proposals.of_rows([Q.row_tokens(r) for r in want], ld=MAX_LEN)
    s = Q.run_loop(drafts, MAX_LEN, model, keys, sample, SEED, S.Params(1.0), prop, steps=steps, ctx=ctx)
    none = Q.Proposals.of_rows([[] for _ in range(B)], ld=MAX_LEN)
    t = Q.run_loop(drafts, MAX_LEN, model, keys, sample, SEED, S.Params(1.0), none, steps=plain, ctx=ctx)
    assert U.first_difference(s.out, want) is None and U.first_difference(t.out, want) is None
    assert len(steps) == s.words["steps"] <= bound, (len(steps), bound)
    assert len(steps) < len(plain)


# -- 4 ----------------------------------------------------------------------------------------------------------------------------
DEFECTS = ["tie-order", "tie-sign", "eos-in-draft", "writes-draft-1", "inactive-written", "bos-off-by-one", "no-fallback",
           "ineligible-chosen"]


def standin(defect=None):
    """k_proposal_drafts as it is written: one wave per slot; lane l holds shift l - 32, counts its agreement, packs (count, tie
    order, lane) into one integer, the wave takes the maximum over a butterfly, and lane l of every pass of 64 stores token
    pass * 64 + l."""
    def fn(drafts, draft0, act_idx, n_active, front, gen, prop, src_of, ctx=Q.CTX, bos=BOS, eos=EOS, pad=PAD, repl=Q.REPL):
        out = np.array(drafts, copy=True)
        B, N_, D = out.shape
        slots = range(B) if defect == "inactive-written" else range(n_active)
        for slot in slots:
            b = int(act_idx[slot])
            f, s = int(front[b]), int(src_of[b])
            q, length = prop.table[s], int(prop.length[s])
            keys = []
            for lane in range(64):
                d = lane - 32
                c = 0
                for a in range(ctx):
                    gi, qi = f - a, f - 1 - a + d
                    lo = 0 if defect == "bos-off-by-one" else -1
                    if gi >= 0 and lo <= qi < length:
                        c += int((bos if qi < 0 else int(q[qi])) == int(gen[b, gi]))
                ok = c >= 1 and (defect == "ineligible-chosen" or 0 <= f + d < length)
                rank = 2 * abs(d) + (1 if d < 0 else 0)
                if defect == "tie-order":
                    rank = 127 - rank                      # the larger |d| wins a tie
                if defect == "tie-sign":
                    rank = 2 * abs(d) + (1 if d > 0 else 0)
                keys.append(((c << 16) | ((127 - rank) << 8) | lane) if ok else 0)
            o = 32
            while o:                                       # the butterfly: every lane ends with the maximum
                keys = [max(keys[l], keys[l ^ o]) for l in range(64)]
                o >>= 1
            key = keys[0]
            base = f + (key & 0xff) - 32 if key else length
            for p0 in range(0, D, 64):
                for lane in range(64):
                    j = p0 + lane
                    if j >= D:
                        continue
                    i = base + j
                    if 0 <= i < length:
                        t = int(q[i])
                        if t in (eos, pad) and defect != "eos-in-draft":
                            t = repl
                    elif defect == "no-fallback":
                        t = int(out[b, 0, j])
                    else:
                        t = int(draft0[b, j])
                    out[b, 0, j] = t
                    if defect == "writes-draft-1" and N_ > 1:
                        out[b, 1, j] = t
        return out
    return fn


def single_step_cases():
    """Constructed states of one launch.  Structured rows: fronts 0, 1, len - 1, len and beyond; shifts 0, +1, -1, -32, +31 and one
    outside the window; a substitution inside the context; EOS inside; no proposal; an inactive slot.  Random rows over a three-token
    alphabet, where counts tie in every order."""
    out = []
    for N_, D in [(1, 1), (3, 4), (2, 70)]:
        rng = np.random.default_rng(N_ * 7 + D)
        ld = 80
        base = [int(t) for t in rng.permutation(np.arange(3, 63))]       # the rows' tokens behind BOS, all different: no chance agreement
        rows = []                                                         # (front, proposal)
        for f in (0, 1, 29, 30, 35):
            rows.append((f, base[:30]))                                   # len 30: fronts 0, 1, len - 1, len, beyond
        for shift in (1, -1, -32, 31, 33, -33):                           # proposal = the row moved by `shift` (row token i at q[i + shift])
            q = ([int(t) for t in rng.integers(70, 80, size=shift)] + base) if shift > 0 else base[-shift:]
            rows.append((40, q[:ld - 1]))
        sub = list(base)
        sub[38] = 99                                                      # a substitution two tokens before the front
        rows.append((40, sub))
        eos_in = list(base[:45])
        eos_in[42] = EOS
        rows.append((40, eos_in))
        rows.append((12, []))
        rows.append((5, list(base[:20])))                                 # this slot is left inactive
        B = len(rows)
        gen = np.full((B, 64 + D), PAD, dtype=np.int64)
        gen[:, 0] = BOS
        gen[:, 1:61] = base
        front = np.array([f for f, _ in rows])
        prop = Q.Proposals.of_rows([q for _, q in rows], ld=ld)
        drafts = rng.integers(3, 40, size=(B, N_, D))
        draft0 = rng.integers(3, 40, size=(B, D))
        act = np.concatenate([rng.permutation(B - 1), [B - 1]])
        out.append((f"N{N_}-D{D}", drafts, draft0, act, B - 1, front, gen, prop, np.arange(B)))
    rng = np.random.default_rng(99)
    B, D = 160, 3
    gen = rng.integers(3, 6, size=(B, 20))
    gen[:, 0] = BOS
    front = rng.integers(0, 16, size=B)
    prop = Q.Proposals(rng.integers(3, 6, size=(B, 20)), rng.integers(0, 21, size=B))
    out.append(("ties", rng.integers(6, 40, size=(B, 2, D)), rng.integers(6, 40, size=(B, D)), rng.permutation(B), B, front, gen, prop,
                np.arange(B)))
    return out


def checker(drafts_fn) -> list:
    """What an implementation of the rule is held to, on the host: its rewrite against the restatement on the constructed cases
    (with sentinels where nothing may be written), and the step bound of perfect proposals.  Returns the findings."""
    found = []
    for name, drafts, draft0, act, n_active, front, gen, prop, src_of in single_step_cases():
        for ctx in (2, 4, 8):
            got = drafts_fn(drafts, draft0, act, n_active, front, gen, prop, src_of, ctx=ctx)
            want = Q.proposal_drafts(drafts, draft0, act, n_active, front, gen, prop, src_of, ctx=ctx)
            d = U.first_difference(got, want)
            if d is not None:
                found.append(f"drafts {name} ctx {ctx}: {d}")
            if np.isin(got[act[:n_active], 0], (EOS, PAD)).any():
                found.append(f"drafts {name} ctx {ctx}: EOS or PAD inside a draft")
    rng, model, keys = setting(seed=5)
    B = len(keys)
    sample = np.zeros(B, dtype=np.int64)
    want = X.sequential(B, MAX_LEN, model, keys, sample, SEED, S.Params(1.0))
    steps = []
    prop = Q.Proposals.of_rows([Q.row_tokens(r) for r in want], ld=MAX_LEN)
    s = Q.run_loop(rng.integers(3, V, size=(B, N_D[0], N_D[1])), MAX_LEN, model, keys, sample, SEED, S.Params(1.0), prop,
                   drafts_fn=drafts_fn, steps=steps)
    if U.first_difference(s.out, want) is not None:
        found.append("loop: a row changed")
    if len(steps) > max(-(-int(L) // (N_D[1] + 1)) for L in S.ends(want, PAD, EOS)):
        found.append(f"loop: {len(steps)} steps with perfect proposals")
    return found


def test_cases_cover_what_they_claim():
    """The structured rows select the shifts they were built for (or none), and the random rows hold ties of both kinds."""
    name, drafts, draft0, act, n_active, front, gen, prop, src_of = single_step_cases()[1]
    chosen = [Q.choose_shift(gen[b], int(front[b]), prop.table[b], int(prop.length[b])) for b in range(len(front))]
    assert chosen[:5] == [0, 0, 0, None, None]
    assert chosen[5:11] == [1, -1, -32, 31, None, None]
    assert chosen[11] == 0 and chosen[12] == 0 and chosen[13] is None
    name, drafts, draft0, act, n_active, front, gen, prop, src_of = single_step_cases()[-1]
    sign_ties = size_ties = 0
    for b in range(len(front)):
        f, q, L = int(front[b]), prop.table[b], int(prop.length[b])
        d = Q.choose_shift(gen[b], f, q, L)
        if d is None:
            continue
        c = Q.agreement(gen[b], f, q, L, d)
        same = [e for e in Q.SHIFTS if e != d and 0 <= f + e < L and Q.agreement(gen[b], f, q, L, e) == c]
        sign_ties += int(-d in same and d != 0)
        size_ties += int(any(abs(e) > abs(d) for e in same))
    assert sign_ties >= 2 and size_ties >= 5


def test_standin_agrees_with_the_restatement():
    assert checker(standin()) == []
    assert checker(Q.proposal_drafts) == []


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_defect_is_flagged(defect):
    assert checker(standin(defect)), f"{defect}: not flagged"


def test_rule_is_idempotent_and_equal_rows_select_shift_zero():
    name, drafts, draft0, act, n_active, front, gen, prop, src_of = single_step_cases()[1]
    once = Q.proposal_drafts(drafts, draft0, act, n_active, front, gen, prop, src_of)
    assert np.array_equal(Q.proposal_drafts(once, draft0, act, n_active, front, gen, prop, src_of), once)
    rng = np.random.default_rng(4)
    for ctx in (2, 4, 8):
        for _ in range(50):
            g = [BOS] + [int(t) for t in rng.integers(3, 5, size=30)]     # two tokens: every other shift agrees somewhere
            f = int(rng.integers(0, 30))
            assert Q.choose_shift(g, f, g[1:], 30, ctx) == 0


# -- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_python_refusals_need_no_device():
    # the refusals below come before anything touches the model
    g = tta.TranslationInferenceSamplingSpeculative.__new__(tta.TranslationInferenceSamplingSpeculative)
    with pytest.raises(ValueError, match="not both"):
        g.generate(torch.zeros((1, 3), dtype=torch.int64), prefix=torch.tensor([[5]]), proposal=torch.tensor([[5]]))
    with pytest.raises(ValueError, match="not both"):
        g.generate_many([torch.zeros((1, 3), dtype=torch.int64)], prefixes=[None], proposals=[None])
    for cls in (tta.TranslationInferenceGreedy, tta.TranslationInferenceGreedySpeculative, tta.TranslationInferenceBeamSearch):
        with pytest.raises(TypeError):
            cls.generate(object(), torch.zeros((1, 3), dtype=torch.int64), proposal=torch.tensor([[5]]))
