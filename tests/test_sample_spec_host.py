"""CPU checks of tests/util_sample_spec.py, the restatement the speculative-sampling kernels are held to.

1  Driven by a float64 sampler on a host model, with drafts planted from the rows the plain sampler produces, the restated loop
   returns row for row what position-by-position sampling returns: rows that end on EOS, on PAD and at max_len, with overshoots of
   1 .. D columns, while draft tokens really are accepted.
2  A stand-in written as the kernels are (scalar loops per step row and per slot) agrees with the restatement on every constructed
   case, and each single defect planted in it is flagged by the checkers.
3  The binding: the new symbols and the parameter struct.
"""
import ctypes as C

import numpy as np
import pytest

import util_loop_checks as U
import util_sample_checks as S
import util_sample_spec as X

PAD, BOS, EOS = X.PAD, X.BOS, X.EOS
V = 14
SEED = 77


# -- a host model ----------------------------------------------------------------------------------------------------------------
def host_model(kind_of_row):
    """logits(b, prefix): float64 [V] from a generator seeded by (b, prefix), so a position's logits depend on its own prefix alone.
    Rows of kind "eos" lean to EOS from length 6 on, "pad" to PAD, "long" can emit neither (they run to max_len), "const" emit
    token 7 at every position (all but surely: its logit stands 30 above the rest)."""
    def logits_of(b, prefix):
        rng = np.random.default_rng([b + 1, len(prefix)] + [int(t) + 1 for t in prefix])
        x = 1.5 * rng.standard_normal(V)
        x[BOS] = -np.inf
        kind = kind_of_row[b]
        x[EOS] = 2.5 if (kind == "eos" and len(prefix) >= 6) else -np.inf
        x[PAD] = 2.5 if (kind == "pad" and len(prefix) >= 6) else -np.inf
        if kind == "const":
            x[7] = 30.0
        return x
    return logits_of


def planted_drafts(seq: np.ndarray, N: int, D: int, rng) -> np.ndarray:
    """[B, N, D] drafts without EOS / PAD: windows of the row the plain sampler produces (so that draft tokens are accepted), one of
    them shifted by one position, the rest random; the draft order is shuffled per row."""
    B = seq.shape[0]
    drafts = rng.integers(3, V, size=(B, N, D))
    for b in range(B):
        body = seq[b][(seq[b] != PAD) & (seq[b] != EOS) & (seq[b] != BOS)]
        for n in rng.permutation(N)[:max(1, N - 1)]:
            if len(body) >= D:
                at = int(rng.integers(0, len(body) - D + 1))
                drafts[b, n] = body[at:at + D]
    return drafts


CASES = [(1, 1, 12), (1, 3, 17), (3, 2, 16), (2, 5, 21), (3, 4, 9)]


@pytest.mark.parametrize("N,D,max_len", CASES)
@pytest.mark.parametrize("params", [S.Params(1.0), S.Params(0.7, top_k=5, top_p=0.9), S.Params(0.0)])
def test_loop_returns_the_plain_samplers_rows(N, D, max_len, params):
    rng = np.random.default_rng(N * 100 + D)
    kinds = ["eos", "pad", "long"] * 4
    B = len(kinds)
    model = host_model(kinds)
    key = rng.integers(-2 ** 63, 2 ** 63, B, dtype=np.int64)          # high key words too
    sample = rng.integers(0, 9, B)
    want = X.sequential(B, max_len, model, key, sample, SEED, params)
    end = S.ends(want, PAD, EOS)
    last = want[np.arange(B), end]
    assert (last == EOS).any() and (last == PAD).any() and (~np.isin(last, (EOS, PAD))).any(), "a kind of ending is missing"
    s = X.run_loop(planted_drafts(want, N, D, rng), max_len, model, key, sample, SEED, params)
    d = U.first_difference(s.out, want)
    assert d is None, f"N {N} D {D} max_len {max_len} {params}: {d}"
    w = s.words
    assert w["accepted"] > 0 and w["steps"] < int(end.max()), "no draft token was accepted: the loop went position by position"
    assert w["produced"] - w["accepted"] == w["verified_positions"] // U.rps(N, D) and w["n_active"] == 0 and w["error"] == 0
    # every front of a row that ended at max_len: max_len - 1 exactly or beyond it by up to D columns
    over = s.front[~np.isin(last, (EOS, PAD))] - (max_len - 1)
    assert (over >= 0).all() and (over <= D).all()


def test_overshoots_of_every_size_occur():
    """Rows that run to max_len whose last step lands 1 .. D columns beyond max_len - 1: the dropped columns do not reach the output,
    and an ending token in a dropped column does not end the row early (the output still equals the plain sampler's)."""
    N, D = 2, 4
    seen = set()
    kinds = ["const", "eos"] * 3
    model = host_model(kinds)
    key, sample = np.arange(6, dtype=np.int64) + (1 << 40), np.zeros(6, dtype=np.int64)
    for max_len in range(8, 8 + D + 1):
        rng = np.random.default_rng(max_len)
        drafts = rng.integers(3, V, size=(6, N, D))
        drafts[::2, 1] = 7                          # the second draft of a "const" row is accepted whole at every step
        s = X.run_loop(drafts, max_len, model, key, sample, SEED, S.Params(1.0))
        want = X.sequential(6, max_len, model, key, sample, SEED, S.Params(1.0))
        assert (want[::2, 1:] == 7).all() and U.first_difference(s.out, want) is None
        assert (s.front[::2] % (D + 1) == 0).all()  # D + 1 tokens per step
        seen |= set((s.front[::2] - (max_len - 1)).tolist())
    assert seen == set(range(0, D + 1)), f"overshoots seen: {sorted(seen)}"


# -- a stand-in written as the kernels are, and its defects -------------------------------------------------------------------------
def standin_rows(act_idx, front, n_active, N, D, defect=None):
    R = U.rps(N, D)
    b = np.zeros(n_active * R, dtype=np.int64)
    pos = np.zeros(n_active * R, dtype=np.int64)
    for row in range(n_active * R):
        slot, rs = divmod(row, R)
        br = slot if defect == "key-by-slot" else int(act_idx[slot])
        f = int(front[int(act_idx[slot])])
        b[row] = br
        pos[row] = f + 1 if rs == 0 else f + 2 + (rs - 1) % D - (1 if defect == "pos-off-by-one" else 0)
    return b, pos


def standin_accept(state, pred, defect=None):
    s = state.clone()
    w = s.words
    w.update(dict.fromkeys(U.WORDS[13:], -1))
    Bc = int(w["n_active"])
    if Bc == 0:
        return s
    N, D, R = s.N, s.D, U.rps(s.N, s.D)
    kept, maxf, acc_sum, f_sum = [], 0, 0, 0
    for slot in range(Bc):
        b = int(s.act_idx[slot])
        f = int(s.front[b])
        ps = pred[slot * R:(slot + 1) * R]
        best, bacc = 0, -1
        for n in range(N):
            acc = 0
            while acc < D and s.drafts[b, n, acc] == (ps[0] if acc == 0 else ps[n * D + acc]):
                acc += 1
            if acc > bacc or (defect == "last-draft-wins" and acc == bacc):
                best, bacc = n, acc
        fin = False
        for j in range(bacc + 1):
            t = ps[0] if j == 0 else ps[best * D + j]
            s.gen[b, f + 1 + j] = t
            ending = (t == s.eos) or (t == s.pad and defect != "pad-does-not-end")
            fin |= bool(ending and f + 1 + j < s.max_len)
        nf = f + bacc + 1
        fin |= nf >= s.max_len - 1
        s.front[b] = nf
        s.rec[slot] = [b, best, bacc, f, int(fin)]
        if fin:
            s.out[b, :s.max_len] = s.gen[b, :s.max_len]
            if defect == "copies-past-max-len" and nf >= s.max_len:
                s.out[b, s.max_len - 1] = s.gen[b, nf]           # a token of a dropped column reaches the output's last column
        if not fin or defect == "retired-row-stays":
            kept.append(b)
        maxf, acc_sum, f_sum = max(maxf, f), acc_sum + bacc, f_sum + f
    nn = len(kept)
    s.act_idx[:nn] = kept
    w["n_copy"] = Bc
    w["steps"] += 1
    w["accepted"] += acc_sum
    w["produced"] += acc_sum + Bc
    w["verified_positions"] += Bc * R
    w["kv_prefix_positions"] += f_sum
    w["src_positions"] += Bc * s.Ls
    w["width"] = maxf + D + 2
    w["stop"] = int(nn == 0)
    w["n_active"], w["r_rows"], w["m_rows"] = nn, nn * N, nn * R
    w["host_width"], w["host_n_active"], w["host_stop"], w["host_steps_done"] = w["width"], nn, w["stop"], w["steps"]
    return s


STEP_DEFECTS = ["pad-does-not-end", "last-draft-wins", "copies-past-max-len", "retired-row-stays"]
ROW_DEFECTS = ["pos-off-by-one", "key-by-slot"]
_CASES = {}


def cases():
    if not _CASES:
        _CASES.update({n: (s, p) for n, s, p in X.accept_cases()})
    return _CASES


def test_case_names_are_complete():
    assert sorted(cases()) == sorted(X.ACCEPT_CASE_NAMES)


@pytest.mark.parametrize("name", X.ACCEPT_CASE_NAMES)
def test_standin_agrees_with_the_restatement(name):
    s, pred = cases()[name]
    want = X.sample_accept_step(s, pred)
    X.check_state(standin_accept(s, pred), want, name)
    n = s.words["n_active"]
    fin = int(want.rec[:n, 4].sum())
    # the case is what its name says
    if name.startswith("lengths-"):
        assert {int(a) for a in want.rec[:n, 2]} == set(range(s.D + 1)) and (s.N == 1 or len(set(want.rec[:n, 1])) == s.N)
    if name.startswith("ending-"):
        assert 0 < fin < n and {PAD, EOS} <= {int(want.gen[b, f]) for b, f in zip(want.rec[:n, 0], want.front[want.rec[:n, 0]])}
    if name.startswith("limit-"):
        over = want.front[want.rec[:n, 0]] - (s.max_len - 1)
        assert set(range(-1, s.D + 1)) <= set(over.tolist()) and (want.rec[:n, 4] == (over >= 0) | (want.rec[:n, 4] == 1)).all()
        assert ((over < 0) & (want.rec[:n, 4] == 0)).any() and ((over < 0) & (want.rec[:n, 4] == 1)).any()
    if name.startswith(("retire-", "B1-")):
        assert want.words["stop"] == int(fin == n)
        assert (want.act_idx[:n - fin] == [b for b, fl in zip(want.rec[:n, 0], want.rec[:n, 4]) if not fl]).all()


def flagged(fn) -> bool:
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("defect", STEP_DEFECTS)
def test_accept_checker_flags_each_defect(defect):
    hits = []
    for name, (s, pred) in cases().items():
        want = X.sample_accept_step(s, pred)
        if flagged(lambda: X.check_state(standin_accept(s, pred, defect), want, name)):
            hits.append(name)
    assert hits, f"no case flags the defect {defect}"
    print(f"{defect}: flagged by {len(hits)} of {len(cases())} cases")


@pytest.mark.parametrize("defect", ROW_DEFECTS)
def test_row_mapping_checker_flags_each_defect(defect):
    rng = np.random.default_rng(4)
    for N, D in X.ND:
        B, n_active = 5, 3
        act = rng.permutation(B).astype(np.int32)
        while (act[:n_active] == np.arange(n_active)).all():
            act = rng.permutation(B).astype(np.int32)
        front = rng.permutation(20)[:B].astype(np.int32)              # distinct fronts
        b, pos = X.step_rows(act, front, n_active, N, D)
        gb, gp = standin_rows(act, front, n_active, N, D)
        assert U.first_difference(gb, b) is None and U.first_difference(gp, pos) is None
        gb, gp = standin_rows(act, front, n_active, N, D, defect)
        assert U.first_difference(gb, b) is not None or U.first_difference(gp, pos) is not None, f"N {N} D {D}: {defect} not seen"


@pytest.mark.parametrize("defect", ROW_DEFECTS)
def test_the_loop_sees_a_wrong_row_mapping(defect):
    """The same defects through the whole loop: its rows stop being the plain sampler's."""
    N, D, max_len = 3, 2, 16
    rng = np.random.default_rng(9)
    kinds = ["eos", "pad", "long"] * 2
    model = host_model(kinds)
    key, sample = rng.integers(-2 ** 63, 2 ** 63, 6, dtype=np.int64), np.arange(6)
    want = X.sequential(6, max_len, model, key, sample, SEED, S.Params(1.0))
    drafts = planted_drafts(want, N, D, rng)
    bad = X.run_loop(drafts, max_len, model, key, sample, SEED, S.Params(1.0),
                     rows_fn=lambda a, f, n, N_, D_: standin_rows(a, f, n, N_, D_, defect))
    assert U.first_difference(bad.out, want) is not None


# -- the binding -----------------------------------------------------------------------------------------------------------------
def test_symbols_and_struct():
    from translation_transformer_amd import _native as N
    import translation_transformer_amd as tta
    assert C.sizeof(N.SampleSpecParams) == C.sizeof(N.SampleParams) + 4 * 4
    assert N.SampleSpecParams.draft_len.offset == C.sizeof(N.SampleParams)
    assert len(N.SYMBOLS["ttx_sample_speculative_generate"][1]) == 9
    assert len(N.SYMBOLS["ttx_debug_sample_step"][1]) == 15 and len(N.SYMBOLS["ttx_debug_sample_accept"][1]) == 4
    lib = tta.lib()
    for name in ("ttx_sample_speculative_generate", "ttx_debug_sample_step", "ttx_debug_sample_accept"):
        assert hasattr(lib, name)
    with pytest.raises(TypeError):
        tta.TranslationInferenceSamplingSpeculative(object(), 16, 4, 3, PAD, BOS, EOS, 5)
