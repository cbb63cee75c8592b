"""CPU test of tests/util_bsp_checks.py, the restatement tests/test_gpu_bsp_kernels.py holds the pool's bookkeeping kernels to.

Pooled equals per-batch: the eight restated rules, chained over a work list of 9 batches of 1 - 5 sources under several capacities
and admission schedules, leave in `out`, `summary` and `trace_len` what a per-batch loop written from the reference's scalars
leaves (both fed by the same synthetic step), with the same draft length and group width in force in every iteration, and
scheduling.replay_beam_batch derives that loop's tensor width and model calls from the arrays.
Coverage: the chains the GPU test launches reach every branch the kernel-level test is there for (util_bsp_checks.REQUIRED); a
scenario that stops reaching one fails here, not silently on the GPU.
Checkers can fail: one wrong element in any array or word of a correct State, a cache-slot map that is no permutation or hands
the parent's slot to a finished child, and one wrong element of the caller-side arrays are all caught."""
import numpy as np
import pytest

import util_beam_checks as B
import util_bsp_checks as P

HOST_CHAINS = P.CHAINS + [(sc.name, smart, 64, "eager") for sc in P.scenarios() for smart in (False, True)] + \
              [("plain", True, 5, "lazy"), ("tight", False, 5, "single"), ("raise", True, 6, "third"), ("guard", False, 6, "eager")]


@pytest.fixture(scope="module")
def runs():
    """Every chain once: (final State, log, p, w, kn, coverage)."""
    out = {}
    for key in HOST_CHAINS:
        cov = set()
        out[key] = (*P.run_chain(*key, cov=cov), cov)
    return out


@pytest.mark.parametrize("key", HOST_CHAINS, ids=lambda k: "-".join(str(v) for v in k))
def test_pooled_equals_per_batch(runs, key):
    from translation_transformer_amd.scheduling import replay_beam_batch
    S, log, p, w, kn, _ = runs[key]
    assert w.n_batches >= 8 and set(w.sizes) == {1, 2, 3, 4, 5} and p.C >= max(w.sizes)
    refs = P.check_against_per_batch(S, log, p, w, kn)
    assert not (S.a["row_of"] >= 0).any() and not (S.a["bat_id"] >= 0).any() and S.w[P.W_LIVE] == 0 and S.w[P.W_ERROR] == 0
    replayed = 0
    for r in refs:
        rows = slice(r.rows[0], r.rows[-1] + 1)
        if r.error is None and max(r.iters) > p.T_cap:
            continue                                                       # the trace was cut: the caller asked for less than the replay needs
        rep = replay_beam_batch(S.a["trace_len"][rows], S.a["summary"][rows], p.max_len, p.D0, p.K)
        assert rep.error == r.error, (r.rows, rep.error, r.error)
        if r.error is None:
            assert (rep.model_calls, rep.out_width) == (r.model_calls, r.width), (r.rows, rep, r.model_calls, r.width)
            replayed += 1
    assert replayed or p.T_cap < 10 or p.max_steps


def test_the_gpu_chains_reach_every_branch(runs):
    seen = set().union(*(runs[key][5] for key in P.CHAINS))
    missing = [c for c in P.REQUIRED if c not in seen]
    assert not missing, f"no chained scenario reaches: {missing}"
    for key in P.CHAINS:                                                   # the limits of the chained GPU runs
        p = runs[key][2]
        assert p.C <= 6 and p.K <= 5 and p.D0 <= 5 and p.Ls_cap <= 16 and p.max_len <= 24


def test_synthetic_step_ignores_the_slot():
    """The same source in another slot of another pool, among other sources: the same leaves."""
    kn = P.knobs(seed=5)
    a = P.cand_leaves(kn, 3, 4, 7, [P.BOS, 6, 9], 3, 2)
    b = P.cand_leaves(kn, 3, 4, 7, np.array([P.BOS, 6, 9], np.int32), 3, 2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = P.cand_leaves(kn, 3, 4, 7, [P.BOS, 6, 9], 2, 2)
    assert c[2].nonzero()[0].max() <= 2                                    # no leaf beyond cand_dl
    fin = P.cand_leaves(kn, 3, 4, 7, [P.BOS, 6, P.EOS], 3, 1)
    assert fin[2].tolist() == [1, 0, 0, 0, 0] and fin[3][0, 0] == P.PAD and fin[4][0, 0] == P.score_of(kn, 7, [P.BOS, 6, P.EOS])


def mid_state():
    """A State in the middle of a run (after a select), and the one before it."""
    seen = []

    def keep(op, before, after, *args):
        if op == "select" and len(seen) < 6:
            seen.append((before, after))
    P.run_chain("plain", True, 5, "eager", apply=keep)
    return seen[-1]


def test_compare_catches_one_wrong_element():
    _, S = mid_state()
    P.compare(S.a, S.w, S, "unchanged")
    for k in S.a:
        if S.a[k].size == 0:
            continue
        bad = {n: v.copy() for n, v in S.a.items()}
        flat = bad[k].reshape(-1).view(np.int32 if bad[k].dtype == np.float32 else bad[k].dtype)
        flat[flat.size // 2] ^= 1
        with pytest.raises(AssertionError):
            P.compare(bad, S.w, S, k)
    for i in range(len(S.w)):
        with pytest.raises(AssertionError):
            P.compare(S.a, S.w[:i] + [S.w[i] + 1] + S.w[i + 1:], S, f"word {i}")


def test_cache_slot_checker_catches_a_wrong_map():
    before, after = mid_state()
    P.check_cache_slots(before, after)
    K = after.p.K
    s = int(np.flatnonzero(before.a["row_of"] >= 0)[0])
    twice = after.copy()
    twice.a["cache_slot"][s * K] = twice.a["cache_slot"][s * K + 1]        # no permutation any more
    with pytest.raises(AssertionError):
        P.check_cache_slots(before, twice)
    # a parent with a running and a finished child: the finished one must not inherit
    old = [10, 11, 12]
    new, how = P.cache_slots(old, [1, 1, 0], [True, False, False])
    assert new == [12, 11, 10] and how == {"running", "spare"}
    assert P.cache_slots(old, [0, 0, 0], [True, True, True]) == ([10, 11, 12], {"finished", "spare"})
    assert P.cache_slots(old, [2, 0, 1], [False, True, False]) == ([12, 10, 11], {"running", "finished"})
    # the same on a State: one source, children of parents (1, 1, 0), child 0 finished
    pp = P.params(C=1, K=3, N=1, D0=1, Ls_cap=6, max_len=8, smart=False, T_cap=2)
    b4 = P.init(P.blank(pp, 1, 1))
    b4.a["row_of"][0] = 0
    good = b4.copy()
    good.a["parent"][:], good.a["fin_next"][:], good.a["src_state"][0] = [1, 1, 0], [1, 0, 0], P.RUNNING
    good.a["cache_slot"][:], good.a["cache_slot_parent"][:] = [2, 1, 0], [1, 1, 0]
    P.check_cache_slots(b4, good)
    for name, values in (("cache_slot", [1, 2, 0]), ("cache_slot", [2, 0, 1]), ("cache_slot_parent", [1, 0, 0])):
        bad = good.copy()
        bad.a[name][:] = values                                            # the finished child inherits; nobody inherits; a wrong source of the copy
        with pytest.raises(AssertionError):
            P.check_cache_slots(b4, bad)


def test_per_batch_checker_catches_one_wrong_element():
    S, log, p, w, kn = P.run_chain("plain", False, 5, "eager")
    P.check_against_per_batch(S, log, p, w, kn)
    for k, idx in (("out", (3, 1, 2)), ("summary", (4, 0)), ("summary", (4, 1)), ("summary", (2, 7)), ("trace_len", (5, 0))):
        bad = S.copy()
        bad.a[k][idx] += 1
        with pytest.raises(AssertionError):
            P.check_against_per_batch(bad, log, p, w, kn)
    wrong = dict(log)
    key = sorted(wrong)[3]
    wrong[key] = (wrong[key][0] + 1, wrong[key][1])
    with pytest.raises(AssertionError):
        P.check_against_per_batch(S, wrong, p, w, kn)


def test_rules_keep_the_sentinel_where_they_do_not_write():
    """init on a blank State: what it does not write (tokens, candidate rows, the step's arrays, the caller's rows) stays blank."""
    p = P.params(C=3, K=2, N=2, D0=3, Ls_cap=8, max_len=10, smart=False, T_cap=4)
    S0 = P.blank(p, 4, 2)
    S = P.init(S0)
    for k in ("tok", "drafts_all", "cand_next", "gen", "front", "len", "logp", "drafts32", "leaf_score", "leaf_tok", "leaf_cnt", "chosen",
              "chosen_slot", "out", "trace_len", "summary", "new_slot", "memkv", "src_valid"):
        B.same(S.a[k], S0.a[k], k)
    assert S.w == [0] * 12


def test_the_binding_names_the_ops_and_words_as_the_restatement_does():
    import translation_transformer_amd._native as NA
    assert NA.DEBUG_BSP_OPS == P.OPS and NA.DEBUG_BSP_WORDS == P.CNT_WORDS + P.HOST_WORDS
    assert len(NA.SYMBOLS["ttx_debug_bsp"][1]) == 5
    fields = [n for n, _ in NA.DebugBspArgs._fields_]
    p = P.params(C=2, K=2, N=1, D0=1, Ls_cap=6, max_len=8, smart=False, T_cap=2)
    arrays = set(P.shapes(p, 1, 1, 4)) | set(P.STAGED)
    assert {"d_" + k for k in arrays} == set(NA.DebugBspArgs.POINTERS), "every array of a State and of an admission is an operand"
    assert fields[len(NA.DebugBspArgs.POINTERS):] == ["C", "K", "N", "D0", "Ls_cap", "max_len", "ld", "smart", "lib_ld", "pad", "bos", "eos",
                                                      "repl", "max_steps", "T_cap", "R", "first_row", "kv_row", "Ls_new"]
