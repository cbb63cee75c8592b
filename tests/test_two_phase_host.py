"""CPU checks of the two-phase verify step's restatement (tests/util_two_phase.py), which tests/test_gpu_two_phase.py holds the
kernels to.

  merged == full   k_accept's specification (util_loop_checks.accept_step) reaches the same state from the merged prediction array
                   (probe predictions, draft-pass predictions of the matching slots, filler elsewhere) as from the predictions of
                   the step run in one pass: 2 000 seeded cases, D = 1 and N = 1 included, finishing and PAD-writing rows among them
  the split tells  a stand-in that tests draft 0 only, one that lists the matches in reverse and one that leaves the count stale
                   from a correct one
  the schedule     pool_schedule reproduces a hand-made run of a three-slot pool
"""
import numpy as np
import pytest

import util_loop_checks as U
import util_two_phase as T


def same_state(a: U.LoopState, b: U.LoopState) -> str | None:
    if a.words != b.words:
        return f"words differ: {[(k, a.words[k], b.words[k]) for k in a.words if a.words[k] != b.words[k]]}"
    for name in U.SLOT_ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        if (x is None) != (y is None) or (x is not None and not np.array_equal(x, y)):
            return f"{name} differs"
    return None


def random_case(i: int):
    rng = np.random.default_rng(1000 + i)
    N = 1 if i % 7 == 0 else int(rng.integers(1, 6))
    D = 1 if i % 5 == 0 else int(rng.integers(1, 12))
    B = int(rng.integers(1, 9))
    n_active = int(rng.integers(0, B + 1))
    max_len = 60
    mode = i % 3                                     # plain, per-row rule, slot pool
    fronts = rng.integers(0, max_len - D - 1, size=B)
    s = U.make_state(B, N, D, max_len, fronts, n_active=n_active, seed=i, V=12, row_rule=mode >= 1, pool=mode == 2)
    s.words["n_active"], s.words["r_rows"], s.words["m_rows"] = n_active, n_active * N, n_active * U.rps(N, D)
    if i % 2:                                        # planted accepted lengths (most slots match) ...
        pred = U.plant_random(s, rng, p_fin=0.2, p_pad=0.05)
    else:                                            # ... or random drafts and predictions over 9 tokens (a match now and then)
        pred = rng.integers(0, 12, size=B * U.rps(N, D)).astype(np.int32)
    return s, pred


def test_merged_predictions_give_the_accept_rule_the_same_state():
    n_match = n_miss = 0
    for i in range(2000):
        s, pred = random_case(i)
        n = int(s.words["n_active"])
        pred_probe, act2, pos2, pred2, words = T.two_passes(s.act_idx, s.drafts, pred, n)
        merged = T.merge_pred(pos2, pred_probe, pred2, n, s.N, s.D, np.full_like(pred, 77))
        assert words[0] == int((pos2[:n] >= 0).sum()) and words[3] == n + words[0] * U.rps(s.N, s.D)
        assert list(act2[:words[0]]) == [int(b) for b, p in zip(s.act_idx[:n], pos2[:n]) if p >= 0]
        want, got = U.accept_step(s, pred), U.accept_step(s, merged)
        d = same_state(want, got)
        assert d is None, f"case {i}: {d}"
        # a slot without a match accepts nothing and takes draft 0; a matching slot accepts at least one token
        for g in range(n):
            assert (want.rec[g, 2] >= 1) == (pos2[g] >= 0), (i, g)
            if pos2[g] < 0:
                assert want.rec[g, 1] == 0
        n_match += words[0]
        n_miss += n - words[0]
    assert n_match > 500 and n_miss > 500, (n_match, n_miss)


@pytest.mark.parametrize("defect", T.SPLIT_DEFECTS)
def test_the_split_restatement_rejects_a_defective_stand_in(defect):
    act, pred, drafts, kind = T.split_case(40, 33, 3, 10, seed=3)
    assert {"last_only", "first", "none"} <= set(kind)
    before = np.full(40, -7, dtype=np.int32)
    good = T.probe_split(act, pred, drafts, 33, before, before, 4)
    again = T.probe_split(act, pred, drafts, 33, before, before, 4)
    assert all(np.array_equal(a, b) for a, b in zip(good[:2], again[:2])) and good[2] == again[2]
    bad = T.probe_split(act, pred, drafts, 33, before, before, 4, defect=defect)
    differs = [not np.array_equal(a, b) for a, b in zip(good[:2], bad[:2])] + [good[2] != bad[2]]
    assert any(differs), defect
    assert good[2][0] >= 2 and (good[0][good[2][0]:] == -7).all() and (good[1][33:] == -7).all()


def test_pool_schedule_on_a_hand_made_run():
    # four rows through three slots: fronts after every step (-1 past the last)
    traj = np.full((4, 8), -1, dtype=np.int16)
    traj[:, 0] = 0
    traj[0, 1:4] = [1, 4, 5]                          # 3 steps, matches in its 2nd
    traj[1, 1:2] = [3]                                # 1 step, matches
    traj[2, 1:5] = [1, 2, 3, 4]                       # 4 steps, never
    traj[3, 1:3] = [1, 2]                             # admitted once a slot is free: 2 steps, never
    life, adv = T.slot_steps(traj)
    assert life.tolist() == [3, 1, 4, 2] and adv[0, :3].tolist() == [1, 3, 1]
    assert T.pool_schedule(traj, 3) == [(3, 1), (3, 1), (3, 0), (1, 0)]
    assert T.pool_schedule(traj, 64) == [(4, 1), (3, 1), (2, 0), (1, 0)]
