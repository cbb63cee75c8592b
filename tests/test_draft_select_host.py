"""CPU checks of draft select's restatement (tests/util_draft_select.py), which tests/test_gpu_draft_select.py holds the kernels to.

  merged == full   k_accept's specification (util_loop_checks.accept_step) reaches the same state from the predictions merged out
                   of a compacted draft pass (-1 in the rows of absent drafts) as from the 1 + N*D predictions of the step run in
                   one pass: 2 400 seeded cases with slots where two and three drafts share the matching token, ties in the
                   accepted length and EOS inside the accepted run
  the layout       row bases are the prefix sum of 1 + D * popcount(mask), the row map is a bijection onto the present layout
                   rows in (slot, row) order, and the compacted count is what the masks say
  the defects      rank computed from n instead of popcount, an absent draft's rows filled with row 0's prediction, and a row base
                   without the + 1 for row 0 are each told from the correct restatement
"""
import numpy as np
import pytest
import torch

import util_draft_select as S
import util_loop_checks as U
import util_two_phase as T
from test_two_phase_host import same_state

SENT = U.SENTINEL[torch.int32]


def select_case(i: int):
    """A seeded state and the predictions of its step in one pass, built so that most slots match with 1 .. N drafts present."""
    rng = np.random.default_rng(5000 + i)
    N = int(rng.integers(1, 6)) if i % 4 else 3
    D = 1 if i % 9 == 0 else int(rng.integers(1, 12))
    B = int(rng.integers(1, 9))
    n_active = int(rng.integers(0, B + 1))
    max_len = 60
    mode = i % 3
    s = U.make_state(B, N, D, max_len, rng.integers(0, max_len - D - 1, size=B), n_active=n_active, seed=i, V=12, row_rule=mode >= 1,
                     pool=mode == 2)
    s.words["n_active"], s.words["r_rows"], s.words["m_rows"] = n_active, n_active * N, n_active * U.rps(N, D)
    pred = U.new_pred(s)
    info = dict(two=0, three=0, ties=0, eos_inside=0)
    for slot in range(n_active):
        kind = int(rng.integers(0, 5))
        acc = rng.integers(0, D + 1, size=N)
        if kind == 0:
            acc[:] = 0                                                      # no draft matches
        elif kind == 1 and N >= 2:
            acc[:] = 0
            acc[rng.choice(N, size=2, replace=False)] = rng.integers(1, D + 1, size=2)     # exactly two drafts share the token
        elif kind == 2 and N >= 3:
            acc[:] = 0
            acc[rng.choice(N, size=3, replace=False)] = rng.integers(1, D + 1)             # three share it and tie
        present = int((acc >= 1).sum())
        best = int(acc.max())
        special = []
        if best >= 2 and rng.random() < 0.3:                                # EOS inside the accepted run of the best draft
            special.append((int(np.argmax(acc)), int(rng.integers(1, best)), U.EOS))
            info["eos_inside"] += 1
        U.plant(s, pred, slot, acc, rng, special)
        info["two"] += present == 2
        info["three"] += present >= 3
        info["ties"] += best >= 1 and int((acc == best).sum()) >= 2
    return s, pred, info


def test_merged_compacted_predictions_give_the_accept_rule_the_same_state():
    tot = dict(two=0, three=0, ties=0, eos_inside=0, absent=0, match=0, miss=0)
    for i in range(2400):
        s, pred, info = select_case(i)
        n, N, D = int(s.words["n_active"]), s.N, s.D
        R = U.rps(N, D)
        pred_probe, act2, pos2, mask, base, rmap, pred2c, words = S.two_passes_select(s.act_idx, s.drafts, pred, n)
        merged = S.merge_pred_select(pos2, pred_probe, pred2c, mask, base, n, N, D, np.full_like(pred, 77))
        want, got = U.accept_step(s, pred), U.accept_step(s, merged)
        d = same_state(want, got)
        assert d is None, f"case {i}: {d}"
        # the layout: prefix sums, the compacted count, and a row map that lists the present layout rows in order
        m = words[0]
        sizes = [S.sel_rows(int(mask[p]), D) for p in range(m)]
        assert list(base[:m]) == list(np.cumsum([0] + sizes)[:m]) and words[2] == words[7] == sum(sizes)
        assert words[3] == n + m * R
        present = [p * R + rs for p in range(m) for rs in range(R) if S.sel_row(int(mask[p]), rs, D) is not None]
        assert list(rmap[:words[2]]) == present and (rmap[words[2]:] == SENT).all()
        assert (mask[m:] == SENT).all() and (base[m:] == SENT).all()
        for g in range(n):
            p = int(pos2[g])
            if p < 0:
                continue
            # the best draft of a matching slot is a present one; an absent draft's rows are -1 and a present one's are the full ones
            assert (int(mask[p]) >> int(want.rec[g, 1])) & 1 and want.rec[g, 2] >= 1, (i, g)
            for nn in range(N):
                rows = slice(g * R + 1 + nn * D, g * R + 1 + (nn + 1) * D)
                if (int(mask[p]) >> nn) & 1:
                    assert (merged[rows] == pred[rows]).all()
                else:
                    assert (merged[rows] == S.FILLER).all()
                    tot["absent"] += 1
        for k in info:
            tot[k] += info[k]
        tot["match"] += m
        tot["miss"] += n - m
    assert min(tot.values()) > 200, tot


def defect_case():
    """Slots with masks 0b110, 0b101, 0b011, 0b111, 0b100 and 0 among the live ones of a permuted list."""
    B, N, D = 10, 3, 4
    rng = np.random.default_rng(3)
    act = rng.permutation(B).astype(np.int32)
    drafts = rng.integers(6, 40, size=(B, N, D), dtype=np.int32)
    pred_probe = np.full(B, 50, dtype=np.int32)
    for g, m in enumerate([0b110, 0b101, 0, 0b011, 0b111, 0b100, 0]):
        for n in range(N):
            if (m >> n) & 1:
                drafts[act[g], n, 0] = 50
    return act, pred_probe, drafts, 7


@pytest.mark.parametrize("defect", S.SELECT_DEFECTS)
def test_the_restatement_rejects_a_defective_stand_in(defect):
    act, pred_probe, drafts, n = defect_case()
    B, N, D = drafts.shape
    R = U.rps(N, D)
    before = {k: np.full(B * R if k == "row_map" else B, -7, dtype=np.int32) for k in ("act2", "pos2", "mask", "row_base", "row_map")}
    good = S.select_split(act, pred_probe, drafts, n, before, 4)
    again = S.select_split(act, pred_probe, drafts, n, before, 4)
    assert all(np.array_equal(a, b) for a, b in zip(good[:5], again[:5])) and good[5] == again[5]
    assert list(good[2][:5]) == [0b110, 0b101, 0b011, 0b111, 0b100] and list(good[3][:5]) == [0, 9, 18, 27, 40] and good[5][2] == 45
    bad = S.select_split(act, pred_probe, drafts, n, before, 4, defect=defect)
    pred2c = np.arange(100, 100 + B * R, dtype=np.int32)
    fill = np.full(B * R, 77, dtype=np.int32)
    merged = S.merge_pred_select(good[1], pred_probe, pred2c, good[2], good[3], n, N, D, fill)
    merged_bad = S.merge_pred_select(good[1], pred_probe, pred2c, good[2], good[3], n, N, D, fill, defect=defect)
    differs = [not np.array_equal(a, b) for a, b in zip(good[:5], bad[:5])] + [good[5] != bad[5], not np.array_equal(merged, merged_bad)]
    assert any(differs), defect
    if defect == "absent_gets_row0":
        assert differs == [False] * 6 + [True]              # the split is the same; the merge is what this defect breaks
    if defect == "base_without_row0":
        assert differs[3] and differs[5]                    # row bases and the compacted count
    if defect == "rank_from_n":
        assert differs[4] and differs[6]                    # the row map and the merge, not the bases


def test_executed_rows_on_a_hand_made_run():
    traj = np.full((2, 6), -1, dtype=np.int16)
    traj[:, 0] = 0
    traj[0, 1:4] = [1, 4, 5]
    traj[1, 1:3] = [2, 3]
    tokens = np.array([[1, 10, 11, 12, 13, 14, 2], [1, 20, 21, 22, 2, 0, 0]])
    drafts = np.zeros((2, 3, 2), dtype=np.int64)
    drafts[0, :, 0] = [11, 7, 11]                           # row 0 at front 1 predicts 11: two drafts present
    drafts[1, :, 0] = [20, 8, 9]                            # row 1 at front 0 predicts 20: one draft present
    rows, fewer, several, matched = S.executed_rows(traj, tokens, drafts)
    assert (rows, fewer, several, matched) == (5 + (1 + 2 * 2) + (1 + 2 * 1), 2, 1, 3)
