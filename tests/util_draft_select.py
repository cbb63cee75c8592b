"""Plain restatement of draft select, the third mode of the slot pool's verify step (DESIGN.md "Two-phase verify step";
csrc/ttx_loop_kernels.hip.h: k_probe_split's optional outputs, k_embed's row map, k_merge_pred and k_kvcopy on compacted rows;
csrc/ttx_attn.hip: the SEL instantiations of k_attn3 / k_attn3s).  No GPU call in here.

The rule, restated from the accept rule: a draft whose first token differs from the prediction of the slot's front row has
accepted length 0 whatever its own rows predict, so the draft pass runs, for every matching slot, row 0 and the D rows of each
draft whose first token equals that prediction.  The rows are stored compacted: slot p of the draft pass starts at row_base[p], row
0 first, then the present drafts in the order of n.

  masks_of          per live slot the bit mask of its matching drafts
  sel_row           layout row rs of a slot -> row among its compacted rows, None for a row of an absent draft
  select_split      util_two_phase.probe_split plus masks, row bases, the row map and the compacted count
  merge_pred_select the prediction array k_accept reads, from compacted draft-pass predictions
  kv_commit_select  util_two_phase.kv_commit_split on a compacted QKV buffer
  compact_rows      the rows of a full-layout array that a compacted launch stores, in its order
  executed_rows     rows a pool call sent through the decoder, from the traces, the drafts and the decoded tokens
  h4_state, h4_gen  the four-head fixtures (tests/golden/h4_*, written by tests/golden/make_golden_h4.py): the reference's 2+2-layer
                    model with d = 128 and 4 heads trained on the ten fixture pairs, the trained model of this directory whose
                    verify step runs on k_attn3 / k_attn3s (the tiny one has 2 heads, the head-dimension-64 one 2 of 64)
"""
from __future__ import annotations

import functools
import json

import numpy as np
import torch

import util_loop_checks as U
import util_two_phase as T
from util_models import GOLDEN, load_npz

FILLER = T.FILLER
SELECT_DEFECTS = ["rank_from_n", "absent_gets_row0", "base_without_row0"]


def masks_of(act_idx, pred_probe, drafts, n_active: int) -> np.ndarray:
    """mask[g] for g < n_active: bit n set when drafts[act_idx[g], n, 0] == pred_probe[g]."""
    B, N, D = drafts.shape
    first = drafts[np.asarray(act_idx[:n_active], dtype=np.int64), :, 0]                   # [n_active, N]
    eq = first == np.asarray(pred_probe[:n_active])[:, None]
    return (eq.astype(np.int64) << np.arange(N)[None, :]).sum(axis=1).astype(np.int64)


def popcount(x: int) -> int:
    return bin(int(x)).count("1")


def sel_rows(mask: int, D: int) -> int:
    return 1 + D * popcount(mask)


def sel_row(mask: int, rs: int, D: int, defect=None):
    """Row of layout row ``rs`` among the slot's compacted rows: 0 for row 0, 1 + rank(n) * D + (j-1) for row 1 + n*D + (j-1) of a
    present draft with rank(n) = popcount(mask & ((1 << n) - 1)); None for a row of an absent draft."""
    if rs == 0:
        return 0
    n, j0 = divmod(rs - 1, D)
    if not (int(mask) >> n) & 1:
        return None
    rank = n if defect == "rank_from_n" else popcount(int(mask) & ((1 << n) - 1))
    return 1 + rank * D + j0


def select_split(act_idx, pred_probe, drafts, n_active: int, before: dict, probes_before: int = 0, defect=None):
    """(act2, pos2, mask, row_base, row_map, words).  act2 / pos2 and words[0..6] are util_two_phase.probe_split's, except that
    words[2] (m_rows of the draft pass) is the compacted total; words[3] stays n_active + matches * RPS, what verified_positions
    adds; words[7] = the row count published for the host.  mask / row_base [B]: per matching slot, in the order of act2; row_map
    [B * RPS]: compacted row -> layout row p * RPS + rs.  Entries past the counts keep what ``before`` (a dict of arrays named
    act2, pos2, mask, row_base, row_map) holds."""
    B, N, D = drafts.shape
    R = U.rps(N, D)
    act2, pos2, words = T.probe_split(act_idx, pred_probe, drafts, n_active, before["act2"], before["pos2"], probes_before)
    mask, base, rmap = (np.array(before[k], dtype=np.int32) for k in ("mask", "row_base", "row_map"))
    slot_masks = masks_of(act_idx, pred_probe, drafts, n_active)
    total = 0
    for g in range(n_active):
        p = int(pos2[g])
        if p < 0:
            continue
        m = int(slot_masks[g])
        mask[p], base[p] = m, total
        total += sel_rows(m, D) - (1 if defect == "base_without_row0" else 0)
    for p in range(words[0]):
        for rs in range(R):
            r = sel_row(int(mask[p]), rs, D, defect)
            if r is not None and 0 <= base[p] + r < len(rmap):
                rmap[base[p] + r] = p * R + rs
    words = list(words[:2]) + [total, words[3], words[4], words[5], words[6], total]
    return act2, pos2, mask, base, rmap, words


def merge_pred_select(pos2, pred_probe, pred2c, mask, row_base, n_active: int, N: int, D: int, before, defect=None):
    """pred [B * RPS] in k_accept's layout from the COMPACTED draft-pass predictions ``pred2c``: a matching slot's row 0 and the
    rows of its present drafts from their compacted places, FILLER in the rows of its absent drafts; any other slot as in
    util_two_phase.merge_pred."""
    R = U.rps(N, D)
    out = np.array(before, dtype=np.int32)
    for g in range(n_active):
        p = int(pos2[g])
        if p < 0:
            out[g * R] = pred_probe[g]
            out[g * R + 1:(g + 1) * R] = FILLER
            continue
        for rs in range(R):
            r = sel_row(int(mask[p]), rs, D, defect)
            if r is None:
                out[g * R + rs] = pred2c[row_base[p]] if defect == "absent_gets_row0" else FILLER
            else:
                out[g * R + rs] = pred2c[row_base[p] + r]
    return out


def compact_rows(full: np.ndarray, mask, row_base, n_match: int, N: int, D: int, before: np.ndarray) -> np.ndarray:
    """The compacted image of ``full`` [>= n_match * RPS, ...] (position p's rows at p * RPS ..): row row_base[p] + sel_row of
    every present layout row; the rows past the compacted count keep ``before``."""
    R = U.rps(N, D)
    out = before.copy()
    for p in range(n_match):
        for rs in range(R):
            r = sel_row(int(mask[p]), rs, D)
            if r is not None:
                out[int(row_base[p]) + r] = full[p * R + rs]
    return out


def two_passes_select(act_idx, drafts, pred_full, n_active: int):
    """What the probe and a draft-select draft pass leave, given the predictions ``pred_full`` [B * RPS] of the step run in one pass:
    (pred_probe, act2, pos2, mask, row_base, row_map, pred2c, words), sentinels wherever a pass writes nothing."""
    B, N, D = drafts.shape
    R = U.rps(N, D)
    sent = U.SENTINEL[torch.int32]
    pred_probe = np.full(B, sent, dtype=np.int32)
    pred_probe[:n_active] = np.asarray(pred_full)[:n_active * R:R]
    before = {k: np.full(B * R if k == "row_map" else B, sent, dtype=np.int32) for k in ("act2", "pos2", "mask", "row_base", "row_map")}
    act2, pos2, mask, base, rmap, words = select_split(act_idx, pred_probe, drafts, n_active, before)
    full2 = np.full(B * R, sent, dtype=np.int32)
    for g in range(n_active):
        if pos2[g] >= 0:
            full2[pos2[g] * R:(pos2[g] + 1) * R] = pred_full[g * R:(g + 1) * R]
    pred2c = compact_rows(full2, mask, base, words[0], N, D, np.full(B * R, sent, dtype=np.int32))
    return pred_probe, act2, pos2, mask, base, rmap, pred2c, words


def kv_commit_select(rec, n_copy: int, qkv_c, qkv_probe, pos2, mask, row_base, kcache, vcache, N: int, D: int):
    """util_two_phase.kv_commit_split with the matching slots' rows taken from the compacted ``qkv_c`` [Ld, rows, 3d]."""
    k, v = kcache.copy(), vcache.copy()
    d = k.shape[-1]
    for slot in range(n_copy):
        b, best, n_acc, f = (int(x) for x in rec[slot, :4])
        p = int(pos2[slot])
        if p < 0:
            assert n_acc == 0
            k[:, b, f] = qkv_probe[:, slot, d:2 * d]
            v[:, b, f] = qkv_probe[:, slot, 2 * d:]
            continue
        for j in range(n_acc + 1):
            r = sel_row(int(mask[p]), 0 if j == 0 else 1 + best * D + (j - 1), D)
            assert r is not None, "the best draft of a slot that accepted tokens is a present one"
            k[:, b, f + j] = qkv_c[:, int(row_base[p]) + r, d:2 * d]
            v[:, b, f + j] = qkv_c[:, int(row_base[p]) + r, 2 * d:]
    return k, v


def split_operands(act_idx, pred_probe, drafts, n_active: int):
    """(mask [B], row_base [B], total) of the matching slots in the order of the active list, zeros past the match count (what a
    test hands a kernel that takes the draft pass's operands)."""
    B, N, D = drafts.shape
    sm = masks_of(act_idx, pred_probe, drafts, n_active)
    mask, base = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    total = p = 0
    for g in range(n_active):
        if sm[g]:
            mask[p], base[p] = sm[g], total
            total += sel_rows(int(sm[g]), D)
            p += 1
    return mask, base, total


@functools.lru_cache(maxsize=None)
def h4_state() -> tuple[dict, dict]:
    """(state dict joined from its parts, config) of the four-head model."""
    cfg = json.loads((GOLDEN / "h4_config.json").read_text())
    st = {}
    for i in range(cfg["weight_parts"]):
        st.update(load_npz(f"h4_weights_{i}.npz"))
    assert cfg["embedding_dim"] // cfg["num_heads"] == 32 and cfg["num_heads"] % 4 == 0
    return st, cfg


def h4_gen() -> dict:
    """spec_greedy arrays of h4_gen.npz, prefix stripped: b1_n3_d10_tokens [10, 1, L], b1_n3_d10_calls."""
    return {k[len("spec_greedy__"):]: v for k, v in load_npz("h4_gen.npz").items()}


# ---------------------------------------------------------------------------------------------------------------------------
# what the traces of a pool call say about the rows it ran
def executed_rows(traj: np.ndarray, tokens: np.ndarray, drafts: np.ndarray):
    """(rows, slot-steps with fewer than N drafts present, slot-steps with more than one present, drafts matched) of a pool call in
    which every step was split.  traj [R, max_len + 1]: a row's front after each of its steps; tokens [R, >= max front + 1]: the
    row's decoded tokens (BOS first), so that the probe's prediction at front f is tokens[r, f + 1]; drafts [R, N, D].  A slot-step
    runs 1 row in the probe and, when m >= 1 drafts start with the prediction, 1 + D * m rows in the draft pass."""
    R, N, D = drafts.shape
    life, _ = T.slot_steps(traj)
    rows = fewer = several = matched = 0
    for r in range(R):
        for it in range(int(life[r])):
            f = int(traj[r, it])
            m = int((drafts[r, :, 0] == tokens[r, f + 1]).sum())
            rows += 1 + ((1 + D * m) if m else 0)
            fewer += 1 if 0 < m < N else 0
            several += 1 if m > 1 else 0
            matched += m
    return rows, fewer, several, matched
