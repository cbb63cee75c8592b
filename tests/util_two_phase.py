"""Plain restatement of the two-phase verify step of the slot pool (csrc/ttx_loop_kernels.hip.h: k_probe_split, k_merge_pred and
k_kvcopy's indirection), the operands of their kernel-level tests and what the end-to-end tests read off the traces.  No GPU call
in here: tests/test_two_phase_host.py shows on the CPU that the merged predictions give k_accept's specification
(util_loop_checks.accept_step) the state the full predictions give it, and that the restatement of the split tells a defective
stand-in from a correct one; tests/test_gpu_two_phase.py holds the kernels to it, one launch at a time.

The rule, restated from the accept rule and not from the kernels: a slot's draft rows can change a verify step's result only if
the prediction of its front row equals the first token of one of its drafts; otherwise the accepted length is 0 for every draft,
the first draft is "best", the bonus token is the front row's prediction and only the front row's K/V is committed.

  probe_split       which live slots match, in the order of the active list; slot -> position among them; the counts
  merge_pred        the prediction array k_accept reads, from the probe's and the draft pass's predictions
  kv_commit_split   util_loop_checks.kv_commit with the rows of a slot taken from where the two passes left them
  pool_schedule     the slot-steps of a one-session pool call, step by step, from the per-row traces
"""
from __future__ import annotations

import numpy as np
import torch

import util_loop_checks as U

FILLER = -1                                   # what a slot without a draft pass holds in its draft rows
SPLIT_DEFECTS = ["first_draft_only", "reversed_order", "stale_count"]


def probe_split(act_idx, pred_probe, drafts, n_active: int, act2_before, pos2_before, probes_before: int = 0, defect=None):
    """(act2, pos2, words).  Slot g < n_active is sequence b = act_idx[g] and matches when pred_probe[g] == drafts[b, n, 0] for some
    n.  act2 holds the matching sequences in the order of act_idx, entries past the match count keep what ``act2_before`` holds;
    pos2[g] = the slot's position in act2 or -1, entries at or past n_active keep ``pos2_before``.  words = [n_active, r_rows,
    m_rows of the draft pass, executed rows = n_active + matches * RPS, probe count, and the two words published for the host:
    matches, probe count].  ``defect`` (host test only): one of SPLIT_DEFECTS."""
    B, N, D = drafts.shape
    R = U.rps(N, D)
    act2, pos2 = np.array(act2_before, dtype=np.int32), np.array(pos2_before, dtype=np.int32)
    first = drafts[np.asarray(act_idx[:n_active], dtype=np.int64), :, 0]                # [n_active, N]
    if defect == "first_draft_only":
        first = first[:, :1]
    hit = (first == np.asarray(pred_probe[:n_active])[:, None]).any(axis=1)
    m = int(hit.sum())
    seqs = np.asarray(act_idx[:n_active])[hit]
    act2[:m] = seqs[::-1] if defect == "reversed_order" else seqs
    pos = np.cumsum(hit) - 1
    pos2[:n_active] = np.where(hit, (m - 1 - pos) if defect == "reversed_order" else pos, -1)
    count = 0 if defect == "stale_count" else m
    words = [count, count * N, count * R, n_active + count * R, probes_before + 1, count, probes_before + 1]
    return act2, pos2, words


def merge_pred(pos2, pred_probe, pred2, n_active: int, N: int, D: int, before):
    """pred [B * RPS] in k_accept's layout: a slot with pos2 >= 0 takes the RPS predictions at position pos2 of ``pred2``, any
    other slot pred_probe[slot] in row 0 and FILLER in its draft rows; rows at or past n_active * RPS keep ``before``."""
    R = U.rps(N, D)
    out = np.array(before, dtype=np.int32)
    for g in range(n_active):
        p = int(pos2[g])
        if p >= 0:
            out[g * R:(g + 1) * R] = pred2[p * R:(p + 1) * R]
        else:
            out[g * R] = pred_probe[g]
            out[g * R + 1:(g + 1) * R] = FILLER
    return out


def two_passes(act_idx, drafts, pred_full, n_active: int):
    """What the two passes of a split step leave, given the predictions ``pred_full`` [B * RPS] of the step run in one pass:
    (pred_probe [B], act2, pos2, pred2 [B * RPS], words).  The arrays are sentinels wherever a pass writes nothing."""
    B, N, D = drafts.shape
    R = U.rps(N, D)
    sent = U.SENTINEL[torch.int32]
    pred_probe = np.full(B, sent, dtype=np.int32)
    pred_probe[:n_active] = np.asarray(pred_full)[:n_active * R:R]
    act2, pos2, words = probe_split(act_idx, pred_probe, drafts, n_active, np.full(B, sent, dtype=np.int32), np.full(B, sent, dtype=np.int32))
    pred2 = np.full(B * R, sent, dtype=np.int32)
    for g in range(n_active):
        if pos2[g] >= 0:
            pred2[pos2[g] * R:(pos2[g] + 1) * R] = pred_full[g * R:(g + 1) * R]
    return pred_probe, act2, pos2, pred2, words


def kv_commit_split(rec, n_copy: int, qkv, qkv_probe, pos2, kcache, vcache, N: int, D: int):
    """util_loop_checks.kv_commit for a split step: a slot with pos2 >= 0 takes its step rows from position pos2 of ``qkv``
    [Ld, B * RPS, 3d]; a slot with pos2 == -1 commits the K and V thirds of its row of ``qkv_probe`` [Ld, B, 3d] at front_old and
    nothing else (its record accepts nothing)."""
    k, v = kcache.copy(), vcache.copy()
    d = k.shape[-1]
    R = U.rps(N, D)
    for slot in range(n_copy):
        b, best, n_acc, f = (int(x) for x in rec[slot, :4])
        p = int(pos2[slot])
        if p < 0:
            assert n_acc == 0
            k[:, b, f] = qkv_probe[:, slot, d:2 * d]
            v[:, b, f] = qkv_probe[:, slot, 2 * d:]
            continue
        for j in range(n_acc + 1):
            srow = p * R + (0 if j == 0 else 1 + best * D + (j - 1))
            k[:, b, f + j] = qkv[:, srow, d:2 * d]
            v[:, b, f + j] = qkv[:, srow, 2 * d:]
    return k, v


# ---------------------------------------------------------------------------------------------------------------------------
# split cases of the kernel-level test
KINDS = ["none", "first", "last_only", "shared_first", "replacement", "random"]
REPL = 5                                      # the token the draft maker puts in the place of PAD and EOS


def split_case(B: int, n_active: int, N: int, D: int, seed: int, kinds=None, identity: bool = False, V: int = 40):
    """(act_idx [B], pred_probe [B], drafts [B, N, D], kind per slot).  Per live slot one of KINDS: no draft starts with the
    prediction; draft 0 does; only the last draft does; drafts 0 and 1 share it (N >= 2); the matching first token is REPL;
    random tokens (a match now and then)."""
    rng = np.random.default_rng(seed)
    kinds = kinds or KINDS
    act = (np.arange(B) if identity else rng.permutation(B)).astype(np.int32)
    drafts = rng.integers(6, V, size=(B, N, D), dtype=np.int32)
    pred = rng.integers(6, V, size=B, dtype=np.int32)
    kind = []
    for g in range(n_active):
        b, k = int(act[g]), kinds[int(rng.integers(0, len(kinds)))]
        if k == "shared_first" and N < 2:
            k = "first"
        kind.append(k)
        if k == "none":
            pred[g] = V + 1
        elif k == "first":
            drafts[b, 0, 0] = pred[g]
        elif k == "last_only":
            drafts[b, :, 0] = V + 2 + np.arange(N)
            drafts[b, N - 1, 0] = pred[g]
        elif k == "shared_first":
            drafts[b, 0, 0] = drafts[b, 1, 0] = pred[g]
        elif k == "replacement":
            pred[g] = REPL
            drafts[b, int(rng.integers(0, N)), 0] = REPL
    return act, pred, drafts, kind


# ---------------------------------------------------------------------------------------------------------------------------
# what the traces of a pool call say
def slot_steps(traj: np.ndarray):
    """(lifetime per row, advance per row and step).  traj [R, max_len + 1]: a row's front after each of its steps, 0 at step 0,
    -1 past its last step."""
    traj = np.asarray(traj, dtype=np.int64)
    alive = traj[:, 1:] >= 0
    life = alive.sum(axis=1)
    adv = np.where(alive, traj[:, 1:] - traj[:, :-1], 0)
    return life, adv


def pool_schedule(traj: np.ndarray, capacity: int):
    """The pool steps of a ONE-session call of ttx_greedy_speculative_generate_pool over rows given in this order: per step
    (live slots, matching slots).  A row is admitted into a free slot before a step when the pool is empty or at least
    max(1, capacity / 4) slots are free, takes part in as many steps as its trace has fronts, and matches in a step exactly
    when its front moves by more than 1 there."""
    life, adv = slot_steps(traj)
    R = len(life)
    C = min(capacity, R)
    min_admit = max(1, C // 4)
    cursor, live, steps = 0, [], []
    while True:
        free = C - len(live)
        if cursor < R and (not live or free >= min_admit):
            take = min(free, R - cursor)
            live += [[r, 0] for r in range(cursor, cursor + take)]
            cursor += take
        if not live:
            break
        steps.append((len(live), sum(int(adv[r, it] > 1) for r, it in live)))
        live = [[r, it + 1] for r, it in live if it + 1 < life[r]]
    return steps
