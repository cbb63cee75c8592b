"""The stochastic beam pool (csrc/ttx_sbs_pool.hip.h, include/ttx.h: ttx_sbs_generate_pool) restated in NumPy for the tests, on top
of the step restatement of tests/util_sbs_checks.py: C source slots of K candidates, admission into the lowest free slots, a step per
live slot at the slot's OWN level with its own key and parent count, retirement into the source's row of the outputs, and the words
the pool publishes.  The state arrays carry the kernels' names and layouts, so that the kernel test compares them one to one after
every launch.  No tests here.

``Pool(..., defect=name)`` plants one deviation (the checkers' sensitivity test):
  g_not_reset           admission leaves G of the slot's candidates as the previous source left it
  g_wrong_parity        admission writes G = 0 into the buffer the next iteration WRITES
  level_from_iteration  a slot steps at the pool's iteration count instead of its own level
  stale_key             a reused slot keeps the previous source's key
  fresh_k_parents       a fresh source steps with K live parents (G = 0, phi = 0) instead of one
  retire_early          retirement one level early (level max_len - 2)
  retire_late           retirement one level late (level max_len)
  wrong_row             the outputs of a retiring slot go to the next source's row

Checkers: ``check_admission`` looks at the state right after an admission (what the next step will read), ``check_iteration`` at the
per-slot words after an iteration, ``check_outputs`` compares the pool's outputs with the per-source restatement on the bits.
"""
from __future__ import annotations

import numpy as np

import util_sbs_checks as S

DEFECTS = ("g_not_reset", "g_wrong_parity", "level_from_iteration", "stale_key", "fresh_k_parents", "retire_early", "retire_late",
           "wrong_row")


class Pool:
    """``models[row](prefixes) -> logits [n, V]`` per source row of the call; ``keys[row]``; float64 state (``dtype``)."""

    def __init__(self, models, keys, C: int, K: int, max_len: int, seed: int, temperature: float, pad: int, bos: int, eos: int,
                 dtype=np.float64, defect: str | None = None, src_len=None):
        assert defect is None or defect in DEFECTS
        self.models, self.keys, self.C, self.K, self.max_len = models, [int(k) for k in keys], C, K, max_len
        self.seed, self.temperature, self.pad, self.bos, self.eos, self.dtype, self.defect = seed, temperature, pad, bos, eos, dtype, defect
        self.S = len(models)
        self.src_len = np.asarray(src_len if src_len is not None else np.full(self.S, 2), dtype=np.int32)
        self.ld = max_len + 2
        MC = C * K
        # slots (k_sbsp_init)
        self.row_of = np.full(C, -1, np.int32)
        self.level = np.ones(C, np.int32)
        self.nlive = np.zeros(C, np.int32)
        self.nfin = np.zeros(C, np.int32)
        self.key = np.zeros(C, np.int64)
        self.used = np.zeros(C, bool)             # the slot has held a source before
        self.run_acc = np.zeros(C, np.int32)      # candidates the slot's source has had decoded so far
        self.src_running = np.full(self.S, -7, np.int32)     # per source, written at retirement
        # candidates
        self.cand_next = np.full((MC, self.ld), pad, np.int64)
        self.len_next = np.ones(MC, np.int32)
        self.fin_next = np.ones(MC, np.uint8)
        self.phi_next = np.zeros(MC, dtype)
        self.parent = np.full(MC, -1, np.int32)
        self.parent_draft = np.zeros(MC, np.int32)
        self.cand_src_len = np.ones(MC, np.int32)
        self.g = [np.zeros(MC, dtype), np.zeros(MC, dtype)]       # read by the iteration of that parity, written by the other
        # outputs (sentinels: a row that was never written shows)
        self.out = np.full((self.S, K, max_len), -7, np.int64)
        self.out_logp = np.full((self.S, K), np.nan, dtype)
        self.out_gumbel = np.full((self.S, K), np.nan, dtype)
        self.iteration = 0            # iterations executed = BeamCounters.model_calls; its parity picks the G buffers
        self.running_rows = 0         # BeamCounters.running_cands
        self.steps_of = np.zeros(self.S, np.int32)       # steps each source took
        self.retired_at = np.full(self.S, -1, np.int32)  # the level each source retired at
        self.host = dict(steps_done=0, n_live=0, n_running=0, error=0)

    # -- k_sbsp_admit + k_sbsp_fill ------------------------------------------------------------------------------------------------
    def admit(self, first_row: int, R: int) -> np.ndarray:
        """Sources first_row .. first_row + R - 1 into the lowest free slots; returns new_slot [R] (-1: no slot, error)."""
        new_slot = np.full(R, -1, np.int32)
        s = 0
        for i in range(R):
            while s < self.C and self.row_of[s] >= 0:
                s += 1
            if s >= self.C:
                self.host["error"] = 1
                break
            new_slot[i] = s
            self.row_of[s] = first_row + i
            s += 1
        K, par = self.K, self.iteration & 1
        for i, s in enumerate(new_slot):
            if s < 0:
                continue
            row = first_row + i
            c0 = s * K
            self.cand_next[c0:c0 + K] = self.pad
            self.cand_next[c0, 0] = self.bos
            self.len_next[c0:c0 + K] = 1
            self.fin_next[c0:c0 + K] = 1
            self.fin_next[c0] = 0
            self.phi_next[c0:c0 + K] = 0
            if self.defect == "g_wrong_parity":
                self.g[par ^ 1][c0:c0 + K] = 0
            elif self.defect != "g_not_reset":
                self.g[par][c0:c0 + K] = 0
            self.parent[c0:c0 + K] = -1
            self.parent_draft[c0:c0 + K] = 0
            self.cand_src_len[c0:c0 + K] = self.src_len[row]
            self.level[s], self.nlive[s], self.nfin[s] = 1, 1, 0
            self.run_acc[s] = 1
            if not (self.defect == "stale_key" and self.used[s]):
                self.key[s] = self.keys[row]
            self.used[s] = True
        return new_slot

    # -- the step of one iteration (k_bs_prep's view of the rows, then k_sbs_step_pool) ---------------------------------------------
    def step(self) -> None:
        K, par = self.K, self.iteration & 1
        g_in, g_out = self.g[par], self.g[par ^ 1]
        rows, lens, fin, phi = self.cand_next.copy(), self.len_next.copy(), self.fin_next.copy(), self.phi_next.copy()
        self.running_rows += int((fin == 0).sum())
        for s in range(self.C):
            row = int(self.row_of[s])
            if row < 0:
                continue
            pos = int(self.level[s]) if self.defect != "level_from_iteration" else self.iteration + 1
            width = int(self.level[s])
            beam = int(self.nlive[s])
            c0 = s * K
            if self.defect == "fresh_k_parents" and beam == 1:
                beam = K
                rows[c0:c0 + K] = rows[c0]
                fin[c0:c0 + K] = 0
                phi[c0:c0 + K] = 0
            logits = np.asarray(self.models[row](rows[c0:c0 + beam, :width]))
            st = S.step(logits, phi[c0:c0 + beam], g_in[c0:c0 + beam], fin[c0:c0 + beam] != 0, int(self.key[s]), pos, self.seed,
                        self.temperature, K, self.pad, self.eos, self.dtype)
            new = np.full((K, self.ld), self.pad, np.int64)
            new[:, :width] = rows[c0 + st.parent, :width]
            new[:, width] = st.token
            self.cand_next[c0:c0 + K] = new
            self.phi_next[c0:c0 + K] = st.phi
            g_out[c0:c0 + K] = st.g
            self.parent[c0:c0 + K] = c0 + st.parent
            self.parent_draft[c0:c0 + K] = 0
            self.len_next[c0:c0 + K] = width + 1
            self.fin_next[c0:c0 + K] = st.finished
            self.nfin[s] = int(st.finished.sum())
            self.steps_of[row] += 1
        self.iteration += 1

    # -- k_sbsp_retire ----------------------------------------------------------------------------------------------------------
    def retire(self) -> None:
        """After step(): the G the step wrote is the buffer of the parity the NEXT iteration reads."""
        K = self.K
        g_out = self.g[self.iteration & 1]
        cap = self.max_len - 1 - (1 if self.defect == "retire_early" else 0) + (1 if self.defect == "retire_late" else 0)
        for s in range(self.C):
            row = int(self.row_of[s])
            if row < 0:
                continue
            lvl = int(self.level[s])
            if self.nfin[s] != K and lvl < cap:
                self.level[s], self.nlive[s] = lvl + 1, K
                self.run_acc[s] += K - self.nfin[s]
                continue
            to = (row + 1) % self.S if self.defect == "wrong_row" else row
            c0 = s * K
            self.out[to] = self.cand_next[c0:c0 + K, :self.max_len]
            self.out_logp[to] = self.phi_next[c0:c0 + K]
            self.out_gumbel[to] = g_out[c0:c0 + K]
            self.fin_next[c0:c0 + K] = 1
            self.parent[c0:c0 + K] = -1
            self.retired_at[row] = lvl
            self.src_running[to] = self.run_acc[s]
            self.row_of[s], self.nlive[s] = -1, 0

    # -- k_sbsp_publish ---------------------------------------------------------------------------------------------------------
    def publish(self) -> None:
        live = self.row_of >= 0
        self.host["n_live"] = int(live.sum())
        self.host["n_running"] = int((self.K - self.nfin[live]).sum())
        self.host["steps_done"] = self.iteration

    def run(self, order=None, on_admit=None, on_iteration=None):
        """Every source, admitted in ``order`` whenever slots are free; returns self."""
        order = list(range(self.S)) if order is None else list(order)
        assert sorted(order) == list(range(self.S))
        # the call numbers its sources in admission order: row r of the call is source order[r]
        self.models = [self.models[i] for i in order]
        self.keys = [self.keys[i] for i in order]
        self.src_len = self.src_len[order]
        cursor = 0
        while True:
            free = int((self.row_of < 0).sum())
            take = min(free, self.S - cursor)
            if take:
                slots = self.admit(cursor, take)
                if on_admit:
                    on_admit(self, cursor, slots)
                cursor += take
            if not (self.row_of >= 0).any():
                break
            assert self.iteration <= self.max_len * (self.S + 1), "the pool failed to terminate"
            self.step()
            self.retire()
            self.publish()
            if on_iteration:
                on_iteration(self)
        inv = np.argsort(order)
        self.out, self.out_logp, self.out_gumbel = self.out[inv], self.out_logp[inv], self.out_gumbel[inv]
        self.steps_of, self.retired_at, self.src_running = self.steps_of[inv], self.retired_at[inv], self.src_running[inv]
        return self


def check_admission(pool: Pool, first_row: int, new_slot) -> list:
    """The state the next step reads for the slots just admitted."""
    bad, K = [], pool.K
    g_read = pool.g[pool.iteration & 1]
    for i, s in enumerate(new_slot):
        if s < 0:
            bad.append(f"source {first_row + i} found no slot")
            continue
        c0, row = s * K, first_row + i
        if pool.row_of[s] != row:
            bad.append(f"slot {s}: row_of {pool.row_of[s]}, admitted {row}")
        if (g_read[c0:c0 + K] != 0).any():
            bad.append(f"slot {s}: G of a fresh source is not 0 in the buffer the next step reads")
        if (pool.phi_next[c0:c0 + K] != 0).any() or pool.level[s] != 1 or pool.nlive[s] != 1 or pool.nfin[s] != 0:
            bad.append(f"slot {s}: phi, level, parent count or finished count not reset")
        if pool.key[s] != pool.keys[row]:
            bad.append(f"slot {s}: key {pool.key[s]}, the source's is {pool.keys[row]}")
        if pool.cand_next[c0, 0] != pool.bos or (pool.cand_next[c0, 1:] != pool.pad).any() or (pool.cand_next[c0 + 1:c0 + K] != pool.pad).any():
            bad.append(f"slot {s}: candidate rows carry tokens of the previous source")
        if pool.fin_next[c0] != 0 or (pool.fin_next[c0 + 1:c0 + K] != 1).any() or (pool.parent[c0:c0 + K] != -1).any():
            bad.append(f"slot {s}: one <BOS> candidate without a parent, the others absent")
    return bad


def check_iteration(pool: Pool) -> list:
    """The slot words after step + retire + publish."""
    bad = []
    for s in range(pool.C):
        if pool.row_of[s] < 0:
            continue
        if pool.nlive[s] != pool.K:
            bad.append(f"slot {s}: a source past its first level has {pool.nlive[s]} parents")
        if not 2 <= pool.level[s] <= pool.max_len - 1:
            bad.append(f"slot {s}: level {pool.level[s]} outside [2, max_len - 1] after an iteration")
        if pool.nfin[s] == pool.K:
            bad.append(f"slot {s}: all candidates finished but the slot is still live")
    if pool.host["n_live"] != int((pool.row_of >= 0).sum()) or pool.host["steps_done"] != pool.iteration:
        bad.append("published words do not match the state")
    return bad


def reference(models, keys, K: int, max_len: int, seed: int, temperature: float, pad: int, bos: int, eos: int, dtype=np.float64):
    """The per-source restatement: (rows [S, K, max_len], phi [S, K], g [S, K], steps [S])."""
    res = [S.search(m, int(k), seed, temperature, K, max_len, pad, bos, eos, dtype) for m, k in zip(models, keys)]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]),
            np.array([len(r[4]) for r in res], np.int32))


def check_outputs(pool: Pool, ref) -> list:
    """Pool outputs against ``reference(...)`` on the bits, and each source's step count against its own search's."""
    rows, phi, g, steps = ref
    bad = []
    for r in range(len(rows)):
        if not np.array_equal(pool.out[r], rows[r]):
            bad.append(f"source {r}: tokens differ")
        if pool.out_logp[r].tobytes() != phi[r].astype(pool.dtype).tobytes():
            bad.append(f"source {r}: logp differs")
        if pool.out_gumbel[r].tobytes() != g[r].astype(pool.dtype).tobytes():
            bad.append(f"source {r}: gumbel differs")
        if pool.steps_of[r] != steps[r]:
            bad.append(f"source {r}: {pool.steps_of[r]} steps, its own search takes {steps[r]}")
    return bad
