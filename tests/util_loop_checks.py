"""Plain restatement of the greedy-speculative loop kernels (csrc/ttx_loop_kernels.hip.h: k_embed, k_argmax, k_accept, k_kvcopy,
k_greedy_accept), the operands of their kernel-level tests and the checkers.  No GPU call in here, so that
tests/test_loop_checks_host.py can pin the restatement to the reference's goldens and show on the CPU that each checker fails
when it should; tests/test_gpu_loop_kernels.py holds the kernels to it, one launch at a time.

The rules are restated from the reference's loop (src/decoding/speculative_decoding.py:93-171 through oracle/decoding.py), in
NumPy over whole batches, not from the kernels.  All of it is integer or bit-copy work: every check is exact equality.

  accept_step     one verify step's bookkeeping on a LoopState (see its docstring for the rules)
  greedy_step     plain greedy decoding's step (standard_decoding.py:45-53)
  embed_full / embed_step, argmax_first, kv_commit   the other kernels
  Buf             an operand inside a larger sentinel-filled allocation (guard margins in front and behind)
  DeviceLoop      a LoopState's arrays as Bufs on a device + check(): (a) equality with the restatement, (b) intact margins,
                  (c) every element the rule does not write still holds what it held (the restatement carries the sentinels)
"""
from __future__ import annotations

import copy

import numpy as np
import torch

PAD, BOS, EOS = 0, 1, 2
GUARD = 64                                   # elements in front of and behind every operand (16-byte alignment is kept)
SENTINEL = {torch.uint8: 0xAA, torch.int16: -21846, torch.int32: -1431655766, torch.int64: -6148914691236517206}      # 0xAA.. patterns
FLOAT_FILL = 0x7FD5AAAA                      # quiet NaN with a payload: what a float output holds before its launch
NP_OF = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32}

WORDS = ["n_active", "r_rows", "m_rows", "stop", "width", "steps", "error", "n_copy", "accepted", "produced",
         "verified_positions", "kv_prefix_positions", "src_positions", "host_stop", "host_steps_done", "host_width", "host_n_active"]
STATE_WORDS = WORDS[:13]                     # the DecState; the last four are the words published for the host
SLOT_ARRAYS = ["act_idx", "front", "gen", "drafts", "rec", "out", "haspad", "traj", "fin_step", "rstep", "row_of", "pool_out",
               "pool_traj", "pool_fin_step"]
DTYPES = {"out": torch.int64, "pool_out": torch.int64, "traj": torch.int16, "pool_traj": torch.int16}


def rps(N: int, D: int) -> int:
    """Rows of one running sequence in a verify step: row 0 = the front token, row 1 + n*D + (j-1) = token j of draft n."""
    return 1 + N * D


# ---------------------------------------------------------------------------------------------------------------------------
# guarded operands
class Buf:
    """``shape`` elements of ``dtype`` inside an allocation with GUARD sentinel elements on either side, exposed as ``v``."""

    def __init__(self, shape, dtype, device="cpu", data=None):
        self.shape, self.dtype = tuple(int(s) for s in shape), dtype
        self.n = int(np.prod(self.shape)) if len(self.shape) else 1
        self.buf = torch.empty(self.n + 2 * GUARD, dtype=dtype, device=device)
        self.v = self.buf[GUARD:GUARD + self.n].view(self.shape)
        self.reset()
        if data is not None:
            self.set(data)

    def reset(self) -> None:
        if self.dtype == torch.float32:
            self.buf.view(torch.int32).fill_(FLOAT_FILL)
        else:
            self.buf.fill_(SENTINEL[self.dtype])

    def set(self, data) -> None:
        a = np.ascontiguousarray(np.asarray(data), dtype=NP_OF[self.dtype]).reshape(self.shape)
        self.v.copy_(torch.from_numpy(a))

    def get(self) -> np.ndarray:
        """A host copy; fp32 comes back as its int32 bit patterns (the comparisons are bit comparisons)."""
        a = self.v.detach().cpu().numpy().copy()
        return a.view(np.int32) if self.dtype == torch.float32 else a

    def margins(self) -> str | None:
        w = self.buf.view(torch.int32) if self.dtype == torch.float32 else self.buf
        fill = FLOAT_FILL if self.dtype == torch.float32 else SENTINEL[self.dtype]
        for name, part in (("front", w[:GUARD]), ("rear", w[GUARD + self.n:])):
            bad = torch.nonzero(part != fill)
            if bad.numel():
                return f"{name} guard margin overwritten at element {int(bad[0])}"
        return None


def sentinel_array(shape, dtype) -> np.ndarray:
    if dtype == torch.float32:
        return np.full(shape, FLOAT_FILL, dtype=np.int32).view(np.float32)
    return np.full(shape, SENTINEL[dtype], dtype=NP_OF[dtype])


def first_difference(got: np.ndarray, want: np.ndarray) -> str | None:
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return None
    idx = tuple(int(i) for i in bad[0])
    return f"{len(bad)} of {got.size} elements differ; first at {idx}: got {got[idx]!r} expected {want[idx]!r}"


def check_buf(buf: Buf, want: np.ndarray, what: str) -> None:
    """(a) + (c): the operand equals the restatement's array, whose unwritten elements hold what they held before; (b) margins."""
    if want.dtype == np.float32:
        want = want.view(np.int32)
    d = first_difference(buf.get(), want.reshape(buf.shape))
    assert d is None, f"{what}: {d}"
    m = buf.margins()
    assert m is None, f"{what}: {m}"


# ---------------------------------------------------------------------------------------------------------------------------
# argmax, embedding, K/V commit
def argmax_first(logits: np.ndarray, live: int, before: np.ndarray) -> np.ndarray:
    """pred[row] = first index of the row's maximum for rows < live (-0.0 == 0.0; all -inf and all-NaN rows give 0); the rows at
    or beyond ``live`` keep what ``before`` holds.  Rows that mix NaN with other values are outside the contract (mixed_nan_rows)."""
    out = before.copy()
    for r in range(live):
        row = logits[r]
        if np.isnan(row).all():
            out[r] = 0
            continue
        m = row.max()                        # NaN for a mixed row: such rows are excluded by the caller
        hit = np.nonzero(row == m)[0]
        out[r] = hit[0] if len(hit) else 0
    return out


def mixed_nan_rows(logits: np.ndarray) -> np.ndarray:
    n = np.isnan(logits)
    return n.any(axis=1) & ~n.all(axis=1)


def check_argmax(got: np.ndarray, logits: np.ndarray, live: int, before: np.ndarray, what: str) -> None:
    want = argmax_first(logits, live, before)
    mixed = np.zeros(len(before), dtype=bool)
    mixed[:live] = mixed_nan_rows(logits[:live])
    d = first_difference(got[~mixed], want[~mixed])
    assert d is None, f"{what}: {d}"
    V = logits.shape[1]
    assert ((got[mixed] >= 0) & (got[mixed] < V)).all(), f"{what}: a row mixing NaN and numbers gave an id outside [0, V)"


def lookup(table: np.ndarray, pe: np.ndarray, tok: np.ndarray, pos: np.ndarray) -> np.ndarray:
    """table[tok] + pe[pos + 1] in fp32; ids outside [0, V) are looked up as id 0."""
    tok = np.where((tok < 0) | (tok >= table.shape[0]), 0, tok)
    with np.errstate(over="ignore", invalid="ignore"):
        return (table[tok].astype(np.float32) + pe[pos + 1].astype(np.float32)).astype(np.float32)


def embed_full(table, pe, tok: np.ndarray, L: int, before: np.ndarray) -> np.ndarray:
    """Full mode: row r holds token tok[r] at position r % L."""
    out = before.copy()
    rows = len(tok)
    out[:rows] = lookup(table, pe, tok, np.arange(rows) % L)
    return out


def embed_step(table, pe, act_idx, front, gen, drafts, n_active: int, before: np.ndarray) -> np.ndarray:
    """Step mode: slot g < n_active is sequence b = act_idx[g] at front f: row 0 = gen[b, f] at position f, row 1 + n*D + (j-1) =
    drafts[b, n, j-1] at position f + j.  Rows beyond n_active * (1 + N*D) keep what ``before`` holds."""
    out = before.copy()
    B, N, D = drafts.shape
    R = rps(N, D)
    for g in range(n_active):
        b = int(act_idx[g])
        f = int(front[b])
        tok = np.concatenate([[gen[b, f]], drafts[b].reshape(-1)])
        pos = np.concatenate([[f], np.tile(f + 1 + np.arange(D), N)])
        out[g * R:(g + 1) * R] = lookup(table, pe, tok, pos)
    return out


def kv_commit(rec: np.ndarray, n_copy: int, qkv: np.ndarray, kcache: np.ndarray, vcache: np.ndarray, N: int, D: int):
    """For slot < n_copy with record (b, best, n_acc, front_old, .) and j = 0 .. n_acc: position front_old + j of cache row b takes
    the K and V thirds of the slot's step row for token j of draft ``best`` (row 0 for j = 0, else 1 + best*D + (j-1)), in every
    layer, bit for bit.  qkv [Ld, B * (1 + N*D), 3d], caches [Ld, B, Lc, d] as int32 bit patterns or floats.  Returns new caches."""
    k, v = kcache.copy(), vcache.copy()
    d = k.shape[-1]
    R = rps(N, D)
    for slot in range(n_copy):
        b, best, n_acc, f = (int(x) for x in rec[slot, :4])
        for j in range(n_acc + 1):
            srow = slot * R + (0 if j == 0 else 1 + best * D + (j - 1))
            k[:, b, f + j] = qkv[:, srow, d:2 * d]
            v[:, b, f + j] = qkv[:, srow, 2 * d:]
    return k, v


def kv_operands(rec: np.ndarray, n_copy: int, B: int, N: int, D: int, d: int, Ld: int, Lc: int, seed: int) -> dict:
    """qkv [Ld, B * (1 + N*D), 3d] of random bit patterns (NaNs of every kind included: the commit is a bit copy) and the two
    caches [Ld, B, Lc, d] full of the float fill."""
    rng = np.random.default_rng(seed)
    assert all(int(r[3]) + int(r[2]) + 1 <= Lc for r in rec[:n_copy])
    qkv = rng.integers(-2 ** 31, 2 ** 31, size=(Ld, B * rps(N, D), 3 * d), dtype=np.int64).astype(np.int32).view(np.float32)
    return {"qkv": qkv, "k0": sentinel_array((Ld, B, Lc, d), torch.float32), "v0": sentinel_array((Ld, B, Lc, d), torch.float32)}


# ---------------------------------------------------------------------------------------------------------------------------
# the loop state and one verify step's bookkeeping
class LoopState:
    """Everything k_accept reads and writes: scalars (B, N, D, Ls, max_len, gen_ld, row_rule, pool, traj_ld, pool_rows), the
    arrays of SLOT_ARRAYS (NumPy; None where the mode has none) and ``words`` (WORDS: the DecState and the host's words)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def clone(self) -> "LoopState":
        return copy.deepcopy(self)


def gather_pred(pred: np.ndarray, Bc: int, N: int, D: int) -> np.ndarray:
    """[Bc, N, D + 1]: the prediction at position f + j on draft n = row 0 of the slot for j = 0, else row 1 + n*D + (j-1)."""
    R = rps(N, D)
    p = np.asarray(pred)[:Bc * R].reshape(Bc, R)
    return np.concatenate([np.repeat(p[:, :1], N, axis=1)[:, :, None], p[:, 1:].reshape(Bc, N, D)], axis=2)


def accept_step(state: LoopState, pred: np.ndarray) -> LoopState:
    """One verify step's bookkeeping (speculative_decoding.py:122-172), returning the new state.

    For each running slot (act_idx[0, n_active)): a draft's accepted length is the leading run of agreement between the draft and
    the predictions; the best draft is the FIRST maximum; tokens j = 0 .. n_acc of the best draft's predictions are written after
    the front (the last one is the bonus token), the front moves by n_acc + 1; the row is finished iff a WRITTEN token is EOS.
    width = max(old fronts) + D + 2.  Finished rows go to ``out`` up to min(width, max_len) columns (max_len under row_rule); the
    running list is compacted in order and the entries beyond the new count stay as they were.  error 1: a row finished at width >
    max_len.  The loop stops when nobody runs or width >= max_len.  row_rule: no width stop; a row retires (flags 2) once f + D + 2
    >= max_len, its front after step ``it`` goes to traj[it] (it < traj_ld), fin_step = it when it finishes, error 3 when a
    still-running row ever wrote a PAD; pool: ``it`` counts per slot (rstep) and the caller-side rows are those of row_of.
    Quirk 2 (no row_rule): when a still-running row ever wrote a PAD and some column up to the largest running front is PAD in
    every running row, the reference's next step raises: error 2, stop."""
    s = state.clone()
    w = s.words
    w.update(dict.fromkeys(WORDS[13:], -1))                              # the host's words: -1 until this step publishes them
    Bc = int(w["n_active"])
    if Bc == 0:
        return s                                                        # nothing runs, nothing is published
    N, D, R = s.N, s.D, rps(s.N, s.D)
    rows = s.act_idx[:Bc].copy()
    f = s.front[rows].astype(np.int64)
    P = gather_pred(pred, Bc, N, D)
    agree = s.drafts[rows] == P[:, :, :D]
    n_ok = np.cumprod(agree, axis=2).sum(axis=2)
    best = n_ok.argmax(axis=1)                                          # first maximum
    ar = np.arange(Bc)
    n_acc = n_ok[ar, best]
    chosen = P[ar, best]                                                # [Bc, D + 1]
    written = np.arange(D + 1)[None, :] <= n_acc[:, None]
    cols = f[:, None] + 1 + np.arange(D + 1)[None, :]
    s.gen[rows[:, None].repeat(D + 1, 1)[written], cols[written]] = chosen[written]
    new_front = f + n_acc + 1
    s.front[rows] = new_front
    fin = (written & (chosen == s.eos)).any(axis=1)
    sawpad = (written & (chosen == s.pad)).any(axis=1)
    s.haspad[rows[sawpad]] = 1
    width = int(f.max()) + D + 2
    flags = fin.astype(np.int64)
    if s.row_rule:
        flags[~fin & (f + D + 2 >= s.max_len)] = 2
        if s.pool:
            it = s.rstep[rows] + 1
            s.rstep[rows] = it
            trows, traj, fins = s.row_of[rows], s.pool_traj, s.pool_fin_step
        else:
            it = np.full(Bc, int(w["steps"]) + 1)
            trows, traj, fins = rows, s.traj, s.fin_step
        ok = it < s.traj_ld
        traj[trows[ok], it[ok]] = new_front[ok]
        fins[trows[fin]] = it[fin]
    s.rec[:Bc] = np.stack([rows, best, n_acc, f, flags], axis=1)
    wout = s.max_len if s.row_rule else min(width, s.max_len)
    if s.pool:
        s.pool_out[s.row_of[rows[fin]], :wout] = s.gen[rows[fin], :wout]
    else:
        s.out[rows[fin], :wout] = s.gen[rows[fin], :wout]
    kept = rows[flags == 0]
    nn = len(kept)
    s.act_idx[:nn] = kept
    w["n_copy"] = Bc
    w["steps"] += 1
    w["accepted"] += int(n_acc.sum())
    w["produced"] += int(n_acc.sum()) + Bc
    w["verified_positions"] += Bc * R
    w["kv_prefix_positions"] += int(f.sum())
    w["src_positions"] += Bc * s.Ls
    w["width"] = width
    if fin.any() and width > s.max_len and not s.row_rule:
        w["error"] = 1
    stop = nn == 0 or (not s.row_rule and width >= s.max_len)
    suspect = bool(s.haspad[kept].any())
    if s.row_rule and suspect:
        w["error"] = 3
    if not stop and suspect and not s.row_rule:
        maxf = int(s.front[kept].max())
        if (s.gen[kept, :maxf + 1] == s.pad).all(axis=0).any():
            w["error"] = 2
            stop = True
    w["stop"] = int(stop)
    w["n_active"] = 0 if stop else nn
    w["r_rows"] = 0 if stop else nn * N
    w["m_rows"] = 0 if stop else nn * R
    w["host_width"], w["host_n_active"], w["host_stop"], w["host_steps_done"] = width, w["n_active"], int(stop), w["steps"]
    return s


def greedy_step(state: LoopState, pred: np.ndarray) -> LoopState:
    """Plain greedy decoding's step (standard_decoding.py:45-53; N = 1, D = 0): every row [0, n_active) appends its prediction at
    the shared front + 1; nothing retires; the loop ends when every row emitted EOS or PAD at this very step, or once column
    max_len - 1 is written."""
    s = state.clone()
    w = s.words
    w.update(dict.fromkeys(WORDS[13:], -1))
    Bc = int(w["n_active"])
    if Bc == 0:
        return s
    f = int(s.front[0])
    t = np.asarray(pred)[:Bc]
    s.gen[:Bc, f + 1] = t
    s.front[:Bc] = f + 1
    s.rec[:Bc] = np.stack([np.arange(Bc), np.zeros(Bc), np.zeros(Bc), np.full(Bc, f), np.zeros(Bc)], axis=1)
    w["n_copy"] = Bc
    w["steps"] += 1
    w["produced"] += Bc
    w["verified_positions"] += Bc
    w["kv_prefix_positions"] += Bc * f
    w["src_positions"] += Bc * s.Ls
    w["width"] = f + 2
    stop = bool(((t == s.eos) | (t == s.pad)).all()) or f + 1 >= s.max_len - 1
    w["stop"] = int(stop)
    if stop:
        w["n_active"] = w["r_rows"] = w["m_rows"] = 0
    w["host_width"], w["host_stop"], w["host_steps_done"] = f + 2, int(stop), w["steps"]
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# operand builders
def make_state(B: int, N: int, D: int, max_len: int, fronts, n_active: int | None = None, seed: int = 0, V: int = 40,
               row_rule: bool = False, pool: bool = False, Ls: int = 7, steps: int = 3, permute: bool = True) -> LoopState:
    """A loop state as production could hold it before a verify step: gen rows are BOS, real tokens up to the front and PAD
    behind it; ``fronts`` (scalar or [B]) must leave front + D + 2 <= gen_ld = max_len + D + 2.  act_idx is a permutation of the
    rows (the first n_active run).  Every array the step writes INTO (rec, out, traj, fin_step, the pool's caller-side rows)
    starts as sentinels, so that a write the rule does not make is seen; the counters start beyond 2^32."""
    rng = np.random.default_rng(seed)
    n_active = B if n_active is None else n_active
    gen_ld = max_len + D + 2
    front = np.broadcast_to(np.asarray(fronts, dtype=np.int32), (B,)).copy()
    assert (front >= 0).all() and (front + D + 2 <= gen_ld).all()
    gen = np.full((B, gen_ld), PAD, dtype=np.int32)
    body = rng.integers(3, V, size=(B, gen_ld), dtype=np.int32)
    live = np.arange(gen_ld)[None, :] <= front[:, None]
    gen[live] = body[live]
    gen[:, 0] = BOS
    act = (rng.permutation(B) if permute else np.arange(B)).astype(np.int32)
    traj_ld = max_len + 1
    pool_rows = B + 5
    s = LoopState(B=B, N=N, D=D, Ls=Ls, max_len=max_len, gen_ld=gen_ld, pad=PAD, bos=BOS, eos=EOS, V=V, row_rule=int(row_rule or pool),
                  pool=int(pool), traj_ld=traj_ld, pool_rows=pool_rows,
                  act_idx=act, front=front, gen=gen, drafts=rng.integers(3, V, size=(B, N, max(D, 1)), dtype=np.int32),
                  rec=sentinel_array((B, 5), torch.int32), out=sentinel_array((B, max_len), torch.int64),
                  haspad=np.zeros(B, dtype=np.int32), traj=None, fin_step=None, rstep=None, row_of=None, pool_out=None,
                  pool_traj=None, pool_fin_step=None)
    if s.row_rule and not pool:
        s.traj = sentinel_array((B, traj_ld), torch.int16)
        s.fin_step = sentinel_array((B,), torch.int32)
    if pool:
        s.out = None
        s.rstep = rng.integers(0, 6, size=B, dtype=np.int32)
        s.row_of = rng.permutation(pool_rows)[:B].astype(np.int32)
        s.pool_out = sentinel_array((pool_rows, max_len), torch.int64)
        s.pool_traj = sentinel_array((pool_rows, traj_ld), torch.int16)
        s.pool_fin_step = sentinel_array((pool_rows,), torch.int32)
    big = 1 << 33
    s.words = dict.fromkeys(WORDS, -1)
    s.words.update(n_active=n_active, r_rows=n_active * N, m_rows=n_active * rps(N, D), stop=0, width=int(front.max()) + 1, steps=steps,
                   error=0, n_copy=0, accepted=big + 11, produced=big + 23, verified_positions=big + 37, kv_prefix_positions=big + 41,
                   src_positions=big + 53)
    return s


def init_state(drafts: np.ndarray, max_len: int, Ls: int, row_rule: bool = False) -> LoopState:
    """The state a generate call starts from (speculative_decoding.py:80-93): every row runs, holds <BOS> at front 0, the output is
    PAD, width 1, and `while width < max_len` already fails for max_len <= 1."""
    B, N, D = drafts.shape
    s = make_state(B, N, D, max_len, 0, seed=0, Ls=Ls, steps=0, permute=False, row_rule=row_rule)
    s.drafts = np.asarray(drafts, dtype=np.int32).copy()
    s.out[:] = PAD
    if row_rule:
        s.traj[:] = -1
        s.traj[:, 0] = 0
        s.fin_step[:] = 0
    stop = int(1 >= max_len)
    n = 0 if stop else B
    s.words.update(n_active=n, r_rows=n * N, m_rows=n * rps(N, D), stop=stop, width=1, accepted=0, produced=0, verified_positions=0,
                   kv_prefix_positions=0, src_positions=0)
    return s


def other_token(t: int, V: int) -> int:
    """A real token (3 .. V-1) different from ``t``."""
    return 3 + (max(int(t), 3) - 3 + 1) % (V - 3)


def plant(s: LoopState, pred: np.ndarray, slot: int, acc, rng, special=()) -> None:
    """Make the predictions and drafts of running slot ``slot`` such that draft n is accepted for exactly acc[n] tokens.  Row 0 of
    the slot predicts position f for every draft, so acc[n] >= 1 makes the drafts share their first token.  ``special``: (n, j, tok)
    puts ``tok`` at the prediction for position f + j on draft n (j = 0: on all drafts) while keeping the accepted lengths."""
    N, D, V = s.N, s.D, s.V
    b = int(s.act_idx[slot])
    P = rng.integers(3, V, size=(N, D + 1))
    P[:, 0] = P[0, 0]
    for n, j, tok in special:
        if j == 0:
            P[:, 0] = tok
        elif j <= D:
            P[n, j] = tok
    acc = np.asarray(acc, dtype=np.int64)
    assert acc.shape == (N,) and (acc >= 0).all() and (acc <= D).all()
    j = np.arange(D)[None, :]
    tail = rng.integers(3, V, size=(N, D))                               # beyond the first mismatch: anything
    miss = 3 + (np.maximum(P[:, :D], 3) - 3 + 1) % (V - 3)                # other_token of the prediction
    s.drafts[b] = np.where(j < acc[:, None], P[:, :D], np.where(j == acc[:, None], miss, tail))
    R = rps(N, D)
    pred[slot * R] = P[0, 0]
    pred[slot * R + 1:(slot + 1) * R] = P[:, 1:].reshape(-1)


def new_pred(s: LoopState) -> np.ndarray:
    """Predictions for every slot the state could run (B slots), sentinel-free: the rows beyond the running ones are never read."""
    return np.full(s.B * rps(s.N, s.D), 3, dtype=np.int32)


def plant_random(s: LoopState, rng, p_fin: float = 0.0, p_pad: float = 0.0) -> np.ndarray:
    """Seeded predictions for all running slots: random accepted lengths (ties included), and with probability ``p_fin`` an EOS
    (``p_pad``: a PAD) somewhere among the chosen draft's predictions, written or not."""
    pred = new_pred(s)
    for slot in range(int(s.words["n_active"])):
        acc = rng.integers(0, s.D + 1, size=s.N)
        special = []
        if rng.random() < p_fin:
            special.append((int(rng.integers(0, s.N)), int(rng.integers(0, s.D + 1)), EOS))
        if rng.random() < p_pad:
            special.append((int(rng.integers(0, s.N)), int(rng.integers(0, s.D + 1)), PAD))
        plant(s, pred, slot, acc, rng, special)
    return pred


# ---------------------------------------------------------------------------------------------------------------------------
# a state's arrays as guarded operands, and the checker
class DeviceLoop:
    def __init__(self, s: LoopState, device="cpu"):
        self.device = device
        self.bufs = {}
        for name in SLOT_ARRAYS:
            a = getattr(s, name)
            if a is not None:
                self.bufs[name] = Buf(a.shape, DTYPES.get(name, torch.int32), device, a)
        self.pred = Buf((s.B * rps(s.N, s.D),), torch.int32, device)
        self.words = dict(s.words)

    def load(self, s: LoopState) -> None:
        for name, b in self.bufs.items():
            b.set(getattr(s, name))
        self.words = dict(s.words)

    def tensors(self) -> dict:
        return {name: b.v for name, b in self.bufs.items()}

    def entry_words(self) -> list:
        return [int(self.words[k]) for k in STATE_WORDS]

    def set_exit_words(self, words) -> None:
        self.words = dict(zip(WORDS, (int(x) for x in words)))


def check_loop(dev: DeviceLoop, want: LoopState, what: str) -> None:
    """Every array and every word against the restatement's state after the step; margins intact."""
    for name, b in dev.bufs.items():
        check_buf(b, getattr(want, name), f"{what}: {name}")
    m = dev.pred.margins()
    assert m is None, f"{what}: pred: {m}"
    bad = [f"{k}: got {dev.words[k]} expected {want.words[k]}" for k in WORDS if int(dev.words[k]) != int(want.words[k])]
    assert not bad, f"{what}: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------
# the single-step cases of k_accept (shared by the GPU module and the host module's stand-in)
ND = [(1, 1), (3, 10), (7, 17), (23, 5)]
BATCHES = [1, 5, 64, 65, 256, 257, 300, 1024, 1025, 1100]


def tie_patterns(N: int, D: int) -> list:
    """Accepted lengths per draft: 0 .. D on the first, a middle and the last draft alone, and ties in every position order."""
    out = []
    for which in sorted({0, N // 2, N - 1}):
        for a in range(D + 1):
            acc = [0] * N
            acc[which] = a
            out.append(acc)
    hi, lo = D, D // 2
    if N >= 2:
        first, mid, last = 0, N // 2, N - 1
        for pair in ({first, last}, {first, mid}, {mid, last}, set(range(N))):
            for a, b in ((hi, lo), (lo, hi), (hi, hi), (0, 0)):
                out.append([a if n in pair else b for n in range(N)])
    return out


def grid_case(B: int, n_active: int, N: int, D: int, seed: int) -> tuple:
    """Ragged fronts (0 included), a permuted act_idx over n_active of B rows, the tie patterns on the first slots and seeded
    lengths on the rest, an EOS somewhere among the predictions of about a third of the slots."""
    rng = np.random.default_rng(seed)
    max_len = 60
    fronts = rng.integers(0, max_len - D - 3, size=B)
    fronts[rng.integers(0, B)] = 0
    s = make_state(B, N, D, max_len, fronts, n_active=n_active, seed=seed)
    pred = plant_random(s, rng, p_fin=0.35)
    for slot, acc in zip(range(n_active), tie_patterns(N, D)):
        plant(s, pred, slot, acc, rng)
    return s, pred


def eos_case(N: int, D: int, seed: int = 5) -> tuple:
    """One slot per EOS placement around a chosen draft accepted for a = max(D // 2, 1) tokens (the chosen draft is the last one, another
    draft gets a - 1): EOS at each position of the accepted run, as the bonus token, one past it, at the end of the tail, and at
    every position of a draft that was not chosen."""
    rng = np.random.default_rng(seed)
    a = max(D // 2, 1)
    best = N - 1
    acc = [a - 1] * N
    acc[best] = a
    places = [(best, j) for j in range(0, min(a + 2, D + 1))] + [(best, D)]
    if N > 1:
        places += [(0, j) for j in range(1, D + 1)]
    B = len(places) + 1
    s = make_state(B, N, D, 80, rng.integers(0, 40, size=B), seed=seed)
    pred = new_pred(s)
    for slot, (n, j) in enumerate(places):
        plant(s, pred, slot, acc, rng, [(n, j, EOS)])
    plant(s, pred, B - 1, acc, rng)
    return s, pred


def finish_case(B: int, n_fin: int, seed: int, N: int = 3, D: int = 10, threads_note: str = "") -> tuple:
    """Exactly ``n_fin`` of B running rows finish (an EOS as the first written token), scattered over the slots."""
    rng = np.random.default_rng(seed)
    s = make_state(B, N, D, 150, rng.integers(0, 100, size=B), seed=seed)
    pred = new_pred(s)
    fin = set(rng.permutation(B)[:n_fin].tolist())
    for slot in range(B):
        plant(s, pred, slot, rng.integers(0, D + 1, size=N), rng, [(0, 0, EOS)] if slot in fin else [])
    return s, pred


def width_case(delta: int, finisher: bool, seed: int = 9) -> tuple:
    """width = max_len + delta after the step; one row finishes or none does."""
    rng = np.random.default_rng(seed)
    B, N, D, max_len = 6, 3, 10, 50
    fronts = rng.integers(0, 20, size=B)
    fronts[2] = max_len + delta - D - 2
    s = make_state(B, N, D, max_len, fronts, seed=seed)
    pred = new_pred(s)
    for slot in range(B):
        plant(s, pred, slot, rng.integers(0, D + 1, size=N), rng, [(0, 0, EOS)] if finisher and slot == 4 else [])
    return s, pred


def pad_case(all_pad_column: bool, seed: int = 13) -> tuple:
    """A PAD among the written tokens of one row (haspad); with ``all_pad_column`` column 3 is PAD in every running row, which is
    the reference's quirk 2: error 2 and stop."""
    rng = np.random.default_rng(seed)
    B, N, D = 5, 3, 10
    s = make_state(B, N, D, 150, rng.integers(6, 30, size=B), seed=seed)
    if all_pad_column:
        s.gen[:, 3] = PAD
    pred = new_pred(s)
    for slot in range(B):
        plant(s, pred, slot, [4, 2, 0], rng, [(0, 2, PAD)] if slot == 1 else [])
    return s, pred


def row_rule_case(pool: bool, late: bool = False, seed: int = 17) -> tuple:
    """row_rule (``pool``: the slot pool): some rows so far right that they retire with flags 2, some finish, the rest run on;
    ``late``: the step number is beyond traj_ld, so that no traj column may be written."""
    rng = np.random.default_rng(seed)
    B, N, D, max_len = 40, 3, 10, 60
    fronts = rng.integers(0, 30, size=B)
    fronts[::5] = rng.integers(max_len - D - 2, max_len - D + 4, size=len(fronts[::5]))      # f + D + 2 >= max_len
    s = make_state(B, N, D, max_len, fronts, n_active=33, seed=seed, row_rule=True, pool=pool, steps=(max_len + 5 if late else 4))
    if pool and late:
        s.rstep[:] = rng.integers(max_len, max_len + 9, size=B)
    pred = plant_random(s, rng, p_fin=0.5, p_pad=0.1)
    return s, pred


def dedicated_cases() -> list:
    """(name, state, pred) of every constructed single-step case beyond the B x n_active x (N, D) grid."""
    out = []
    for N, D in ND:
        B = len(tie_patterns(N, D))
        out.append((f"lengths-N{N}-D{D}",) + grid_case(B, B, N, D, seed=100 + N))
        out.append((f"eos-N{N}-D{D}",) + eos_case(N, D))
    out.append(("finish-nobody",) + finish_case(300, 0, 21))
    out.append(("finish-everybody-5",) + finish_case(5, 5, 22))
    out.append(("finish-everybody-300",) + finish_case(300, 300, 23))
    out.append(("finish-256-of-1100",) + finish_case(1100, 256, 24))
    out.append(("finish-257-of-1100",) + finish_case(1100, 257, 25))
    out.append(("finish-all-1100",) + finish_case(1100, 1100, 26))
    out.append(("finish-257-of-300",) + finish_case(300, 257, 27))
    out.append(("pad-written",) + pad_case(False))
    out.append(("pad-column-quirk2",) + pad_case(True))
    for delta in (-1, 0, 1, 3):
        for fin in (False, True):
            out.append((f"width-maxlen{delta:+d}-{'finisher' if fin else 'nofinisher'}",) + width_case(delta, fin))
    out.append(("row-rule",) + row_rule_case(False))
    out.append(("row-rule-late",) + row_rule_case(False, late=True))
    out.append(("pool",) + row_rule_case(True))
    out.append(("pool-late",) + row_rule_case(True, late=True))
    return out
