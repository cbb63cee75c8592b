"""NumPy restatement of k_syntax_mask (csrc/ttx_syntax.hip.h; include/ttx.h "Syntax-constrained sampling" is the contract).

A syntax table gives one int8 class per vocabulary id: -1 FORBID, 1 OPEN, 2 CLOSE, 3 + l ring label l (0 <= l < 64), anything else
neutral.  For a row prefix P (the tokens after BOS; an id outside [0, V) and a FORBID token count as neutral)
    depth = #OPEN - #CLOSE,   R = XOR of 1 << l over its ring tokens,   need = max(depth, 0) + popcount(R),
and for the position pos being predicted left = (max_len - 1) - pos.  Token v keeps its logit's BITS if it is allowed, otherwise the
logit becomes -inf:
    EOS (the call's, whatever its class): depth == 0 and R == 0;  FORBID: never;  neutral: need + 1 <= left;  OPEN: need + 2 <= left;
    CLOSE: depth > 0;  ring l with bit l set in R: always;  ring l with bit l clear: need + 2 <= left.
Rows at or beyond ``m_live`` are not written.  The three row mappings are written out below from the arrays the kernel reads; each
gives, per logits row, the list of prefix tokens and the position.
"""
import numpy as np

FORBID, OPEN, CLOSE, RING0, RINGS = -1, 1, 2, 3, 64


def step_rps(N: int, D: int) -> int:
    """Rows per slot of a verify step: the front row and D rows for each of the N drafts."""
    return 1 + N * D


# -- the rule ------------------------------------------------------------------------------------------------------------------------
def state(cls, prefix) -> tuple:
    """(depth, R) of a prefix, R as a Python integer of up to 64 bits."""
    cls = np.asarray(cls)
    depth, ring = 0, 0
    for t in prefix:
        t = int(t)
        if not 0 <= t < len(cls):
            continue
        c = int(cls[t])
        if c == OPEN:
            depth += 1
        elif c == CLOSE:
            depth -= 1
        elif RING0 <= c < RING0 + RINGS:
            ring ^= 1 << (c - RING0)
    return depth, ring


def need_of(depth: int, ring: int) -> int:
    return max(depth, 0) + bin(ring).count("1")


def allowed(cls, depth: int, ring: int, pos: int, max_len: int, eos: int) -> np.ndarray:
    """Bool[V]: the tokens a row in state (depth, R) may emit at column ``pos`` of ``max_len``."""
    cls = np.asarray(cls).astype(np.int64)
    V = len(cls)
    left = (max_len - 1) - pos
    need = need_of(depth, ring)
    is_ring = (cls >= RING0) & (cls < RING0 + RINGS)
    label = np.where(is_ring, cls - RING0, 0)
    open_bits = np.array([(ring >> l) & 1 for l in range(RINGS)], dtype=bool)
    closes = is_ring & open_bits[label]
    ok = np.full(V, need + 1 <= left)                       # neutral, and every class value that is not listed
    ok[cls == FORBID] = False
    ok[cls == OPEN] = need + 2 <= left
    ok[cls == CLOSE] = depth > 0
    ok[is_ring] = need + 2 <= left
    ok[closes] = True
    if 0 <= eos < V:
        ok[eos] = depth == 0 and ring == 0
    return ok


# -- the three row mappings: per logits row (prefix tokens, position) ---------------------------------------------------------------------
def rows_plain(tok, front0: int, M: int) -> list:
    """k_sample's rows: the prefix of row r is tok[r][1 .. front0], pos = front0 + 1."""
    tok = np.asarray(tok)
    return [(tok[r, 1:front0 + 1].tolist(), front0 + 1) for r in range(M)]


def rows_step(tok, front, act_idx, drafts, M: int, N: int, D: int, row_map=None) -> list:
    """k_sample_step's layout: lrow = row_map ? row_map[row] : row, b = act_idx[lrow // RPS], rs = lrow % RPS, f = front[b];
    rs == 0: tok[b][1 .. f], pos = f + 1;  rs = 1 + n * D + j: tokens 0 .. j of draft n of b appended, pos = f + 2 + j."""
    tok, front, act_idx = np.asarray(tok), np.asarray(front), np.asarray(act_idx)
    rps = step_rps(N, D)
    out = []
    for row in range(M):
        lrow = row if row_map is None else int(np.asarray(row_map)[row])
        b, rs = int(act_idx[lrow // rps]), lrow % rps
        f = int(front[b])
        prefix, pos = tok[b, 1:f + 1].tolist(), f + 1
        if rs != 0 and D > 0:
            n, j = (rs - 1) // D, (rs - 1) % D
            prefix = prefix + np.asarray(drafts)[b, n, :j + 1].tolist()
            pos = f + 2 + j
        out.append((prefix, pos))
    return out


def rows_teacher(hyp, M: int, T: int) -> list:
    """Teacher-forced logits [R, T, V]: row r * T + t takes hyp[r][1 .. t], pos = t + 1 (k_hyp_logq's positions)."""
    hyp = np.asarray(hyp)
    return [(hyp[row // T, 1:row % T + 1].tolist(), row % T + 1) for row in range(M)]


# -- the masked logits and the checker -------------------------------------------------------------------------------------------------------
def mask_rows(cls, rows, max_len: int, eos: int) -> np.ndarray:
    """Bool[len(rows), V]: the allowed set of every (prefix, pos)."""
    return np.stack([allowed(cls, *state(cls, p), pos, max_len, eos) for p, pos in rows])


def apply(logits_f32: np.ndarray, cls, rows, max_len: int, eos: int, m_live: int | None = None) -> np.ndarray:
    """The masked logits [M, V] (a new array): in rows below ``m_live`` (default: all) the forbidden ids become -inf, every other
    entry keeps its bits."""
    x = np.array(logits_f32, dtype=np.float32, copy=True)
    M = x.shape[0]
    live = M if m_live is None else min(int(m_live), M)
    if live:
        ok = mask_rows(cls, rows[:live], max_len, eos)
        xb = x.view(np.uint32)
        xb[:live][~ok] = np.array([-np.inf], dtype=np.float32).view(np.uint32)[0]
    return x


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def first_difference(got: np.ndarray, want: np.ndarray):
    """(row, token) of the first entry whose BITS differ, or None."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"shape {g.shape} against {w.shape}"
    d = np.argwhere(g != w)
    return None if len(d) == 0 else (int(d[0][0]), int(d[0][1]))


def check(got: np.ndarray, logits_f32, cls, rows, max_len: int, eos: int, m_live=None, what: str = "") -> None:
    """AssertionError naming the first (row, token) at which ``got`` is not the restatement, on the bits."""
    want = apply(logits_f32, cls, rows, max_len, eos, m_live)
    at = first_difference(got, want)
    if at is not None:
        r, v = at
        live = "live" if m_live is None or r < m_live else "dead"
        st = ""
        if live == "live":
            depth, ring = state(cls, rows[r][0])
            st = f"; depth {depth}, R {ring:#x}, pos {rows[r][1]}, class {int(np.asarray(cls)[v])}"
        raise AssertionError(f"{what}: row {r} ({live}) token {v}: got bits {bits(got)[r, v]:#010x}, the rule gives "
                             f"{bits(want)[r, v]:#010x} from logit bits {bits(logits_f32)[r, v]:#010x}{st}")


# -- row checks on generated rows ------------------------------------------------------------------------------------------------------------
def row_report(cls, row, eos: int) -> tuple:
    """(finished, balanced, holds a FORBID token) of an output row (BOS in column 0; columns after the first EOS are not read)."""
    cls = np.asarray(cls)
    toks = []
    finished = False
    for t in row[1:]:
        if int(t) == eos:
            finished = True
            break
        toks.append(int(t))
    depth, ring = state(cls, toks)
    forbid = any(0 <= t < len(cls) and cls[t] == FORBID for t in toks)
    return finished, depth == 0 and ring == 0, forbid


# -- inputs of the kernel tests ------------------------------------------------------------------------------------------------------------
NAN_PAYLOADS = np.array([0x7FC01234, 0xFFC0BEEF, 0x7F800001], dtype=np.uint32).view(np.float32)


def make_logits(rng, M: int, V: int) -> np.ndarray:
    """Random logits with signed zeros, -inf and NaNs with payloads spread over them: the kernel must not read, let alone change, any."""
    x = (rng.standard_normal((M, V)) * 4).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    flat[rng.choice(n, max(1, n // 9), replace=False)] = np.float32(-0.0)
    flat[rng.choice(n, max(1, n // 13), replace=False)] = np.float32(0.0)
    flat[rng.choice(n, max(1, n // 11), replace=False)] = -np.inf
    idx = rng.choice(n, max(3, n // 17), replace=False)
    flat.view(np.uint32)[idx] = NAN_PAYLOADS.view(np.uint32)[np.arange(len(idx)) % 3]
    return x


def make_cls(rng, V: int, labels=(0, 1, 5, 63), n_open: int = 2, n_close: int = 2, n_forbid: int = 3) -> np.ndarray:
    """A table over V ids: ids 0, 1, 3 forbidden (PAD, BOS, "?" of the fixture layout; 2 is EOS and stays neutral), then opens,
    closes and two ids per ring label spread over the rest, and two values outside the listed classes (they count as neutral)."""
    cls = np.zeros(V, dtype=np.int8)
    cls[[0, 1, 3][:n_forbid]] = FORBID
    free = rng.permutation(np.arange(4, V))
    k = 0
    for c, n in ((OPEN, n_open), (CLOSE, n_close)):
        cls[free[k:k + n]] = c
        k += n
    for l in labels:
        n = 2 if V > 40 else 1
        cls[free[k:k + n]] = RING0 + l
        k += n
    if V > 60:
        cls[free[k]], cls[free[k + 1]] = 100, -7
    return cls


def ids_of(cls, c: int) -> np.ndarray:
    return np.nonzero(np.asarray(cls) == c)[0]


def random_prefix(rng, cls, length: int, eos: int) -> list:
    """``length`` tokens drawn so that depth never goes negative; opens, closes and ring tokens are frequent."""
    cls = np.asarray(cls)
    V = len(cls)
    special = np.nonzero((cls > 0) & (cls < RING0 + RINGS))[0]
    neutral = np.nonzero(cls == 0)[0]
    neutral = neutral[neutral != eos]
    out, depth = [], 0
    for _ in range(length):
        t = int(rng.choice(special)) if rng.random() < 0.5 and len(special) else int(rng.integers(4, V))
        if t == eos or (cls[t] == CLOSE and depth == 0):
            t = int(rng.choice(neutral))
        depth += int(cls[t] == OPEN) - int(cls[t] == CLOSE)
        out.append(t)
    return out
