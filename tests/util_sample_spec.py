"""Plain restatement of speculative seeded sampling (include/ttx.h: ttx_sample_speculative_generate; csrc/ttx_sample.hip.h:
k_sample_step; csrc/ttx_loop_kernels.hip.h: k_sample_accept) for the tests: the step row -> (decoder row, position) mapping, the
accept step on a util_loop_checks.LoopState, a host loop that drives both with a float64 sampler, and the constructed single-step
cases.  No GPU call and no test in here.  tests/test_sample_spec_host.py shows on the CPU that the restatement reproduces
position-by-position sampling and that its checkers fail when they should; the GPU modules hold the kernels to it.

The rules are restated from the contract in include/ttx.h, in NumPy over whole batches, not from the kernels.

  step_rows          live step row -> (decoder row b, position it predicts)
  sample_accept_step one accept step under the sampling rule
  init_state         the state a call starts from
  draw_step          the draws of every live step row from a host model: logits(b, prefix) -> float64 [V]
  run_loop           init_state, then draw_step + an accept step until the loop stops
  sequential         the same rows sampled position by position (the plain sampler on the same host model)
"""
from __future__ import annotations

import numpy as np

import util_loop_checks as U
import util_sample_checks as S

PAD, BOS, EOS = U.PAD, U.BOS, U.EOS


def step_rows(act_idx: np.ndarray, front: np.ndarray, n_active: int, N: int, D: int) -> tuple:
    """(b, pos), each [n_active * (1 + N*D)]: step row slot * RPS + rs belongs to decoder row b = act_idx[slot] at front f = front[b];
    rs = 0 predicts position f + 1, the row of token j (0-based) of any draft predicts position f + 2 + j."""
    R = U.rps(N, D)
    rows = np.asarray(act_idx)[:n_active].astype(np.int64)
    ahead = np.concatenate([[1], np.tile(2 + np.arange(D), N)])
    b = np.repeat(rows, R)
    pos = np.repeat(np.asarray(front)[rows].astype(np.int64), R) + np.tile(ahead, n_active)
    return b, pos


def sample_accept_step(state: U.LoopState, pred: np.ndarray) -> U.LoopState:
    """One accept step under the sampling rule, returning the new state.

    For each running slot: a draft's accepted length is the leading run of agreement between the draft and the draws; the best
    draft is the FIRST maximum; draws j = 0 .. n_acc of the best draft are written after the front (the last one is the bonus
    token) and the front moves by n_acc + 1.  A row ends (flags 1) iff a written token in a column below max_len is EOS or PAD, or
    its new front is >= max_len - 1.  Ended rows go to out[row, :max_len]; the running list is compacted in order and the entries
    beyond the new count stay as they were.  width = max(old fronts) + D + 2.  The loop stops when nobody runs.  haspad and error
    are not touched."""
    s = state.clone()
    w = s.words
    w.update(dict.fromkeys(U.WORDS[13:], -1))
    Bc = int(w["n_active"])
    if Bc == 0:
        return s
    N, D, R = s.N, s.D, U.rps(s.N, s.D)
    rows = s.act_idx[:Bc].copy()
    f = s.front[rows].astype(np.int64)
    P = U.gather_pred(pred, Bc, N, D)
    n_ok = np.cumprod(s.drafts[rows] == P[:, :, :D], axis=2).sum(axis=2)
    best = n_ok.argmax(axis=1)
    ar = np.arange(Bc)
    n_acc = n_ok[ar, best]
    chosen = P[ar, best]
    written = np.arange(D + 1)[None, :] <= n_acc[:, None]
    cols = f[:, None] + 1 + np.arange(D + 1)[None, :]
    s.gen[rows[:, None].repeat(D + 1, 1)[written], cols[written]] = chosen[written]
    new_front = f + n_acc + 1
    s.front[rows] = new_front
    ending = written & ((chosen == s.eos) | (chosen == s.pad)) & (cols < s.max_len)
    fin = ending.any(axis=1) | (new_front >= s.max_len - 1)
    s.rec[:Bc] = np.stack([rows, best, n_acc, f, fin.astype(np.int64)], axis=1)
    s.out[rows[fin], :s.max_len] = s.gen[rows[fin], :s.max_len]
    kept = rows[~fin]
    nn = len(kept)
    s.act_idx[:nn] = kept
    width = int(f.max()) + D + 2
    w["n_copy"] = Bc
    w["steps"] += 1
    w["accepted"] += int(n_acc.sum())
    w["produced"] += int(n_acc.sum()) + Bc
    w["verified_positions"] += Bc * R
    w["kv_prefix_positions"] += int(f.sum())
    w["src_positions"] += Bc * s.Ls
    w["width"] = width
    stop = nn == 0
    w["stop"] = int(stop)
    w["n_active"], w["r_rows"], w["m_rows"] = nn, nn * N, nn * R
    w["host_width"], w["host_n_active"], w["host_stop"], w["host_steps_done"] = width, nn, int(stop), w["steps"]
    return s


def init_state(drafts: np.ndarray, max_len: int, Ls: int) -> U.LoopState:
    """What a call starts from: util_loop_checks.init_state with the plain sampler's output (BOS in column 0, PAD behind it)."""
    s = U.init_state(drafts, max_len, Ls)
    s.out[:, 0] = BOS
    return s


def make_state(B: int, N: int, D: int, max_len: int, fronts, n_active=None, seed: int = 0, V: int = 40) -> U.LoopState:
    """util_loop_checks.make_state as this path holds it: haspad stays zero and the drafts hold neither EOS nor PAD."""
    return U.make_state(B, N, D, max_len, fronts, n_active=n_active, seed=seed, V=V)


def check_state(got: U.LoopState, want: U.LoopState, what: str) -> None:
    """Every array and word of ``got`` against ``want``: exact equality (the host module's checker; the GPU modules use
    util_loop_checks.check_loop, which adds the guard margins)."""
    for name in U.SLOT_ARRAYS:
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), f"{what}: {name}"
        if a is not None:
            d = U.first_difference(np.asarray(a), np.asarray(b))
            assert d is None, f"{what}: {name}: {d}"
    bad = [f"{k}: got {got.words[k]} expected {want.words[k]}" for k in U.WORDS if int(got.words[k]) != int(want.words[k])]
    assert not bad, f"{what}: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------
# a host loop on a host model
def draw_step(s: U.LoopState, logits_of, key: np.ndarray, sample: np.ndarray, seed: int, p: S.Params, rows_fn=step_rows) -> np.ndarray:
    """pred [B * RPS]: for every live step row the float64 sampler's token from the host model's logits for the row's own prefix
    (the decoder row's tokens through its front, then the draft tokens up to the row's) and the uniform of the (b, pos) that
    ``rows_fn`` gives.  The rows beyond the live ones hold 3."""
    pred = U.new_pred(s)
    n = int(s.words["n_active"])
    b, pos = rows_fn(s.act_idx, s.front, n, s.N, s.D)
    R = U.rps(s.N, s.D)
    for row in range(n * R):
        slot, rs = divmod(row, R)
        br = int(s.act_idx[slot])                   # the prefix is the layout's; (b, pos) only key the draw
        prefix = list(s.gen[br, :s.front[br] + 1])
        if rs:
            d, j = divmod(rs - 1, s.D)
            prefix += list(s.drafts[br, d, :j + 1])
        u = float(S.uniform(seed, key[b[row]], sample[b[row]], int(pos[row])))
        pred[row] = S.sample64(logits_of(br, tuple(int(t) for t in prefix)), u, p)
    return pred


def run_loop(drafts: np.ndarray, max_len: int, logits_of, key, sample, seed: int, p: S.Params, step_fn=sample_accept_step,
             rows_fn=step_rows) -> U.LoopState:
    """The whole loop on the host; returns the final state (``out`` [B, max_len], ``words``)."""
    s = init_state(drafts, max_len, Ls=drafts.shape[2] + 2)
    steps = 0
    while not s.words["stop"]:
        steps += 1
        assert steps <= max_len + 2, "the loop did not end by itself"
        s = step_fn(s, draw_step(s, logits_of, key, sample, seed, p, rows_fn))
    return s


def sequential(B: int, max_len: int, logits_of, key, sample, seed: int, p: S.Params) -> np.ndarray:
    """[B, max_len]: the plain sampler on the same host model: BOS, one token per position until EOS, PAD or the last column."""
    out = np.full((B, max_len), PAD, dtype=np.int64)
    out[:, 0] = BOS
    for b in range(B):
        for pos in range(1, max_len):
            t = S.sample64(logits_of(b, tuple(int(x) for x in out[b, :pos])), float(S.uniform(seed, key[b], sample[b], pos)), p)
            out[b, pos] = t
            if t in (EOS, PAD):
                break
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# constructed single-step cases of the accept step (shared by the GPU module and the host module's stand-in)
def lengths_case(N: int, D: int, seed: int = 3) -> tuple:
    """Accepted lengths 0 .. D on each draft and ties in every order (util_loop_checks.tie_patterns), far from max_len."""
    rng = np.random.default_rng(seed)
    pats = U.tie_patterns(N, D)
    B = len(pats) + 2
    s = make_state(B, N, D, 80, rng.integers(0, 40, size=B), n_active=len(pats), seed=seed)
    pred = U.new_pred(s)
    for slot, acc in enumerate(pats):
        U.plant(s, pred, slot, acc, rng)
    return s, pred


def ending_case(N: int, D: int, seed: int = 5) -> tuple:
    """EOS and PAD as the bonus token after every accepted length (rows end), and EOS / PAD one past the bonus token, at the end of
    the chosen draft's draws and on a draft that was not chosen (rows run on).  The chosen draft is the last one."""
    rng = np.random.default_rng(seed)
    best = N - 1
    cases = []
    for a in range(D + 1):
        acc = [max(a - 1, 0)] * N
        acc[best] = a
        for tok in (EOS, PAD):
            cases.append((acc, [(best, a, tok)]))                         # the bonus token: position a of the chosen draft's draws
            if a + 1 <= D:
                cases.append((acc, [(best, a + 1, tok)]))                 # one past it: not written
        if N > 1 and a >= 1:
            cases.append((acc, [(0, D, EOS)]))                            # a draft that was not chosen
    B = len(cases) + 1
    s = make_state(B, N, D, 90, rng.integers(0, 40, size=B), seed=seed)
    pred = U.new_pred(s)
    for slot, (acc, special) in enumerate(cases):
        U.plant(s, pred, slot, acc, rng, special)
    U.plant(s, pred, B - 1, [0] * N, rng)
    return s, pred


def limit_case(N: int, D: int, seed: int = 7) -> tuple:
    """Fronts around max_len - 1: for every accepted length a, old fronts such that the new front lands on max_len - 2 (runs on),
    max_len - 1 exactly and max_len .. max_len - 1 + D (overshoot by 1 .. D; only reachable when a is large enough); with an EOS as the
    bonus token in a kept column and in a dropped one."""
    rng = np.random.default_rng(seed)
    max_len = 3 * D + 9
    cases = []
    for a in range(D + 1):
        for land in range(max_len - 2, max_len + D):
            f = land - a - 1
            if f > max_len - 2:                                           # such a row is not running any more
                continue
            cases.append((f, a, None))
            cases.append((f, a, EOS))
    B = len(cases)
    s = make_state(B, N, D, max_len, max_len - 2, seed=seed)             # real tokens up to column max_len - 2 in every row
    for slot, (f, _, _) in enumerate(cases):
        b = int(s.act_idx[slot])
        s.front[b] = f
        s.gen[b, f + 1:] = PAD
    s.words["width"] = int(s.front.max()) + 1
    pred = U.new_pred(s)
    for slot, (f, a, tok) in enumerate(cases):
        acc = [0] * N
        acc[N // 2] = a
        U.plant(s, pred, slot, acc, rng, [] if tok is None else [(N // 2, a, tok)])
    return s, pred


def retire_case(B: int, n_fin: int, seed: int, N: int = 2, D: int = 2) -> tuple:
    """Exactly ``n_fin`` of B running rows end (an EOS or a PAD as the first written token), scattered over the slots."""
    rng = np.random.default_rng(seed)
    s = make_state(B, N, D, 60, rng.integers(0, 40, size=B), seed=seed)
    pred = U.new_pred(s)
    fin = set(rng.permutation(B)[:n_fin].tolist())
    for slot in range(B):
        if slot in fin:                                                   # nothing accepted: a draft never holds EOS or PAD
            U.plant(s, pred, slot, [0] * N, rng, [(0, 0, EOS if slot % 2 else PAD)])
        else:
            U.plant(s, pred, slot, rng.integers(0, D + 1, size=N), rng)
    return s, pred


ND = [(1, 1), (1, 3), (3, 2), (2, 5)]


def accept_cases() -> list:
    out = []
    for N, D in ND:
        out.append((f"lengths-N{N}-D{D}",) + lengths_case(N, D))
        out.append((f"ending-N{N}-D{D}",) + ending_case(N, D))
        out.append((f"limit-N{N}-D{D}",) + limit_case(N, D))
    out.append(("retire-some-of-40",) + retire_case(40, 13, 11))
    out.append(("retire-all-of-7",) + retire_case(7, 7, 12))
    out.append(("retire-none-of-7",) + retire_case(7, 0, 13))
    out.append(("B1-runs",) + retire_case(1, 0, 14))
    out.append(("B1-ends",) + retire_case(1, 1, 15))
    out.append(("retire-120-of-300",) + retire_case(300, 120, 16))
    out.append(("retire-270-of-300",) + retire_case(300, 270, 17))       # more than the finished-row list holds
    out.append(("retire-all-of-300",) + retire_case(300, 300, 18))
    out.append(("retire-400-of-1100",) + retire_case(1100, 400, 19))     # two rounds of the slot loop at 1 024 threads
    return out


ACCEPT_CASE_NAMES = [f"{k}-N{N}-D{D}" for N, D in ND for k in ("lengths", "ending", "limit")] + \
    ["retire-some-of-40", "retire-all-of-7", "retire-none-of-7", "B1-runs", "B1-ends", "retire-120-of-300", "retire-270-of-300",
     "retire-all-of-300", "retire-400-of-1100"]
