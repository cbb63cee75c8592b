"""Helpers of the score-list tests: a NumPy restatement of k_sl_extents, k_sl_pack, k_sl_unpack (csrc/ttx_score_list.hip.h) and of
scheduling.score_plan, written from the rules in include/ttx.h, and a checker that names the first differing batch, row and
column.  A batch is a dict {"src": int64 [B, Ls], "hyp": int64 [B, N, W]}; sources and hypothesis rows are numbered in list order."""
from __future__ import annotations

import numpy as np

PAD, BOS, EOS = 0, 1, 2


def row_n(h, pad: int = PAD, eos: int = EOS) -> int:
    """The column of the first EOS at a column >= 1, else the last column >= 1 holding a non-PAD token, else 0."""
    h = np.asarray(h)
    for c in range(1, len(h)):
        if h[c] == eos:
            return c
    for c in range(len(h) - 1, 0, -1):
        if h[c] != pad:
            return c
    return 0


def locate(batches: list, s: int) -> tuple:
    """(batch, row of the batch) of source s of the list."""
    for i, b in enumerate(batches):
        if s < b["src"].shape[0]:
            return i, s
        s -= b["src"].shape[0]
    raise IndexError("source outside the list")


def extents(batches: list, pad: int = PAD, eos: int = EOS) -> tuple:
    """(e int32 [S], ls int32 [S], n int32 [R])."""
    e, ls, n = [], [], []
    for b in batches:
        for x, rows in zip(b["src"], b["hyp"]):
            ns = [row_n(h, pad, eos) for h in rows]
            n += ns
            e.append(max(2, 1 + max(ns)))
            nz = np.flatnonzero(np.asarray(x) != pad)
            ls.append(max(1, 1 + (int(nz[-1]) if len(nz) else -1)))
    return np.asarray(e, np.int32), np.asarray(ls, np.int32), np.asarray(n, np.int32)


def pack(batches: list, sel, N: int, Wc: int, Lsc: int, pad: int = PAD) -> tuple:
    """(src_c int64 [Bc, Lsc], hyp_c int64 [Bc * N, Wc]) of the chunk whose sources are ``sel``."""
    src_c = np.full((len(sel), Lsc), pad, np.int64)
    hyp_c = np.full((len(sel) * N, Wc), pad, np.int64)
    for j, s in enumerate(sel):
        i, b = locate(batches, int(s))
        x, h = np.asarray(batches[i]["src"][b]), np.asarray(batches[i]["hyp"][b])
        assert h.shape[0] == N
        src_c[j, :min(len(x), Lsc)] = x[:Lsc]
        hyp_c[j * N:(j + 1) * N, :min(h.shape[1], Wc)] = h[:, :Wc]
    return src_c, hyp_c


def unpack(batches: list, sel, N: int, Wc: int, score_c, length_c, fin_c, tok_c, out: dict) -> dict:
    """Scatter a chunk's results into ``out``: {"score", "length", "finished": per batch [B, N]; "tok": per batch [B, N, W_i - 1]},
    arrays that keep whatever they held where the chunk writes nothing."""
    for j, s in enumerate(sel):
        i, b = locate(batches, int(s))
        Wi = batches[i]["hyp"].shape[2]
        for k in range(N):
            g = j * N + k
            out["score"][i][b, k], out["length"][i][b, k], out["finished"][i][b, k] = score_c[g], length_c[g], fin_c[g]
            if tok_c is not None:
                m = min(Wc, Wi) - 1
                out["tok"][i][b, k, :m] = tok_c[g, :m]
                out["tok"][i][b, k, m:] = 0.0
    return out


def plan(N_of, e, ls, max_rows: int) -> list:
    """score_plan restated with plain loops: [(sources, N, W, Ls)], in run order."""
    S = len(N_of)
    order = sorted(range(S), key=lambda s: (int(N_of[s]), int(e[s]), int(ls[s]), s))
    chunks, cur = [], []
    for s in order:
        if cur:
            W = max(int(e[t]) for t in cur + [s])
            if N_of[s] != N_of[cur[0]] or (len(cur) + 1) * int(N_of[s]) * (W - 1) > max_rows:
                chunks.append(cur)
                cur = []
        cur.append(s)
    chunks.append(cur)
    out = [(c, int(N_of[c[0]]), max(int(e[s]) for s in c), max(int(ls[s]) for s in c)) for c in chunks]
    idx = sorted(range(len(out)), key=lambda c: (-len(out[c][0]) * out[c][1] * (out[c][2] - 1), c))
    return [out[c] for c in idx]


def first_difference(got: list, want: list, what: str = "value"):
    """None when the per-batch arrays agree exactly (NaN equal to NaN, shapes included), else a message naming the first differing
    batch, row and column.  ``got`` / ``want``: one array per batch, [rows...] or [rows..., columns]."""
    if len(got) != len(want):
        return f"{what}: {len(got)} batches for {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape:
            return f"{what}: batch {i} has shape {g.shape}, expected {w.shape}"
        same = (g == w) | ((g != g) & (w != w))
        if not same.all():
            idx = tuple(int(x) for x in np.argwhere(~same)[0])
            row, col = (idx[:-1], idx[-1]) if g.ndim >= 2 else (idx, None)
            return (f"{what}: batch {i}, row {row if len(row) != 1 else row[0]}" + (f", column {col}" if col is not None else "") +
                    f": got {g[idx].item()!r}, expected {w[idx].item()!r}")
    return None


def make_batch(rng: np.random.Generator, B: int, Ls: int, N: int, W: int, V: int = 12) -> dict:
    """Random tokens in [3, V), column 0 = BOS: every row full and unfinished until a test edits it."""
    hyp = rng.integers(3, V, (B, N, W)).astype(np.int64)
    hyp[:, :, 0] = BOS
    return {"src": rng.integers(3, V, (B, Ls)).astype(np.int64), "hyp": hyp}
