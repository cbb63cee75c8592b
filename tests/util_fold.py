"""Helpers of the fold tests (no test in here): a NumPy restatement of the rule of ttx_fold_hypotheses, written from the contract
in include/ttx.h and not from the kernel, a checker that names the first differing (output, source, index), the row layouts the
kernel tests fold, and one guarded call of the entry point on device arrays."""
import functools
import math

import numpy as np

FIRST, SCORE, COUNT = 0, 1, 2
UNFINISHED_LAST, DEBUG_NO_FILTER = 1, 2
OUTPUTS = ("first", "rank_of", "n_unique", "perm", "count", "score", "out", "logmass")


def row_extent(row, eos):
    """(c, finished) of one row: c = the column of the first eos + 1, or the row's width when it holds none."""
    hits = np.nonzero(np.asarray(row) == eos)[0]
    return (int(hits[0]) + 1, True) if hits.size else (len(row), False)


def fold_reference(hyp, scores=None, order=SCORE, flags=0, pad=0, eos=2):
    """The rule.  hyp int64 [B, N, W]; scores float32 [B, N] or None.  Returns a dict of the eight outputs as NumPy arrays
    (``logmass`` float32 and ``logmass64`` the float64 value it was rounded from; both None without scores)."""
    hyp = np.asarray(hyp, dtype=np.int64)
    B, N, W = hyp.shape
    if scores is None and order == SCORE:
        raise ValueError("the SCORE order needs scores")
    sc = None
    if scores is not None:
        sc = np.asarray(scores, dtype=np.float32).copy()
        sc[np.isnan(sc)] = -np.inf
    unf_last = bool(flags & UNFINISHED_LAST)
    res = {"first": np.zeros((B, N), np.int32), "rank_of": np.zeros((B, N), np.int32), "n_unique": np.zeros(B, np.int32),
           "perm": np.full((B, N), -1, np.int32), "count": np.zeros((B, N), np.int32),
           "score": np.full((B, N), -np.inf, np.float32), "out": np.full((B, N, W), pad, np.int64),
           "logmass": None if sc is None else np.zeros(B, np.float32), "logmass64": None if sc is None else np.zeros(B, np.float64)}
    for b in range(B):
        seen, first, fin = {}, [], []
        for j in range(N):
            c, f = row_extent(hyp[b, j], eos)
            key = (c, tuple(int(t) for t in hyp[b, j, :c]))
            first.append(seen.setdefault(key, j))
            fin.append(f)
        reps = [j for j in range(N) if first[j] == j]
        count = {a: sum(1 for j in range(N) if first[j] == a) for a in reps}

        def precedes(a, c):
            if unf_last and fin[a] != fin[c]:
                return fin[a]
            if order == COUNT and count[a] != count[c]:
                return count[a] > count[c]
            if order == SCORE or (order == COUNT and sc is not None):
                if sc[b, a] > sc[b, c]:
                    return True
                if sc[b, a] < sc[b, c]:
                    return False
            return a < c

        ranked = sorted(reps, key=functools.cmp_to_key(lambda a, c: 0 if a == c else (-1 if precedes(a, c) else 1)))
        rank = {a: r for r, a in enumerate(ranked)}
        U = len(ranked)
        res["first"][b] = first
        res["rank_of"][b] = [rank[first[j]] for j in range(N)]
        res["n_unique"][b] = U
        for r, a in enumerate(ranked):
            res["perm"][b, r] = a
            res["count"][b, r] = count[a]
            if sc is not None:
                res["score"][b, r] = sc[b, a]
            res["out"][b, r] = hyp[b, a]
        if sc is not None:
            m = max(float(sc[b, a]) for a in ranked)
            if m == -math.inf:
                v = -math.inf
            else:
                acc = 0.0
                for a in ranked:
                    acc += math.exp(float(sc[b, a]) - m)
                v = m + math.log(acc)
            res["logmass64"][b] = v
            res["logmass"][b] = np.float32(v)
    return res


def logmass_ok(got, want64):
    """|got - fp32(want64)| within one fp32 spacing of the rounded float64 value; an infinite value must match exactly."""
    w = np.float32(want64)
    if not np.isfinite(w):
        return bool(got == w)
    return bool(np.isfinite(got)) and abs(float(got) - float(w)) <= float(np.spacing(np.abs(w)))


def first_difference(got: dict, want: dict, names=OUTPUTS):
    """None when every output of ``got`` named in ``names`` (and present, not None) equals the restatement's, else
    ``(output, source, index)`` of the first difference.  Floats are compared on their bits (``score``), ``logmass`` by
    ``logmass_ok``."""
    for name in names:
        g = got.get(name)
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(want[name])
        if g.shape != w.shape:
            return (name, -1, -1)
        if name == "logmass":
            for b in range(g.shape[0]):
                if not logmass_ok(g[b], want["logmass64"][b]):
                    return (name, b, 0)
            continue
        if name == "score":
            g, w = g.view(np.int32), w.view(np.int32)
        bad = np.argwhere(g != w)
        if bad.size:
            return (name, int(bad[0][0]), int(bad[0][1]) if bad.shape[1] > 1 else 0)
    return None


def assert_fold_equal(got: dict, want: dict, names=OUTPUTS, what: str = ""):
    d = first_difference(got, want, names)
    if d is not None:
        name, b, i = d
        g, w = np.asarray(got[name]), np.asarray(want[name])
        detail = f"got {g[b].ravel()[:16]} want {w[b].ravel()[:16]}" if b >= 0 else f"shapes {g.shape} / {w.shape}"
        raise AssertionError(f"{what}: output {name!r} differs first at source {b}, index {i}: {detail}")


# ---- row layouts: one source's [N, W] block each.  Tokens are drawn from [3, 40) unless a layout says otherwise. ----
LAYOUTS = ("equal", "distinct", "last_col", "after_eos", "col0", "eos0", "no_eos", "eos_last", "prefix", "bit40", "mixed")


def _body(rng, W):
    return rng.integers(3, 40, size=W, dtype=np.int64)


def layout_rows(kind: str, N: int, W: int, rng, pad: int = 0, eos: int = 2):
    rows = np.empty((N, W), np.int64)
    base = _body(rng, W)
    if kind == "equal":                                   # all rows equal (an EOS in the middle when there is room)
        if W >= 3:
            base[W // 2] = eos
        rows[:] = base
    elif kind == "distinct":                              # all rows distinct: a row's index sits in column 0 (no row is the EOS)
        rows[:] = base
        rows[:, 0] = 100 + np.arange(N)
        if W >= 2:
            rows[:, W - 1] = eos
    elif kind == "last_col":                              # differ only in the last compared column: W - 1 without an EOS, and
        rows[:] = base                                    # the column before the EOS with one
        half = N // 2
        rows[:half, W - 1] = 50 + (np.arange(half) % 3)
        if W >= 2:
            rows[half:, W - 1] = eos
            rows[half:, W - 2] = 60 + (np.arange(N - half) % 3)
        else:
            rows[half:, 0] = 70
    elif kind == "after_eos":                             # equal up to the EOS, noise behind it: must fold
        e = min(W - 1, max(0, W // 3))
        for j in range(N):
            rows[j] = _body(rng, W)
            rows[j, :e] = base[:e]
            rows[j, e] = eos
            if j % 3 == 1 and e + 1 < W:
                rows[j, e + 1] = eos                      # a second EOS behind the first changes nothing
    elif kind == "col0":                                  # differ only in column 0, three values
        if W >= 2:
            base[W - 1] = eos
        rows[:] = base
        rows[:, 0] = 80 + (np.arange(N) % 3)
    elif kind == "eos0":                                  # EOS in column 0: one hypothesis whatever follows; a few rows differ
        for j in range(N):
            rows[j] = _body(rng, W)
            rows[j, 0] = eos if j % 4 != 3 else 90
    elif kind == "no_eos":                                # no EOS: the whole row is compared, PAD included
        for j in range(N):
            rows[j] = base
            cut = W - (j % 3)
            rows[j, cut:] = pad
    elif kind == "eos_last":                              # EOS in the last column against the same row without it
        rows[:] = base
        rows[::2, W - 1] = eos
        rows[1::2, W - 1] = 95
    elif kind == "prefix":                                # rows of different length sharing a prefix
        for j in range(N):
            rows[j] = base
            e = (j * 7) % W
            rows[j, e] = eos
            rows[j, e + 1:] = pad
    elif kind == "bit40":                                 # ids that differ only in bit 40
        if W >= 2:
            base[W - 1] = eos
        rows[:] = base
        rows[1::2, 0] = base[0] + (1 << 40)
    elif kind == "mixed":                                 # a small pool of hypotheses drawn with repeats
        pool = []
        for k in range(max(1, min(N, 6))):
            r = _body(rng, W)
            if k % 3 != 2:
                e = int(rng.integers(0, W))
                r[e] = eos
                r[e + 1:] = pad
            pool.append(r)
        for j in range(N):
            rows[j] = pool[int(rng.integers(0, len(pool)))]
    else:
        raise ValueError(kind)
    return rows


SPECIAL_SCORES = np.array([0.0, -0.0, -np.inf, 1e-40, -1e-40, -1.5, -1.5, -3.25, 2.0], np.float32)


def case_scores(B: int, N: int, rng, nan: bool = True):
    """Scores that tie: +-0.0, equal values, -inf, denormals, and (``nan``) a NaN here and there; a repeat's score is drawn
    independently of its representative's."""
    sc = SPECIAL_SCORES[rng.integers(0, len(SPECIAL_SCORES), size=(B, N))].copy()
    some = rng.random((B, N)) < 0.3
    sc[some] = -rng.random(int(some.sum())).astype(np.float32) * 4
    if nan:
        sc[rng.random((B, N)) < 0.05] = np.nan
    return sc


def make_case(B: int, N: int, W: int, seed: int, kinds=LAYOUTS, pad: int = 0, eos: int = 2):
    """hyp [B, N, W] whose sources cycle through ``kinds``, and scores [B, N]."""
    rng = np.random.default_rng(seed)
    hyp = np.stack([layout_rows(kinds[(b + seed) % len(kinds)], N, W, rng, pad, eos) for b in range(B)])
    return hyp, case_scores(B, N, rng)


# ---- one guarded call of the entry point ----
GUARD = 64
SENT_I32, SENT_I64, SENT_F32 = -123456789, -987654321987, -7.25


def fold_call(lib, hyp, scores, order, flags, pad=0, eos=2, ld=None, want=OUTPUTS, session=None, W=None, N=None, B=None):
    """ttx_fold_hypotheses on device copies of ``hyp`` (rows laid out with stride ``ld``, sentinels in the gap) and ``scores``;
    every array sits between guard margins, which must come back untouched.  ``want``: the outputs handed in (the rest NULL).
    ``B`` / ``N`` / ``W`` override what the call is told (for the refusals).  Returns ``(rc, outputs)`` with the outputs as NumPy
    arrays (None where not asked for), whatever rc is."""
    import ctypes as C
    import torch
    hyp = np.asarray(hyp, np.int64)
    b_, n_, w_ = hyp.shape
    ld = w_ if ld is None else ld
    dev = torch.device("cuda", 0)

    def guarded(payload: np.ndarray):
        flat = payload.ravel()
        host = np.full(flat.size + 2 * GUARD, {np.dtype(np.int32): SENT_I32, np.dtype(np.int64): SENT_I64,
                                               np.dtype(np.float32): SENT_F32}[flat.dtype], flat.dtype)
        host[GUARD:GUARD + flat.size] = flat
        return torch.from_numpy(host).to(dev), host

    laid = np.full((b_ * n_, max(ld, w_)), SENT_I64, np.int64)
    laid[:, :w_] = hyp.reshape(b_ * n_, w_)
    d_hyp, _ = guarded(laid)
    d_sc = guarded(np.asarray(scores, np.float32))[0] if scores is not None else None
    shapes = {"first": ((b_, n_), np.int32), "rank_of": ((b_, n_), np.int32), "n_unique": ((b_,), np.int32),
              "perm": ((b_, n_), np.int32), "count": ((b_, n_), np.int32), "score": ((b_, n_), np.float32),
              "out": ((b_, n_, w_), np.int64), "logmass": ((b_,), np.float32)}
    sent = {np.int32: SENT_I32, np.int64: SENT_I64, np.float32: SENT_F32}
    bufs = {}
    for name in want:
        shape, dt = shapes[name]
        bufs[name] = guarded(np.full(shape, sent[dt], dt))
    esz = {np.int32: 4, np.int64: 8, np.float32: 4}

    def ptr(name):
        if name not in bufs:
            return None
        return bufs[name][0].data_ptr() + GUARD * esz[shapes[name][1]]
    rc = lib.ttx_fold_hypotheses(session, d_hyp.data_ptr() + GUARD * 8, b_ if B is None else B, n_ if N is None else N,
                                 w_ if W is None else W, ld, pad, eos, None if d_sc is None else d_sc.data_ptr() + GUARD * 4,
                                 order, flags, ptr("first"), ptr("rank_of"), ptr("n_unique"), ptr("perm"), ptr("count"),
                                 ptr("score"), ptr("out"), ptr("logmass"), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    out = {name: None for name in OUTPUTS}
    for name, (t, host) in bufs.items():
        back = t.cpu().numpy()
        shape, dt = shapes[name]
        size = int(np.prod(shape))
        assert (back[:GUARD].view(np.uint8) == host[:GUARD].view(np.uint8)).all(), f"{name}: the margin in front was written"
        assert (back[GUARD + size:].view(np.uint8) == host[GUARD + size:].view(np.uint8)).all(), f"{name}: the margin behind was written"
        out[name] = back[GUARD:GUARD + size].reshape(shape)
    return rc, out


def untouched(outputs: dict) -> bool:
    """Every handed-in output still holds its sentinel in every element (a refused call launched nothing)."""
    sent = {np.dtype(np.int32): SENT_I32, np.dtype(np.int64): SENT_I64, np.dtype(np.float32): SENT_F32}
    return all((v == sent[v.dtype]).all() for v in outputs.values() if v is not None)
