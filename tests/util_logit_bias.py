"""NumPy restatement of k_logit_bias (csrc/ttx_logit_bias.hip.h; include/ttx.h "Per-source logit bias" is the contract).

The rule: a live logits row of source s becomes x' = x + bias[s], ONE rounded fp32 add per entry, except where the bias entry is
exactly zero (+0.0 or -0.0): there the logit keeps its bits.  ``np.float32`` addition is IEEE round-to-nearest, the kernel's
``__fadd_rn``, so equality is asked on the BITS (``check`` compares the uint32 views; two NaNs with the same bits are equal).
Rows at or beyond ``m_live`` are not written.  The two row mappings are written out below from the arrays the kernels read.
"""
import numpy as np


def step_rps(N: int, D: int) -> int:
    """Rows per slot of a verify step: the front row and D rows for each of the N drafts."""
    return 1 + N * D


def rows_plain(src, M: int, rows_per_src: int = 1) -> np.ndarray:
    """Plain mapping: logits row r is decoder row r; its bias row is src[r], or r // rows_per_src without a map."""
    if src is None:
        return np.arange(M) // rows_per_src
    return np.asarray(src)[:M].astype(np.int64)


def rows_step(act_idx, src, M: int, N: int, D: int, row_map=None) -> np.ndarray:
    """Step layout (k_sample_step's): lrow = row_map ? row_map[row] : row, b = act_idx[lrow // RPS], bias row src[b]."""
    rps = step_rps(N, D)
    lrow = np.arange(M) if row_map is None else np.asarray(row_map)[:M].astype(np.int64)
    return np.asarray(src)[np.asarray(act_idx)[lrow // rps]].astype(np.int64)


def apply(logits_f32: np.ndarray, bias_f32: np.ndarray, row_to_src, m_live: int | None = None) -> np.ndarray:
    """The biased logits [M, V] (a new array): rows below ``m_live`` (default: all) take bias row ``row_to_src[row]``."""
    x = np.array(logits_f32, dtype=np.float32, copy=True)
    b = np.asarray(bias_f32, dtype=np.float32)
    M, V = x.shape
    live = M if m_live is None else min(int(m_live), M)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(live):
            br = b[int(row_to_src[r]), :V]
            x[r] = np.where(br != 0, x[r] + br, x[r])          # np.float32 + np.float32: one rounded add; zero entries skipped
    return x


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def first_difference(got: np.ndarray, want: np.ndarray):
    """(row, token) of the first entry whose BITS differ, or None."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"shape {g.shape} against {w.shape}"
    d = np.argwhere(g != w)
    return None if len(d) == 0 else (int(d[0][0]), int(d[0][1]))


def check(got: np.ndarray, logits_f32, bias_f32, row_to_src, m_live=None, what: str = "") -> None:
    """AssertionError naming the first (row, token) at which ``got`` is not the restatement, on the bits."""
    want = apply(logits_f32, bias_f32, row_to_src, m_live)
    at = first_difference(got, want)
    if at is not None:
        r, v = at
        live = "live" if m_live is None or r < m_live else "dead"
        raise AssertionError(f"{what}: row {r} ({live}) token {v}: got {np.float32(got[r, v])!r} (bits {bits(got)[r, v]:#010x}), the rule gives "
                             f"{want[r, v]!r} (bits {bits(want)[r, v]:#010x}) from logit {np.float32(logits_f32[r, v])!r}")


# -- inputs of the kernel tests ---------------------------------------------------------------------------------------------------
SPECIAL_BIAS = np.array([0.0, -0.0, -np.inf, 8.0, -8.0, 1e-40, -1e-40, 0.5], dtype=np.float32)      # 1e-40: a denormal


def make_logits(rng, M: int, V: int) -> np.ndarray:
    x = (rng.standard_normal((M, V)) * 4).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    flat[rng.choice(n, max(1, n // 9), replace=False)] = np.float32(-0.0)
    flat[rng.choice(n, max(1, n // 11), replace=False)] = -np.inf
    return x


def make_bias(rng, S: int, V: int, ld: int | None = None) -> np.ndarray:
    """[S, ld] with the special values spread over every row; columns at or beyond V (the row's padding) hold a poison value."""
    ld = V if ld is None else ld
    b = (rng.standard_normal((S, ld)) * 2).astype(np.float32)
    pick = rng.integers(0, len(SPECIAL_BIAS) + 3, size=(S, ld))
    special = pick < len(SPECIAL_BIAS)
    b[special] = SPECIAL_BIAS[pick[special]]
    b[:, V:] = np.float32(777.0)
    return b
