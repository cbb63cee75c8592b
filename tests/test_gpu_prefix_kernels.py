"""The kernels of forced target prefixes (csrc/ttx_sample.hip.h), one launch at a time on operands the test builds, against the
restatement of tests/util_prefix.py (tests/test_prefix_host.py shows that its checker can fail).  Everything is exact: integers in,
integers out.  Every element the rule does not write holds its sentinel afterwards, and every array stands between guard margins.

k_prefix_drafts       ttx_debug_prefix_drafts: windows wholly inside the prefix, across its end, at it, beyond it, without a prefix; a
                      compacted active list; EOS and PAD of a prefix as the replace token; two rows of one source; a draft wider than
                      a wave.
k_sample_step         ttx_debug_sample_step_prefix at one vocabulary per VPL class: the full layout, the probe layout, a row map of
                      draft select.  Forced rows hold the prefix token although their logits are NaN; every other row equals
                      ttx_debug_sample_step_select's on the same operands.
k_sample              ttx_debug_sample_prefix: forced EOS and PAD set done, done rows emit PAD, rows beyond the live count stay.
"""
import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_prefix as F
import util_sample_pool as P
import util_sample_spec as X
from test_gpu_sample_kernel import make_logits
from test_gpu_sample_step_kernel import B, DEV, SETTINGS, StepOperands

pytestmark = pytest.mark.gpu
PAD, BOS, EOS, REPL = 0, 1, 2, 3
I32 = torch.int32
SENT = U.SENTINEL[I32]


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


class Table:
    """A prefix table of 4 sources between guard margins and the rows' lengths and sources: rows 0 and 3 share source 0."""

    def __init__(self, D: int, V: int, seed: int, rows: int = B):
        rng = np.random.default_rng(seed)
        self.ld = 3 * D + 8
        self.length_of_src = np.array([2 * D + 3, 0, D + 1, self.ld])
        self.tab = rng.integers(4, V, size=(4, self.ld))
        self.tab[0, 2], self.tab[0, 4] = V + 5, -4                       # ids outside the vocabulary: emitted as 0
        self.tab[0, 1], self.tab[0, D - 1], self.tab[2, 0] = EOS, PAD, EOS   # places 2 and D of source 0 (D = 1: places 2 and 1)
        self.src = np.resize(np.array([0, 1, 2, 0, 3]), rows)
        self.pre = F.Prefixes(self.tab, self.length_of_src)
        self.d_tab = U.Buf(self.tab.shape, I32, DEV, self.tab)
        self.d_len = U.Buf((rows,), I32, DEV, self.length_of_src[self.src])
        self.d_src = U.Buf((rows,), I32, DEV, self.src)

    def kw(self) -> dict:
        return dict(prefix_tok=self.d_tab.v, prefix_len=self.d_len.v, prefix_src=self.d_src.v)

    def margins(self):
        for b in (self.d_tab, self.d_len, self.d_src):
            assert b.margins() is None, b.margins()


def fronts_for(D: int) -> np.ndarray:
    """By decoder row (sources 0, 1, 2, 0, 3 with lengths 2D + 3, 0, D + 1, 2D + 3, 3D + 8): the window wholly inside the prefix, no
    prefix, f == plen, the window across the prefix's end (f + 1 <= plen < f + D when D > 1), and f > plen."""
    return np.array([0, 5, D + 1, D + 4, 3 * D + 9], dtype=np.int32)


@pytest.mark.parametrize("N,D", [(1, 1), (3, 4), (2, 70)])
def test_prefix_drafts(native, N, D):
    rng = np.random.default_rng(N * 10 + D)
    t = Table(D, 40, seed=D)
    front = fronts_for(D)
    drafts_np = rng.integers(4, 40, size=(B, N, D))
    draft0_np = rng.integers(4, 40, size=(B, D))
    for act_np, n_active in ([3, 0, 4, 1, 2], B), ([4, 3, 0, 2, 1], 3), ([1, 3, 0, 2, 4], 0):
        act = U.Buf((B,), I32, DEV, act_np)
        fr = U.Buf((B,), I32, DEV, front)
        drafts = U.Buf((B, N, D), I32, DEV, drafts_np)
        draft0 = U.Buf((B, D), I32, DEV, draft0_np)
        native.debug_prefix_drafts(act.v, fr.v, drafts.v, draft0.v, n_active=n_active, eos=EOS, pad=PAD, replace=REPL, **t.kw())
        torch.cuda.synchronize()
        want = F.prefix_drafts(drafts_np, draft0_np, act_np, n_active, front, t.pre, t.src, EOS, PAD, REPL)
        U.check_buf(drafts, want.astype(np.int32), f"N {N} D {D} n_active {n_active}")
        for b in (act, fr, draft0):
            assert b.margins() is None, b.margins()
        t.margins()
        assert np.array_equal(draft0.get(), draft0_np) and np.array_equal(fr.get(), front)
        live = np.asarray(act_np[:n_active], dtype=np.int64)
        assert not np.isin(want[live, 0], (EOS, PAD)).any()
        assert np.array_equal(want[:, 1:], drafts_np[:, 1:])              # drafts 1 .. N-1 are the source windows
        if n_active == B:
            assert (want[0, 0] == REPL).sum() == (1 if D == 1 else 2)    # the PAD (and the EOS) of source 0's prefix, as the replace token
            assert np.array_equal(want[1, 0], draft0_np[1]) and np.array_equal(want[4, 0], draft0_np[4])       # plen 0; f > plen
            assert np.array_equal(want[2, 0], draft0_np[2])              # f == plen: the source draft again
            if D > 1:                                                    # across the end: prefix up to column plen, the source draft behind
                k = int(t.length_of_src[0]) - int(front[3])
                assert 0 < k < D and np.array_equal(want[3, 0, k:], draft0_np[3, k:]) and want[3, 0, 0] == t.tab[0, front[3]]
        # a second launch on its own output changes nothing: the rewrite reads draft0, never the live drafts
        native.debug_prefix_drafts(act.v, fr.v, drafts.v, draft0.v, n_active=n_active, eos=EOS, pad=PAD, replace=REPL, **t.kw())
        torch.cuda.synchronize()
        U.check_buf(drafts, want.astype(np.int32), f"N {N} D {D} n_active {n_active}: second launch")


def forced_rows(ops: StepOperands, t: Table, n_active: int, N: int, D: int):
    """(b, pos, forced) of the live layout rows; the probe layout D = 0 has one row per slot at front + 1."""
    if D == 0:
        b = ops.act_np[:n_active].astype(np.int64)
        pos = ops.front_np[b].astype(np.int64) + 1
    else:
        b, pos = X.step_rows(ops.act_np, ops.front_np, n_active, N, D)
    return b, pos, pos <= t.length_of_src[t.src[b]]


def launch_step(native, ops, t, N, D, n_active, row_map, x, prefix: bool, **kw) -> np.ndarray:
    n_rows = len(x)
    logits = U.Buf(x.shape, torch.float32, DEV, x)
    pred = U.Buf((n_rows + 3,), I32, DEV)
    rm = None if row_map is None else U.Buf((n_rows,), I32, DEV, row_map)
    args = (logits.v, ops.key.v, ops.smp.v, ops.act.v, ops.front.v, pred.v)
    common = dict(B=B, n=N, d=D, n_active=n_active, n_rows=n_rows, row_map=None if rm is None else rm.v, **kw)
    if prefix:
        native.debug_sample_step_prefix(*args, **common, **t.kw())
    else:
        native.debug_sample_step_select(*args, **common)
    torch.cuda.synchronize()
    for b in (logits, pred, ops.key, ops.smp, ops.act, ops.front) + (() if rm is None else (rm,)):
        assert b.margins() is None, b.margins()
    t.margins()
    got = pred.get()
    assert (got[n_rows:] == SENT).all()
    return got[:n_rows]


@pytest.mark.parametrize("layout", ["full", "probe", "row-map"])
@pytest.mark.parametrize("V", [40, 300, 1024])
def test_sample_step_prompted(native, V, layout):
    N, D = (1, 0) if layout == "probe" else (3, 4)
    Dt = max(D, 4)
    R = U.rps(N, D)
    ops = StepOperands(make_logits(B * U.rps(N, max(D, 1)), V, seed=V + len(layout)), N, max(D, 1), seed=V)
    t = Table(Dt, V, seed=V)
    ops.front_np = fronts_for(Dt)
    ops.front.set(ops.front_np)
    n_active = B
    b, pos, forced = forced_rows(ops, t, n_active, N, D)
    assert forced.any() and (~forced).any()
    row_map = P.select_row_map([0b101, 0b010, 0b111, 0b001, 0b110], N, D) if layout == "row-map" else None
    sel = np.arange(n_active * R) if row_map is None else row_map
    x = ops.x[:n_active * R][sel].copy()
    clean = x.copy()
    x[forced[sel]] = np.nan                                               # a forced row does not read its logits
    want_forced = np.array([t.pre.token(int(t.src[bb]), int(pp), V) if f else -1 for bb, pp, f in zip(b, pos, forced)])[sel]
    if layout != "probe":
        assert (want_forced[forced[sel]] == 0).any(), "no id outside the vocabulary among the forced tokens"
    for i, kw in enumerate(SETTINGS + [dict(temperature=0.0)]):
        seed = 0x9E3779B97F4A7C15 ^ (i << 40)
        got = launch_step(native, ops, t, N, D, n_active, row_map, x, True, seed=seed, pad=PAD, eos=EOS, **kw)
        free = launch_step(native, ops, t, N, D, n_active, row_map, clean, False, seed=seed, pad=PAD, eos=EOS, **kw)
        f = forced[sel]
        assert np.array_equal(got[f], want_forced[f]), f"V {V} {layout} {kw}: forced rows {got[f].tolist()} want {want_forced[f].tolist()}"
        assert np.array_equal(got[~f], free[~f]), f"V {V} {layout} {kw}: an unforced row differs from the unprompted launch"


@pytest.mark.parametrize("V", [40, 300, 1024])
def test_sample_prompted(native, V):
    m = 9
    rng = np.random.default_rng(V)
    t = Table(4, V, seed=V + 1, rows=m)
    x = make_logits(m, V, seed=V)
    key = U.Buf((m,), torch.int64, DEV, rng.integers(-2 ** 63, 2 ** 63, m, dtype=np.int64))
    smp = U.Buf((m,), I32, DEV, rng.integers(0, 2 ** 31, m))
    done_np = np.zeros(m, dtype=np.int32)
    done_np[[3, 6]] = 1                                                   # a done row inside its prefix and one outside emit PAD
    # positions 1 (the EOS of source 2), 2 (the EOS of source 0), 6, 3 (an id outside V), 4 (the PAD of source 0), 5 (a negative id), 13
    for front, live in [(0, m), (1, m), (5, m), (2, 6), (3, m), (4, m), (12, m)]:
        pos = front + 1
        forced = pos <= t.length_of_src[t.src]
        xf = x.copy()
        xf[forced] = np.nan
        for kw in (SETTINGS[0], dict(temperature=0.0)):
            outs = []
            for prefix, logits_np in ((True, xf), (False, x)):
                logits = U.Buf((m, V), torch.float32, DEV, logits_np)
                fr = U.Buf((1,), I32, DEV, [front])
                done = U.Buf((m,), I32, DEV, done_np)
                pred = U.Buf((m,), I32, DEV)
                m_live = torch.tensor([live], dtype=I32, device=DEV)
                args = (logits.v, key.v, smp.v, done.v, fr.v, pred.v, m, m_live)
                if prefix:
                    native.debug_sample_prefix(*args, seed=9, pad=PAD, eos=EOS, **kw, **t.kw())
                else:
                    native.debug_sample(*args, seed=9, pad=PAD, eos=EOS, **kw)
                torch.cuda.synchronize()
                for b in (logits, key, smp, fr, done, pred):
                    assert b.margins() is None, b.margins()
                t.margins()
                outs.append((pred.get(), done.get()))
            (tok, dn), (tok0, dn0) = outs
            for r in range(m):
                what = f"V {V} front {front} row {r} {kw}"
                if r >= live:
                    assert tok[r] == SENT and dn[r] == done_np[r], what + ": a row beyond the live count was touched"
                elif done_np[r]:
                    assert tok[r] == PAD and dn[r] == 1, what
                elif forced[r]:
                    want = t.pre.token(int(t.src[r]), pos, V)
                    assert tok[r] == want and dn[r] == int(want in (EOS, PAD)), what + f": got {tok[r]} done {dn[r]}, forced {want}"
                else:
                    assert tok[r] == tok0[r] and dn[r] == dn0[r], what + ": an unforced row differs from the unprompted launch"
    assert t.tab[0, 1] == EOS and t.tab[0, 3] == PAD and t.tab[2, 0] == EOS      # the forced EOS and PAD the fronts above reach


def test_refused_arguments(native):
    from translation_transformer_amd._native import TtxError
    N, D = 3, 4
    t = Table(D, 40, seed=1)
    act = U.Buf((B,), I32, DEV, [3, 0, 4, 1, 2])
    fr = U.Buf((B,), I32, DEV, fronts_for(D))
    drafts = U.Buf((B, N, D), I32, DEV)
    draft0 = U.Buf((B, D), I32, DEV, np.full((B, D), 7))
    long_len = U.Buf((B,), I32, DEV, np.full(B, t.ld + 1))
    bad_src = U.Buf((B,), I32, DEV, np.full(B, 4))
    neg_front = U.Buf((B,), I32, DEV, np.full(B, -1))
    for kw in (dict(prefix_len=long_len.v), dict(prefix_src=bad_src.v), dict(n_active=B + 1), dict(front=neg_front.v)):
        a = {**dict(front=fr.v, n_active=B), **t.kw(), **kw}
        with pytest.raises(TtxError):
            native.debug_prefix_drafts(act.v, a.pop("front"), drafts.v, draft0.v, **a)
    torch.cuda.synchronize()
    assert (drafts.get() == SENT).all() and drafts.margins() is None     # nothing was launched
