"""k_syntax_mask (csrc/ttx_syntax.hip.h), one launch at a time through ttx_debug_syntax_mask, EXACT against the NumPy restatement of
tests/util_syntax.py: a forbidden entry is -inf, every other logit keeps its bits (the logits carry signed zeros, -inf and NaNs with
payloads; the kernel never reads them).

Vocabularies 30, 67, 256 and 1 024 (one trip of the lanes, a trip and a tail, four and sixteen trips); committed prefixes of 0, 1, 63,
64, 65 and 130 tokens (a lane's first trip with and without its last lane, its second trip, its third); the step layout at
(N, D) = (1, 0), (1, 4) and (3, 10), with and without a row map that drops drafts; the teacher-forced mapping at T = 3 and 70; for
each, a max_len that puts the rows at left = 0, 1, 2, need and need + 1; ring labels 0 and 63 (bit 0 of the low word, bit 31 of the high
word of the XOR); a live-row count on the device below the launch's row count.  Rows at or beyond the live count and the guard
margins on both sides of every operand must keep their sentinels; no input array may be written."""
import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_syntax as Y

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS = 2
VS = [30, 67, 256, 1024]
PREFIXES = [0, 1, 63, 64, 65, 130]
FILL = np.array([U.FLOAT_FILL], dtype=np.int32).view(np.float32)[0]          # what a dead row holds before and after the launch


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def buf(a, dtype) -> U.Buf:
    a = np.asarray(a)
    return U.Buf(a.shape, dtype, DEV, a)


def special_ids(cls) -> dict:
    return {"open": int(Y.ids_of(cls, Y.OPEN)[0]), "close": int(Y.ids_of(cls, Y.CLOSE)[0]), "r0": int(Y.ids_of(cls, Y.RING0)[0]),
            "r63": int(Y.ids_of(cls, Y.RING0 + 63)[0])}


def lens_for(rows, anchor: int) -> list:
    """The max_len values that put row ``anchor`` at left = 0, 1, 2, need and need + 1."""
    _, pos, need = rows[anchor]
    return sorted({pos + 1 + left for left in (0, 1, 2, need, need + 1)})


def with_need(cls, rows) -> list:
    """(prefix, pos, need) of every (prefix, pos)."""
    return [(p, pos, Y.need_of(*Y.state(cls, p))) for p, pos in rows]


def launch(native, x, cls, max_len, rows, live, what, *, tok, tok_dtype=torch.int32, front=None, act=None, row_map=None, drafts=None, N=1,
           D=0, T=0, live_on_device=True) -> None:
    """One launch; the result must be the restatement on the bits, dead rows, every margin and every input untouched."""
    x = x.copy()
    x[live:] = FILL                                                  # sentinels in the rows the kernel must not write
    lg = U.Buf(x.shape, torch.float32, DEV, x)
    table = buf(cls.view(np.uint8), torch.uint8)                     # int8 classes inside a guarded byte buffer
    ins = {"tok": buf(tok, tok_dtype)}
    for name, a in (("front", front), ("act", act), ("row_map", row_map), ("drafts", drafts)):
        if a is not None:
            ins[name] = buf(a, torch.int32)
    if live_on_device:
        ins["m"] = buf([live], torch.int32)
    before = {k: b.get().copy() for k, b in ins.items()}
    v = lambda k: ins[k].v if k in ins else None
    native.debug_syntax_mask(lg.v, table.v.view(torch.int8), max_len, EOS, ins["tok"].v, front=v("front"), m_live=v("m"), act_idx=v("act"),
                             row_map=v("row_map"), drafts=v("drafts"), n=N, d=D, t=T)
    torch.cuda.synchronize()
    got = lg.v.detach().cpu().numpy().copy()
    Y.check(got, x, cls, [(p, pos) for p, pos, _ in rows], max_len, EOS, live, f"{what}, max_len {max_len}")
    assert lg.margins() is None, f"{what}: logits: {lg.margins()}"
    assert table.margins() is None and (table.get() == cls.view(np.uint8)).all(), f"{what}: the class table was written"
    for k, b in ins.items():
        assert b.margins() is None, f"{what}: {k}: {b.margins()}"
        assert (b.get() == before[k]).all(), f"{what}: {k} was written"


def committed(rng, cls, B: int, lengths, ld: int, dtype=np.int32) -> np.ndarray:
    """[B, ld] rows: BOS, a random prefix of the row's length (branches, rings 0 and 63 and ids outside the vocabulary among them),
    then a poison id the kernel must not count."""
    ids = special_ids(cls)
    tok = np.full((B, ld), ids["open"], dtype=dtype)                  # poison beyond the prefix: an OPEN would show in every state
    tok[:, 0] = 1
    for b, n in enumerate(lengths):
        p = Y.random_prefix(rng, cls, n, EOS)
        for k, t in ((0, ids["r0"]), (n // 2, ids["r63"]), (n - 1, ids["open"])):      # label 0 first, label 63 midway, an OPEN last
            if 0 <= k < n and (b + k) % 2 == 0:
                p[k] = t
        if n > 3:
            p[1], p[2] = len(cls) + 3, -1                              # outside [0, V): neutral, and no table read
        tok[b, 1:1 + n] = p
    return tok


@pytest.mark.parametrize("V", VS)
def test_plain_mapping(native, V):
    rng = np.random.default_rng(V)
    cls = Y.make_cls(rng, V)
    M, live = 9, 7
    for f in PREFIXES:
        tok = committed(rng, cls, M, [f] * M, f + 6)
        rows = with_need(cls, Y.rows_plain(tok, f, M))
        x = Y.make_logits(rng, M, V)
        for max_len in lens_for(rows, 0):
            launch(native, x, cls, max_len, rows, live, f"plain V {V} prefix {f}", tok=tok, front=[f])
    launch(native, x, cls, 140, rows, M, f"plain V {V}, no live count", tok=tok, front=[130], live_on_device=False)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("N,D", [(1, 0), (1, 4), (3, 10)])
def test_step_layout_with_and_without_a_row_map(native, V, N, D):
    rng = np.random.default_rng(1000 * N + 10 * D + V)
    cls = Y.make_cls(rng, V)
    ids = special_ids(cls)
    rps = Y.step_rps(N, D)
    B = 7
    fronts = np.array([0, 1, 63, 64, 65, 130, 5])
    tok = committed(rng, cls, B, fronts, 130 + D + 2)
    pool = np.concatenate([np.arange(4, V), [ids["open"], ids["close"], ids["r0"], ids["r63"]] * 6, [V + 9, -2]])
    drafts = rng.choice(pool, size=(B, N, max(D, 1))).astype(np.int32)
    drafts[2, 0, :min(D, 3)] = [ids["r63"], ids["open"], ids["close"]][:min(D, 3)]
    for act in ([5, 2] if rps > 20 else [5, 0, 3, 2, 4, 1]), ([3, 4] if rps > 20 else [6, 1, 2]):
        act = np.array(act)
        full = len(act) * rps
        assert full <= 64
        x = Y.make_logits(rng, full + 2, V)
        rows = with_need(cls, Y.rows_step(tok, fronts, act, drafts, full, N, D)) + [([], 1, 0)] * 2
        for anchor in (0, full - 1):
            for max_len in lens_for(rows, anchor):
                launch(native, x, cls, max_len, rows, full, f"step V {V} N {N} D {D}", tok=tok, front=fronts, act=act,
                       drafts=drafts if D else None, N=N, D=D)
        launch(native, x, cls, 140, rows, full - rps // 2 - 1, f"step V {V} N {N} D {D}, fewer live rows", tok=tok, front=fronts, act=act,
               drafts=drafts if D else None, N=N, D=D)
        # a compacted pass: every slot keeps its row 0 and a subset of its drafts (slot s drops draft s % N; with N = 1 every other
        # slot drops its only draft); the probe layout has nothing to drop and goes through a map that reorders its slots
        keep = []
        for s in range(len(act)):
            keep.append(s * rps)
            for n in range(N):
                if D and not (n == s % N and (N > 1 or s % 2 == 0)):
                    keep.extend(s * rps + 1 + n * D + j for j in range(D))
        if D == 0:
            keep = keep[::-1]
        row_map = np.array(keep + [0, 0])
        live = len(keep)
        rows = with_need(cls, Y.rows_step(tok, fronts, act, drafts, live, N, D, row_map)) + [([], 1, 0)] * 2
        xm = Y.make_logits(rng, live + 2, V)
        for max_len in lens_for(rows, live - 1):
            launch(native, xm, cls, max_len, rows, live, f"compacted V {V} N {N} D {D}", tok=tok, front=fronts, act=act, row_map=row_map,
                   drafts=drafts if D else None, N=N, D=D)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("T", [3, 70])
def test_teacher_forced_mapping(native, V, T):
    rng = np.random.default_rng(7 * T + V)
    cls = Y.make_cls(rng, V)
    R = 5 if T == 3 else 2
    hyp = committed(rng, cls, R, [T] * R, T + 3, dtype=np.int64)
    hyp[0, 2] = EOS                                              # rows go on after EOS as PAD does in a hypothesis: the state just runs on
    M = R * T
    rows = with_need(cls, Y.rows_teacher(hyp, M, T))
    x = Y.make_logits(rng, M, V)
    for anchor in (T - 1, M - 1):
        for max_len in lens_for(rows, anchor):
            launch(native, x, cls, max_len, rows, M - 2, f"teacher-forced V {V} T {T}", tok=hyp, tok_dtype=torch.int64, T=T)
    launch(native, x, cls, T + 1, rows, M, f"teacher-forced V {V} T {T}, no live count", tok=hyp, tok_dtype=torch.int64, T=T, live_on_device=False)


def test_sixty_four_rows_and_the_special_values(native):
    rng = np.random.default_rng(64)
    V, M = 256, 64                                               # 16 workgroups of four waves
    cls = Y.make_cls(rng, V)
    tok = committed(rng, cls, M, [65] * M, 72)
    rows = with_need(cls, Y.rows_plain(tok, 65, M))
    x = Y.make_logits(rng, M, V)
    assert np.isnan(x).any() and (Y.bits(x) == 0x80000000).any() and np.isinf(x).any(), "the special logits are missing"
    assert len({r[2] for r in rows}) > 3, "the rows share one state: the check shows little"
    for max_len in (67, 70, 80):
        launch(native, x, cls, max_len, rows, 61, "64 rows", tok=tok, front=[65])
    # an all-neutral table far from the end: no bit changes anywhere
    zero = np.zeros(V, dtype=np.int8)
    launch(native, x, zero, 500, with_need(zero, Y.rows_plain(tok, 65, M)), M, "an all-neutral table", tok=tok, front=[65])
    got = Y.apply(x, zero, Y.rows_plain(tok, 65, M), 500, EOS)
    assert Y.first_difference(got, x) is None


def test_refused_arguments(native):
    from translation_transformer_amd._native import TtxError
    x = torch.zeros((4, 8), dtype=torch.float32, device=DEV)
    cls = torch.zeros(8, dtype=torch.int8, device=DEV)
    tok = torch.ones((4, 6), dtype=torch.int32, device=DEV)
    front = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(TtxError):
        native.debug_syntax_mask(x, cls, 10, EOS, tok)                                         # the plain mapping needs front
    with pytest.raises(TtxError):
        native.debug_syntax_mask(x, cls, 10, EOS, tok, front=front, act_idx=front, n=0, d=0)   # N < 1
    with pytest.raises(TtxError):
        native.debug_syntax_mask(x, cls, 10, EOS, tok, front=front, act_idx=front, n=1, d=3)   # D > 0 without drafts
    with pytest.raises(TtxError):
        native.debug_syntax_mask(x, cls, 10, EOS, tok.long(), t=3)                             # M is no multiple of T
    assert bool((x == 0).all())
