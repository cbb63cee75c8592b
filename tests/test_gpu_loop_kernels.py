"""The integer and bookkeeping half of a greedy-speculative verify step, one launch at a time: k_embed<true|false>, k_argmax,
k_accept (256 and 1 024 threads), k_greedy_accept and k_kvcopy of csrc/ttx_loop_kernels.hip.h through ttx_debug_embed,
ttx_debug_argmax, ttx_debug_accept and ttx_debug_kvcopy, on operands the test builds, against the plain restatement of
tests/util_loop_checks.py.  All of it is integer or bit-copy work: every check is exact equality — the restatement's value for every
element a rule writes, the sentinel (or the earlier content) in every element it does not, and intact guard margins around every
array.  tests/test_loop_checks_host.py pins the restatement to the reference's goldens and shows that each checker can fail.

Paths of the kernels these cases execute on purpose:
  k_accept   256 threads (B <= 256), 1 024 threads in one round (B <= 1 024) and in two rounds of the slot loop and of the ordered
             compaction (B = 1 025, 1 100); the finished-row list (<= 256 finishers) and the fallback copy that scans all slots (257
             of 300, 257 and 1 100 of 1 100); the first maximum among drafts in every tie order; EOS in the accepted run, as the
             bonus token, one past it, at the end of the tail and in a draft that was not chosen; haspad and the quirk-2 scan (error
             2); width = max_len - 1, max_len, beyond (error 1 with a finisher); row_rule's flags 2, traj / fin_step and error 3; the
             pool's rstep / row_of and caller-side rows; K consecutive steps on one device state
  k_argmax   V below, at and above multiples of 64 (one pass, several, a ragged last pass), ties across lanes and across the passes
             of one lane, -0.0 against 0.0, -inf rows, +inf, all-NaN rows, live counts 0 / middle / m_max
  k_embed    position row pos + 1, row 0 against the draft rows, d = 64 (48 idle lanes) .. 1 024 (four passes), rows beyond m_rows, ids
             outside [0, V)
  k_kvcopy   source row 1 + best*D + (j-1) for n_acc 0 .. D and best 0 .. N-1, front_old 0 and up to the last cache position, slots at or
             beyond n_copy, d = 64 / 256 / 1 024, one and three layers
"""
import numpy as np
import pytest
import torch

import util_loop_checks as U

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    return t


# -- argmax ------------------------------------------------------------------------------------------------------------------
KINDS = 8


def argmax_logits(m_max: int, V: int, seed: int) -> np.ndarray:
    """Random rows and planted ones, the kind of row r being (r + m_max) % 8: 0 random, 1 the maximum in two neighbouring lanes,
    2 the maximum in two passes of one lane (columns c and c + 64), 3 -0.0 before 0.0 above negatives, 4 all -inf, 5 one +inf,
    6 all NaN, 7 NaN mixed with numbers (outside the contract)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m_max, V)).astype(np.float32)
    for r in range(m_max):
        kind = (r + m_max) % KINDS
        c = int(rng.integers(0, V))
        if kind == 1 and V >= 2:
            c = min(c, V - 2)
            x[r, [c, c + 1]] = 7.5
        elif kind == 2 and V > 64:
            c = int(rng.integers(0, V - 64))
            x[r, [c, c + 64]] = 7.5
            if c + 128 < V:
                x[r, c + 128] = 7.5
        elif kind == 3:
            x[r] = -np.abs(x[r]) - 1.0
            if V >= 2:
                c = min(c, V - 2)
                x[r, c], x[r, int(rng.integers(c + 1, V))] = -0.0, 0.0
        elif kind == 4:
            x[r] = -np.inf
        elif kind == 5:
            x[r, c] = np.inf
        elif kind == 6:
            x[r] = np.nan
        elif kind == 7:
            x[r, rng.integers(0, V, size=max(V // 3, 1))] = np.nan
    return x


@pytest.mark.parametrize("m_max", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("V", [1, 12, 63, 64, 65, 300, 1024, 1030])
def test_argmax(native, V, m_max):
    x = argmax_logits(m_max, V, seed=V * 1000 + m_max)
    logits = U.Buf((m_max, V), torch.float32, DEV, x)
    pred = U.Buf((m_max,), torch.int32, DEV)
    before = U.sentinel_array((m_max,), torch.int32)
    for live in [None] + sorted({0, m_max // 2, m_max}):
        pred.reset()
        m_live = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
        native.debug_argmax(logits.v, pred.v, m_max, m_live)
        torch.cuda.synchronize()
        what = f"V {V} m_max {m_max} live {live}"
        U.check_argmax(pred.get(), x, m_max if live is None else live, before, what)
        assert pred.margins() is None, f"{what}: {pred.margins()}"


# -- embedding ---------------------------------------------------------------------------------------------------------------
def tables(V: int, d: int, pe_rows: int, seed: int):
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((V, d)).astype(np.float32)
    pe = rng.standard_normal((pe_rows, d)).astype(np.float32)
    table[1, :4] = [np.inf, -0.0, 1e-41, 3e38]                            # inf, a signed zero, a denormal, near overflow
    pe[1, :4] = [1.0, -0.0, 1e-41, 3e38]
    return table, pe


@pytest.mark.parametrize("L", [1, 7])
@pytest.mark.parametrize("d", [64, 128, 256, 512, 1024])
def test_embed_full(native, d, L):
    V, rows = 37, 23                                                     # 23 rows: the last workgroup has one live wave of four
    table, pe = tables(V, d, L + 1, seed=d + L)
    rng = np.random.default_rng(d * 7 + L)
    tok = rng.integers(0, V, size=rows).astype(np.int32)
    tok[:4] = [1, V, -1, 2 ** 31 - 1]                                     # ids outside [0, V) are looked up as id 0
    tb, pb, kb = U.Buf(table.shape, torch.float32, DEV, table), U.Buf(pe.shape, torch.float32, DEV, pe), U.Buf((rows,), torch.int32, DEV, tok)
    x = U.Buf((rows + 5, d), torch.float32, DEV)
    before = x.get().view(np.float32)
    native.debug_embed(tb.v, pb.v, x.v, tok=kb.v, rows=rows, L=L)
    torch.cuda.synchronize()
    U.check_buf(x, U.embed_full(table, pe, tok, L, before), f"d {d} L {L}")


@pytest.mark.parametrize("N,D", [(1, 1), (3, 10), (23, 5)])
@pytest.mark.parametrize("d", [64, 128, 256, 512, 1024])
def test_embed_step(native, d, N, D):
    B, n_active, V = 7, 4, 37
    fronts = np.array([0, 9, 1, 30, 17, 0, 5])
    s = U.make_state(B, N, D, 40, fronts, n_active=n_active, seed=d + N, V=V)
    s.gen[s.act_idx[1], s.front[s.act_idx[1]]] = V + 3                  # an id outside [0, V) at a front and in a draft
    s.drafts[s.act_idx[0], N - 1, D - 1] = -5
    table, pe = tables(V, d, int(fronts.max()) + D + 2, seed=d)
    bufs = {k: U.Buf(a.shape, torch.int32, DEV, a) for k, a in (("act_idx", s.act_idx), ("front", s.front), ("gen", s.gen), ("drafts", s.drafts))}
    tb, pb = U.Buf(table.shape, torch.float32, DEV, table), U.Buf(pe.shape, torch.float32, DEV, pe)
    x = U.Buf((B * U.rps(N, D), d), torch.float32, DEV)
    before = x.get().view(np.float32)
    for live in (n_active, 0, B - 1):
        x.reset()
        native.debug_embed(tb.v, pb.v, x.v, act_idx=bufs["act_idx"].v, front=bufs["front"].v, gen=bufs["gen"].v, drafts=bufs["drafts"].v,
                           B=B, n=N, d=D, n_active=live, step=True)
        torch.cuda.synchronize()
        U.check_buf(x, U.embed_step(table, pe, s.act_idx, s.front, s.gen, s.drafts, live, before), f"d {d} N {N} D {D} live {live}")
    for k, b in bufs.items():
        assert b.margins() is None and (b.get() == getattr(s, k)).all(), f"{k} was written"


# -- accept ------------------------------------------------------------------------------------------------------------------
def launch_accept(native, dev: U.DeviceLoop, s: U.LoopState, pred: np.ndarray, threads: int = 0, greedy: bool = False) -> None:
    dev.pred.set(pred)
    words = native.debug_accept(dev.entry_words(), B=s.B, n=s.N, d=s.D, Ls=s.Ls, max_len=s.max_len, pad=s.pad, bos=s.bos, eos=s.eos,
                                gen_ld=s.gen_ld, greedy=greedy, threads=threads, row_rule=bool(s.row_rule), pool=bool(s.pool),
                                traj_ld=s.traj_ld, pool_rows=s.pool_rows, pred=dev.pred.v, **dev.tensors())
    dev.set_exit_words(words)


def legal_threads(B: int) -> list:
    return [0, 1024] + ([256] if B <= 256 else [])


def run_single_step(native, name: str, s: U.LoopState, pred: np.ndarray) -> U.LoopState:
    want = U.accept_step(s, pred)
    dev = U.DeviceLoop(s, DEV)
    for threads in legal_threads(s.B):
        dev.load(s)
        launch_accept(native, dev, s, pred, threads)
        U.check_loop(dev, want, f"{name}, threads {threads}")           # the same restatement for every block size: identical results
    return want


GRID = [(B, n, N, D) for B in U.BATCHES for n in sorted({B, max(B // 2, 1), 1}, reverse=True) for N, D in U.ND]


@pytest.mark.parametrize("B,n_active,N,D", GRID)
def test_accept_grid(native, B, n_active, N, D):
    s, pred = U.grid_case(B, n_active, N, D, seed=B * 31 + n_active + N)
    want = run_single_step(native, f"B {B} n_active {n_active} N {N} D {D}", s, pred)
    assert want.words["n_copy"] == n_active


_DEDICATED = {}


def dedicated(name):
    if not _DEDICATED:
        _DEDICATED.update({n: (s, p) for n, s, p in U.dedicated_cases()})
    return _DEDICATED[name]


DEDICATED_NAMES = [f"{k}-N{N}-D{D}" for N, D in U.ND for k in ("lengths", "eos")] + \
    ["finish-nobody", "finish-everybody-5", "finish-everybody-300", "finish-256-of-1100", "finish-257-of-1100", "finish-all-1100",
     "finish-257-of-300", "pad-written", "pad-column-quirk2"] + \
    [f"width-maxlen{d:+d}-{f}" for d in (-1, 0, 1, 3) for f in ("nofinisher", "finisher")] + ["row-rule", "row-rule-late", "pool", "pool-late"]


@pytest.mark.parametrize("name", DEDICATED_NAMES)
def test_accept_constructed(native, name):
    s, pred = dedicated(name)
    want = run_single_step(native, name, s, pred)
    n = s.words["n_active"]
    fin = int((want.rec[:n, 4] == 1).sum())
    # the case is what its name says (the restatement decides, the kernel was held to it above)
    if name.startswith("finish-"):
        expect = {"nobody": 0, "everybody-5": 5, "everybody-300": 300, "256-of-1100": 256, "257-of-1100": 257, "all-1100": 1100, "257-of-300": 257}
        assert fin == expect[name[len("finish-"):]]
        assert want.words["stop"] == int(fin == n)
    if name == "pad-written":
        assert want.haspad.sum() == 1 and want.words["error"] == 0 and want.words["stop"] == 0
    if name == "pad-column-quirk2":
        assert want.words["error"] == 2 and want.words["stop"] == 1
    if name.startswith("width-"):
        delta = int(name.split("maxlen")[1][:2])
        assert want.words["width"] == s.max_len + delta and want.words["stop"] == int(delta >= 0)
        assert want.words["error"] == int(delta > 0 and name.endswith("-finisher"))
    if name.startswith(("row-rule", "pool")):
        assert (want.rec[:n, 4] == 2).any() and fin > 0 and (want.rec[:n, 4] == 0).any() and want.words["stop"] == 0
        traj = want.pool_traj if s.pool else want.traj
        assert (traj != U.SENTINEL[torch.int16]).any() != name.endswith("-late")
    if name.startswith("lengths-"):
        assert len({tuple(r) for r in want.rec[:n, 1:3]}) >= min(s.D + 1, 3)
    if name.startswith("eos-"):
        assert 0 < fin < n


def test_accept_with_nobody_running_publishes_nothing(native):
    s, pred = U.grid_case(5, 0, 3, 10, seed=1)
    want = run_single_step(native, "n_active 0", s, pred)
    assert want.words["host_steps_done"] == -1 and want.words["steps"] == s.words["steps"]


@pytest.mark.parametrize("B", [300, 1100])
def test_accept_replay(native, B):
    """Consecutive steps on ONE device state (only the step's predictions and the drafts they are planted in are uploaded): the device
    state after every step equals the restatement's, so nothing is carried wrongly from step to step.  The run ends by itself."""
    rng = np.random.default_rng(B)
    s = U.init_state(rng.integers(3, 40, size=(B, 3, 10)), 150, Ls=9)
    dev = U.DeviceLoop(s, DEV)
    steps = 0
    while not s.words["stop"]:
        assert steps < 40, "the replay did not end by itself"
        pred = U.plant_random(s, rng, p_fin=0.8)
        dev.bufs["drafts"].set(s.drafts)
        s = U.accept_step(s, pred)
        launch_accept(native, dev, s, pred)
        steps += 1
        U.check_loop(dev, s, f"B {B}, step {steps}")
    print(f"B {B}: {steps} steps, error {s.words['error']}, width {s.words['width']}")
    assert steps >= 8


@pytest.mark.parametrize("B", [1, 10, 257])
def test_greedy_accept(native, B):
    """k_greedy_accept step by step: once until every row emits EOS or PAD at the same step, once until column max_len - 1."""
    for max_len, end_at in ((12, 6), (9, None)):
        rng = np.random.default_rng(B + max_len)
        s = U.make_state(B, 1, 0, max_len, 0, seed=B, permute=False)
        s.haspad = None
        dev = U.DeviceLoop(s, DEV)
        steps = 0
        while not s.words["stop"]:
            steps += 1
            assert steps < max_len
            pred = rng.integers(3, 30, size=B).astype(np.int32)
            pred[rng.random(B) < 0.3] = U.EOS                            # a row's own EOS ends nothing
            if B > 1 and steps != end_at:
                pred[int(rng.integers(0, B))] = 5
            if steps == end_at:
                pred[:] = rng.choice([U.EOS, U.PAD], size=B)
                pred[0] = U.EOS
            elif B == 1 and pred[0] == U.EOS:
                pred[0] = 5
            s = U.greedy_step(s, pred)
            launch_accept(native, dev, s, pred, greedy=True)
            U.check_loop(dev, s, f"greedy B {B} max_len {max_len} step {steps}")
        assert steps == (end_at or max_len - 1)


# -- K/V commit --------------------------------------------------------------------------------------------------------------
def kv_case():
    """Records of a real accept step: n_acc 0 .. D on the first, middle and last draft, ties, front_old 0 and max_len (the commit then
    ends on the cache row's last position), 37 of 41 slots running."""
    N, D, max_len = 3, 10, 30
    pats = U.tie_patterns(N, D)
    B, n_active = len(pats) - 8, len(pats) - 12
    rng = np.random.default_rng(77)
    fronts = rng.integers(0, max_len + 1, size=B)
    s = U.make_state(B, N, D, max_len, fronts, n_active=n_active, seed=77)
    s.front[s.act_idx[D]] = max_len                                      # slot D is accepted for D tokens on draft 0: the last position
    s.front[s.act_idx[0]] = 0
    pred = U.new_pred(s)
    for slot in range(n_active):
        U.plant(s, pred, slot, pats[slot], rng)
    return s, pred


@pytest.mark.parametrize("Ld", [1, 3])
@pytest.mark.parametrize("d", [64, 256, 1024])
def test_kvcopy(native, d, Ld):
    s, pred = kv_case()
    dev = U.DeviceLoop(s, DEV)
    launch_accept(native, dev, s, pred)
    want = U.accept_step(s, pred)
    U.check_loop(dev, want, "the accept step the records come from")
    rec, n_copy, Lc = want.rec, want.words["n_copy"], s.max_len + s.D + 1
    live = rec[:n_copy]
    assert n_copy < s.B and {0, s.D} <= set(live[:, 2]) and {0, s.N - 1} <= set(live[:, 1]) and 0 in live[:, 3]
    assert (live[:, 3] + live[:, 2] + 1).max() == Lc
    ops = U.kv_operands(rec, n_copy, s.B, s.N, s.D, d, Ld, Lc, seed=d + Ld)
    qkv = U.Buf(ops["qkv"].shape, torch.float32, DEV, ops["qkv"])
    kc, vc = U.Buf(ops["k0"].shape, torch.float32, DEV), U.Buf(ops["v0"].shape, torch.float32, DEV)
    native.debug_kvcopy(dev.bufs["rec"].v, n_copy, qkv.v, kc.v, vc.v, s.N, s.D, d, s.B)
    torch.cuda.synchronize()
    wk, wv = U.kv_commit(rec, n_copy, ops["qkv"], ops["k0"], ops["v0"], s.N, s.D)
    U.check_buf(kc, wk, f"K cache, d {d} Ld {Ld}")                        # every word: the accepted rows' bits, the fill everywhere else
    U.check_buf(vc, wv, f"V cache, d {d} Ld {Ld}")
    b, _, n_acc, f = (int(t) for t in live[0, :4])
    assert (kc.get()[:, b, f + n_acc + 1] == U.FLOAT_FILL).all()           # the position after the bonus token's
    assert qkv.margins() is None and (qkv.get() == ops["qkv"].view(np.int32)).all()
    native.debug_kvcopy(dev.bufs["rec"].v, 0, qkv.v, kc.v, vc.v, s.N, s.D, d, s.B)      # n_copy = 0: nothing moves
    torch.cuda.synchronize()
    U.check_buf(kc, wk, "n_copy 0")


# -- arguments a kernel cannot take are refused, nothing is launched ----------------------------------------------------------
def test_invalid_arguments_are_refused(native, tta):
    s, pred = U.grid_case(300, 300, 3, 10, seed=2)
    dev = U.DeviceLoop(s, DEV)

    def refused(fn, *a, **kw):
        with pytest.raises(tta.TtxError) as e:
            fn(*a, **kw)
        assert e.value.code == -1

    refused(launch_accept, native, dev, s, pred, 256)                    # production never launches 256 threads for B > 256
    refused(launch_accept, native, dev, s, pred, 512)
    dev.words["n_active"] = 301
    refused(launch_accept, native, dev, s, pred)
    dev.words["n_active"] = -1
    refused(launch_accept, native, dev, s, pred)
    dev.load(s)
    short = U.LoopState(**{**s.__dict__, "gen_ld": s.gen_ld - s.D - 3})    # too small for front + D + 2 of the rightmost row
    refused(launch_accept, native, dev, short, pred)
    keep = dev.bufs.pop("front")
    refused(launch_accept, native, dev, s, pred)                         # a required pointer is null
    dev.bufs["front"] = keep
    launch_accept(native, dev, s, pred)                                  # and nothing was launched in between
    U.check_loop(dev, U.accept_step(s, pred), "after the refusals")

    x = torch.zeros(8 * 64 + 4, dtype=torch.float32, device=DEV)
    table, pe = torch.zeros(5, 64, device=DEV), torch.zeros(9, 64, device=DEV)
    tok = torch.zeros(8, dtype=torch.int32, device=DEV)
    refused(native.debug_embed, table, pe, x[1:], tok=tok, rows=8, L=3)                      # misaligned output
    refused(native.debug_embed, table[:, :32].contiguous(), pe[:, :32].contiguous(), x, tok=tok, rows=8, L=3)   # d = 32
    refused(native.debug_embed, table, pe, x, tok=tok, rows=8, L=9)                          # positional table too short
    refused(native.debug_embed, table, pe, x, tok=None, rows=8, L=3)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    gen, drafts = torch.zeros(2, 12, dtype=torch.int32, device=DEV), torch.zeros(2, 1, 2, dtype=torch.int32, device=DEV)
    refused(native.debug_embed, table, pe, x, act_idx=i32(0, 1), front=i32(0, 0), gen=gen, drafts=drafts, B=2, n=1, d=2, n_active=3, step=True)
    refused(native.debug_embed, table, pe, x, act_idx=i32(0, 1), front=i32(0, 9), gen=gen, drafts=drafts, B=2, n=1, d=2, n_active=2, step=True)
    refused(native.debug_embed, table, pe, x, act_idx=i32(0, 2), front=i32(0, 0), gen=gen, drafts=drafts, B=2, n=1, d=2, n_active=2, step=True)
    logits, out = torch.zeros(4, 10, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    refused(native.debug_argmax, logits, out, 4, i32(5))
    refused(native.debug_argmax, logits, out, 0)
    rec = torch.tensor([[0, 0, 2, 9, 0], [1, 0, 0, 0, 0]], dtype=torch.int32, device=DEV)
    qkv, cache = torch.zeros(1, 2 * 3, 3 * 64, device=DEV), torch.zeros(1, 2, 11, 64, device=DEV)
    refused(native.debug_kvcopy, rec, 3, qkv, cache, cache.clone(), 1, 2, 64, 2)             # n_copy > B
    refused(native.debug_kvcopy, rec, 2, qkv, cache, cache.clone(), 1, 2, 64, 2)             # front_old + n_acc + 1 = 12 > 11 positions
    refused(native.debug_kvcopy, rec, 2, qkv, cache, cache.clone(), 1, 2, 96, 2)             # d = 96
    assert float(cache.abs().sum()) == 0.0
