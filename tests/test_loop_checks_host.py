"""The restatement of tests/util_loop_checks.py is the reference's loop, and its checkers can fail.  No GPU.

1. Driven step by step with the CPU oracle model's argmax predictions on the tiny weights (full-prefix decode_tgt, gathered into
   the 1 + N*D row layout of a verify step), accept_step reproduces tests/golden/gen_spec_greedy.npz — tokens AND call counts —
   and raises exactly where GreedySpeculativeOracle does.  short_m45 is the case that tells width = max front + D + 2 from + 3.
2. A NumPy stand-in "kernel" (scalar loops over slots, written into the guarded operands) passes every checker; the stand-in with
   ONE defect a kernel could have is flagged by the checker that claims to catch it.
"""
import numpy as np
import pytest
import torch

import util_loop_checks as U
from oracle.decoding import GreedySpeculativeOracle
from oracle.drafting import make_drafts
from oracle.model import OracleTransformer, config_from_state
from util_models import load_npz, fixture_tokens, tiny_state, PAD, BOS, EOS


@pytest.fixture(scope="module")
def model():
    st, cfg = tiny_state()
    return OracleTransformer(config_from_state(st, cfg["num_heads"]), st)


class Raised(RuntimeError):
    pass


def drive(model, src: torch.Tensor, max_len: int, D: int, N: int, c: int):
    """The reference's generate() with accept_step as its bookkeeping: (tokens [B, max_len], model calls)."""
    mask = src == model.src_pad_token_i
    memory = model.encode_src(src, mask)
    drafts = make_drafts(src[:, 1:], D, N, 1, max_len, EOS, PAD, c).numpy()
    Dd = drafts.shape[2]
    s = U.init_state(drafts, max_len, Ls=int(src.size(1)))
    R = U.rps(N, Dd)
    while not s.words["stop"]:
        Bc = s.words["n_active"]
        rows = s.act_idx[:Bc]
        f = s.front[rows]
        W = int(f.max()) + Dd + 1                                       # decoder input columns: up to the last draft token
        inp = np.repeat(s.gen[rows, :W], N, axis=0).astype(np.int64)
        cols = f.repeat(N)[:, None] + 1 + np.arange(Dd)[None, :]
        np.put_along_axis(inp, cols, s.drafts[rows].reshape(Bc * N, Dd).astype(np.int64), axis=1)
        sel = torch.from_numpy(np.repeat(rows, N).astype(np.int64))
        p = model.decode_tgt(torch.from_numpy(inp), memory[sel], memory_pad_mask=mask[sel]).argmax(dim=2).numpy().reshape(Bc, N, W)
        pred = np.zeros(s.B * R, dtype=np.int32)
        for g in range(Bc):
            pred[g * R] = p[g, 0, f[g]]
            pred[g * R + 1:(g + 1) * R] = p[g, :, f[g] + 1:f[g] + 1 + Dd].reshape(-1)
        s = U.accept_step(s, pred)
        if s.words["error"]:
            raise Raised(s.words["error"])
    return s.out[:, None, :], s.words["steps"]


GOLD_CASES = [(bsz, N, D) for bsz in (1, 4, 10) for N in (1, 3, 7) for D in (5, 10, 17)]


@pytest.mark.parametrize("bsz,N,D", GOLD_CASES)
def test_restatement_reproduces_the_reference_goldens(model, bsz, N, D):
    gold = load_npz("gen_spec_greedy.npz")
    src, _, c, _ = fixture_tokens()
    outs, calls = zip(*[drive(model, src[i:i + bsz], 150, D, N, c) for i in range(0, 10, bsz)])
    np.testing.assert_array_equal(np.concatenate(outs), gold[f"b{bsz}_n{N}_d{D}_tokens"])
    assert sum(calls) == int(gold[f"b{bsz}_n{N}_d{D}_calls"])


@pytest.mark.parametrize("max_len", [30, 45])
def test_restatement_reproduces_the_short_goldens(model, max_len):
    gold = load_npz("gen_spec_greedy.npz")
    src, _, c, _ = fixture_tokens()
    out, calls = drive(model, src, max_len, 10, 3, c)
    np.testing.assert_array_equal(out, gold[f"short_m{max_len}_tokens"])
    assert calls == int(gold[f"short_m{max_len}_calls"])


@pytest.mark.parametrize("max_len,D,N", [(150, 10, 3), (150, 4, 2), (45, 4, 2), (45, 10, 3), (40, 4, 2), (30, 10, 3), (27, 4, 2),
                                         (57, 4, 2), (20, 8, 2), (12, 6, 1)])
def test_restatement_raises_where_the_oracle_does(model, max_len, D, N):
    src, _, c, _ = fixture_tokens()
    outcomes = []
    for lo, hi in ((0, 3), (3, 4), (4, 8), (8, 10), (0, 10), (5, 9), (6, 7)):
        sel = src[lo:hi]
        sel = sel[:, :int((sel != PAD).sum(1).max())]
        g = GreedySpeculativeOracle(model, max_len, D, N, PAD, BOS, EOS, c)
        try:
            want = g.generate(sel).numpy()
        except RuntimeError:
            want = None
        try:
            got, calls = drive(model, sel, max_len, D, N, c)
        except Raised:
            got = None
        assert (got is None) == (want is None), f"rows {lo}:{hi}: oracle {'raises' if want is None else 'runs'}"
        if want is not None:
            np.testing.assert_array_equal(got, want)
            assert calls == g.model_calls_num
        outcomes.append(want is None)
    print(f"max_len={max_len} D={D} N={N}: {sum(outcomes)} of {len(outcomes)} batches raise")


# ---------------------------------------------------------------------------------------------------------------------------
# the stand-in kernels and their defects
def standin_accept(state, pred, defect=None):
    """k_accept's job done slot by slot in plain Python, with one defect on request."""
    s = state.clone()
    w = s.words
    w.update(dict.fromkeys(U.WORDS[13:], -1))
    Bc = w["n_active"]
    if Bc == 0:
        return s
    N, D, R = s.N, s.D, U.rps(s.N, s.D)
    maxfront, sum_acc, sum_f, n_fin = 0, 0, 0, 0
    recs = []
    for slot in range(Bc):
        b = int(s.act_idx[slot])
        f = int(s.front[b])
        row = pred[slot * R:(slot + 1) * R]
        at = lambda n, j: int(row[0]) if j == 0 else int(row[1 + n * D + (j - 1)])
        best, bacc, accs = 0, -1, []
        for n in range(N):
            acc = 0
            while acc < D and s.drafts[b, n, acc] == at(n, acc):
                acc += 1
            accs.append(acc)
            if acc > bacc or (defect == "last draft on a tie" and acc == bacc):
                best, bacc = n, acc
        n_written = bacc if defect == "bonus token dropped" else bacc + 1
        fin = sawpad = False
        for j in range(n_written):
            t = at(best, j)
            s.gen[b, f + 1 + j] = t
            fin |= t == s.eos
            sawpad |= t == s.pad
        if defect == "EOS in the rejected tail finishes the row":
            fin |= any(at(best, j) == s.eos for j in range(D + 1))
        if defect == "EOS in a draft that was not chosen finishes the row":
            fin |= any(at(n, j) == s.eos for n in range(N) for j in range(accs[n] + 1))
        if sawpad:
            s.haspad[b] = 1
        s.front[b] = f + n_written
        flags = 1 if fin else 0
        if s.row_rule:
            if s.pool:
                s.rstep[b] += 1
                it, trow, traj, fins = int(s.rstep[b]), int(s.row_of[b]), s.pool_traj, s.pool_fin_step
            else:
                it, trow, traj, fins = w["steps"] + 1, b, s.traj, s.fin_step
            if it < s.traj_ld:
                traj[trow, it] = f + n_written
            if fin:
                fins[trow] = it
            elif f + D + 2 >= s.max_len:
                flags = 2
        recs.append((b, best, bacc, f, flags))
        s.rec[slot] = recs[-1]
        maxfront = max(maxfront, f)
        sum_acc += bacc
        sum_f += f
    width = maxfront + D + (3 if defect == "width off by one" else 2)
    wout = s.max_len if s.row_rule else min(width, s.max_len)
    for b, _, _, _, flags in recs:
        if flags == 1:
            n_fin += 1
            if defect == "finished rows beyond the 256th are not copied out" and n_fin > 256:
                continue
            (s.pool_out[s.row_of[b]] if s.pool else s.out[b])[:wout] = s.gen[b, :wout]
    kept = [b for b, _, _, _, flags in recs if flags == 0]
    if defect == "compaction does not keep the order":
        kept = kept[::-1]
    nn = len(kept)
    s.act_idx[:nn] = kept
    w["n_copy"] = Bc
    w["steps"] += 1
    w["accepted"] += sum_acc
    w["produced"] += sum_acc + Bc
    w["verified_positions"] += Bc * R
    w["kv_prefix_positions"] += sum_f
    w["src_positions"] += Bc * s.Ls
    w["width"] = width
    if n_fin and width > s.max_len and not s.row_rule:
        w["error"] = 1
    stop = nn == 0 or (not s.row_rule and width >= s.max_len)
    suspect = any(s.haspad[b] for b in kept)
    if s.row_rule and suspect:
        w["error"] = 3
    if not stop and suspect and not s.row_rule:
        for col in range(max(int(s.front[b]) for b in kept) + 1):
            if all(s.gen[b, col] == s.pad for b in kept):
                w["error"], stop = 2, True
    w["stop"] = int(stop)
    w["n_active"], w["r_rows"], w["m_rows"] = (0, 0, 0) if stop else (nn, nn * N, nn * R)
    w["host_width"], w["host_n_active"], w["host_stop"], w["host_steps_done"] = width, w["n_active"], int(stop), w["steps"]
    return s


def run_standin(state, pred, defect=None):
    """The stand-in's result as a test finds a kernel's: in guarded operands, to be checked against the restatement."""
    dev = U.DeviceLoop(state)
    after = standin_accept(state, pred, defect)
    dev.load(after)
    return dev


CASES = {name: (s, p) for name, s, p in U.dedicated_cases()}
for _B, _n, (_N, _D) in ((5, 3, (3, 10)), (65, 65, (7, 17)), (257, 128, (23, 5)), (300, 1, (1, 1))):
    CASES[f"grid-B{_B}-n{_n}-N{_N}-D{_D}"] = U.grid_case(_B, _n, _N, _D, seed=_B)


@pytest.mark.parametrize("name", sorted(CASES))
def test_standin_accept_passes(name):
    s, pred = CASES[name]
    U.check_loop(run_standin(s, pred), U.accept_step(s, pred), name)


ACCEPT_DEFECTS = [("last draft on a tie", "lengths-N3-D10"),
                  ("bonus token dropped", "lengths-N3-D10"),
                  ("EOS in the rejected tail finishes the row", "eos-N3-D10"),
                  ("EOS in a draft that was not chosen finishes the row", "eos-N3-D10"),
                  ("compaction does not keep the order", "finish-257-of-300"),
                  ("finished rows beyond the 256th are not copied out", "finish-257-of-300"),
                  ("finished rows beyond the 256th are not copied out", "finish-all-1100"),
                  ("width off by one", "finish-nobody"),
                  ("width off by one", "width-maxlen-1-nofinisher")]


@pytest.mark.parametrize("defect,name", ACCEPT_DEFECTS)
def test_defective_accept_is_flagged(defect, name):
    s, pred = CASES[name]
    with pytest.raises(AssertionError):
        U.check_loop(run_standin(s, pred, defect), U.accept_step(s, pred), name)


def test_a_write_into_a_margin_is_flagged():
    s, pred = CASES["pad-written"]
    dev = run_standin(s, pred)
    dev.bufs["rec"].buf[U.GUARD + dev.bufs["rec"].n] = 7                 # one element past the last record
    with pytest.raises(AssertionError, match="margin"):
        U.check_loop(dev, U.accept_step(s, pred), "rec overrun")
    dev = run_standin(s, pred)
    dev.bufs["out"].buf[U.GUARD - 1] = 7
    with pytest.raises(AssertionError, match="margin"):
        U.check_loop(dev, U.accept_step(s, pred), "out underrun")


def test_a_write_the_rule_does_not_make_is_flagged():
    """A finished row copied one column too wide, and a record written for a slot beyond the running ones."""
    s, pred = CASES["eos-N3-D10"]
    want = U.accept_step(s, pred)
    fin_row = int(want.rec[np.nonzero(want.rec[:s.words["n_active"], 4] == 1)[0][0], 0])
    dev = run_standin(s, pred)
    dev.bufs["out"].v[fin_row, want.words["width"]] = PAD
    with pytest.raises(AssertionError, match="out"):
        U.check_loop(dev, want, "wide copy")
    s2, pred2 = CASES["grid-B5-n3-N3-D10"]
    dev = run_standin(s2, pred2)
    dev.bufs["rec"].v[4] = torch.tensor([0, 0, 0, 0, 0], dtype=torch.int32)
    with pytest.raises(AssertionError, match="rec"):
        U.check_loop(dev, U.accept_step(s2, pred2), "record beyond n_active")


def test_greedy_step_is_the_greedy_oracle_loop():
    """greedy_step against a direct replay of standard_decoding.py:45-53 on seeded predictions: columns and the stopping step."""
    rng = np.random.default_rng(3)
    for B, max_len, p_end in ((1, 9, 0.3), (10, 12, 0.6), (10, 7, 0.0), (257, 30, 0.9)):
        s = U.make_state(B, 1, 0, max_len, 0, seed=B, permute=False)
        out = np.full((B, max_len), PAD, dtype=np.int64)
        out[:, 0] = BOS
        steps, done = 0, False
        for i in range(1, max_len):
            t = np.where(rng.random(B) < p_end, rng.choice([EOS, PAD], size=B), rng.integers(3, 30, size=B)).astype(np.int32)
            assert not s.words["stop"]
            s = U.greedy_step(s, t)
            out[:, i] = t
            steps += 1
            if ((t == EOS) | (t == PAD)).all():
                done = True
                break
        assert s.words["stop"] == 1 and s.words["steps"] == 3 + steps and (done or steps == max_len - 1)
        np.testing.assert_array_equal(s.gen[:, :max_len], out)


# -- argmax, embedding, K/V commit ---------------------------------------------------------------------------------------------
def argmax_operands(V=70, rows=9, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, V)).astype(np.float32)
    x[1, [3, 67]] = 9.0                                                  # the maximum twice: the lower index wins
    x[2] = -np.inf
    x[3] = np.nan
    x[4, :] = 0.0
    x[4, 5] = -0.0
    return x


def standin_argmax(x, live, before, defect=None):
    out = before.copy()
    for r in range(len(before) if defect == "rows beyond the live count are written" else live):
        row = x[r]
        best, bi = -np.inf, None
        for c in range(len(row)):
            if row[c] > best or (defect == "last maximum" and row[c] == best and bi is not None):
                best, bi = row[c], c
        out[r] = 0 if bi is None else bi
    return out


@pytest.mark.parametrize("defect", [None, "last maximum", "rows beyond the live count are written"])
def test_argmax_checker(defect):
    x = argmax_operands()
    before = U.sentinel_array((9,), torch.int32)
    got = standin_argmax(x, 6, before, defect)
    if defect is None:
        U.check_argmax(got, x, 6, before, "stand-in")
        mixed = x.copy()
        mixed[0, 4] = np.nan                                             # outside the contract: any id in [0, V) passes
        for any_id in (0, 69):
            g2 = got.copy()
            g2[0] = any_id
            U.check_argmax(g2, mixed, 6, before, "mixed NaN row")
        g2[0] = 70
        with pytest.raises(AssertionError):
            U.check_argmax(g2, mixed, 6, before, "mixed NaN row out of range")
    else:
        with pytest.raises(AssertionError):
            U.check_argmax(got, x, 6, before, defect)


def embed_operands(seed=2):
    rng = np.random.default_rng(seed)
    V, d, B, N, D = 11, 64, 4, 3, 5
    table = rng.standard_normal((V, d)).astype(np.float32)
    pe = rng.standard_normal((40, d)).astype(np.float32)
    s = U.make_state(B, N, D, 30, [0, 7, 3, 12], n_active=3, seed=seed, V=V)
    s.gen[1, 7] = 99                                                     # an id outside [0, V): looked up as id 0
    return table, pe, s


def standin_embed_step(table, pe, s, n_active, before, defect=None):
    out = before.copy()
    R = U.rps(s.N, s.D)
    shift = 0 if defect == "position pos instead of pos + 1" else 1
    for g in range(n_active):
        b = s.act_idx[g]
        f = s.front[b]
        for rs in range(R):
            n, j = (rs - 1) // s.D, (rs - 1) % s.D
            tok, pos = (s.gen[b, f], f) if rs == 0 else (s.drafts[b, n, j], f + 1 + j)
            if rs == 0 and defect == "row 0 takes the first draft token":
                tok = s.drafts[b, 0, 0]
            tok = tok if 0 <= tok < table.shape[0] else 0
            out[g * R + rs] = table[tok] + pe[pos + shift]
    return out


@pytest.mark.parametrize("defect", [None, "position pos instead of pos + 1", "row 0 takes the first draft token"])
def test_embedding_checker(defect):
    table, pe, s = embed_operands()
    rows = s.B * U.rps(s.N, s.D)
    x = U.Buf((rows, 64), torch.float32)
    before = x.get().view(np.float32)
    x.set(standin_embed_step(table, pe, s, 3, before, defect))
    want = U.embed_step(table, pe, s.act_idx, s.front, s.gen, s.drafts, 3, before)
    if defect is None:
        U.check_buf(x, want, "stand-in")
        tok = np.array([3, 99, -1, 5, 0, 10, 7], dtype=np.int32)
        full = (table[np.where((tok < 0) | (tok >= 11), 0, tok)] + pe[np.arange(7) % 3 + 1]).astype(np.float32)
        np.testing.assert_array_equal(U.embed_full(table, pe, tok, 3, np.zeros((9, 64), np.float32))[:7].view(np.int32), full.view(np.int32))
    else:
        with pytest.raises(AssertionError):
            U.check_buf(x, want, defect)


def standin_kvcopy(rec, n_copy, qkv, k, v, N, D, defect=None):
    k, v = k.copy(), v.copy()
    d = k.shape[-1]
    R = U.rps(N, D)
    for slot in range(n_copy):
        b, best, nacc, f = (int(t) for t in rec[slot, :4])
        for j in range(nacc + (2 if defect == "n_acc + 2 rows are committed" else 1)):
            srow = 0 if j == 0 else 1 + best * D + (j if defect == "source row 1 + best*D + j" else j - 1)
            srow = min(srow, R - 1)
            k[:, b, f + j] = qkv[:, slot * R + srow, d:2 * d]
            v[:, b, f + j] = qkv[:, slot * R + srow, 2 * d:]
    return k, v


@pytest.mark.parametrize("defect", [None, "source row 1 + best*D + j", "n_acc + 2 rows are committed"])
def test_kv_commit_checker(defect):
    s, pred = CASES["grid-B5-n3-N3-D10"]
    rec = U.accept_step(s, pred).rec
    ops = U.kv_operands(rec, 3, s.B, s.N, s.D, d=64, Ld=2, Lc=s.max_len + s.D + 1, seed=4)
    k, v = standin_kvcopy(rec, 3, ops["qkv"], ops["k0"], ops["v0"], s.N, s.D, defect)
    kb, vb = U.Buf(k.shape, torch.float32, data=k), U.Buf(v.shape, torch.float32, data=v)
    wk, wv = U.kv_commit(rec, 3, ops["qkv"], ops["k0"], ops["v0"], s.N, s.D)
    if defect is None:
        U.check_buf(kb, wk, "K")
        U.check_buf(vb, wv, "V")
        assert (wk.view(np.int32) != ops["k0"].view(np.int32)).any()
    else:
        with pytest.raises(AssertionError):
            U.check_buf(kb, wk, defect)
        with pytest.raises(AssertionError):
            U.check_buf(vb, wv, defect)
