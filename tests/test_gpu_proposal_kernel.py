"""k_proposal_drafts (csrc/ttx_proposal.hip.h), one launch at a time through ttx_debug_proposal_drafts on operands the test builds,
against the restatement of tests/util_proposal.py (tests/test_proposal_host.py shows that its checker can fail).  Everything is exact:
integers in, integers out.  The draft array starts as sentinels, so every element the rule does not write (drafts 1 .. N-1, the
inactive slot) must hold its sentinel afterwards, and every array stands between guard margins.

Every launch has B = 5 slots, one of them inactive.  The scenarios, four to a launch: fronts 0, 1, len - 1, len and beyond; proposals
that are the row moved by 0, +1, -1, -32, +31 places and by 33 and -33 (outside the window); a substitution inside the context; an EOS
inside the proposal; a proposal of length 0; the window of draft 0 across the proposal's end.
"""
import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_proposal as Q

pytestmark = pytest.mark.gpu
PAD, BOS, EOS, REPL = 0, 1, 2, 3
I32 = torch.int32
SENT = U.SENTINEL[I32]
DEV = "cuda"
B = 5
LD = 80                                        # row length of the proposal table
ROW = 60                                       # tokens of the rows behind BOS


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def scenarios(rng) -> tuple:
    """(base, [(name, front, proposal, expected shift or None)]): ``base`` holds ROW different tokens, so nothing agrees by chance."""
    base = [int(t) for t in rng.permutation(np.arange(4, 4 + ROW))]
    out = []
    for f, d in ((0, 0), (1, 0), (29, 0), (30, None), (35, None)):
        out.append((f"front-{f}-len-30", f, base[:30], d))
    for shift in (1, -1, -32, 31, 33, -33):                                # row token i stands at q[i + shift]
        q = ([int(t) for t in rng.integers(70, 80, size=shift)] + base) if shift > 0 else base[-shift:]
        out.append((f"shift{shift:+d}", 40, q[:LD - 1], shift if -32 <= shift <= 31 else None))
    sub = list(base)
    sub[38] = 99                                                          # the row's column 39: inside the context of front 40
    out.append(("substitution", 40, sub, 0))
    eos_in = list(base[:45])
    eos_in[41] = EOS
    out.append(("eos-inside", 40, eos_in, 0))
    out.append(("len-0", 12, [], None))
    out.append(("across-the-end", 40, base[:42], 0))
    out.append(("last-token", 40, base[:41], 0))
    return base, out


@pytest.mark.parametrize("ctx", [2, 4, 8])
@pytest.mark.parametrize("N,D", [(1, 1), (3, 4), (1, 10), (3, 10), (3, 70)])
def test_proposal_drafts(native, N, D, ctx):
    rng = np.random.default_rng(N * 100 + D)
    base, scen = scenarios(rng)
    gen_ld = ROW + 1 + D + 2
    inactive = ("inactive", 5, base[:20], 0)
    for g0 in range(0, len(scen), B - 1):
        group = scen[g0:g0 + B - 1]
        group = group + [scen[0]] * (B - 1 - len(group))
        hole = (g0 // (B - 1)) % B                                          # the inactive slot moves from launch to launch
        rows = group[:hole] + [inactive] + group[hole:]
        act_np = np.array([b for b in rng.permutation(B) if b != hole] + [hole], dtype=np.int32)
        front_np = np.array([r[1] for r in rows], dtype=np.int32)
        prop = Q.Proposals.of_rows([r[2] for r in rows], ld=LD)
        src_np = rng.permutation(B).astype(np.int32)                       # the table's rows are not in slot order
        tab_np = np.full((B, LD), SENT, dtype=np.int64)
        tab_np[src_np] = np.where(np.arange(LD)[None, :] < prop.length[:, None], prop.table, SENT)    # sentinels behind every length
        table = Q.Proposals(tab_np, prop.length[np.argsort(src_np)])
        gen_np = np.full((B, gen_ld), SENT, dtype=np.int64)                 # sentinels behind every front
        for b, r in enumerate(rows):
            gen_np[b, 0] = BOS
            gen_np[b, 1:r[1] + 1] = base[:r[1]]
        draft0_np = rng.integers(4, 60, size=(B, D))
        act, fr = U.Buf((B,), I32, DEV, act_np), U.Buf((B,), I32, DEV, front_np)
        gen = U.Buf((B, gen_ld), I32, DEV, gen_np)
        drafts = U.Buf((B, N, D), I32, DEV)                                 # all sentinels
        draft0 = U.Buf((B, D), I32, DEV, draft0_np)
        d_tab = U.Buf((B, LD), I32, DEV, tab_np)
        d_len = U.Buf((B,), I32, DEV, prop.length)
        d_src = U.Buf((B,), I32, DEV, src_np)
        kw = dict(proposal_tok=d_tab.v, proposal_len=d_len.v, proposal_src=d_src.v, n_active=B - 1, ctx=ctx, bos=BOS, eos=EOS, pad=PAD,
                  replace=REPL)
        native.debug_proposal_drafts(act.v, fr.v, gen.v, drafts.v, draft0.v, **kw)
        torch.cuda.synchronize()
        before = U.sentinel_array((B, N, D), I32).astype(np.int64)
        want = Q.proposal_drafts(before, draft0_np, act_np, B - 1, front_np, gen_np, table, src_np, ctx, BOS, EOS, PAD, REPL)
        what = f"N {N} D {D} ctx {ctx} launch {g0 // (B - 1)}"
        U.check_buf(drafts, want.astype(np.int32), what)
        for buf, was in ((act, act_np), (fr, front_np), (gen, gen_np), (draft0, draft0_np), (d_tab, tab_np), (d_len, prop.length),
                         (d_src, src_np)):
            assert buf.margins() is None, buf.margins()
            assert np.array_equal(buf.get(), np.asarray(was).astype(np.int32)), what
        # the restatement itself: the shifts the scenarios were built for, nothing outside draft 0 of the active slots
        assert (want[hole] == SENT).all() and (want[:, 1:] == SENT).all(), what
        for b, (name, f, q, d) in enumerate(rows):
            if b == hole:
                continue
            assert Q.choose_shift(gen_np[b], f, q, len(q), ctx) == d, f"{what} {name}"
            assert not np.isin(want[b, 0], (EOS, PAD, SENT)).any(), f"{what} {name}"
            if d is None:
                assert np.array_equal(want[b, 0], draft0_np[b]), f"{what} {name}"
            else:
                k = min(D, max(0, len(q) - (f + d)))                       # tokens the proposal still holds from the aligned place
                assert k >= 1 and np.array_equal(want[b, 0, k:], draft0_np[b, k:]), f"{what} {name}"
                head = [REPL if t in (EOS, PAD) else t for t in q[f + d:f + d + k]]
                assert want[b, 0, :k].tolist() == head, f"{what} {name}"
        # a second launch on its own output changes nothing: the rewrite reads draft0 and the table, never the live drafts
        native.debug_proposal_drafts(act.v, fr.v, gen.v, drafts.v, draft0.v, **kw)
        torch.cuda.synchronize()
        U.check_buf(drafts, want.astype(np.int32), what + ": second launch")


def test_refusals(native):
    z = lambda *s: torch.zeros(s, dtype=I32, device=DEV)
    tta_err = __import__("translation_transformer_amd")._native.TtxError
    act, fr, gen, drafts, draft0 = torch.arange(2, dtype=I32, device=DEV), z(2), z(2, 8), z(2, 1, 3), z(2, 3)
    tab, ln, src = z(2, 6), z(2), z(2)
    ok = dict(proposal_tok=tab, proposal_len=ln, proposal_src=src, n_active=2)
    native.debug_proposal_drafts(act, fr, gen, drafts, draft0, **ok)
    for bad in (dict(ok, ctx=3), dict(ok, n_active=3), dict(ok, proposal_len=ln + 7), dict(ok, proposal_src=src + 2)):
        with pytest.raises(tta_err):
            native.debug_proposal_drafts(act, fr, gen, drafts, draft0, **bad)
    with pytest.raises(tta_err):                                            # a front beyond the row
        native.debug_proposal_drafts(act, fr + 8, gen, drafts, draft0, **ok)
    with pytest.raises(tta_err):                                            # the same slot twice
        native.debug_proposal_drafts(z(2), fr, gen, drafts, draft0, **ok)
