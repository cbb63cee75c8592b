"""The three kernels of the length-bucketed scoring pass on the MI355X (csrc/ttx_score_list.hip.h), one launch at a time through
ttx_debug_score_list, against the NumPy restatement of tests/util_score_list.py.  Results are exact; every output lies between
guard margins, and every element a rule does not write keeps its sentinel."""
import numpy as np
import pytest
import torch

from util_models import tiny_state
from util_score_list import BOS, EOS, PAD, extents, first_difference, make_batch, pack, unpack

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 2, 2), (3, 7, 2, 5, 8), (2, 65, 3, 66, 66), (4, 33, 1, 200, 203)]      # (B, Ls, N, W, ld_hyp)
GUARD = 37                                                                                 # elements on either side of an array
V = 30


@pytest.fixture(scope="module")
def tiny():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    assert cfg["vocab_size"] == V
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)


def host_list() -> list:
    """The four batches, with every kind of row and source the rules tell apart."""
    rng = np.random.default_rng(30)
    L = [make_batch(rng, B, Ls, N, W, V) for B, Ls, N, W, _ in SHAPES]
    L[0]["hyp"][0, 0, 1] = EOS                         # W = 2: EOS in the last (and first scored) column; a source of width 1
    b = L[1]["hyp"]
    b[0, 0, 1:] = PAD                                  # all PAD
    b[0, 1, 1] = EOS                                   # EOS at column 1, tokens after it
    b[1, 0, 4] = EOS                                   # EOS at the last column
    b[1, 1, 2], b[1, 1, 4] = PAD, PAD                  # unfinished with a PAD inside: n = 3
    b[2, 0, 2] = EOS                                   # tokens after the EOS ...
    b[2, 1, 2], b[2, 1, 3] = EOS, EOS                  # ... and a second EOS
    L[1]["src"][0, 2], L[1]["src"][0, 5:] = PAD, PAD   # a source with an interior PAD and a PAD tail
    L[1]["src"][2, :] = PAD                            # an all-PAD source
    c = L[2]["hyp"]
    c[0, 0, 64], c[0, 1, 65], c[0, 2, 63] = EOS, EOS, EOS      # the 64-lane scan's chunk boundary
    c[1, :, 1:] = PAD                                  # a source whose rows are all PAD: e = max(2, 1)
    L[2]["src"][1, 64] = PAD
    d = L[3]["hyp"]
    d[0, 0, 129], d[0, 0, 130:] = EOS, PAD
    d[1, 0, 100:] = PAD                                # unfinished, n = 99
    d[2, 0, 199] = EOS
    d[3, 0, 5], d[3, 0, 150] = EOS, EOS
    L[3]["src"][1, 10:] = PAD
    L[3]["src"][3, 0], L[3]["src"][3, 32] = PAD, PAD
    return L


def device_list(L: list, shift: int = 0):
    """The list on the device: every hypothesis array inside a buffer with GUARD elements around it and ld_hyp - W columns of EOS
    behind every row (a kernel that read them would end the rows early); ``shift`` moves every base by that many elements, off the
    16-byte grid when odd."""
    out = []
    for b, (B, Ls, N, W, ld) in zip(L, SHAPES):
        buf = torch.full((shift + GUARD + B * N * ld + GUARD,), EOS, dtype=torch.int64)
        rows = buf[shift + GUARD:shift + GUARD + B * N * ld].view(B * N, ld)
        rows[:, :W] = torch.from_numpy(b["hyp"].reshape(B * N, W))
        sbuf = torch.full((shift + B * Ls,), 5, dtype=torch.int64)
        sbuf[shift:] = torch.from_numpy(b["src"].reshape(-1))
        dbuf, dsrc = buf.cuda(), sbuf.cuda()
        out.append((dsrc[shift:].view(B, Ls), dbuf[shift + GUARD:shift + GUARD + B * N * ld].view(B * N, ld), N, W))
    return out


def guarded(n: int, dtype, fill):
    """(buffer, view of its n inner elements): GUARD elements of ``fill`` on either side."""
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf: torch.Tensor, fill) -> bool:
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


@pytest.mark.parametrize("shift", [0, 1])
def test_extents(tiny, shift):
    L = host_list()
    D = device_list(L, shift)
    S, R = sum(s[0] for s in SHAPES), sum(s[0] * s[2] for s in SHAPES)
    e_buf, e = guarded(S, torch.int32, -77)
    ls_buf, ls = guarded(S, torch.int32, -77)
    n_buf, n = guarded(R, torch.int32, -77)
    bad_buf, bad = guarded(1, torch.int32, -77)
    tiny.debug_score_list("extents", D, eos=EOS, d_e=e, d_ls=ls, d_n=n, d_bad=bad)
    we, wls, wn = extents(L)
    assert first_difference([n.cpu().numpy()], [wn], "n") is None, first_difference([n.cpu().numpy()], [wn], "n")
    assert first_difference([e.cpu().numpy()], [we], "e") is None, first_difference([e.cpu().numpy()], [we], "e")
    assert first_difference([ls.cpu().numpy()], [wls], "ls") is None, first_difference([ls.cpu().numpy()], [wls], "ls")
    assert int(bad) == 0
    assert all(guards_intact(b, -77) for b in (e_buf, ls_buf, n_buf, bad_buf))
    assert wn.tolist()[:7] == [1, 0, 1, 4, 3, 2, 2] and we.min() == 2 and wls.tolist()[:4] == [1, 5, 7, 1]     # the cases are there
    # n is the length k_hyp_score writes for the same rows
    row0 = 0
    for b, (B, Ls, N, W, _) in zip(L, SHAPES):
        hyp = torch.from_numpy(b["hyp"]).cuda()
        got = tiny.hypothesis_logprobs(torch.zeros((B, N, W - 1, V), device="cuda"), hyp, PAD, EOS).length
        assert torch.equal(got.reshape(-1), n[row0:row0 + B * N])
        row0 += B * N
    # optional outputs may be left out
    e2_buf, e2 = guarded(S, torch.int32, -77)
    ls2_buf, ls2 = guarded(S, torch.int32, -77)
    tiny.debug_score_list("extents", D, eos=EOS, d_e=e2, d_ls=ls2)
    assert torch.equal(e2, e) and torch.equal(ls2, ls)


@pytest.mark.parametrize("where,bit", [("src", 1), ("hyp0", 2), ("hyp_after_eos", 2), ("hyp_last", 2), ("both", 3), ("negative", 2)])
def test_extents_flag_token_ids_outside_the_vocabulary(tiny, where, bit):
    L = host_list()
    if where in ("src", "both"):
        L[3]["src"][2, 32] = V
    if where in ("hyp0", "both"):
        L[2]["hyp"][1, 1, 0] = V + 5                   # column 0 is never scored, torch.nn.Embedding reads it all the same
    if where == "hyp_after_eos":
        L[3]["hyp"][3, 0, 199] = 1 << 40               # behind the first EOS, in the last column
    if where == "hyp_last":
        L[1]["hyp"][2, 1, 4] = V
    if where == "negative":
        L[0]["hyp"][0, 0, 0] = -1
    D = device_list(L)
    S = sum(s[0] for s in SHAPES)
    _, e = guarded(S, torch.int32, -77)
    _, ls = guarded(S, torch.int32, -77)
    _, bad = guarded(1, torch.int32, -77)
    tiny.debug_score_list("extents", D, eos=EOS, d_e=e, d_ls=ls, d_bad=bad)
    assert int(bad) == bit


# (sources, N, W_c, Ls_c): chunk widths below, equal to and above the members' own, odd and even
CHUNKS = [([8, 0, 6, 9], 1, 2, 1), ([8, 0, 6, 9], 1, 151, 20), ([0, 7], 1, 200, 33), ([9, 8, 7, 6, 0], 1, 204, 40), ([0], 1, 3, 2),
          ([3, 1], 2, 3, 4), ([1, 2, 3], 2, 5, 7), ([2], 2, 6, 8), ([3, 1], 2, 9, 11),
          ([5, 4], 3, 65, 64), ([4, 5], 3, 66, 65), ([5], 3, 67, 70)]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("case", range(len(CHUNKS)))
def test_pack(tiny, case, shift):
    sel, N, Wc, Lsc = CHUNKS[case]
    L = host_list()
    D = device_list(L, shift)
    src_buf, src_c = guarded(len(sel) * Lsc, torch.int64, -77)
    hyp_buf, hyp_c = guarded(len(sel) * N * Wc, torch.int64, -77)
    tiny.debug_score_list("pack", D, sel=sel, n=N, w=Wc, ls=Lsc, d_src_c=src_c, d_hyp_c=hyp_c)
    want_src, want_hyp = pack(L, sel, N, Wc, Lsc)
    msg = first_difference([src_c.cpu().numpy().reshape(want_src.shape)], [want_src], "src_c")
    assert msg is None, msg
    msg = first_difference([hyp_c.cpu().numpy().reshape(want_hyp.shape)], [want_hyp], "hyp_c")
    assert msg is None, msg
    assert guards_intact(src_buf, -77) and guards_intact(hyp_buf, -77)


@pytest.mark.parametrize("with_tok", [False, True])
@pytest.mark.parametrize("case", range(len(CHUNKS)))
def test_unpack(tiny, case, with_tok):
    sel, N, Wc, _ = CHUNKS[case]
    L = host_list()
    D = device_list(L)
    rng = np.random.default_rng(100 + case)
    Rc = len(sel) * N
    score_c = rng.standard_normal(Rc).astype(np.float32)
    length_c = rng.integers(0, Wc, Rc).astype(np.int32)
    fin_c = rng.integers(0, 2, Rc).astype(np.uint8)
    tok_c = rng.standard_normal((Rc, Wc - 1)).astype(np.float32)
    rows = np.cumsum([0] + [s[0] * s[2] for s in SHAPES])
    toks = np.cumsum([0] + [s[0] * s[2] * (s[3] - 1) for s in SHAPES])
    R, T = int(rows[-1]), int(toks[-1])
    sc_buf, sc = guarded(R, torch.float32, 9.0)
    ln_buf, ln = guarded(R, torch.int32, -7)
    fn_buf, fn = guarded(R, torch.uint8, 5)
    tk_buf, tk = guarded(T, torch.float32, 9.0)
    dev = lambda a: torch.from_numpy(a).cuda()
    tiny.debug_score_list("unpack", D, sel=sel, n=N, w=Wc, tok_off=toks[:-1] if with_tok else None, d_score_c=dev(score_c),
                          d_length_c=dev(length_c), d_fin_c=dev(fin_c), d_tok_c=dev(tok_c) if with_tok else None, d_score=sc,
                          d_length=ln, d_finished=fn, d_tok_logp=tk if with_tok else None)
    want = {"score": [np.full(s[:1] + s[2:3], 9.0, np.float32) for s in SHAPES], "length": [np.full(s[:1] + s[2:3], -7, np.int32) for s in SHAPES],
            "finished": [np.full(s[:1] + s[2:3], 5, np.uint8) for s in SHAPES],
            "tok": [np.full((s[0], s[2], s[3] - 1), 9.0, np.float32) for s in SHAPES]}
    unpack(L, sel, N, Wc, score_c, length_c, fin_c, tok_c if with_tok else None, want)
    split = lambda t, cuts, shapes: [t.cpu().numpy()[cuts[i]:cuts[i + 1]].reshape(shapes[i].shape) for i in range(len(SHAPES))]
    for name, t, cuts in (("score", sc, rows), ("length", ln, rows), ("finished", fn, rows), ("tok", tk, toks)):
        msg = first_difference(split(t, cuts, want[name]), want[name], name)
        assert msg is None, msg
    assert guards_intact(sc_buf, 9.0) and guards_intact(ln_buf, -7) and guards_intact(fn_buf, 5) and guards_intact(tk_buf, 9.0)


def test_unpack_without_finished(tiny):
    sel, N, Wc, _ = CHUNKS[6]
    D = device_list(host_list())
    Rc, R = len(sel) * N, sum(s[0] * s[2] for s in SHAPES)
    _, sc = guarded(R, torch.float32, 9.0)
    _, ln = guarded(R, torch.int32, -7)
    tiny.debug_score_list("unpack", D, sel=sel, n=N, w=Wc, d_score_c=torch.ones(Rc, device="cuda"),
                          d_length_c=torch.ones(Rc, dtype=torch.int32, device="cuda"), d_fin_c=torch.ones(Rc, dtype=torch.uint8, device="cuda"),
                          d_score=sc, d_length=ln)
    assert int((sc == 1.0).sum()) == Rc and int((ln == 1).sum()) == Rc
