"""Cross-attention maps of hypotheses on the MI355X (k_attn_probs through ttx_debug_attn_probs, ttx_attention_maps,
NativeTransformer.attention_maps, the generators' attention(), predict_with_attention) against the float64 restatement of the
definition (tests/util_attn_maps.py) and the reference's own maps (tests/golden/attn_maps.npz, made by
tests/golden/make_golden_attn.py).  Tolerances are measured at run time: 4 x the distance of an fp32 restatement (the reference's,
or plain NumPy / torch fp32 on the same operands) from float64; everything else is exact."""
import itertools
import json

import numpy as np
import pytest
import torch

import util_attn_maps as A
import util_loop_checks as U
from util_models import PAD, EOS, fixture_tokens, tiny_state
from test_gpu_score import _generators, _module          # the generator table and the Lightning stand-in of the score surface

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def tiny(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)


# -- 1. the kernel alone -----------------------------------------------------------------------------------------------
# (head_dim, H, T, Ls, N): a list, not the product.  The kernel's own boundaries: 64-key slots (63/64/65, 127/128/129), a round of
# 4 slots over the 4 waves (256/257), 16-query tiles (16/17), 16-byte rows (Ls % 4), dynamic LDS above 64 KiB (448/449 with the
# head sums at head dimension 32), the key limit (1024).
KERNEL_CASES = [(32, 1, 1, 1, 1), (32, 3, 2, 2, 3), (64, 8, 63, 63, 1), (32, 8, 64, 64, 3), (64, 3, 65, 65, 1), (32, 3, 17, 127, 3),
                (64, 1, 16, 128, 1), (32, 8, 5, 129, 1), (64, 8, 20, 256, 1), (64, 8, 20, 257, 3), (64, 3, 33, 385, 3),
                (32, 3, 18, 448, 1), (32, 3, 18, 449, 1), (64, 3, 5, 1024, 1), (32, 8, 3, 1024, 3)]
GUARD = 64


def _operands(dh, H, T, Ls, N, seed, ragged_ld):
    rng = np.random.default_rng(seed)
    Rm = 4 if N == 1 else 3
    R = Rm * N
    ldq, ldkv = (H * dh + 5, H * dh + 3) if ragged_ld else (H * dh, 2 * H * dh)
    q = rng.standard_normal((R * T, ldq)).astype(np.float32)
    k = rng.standard_normal((Rm * Ls, ldkv)).astype(np.float32)
    scale = 1.0 / np.sqrt(dh)
    top = max(np.abs(q[:, h * dh:(h + 1) * dh] @ k[:, h * dh:(h + 1) * dh].T).max() for h in range(H)) * scale
    q *= np.float32(6.0 / top)                                            # |score| <= 6
    key_pad = np.zeros((Rm, Ls), np.uint8)
    key_pad[0, Ls - Ls // 3:] = 1                                          # trailing
    key_pad[1, 1::5] = 1                                                   # interior
    key_pad[2, :] = 1                                                      # a source that is all PAD
    mem_row = (np.arange(R) // N).astype(np.int32)
    length = np.array([(T, 0, 1, (T + 1) // 2)[(r + r // 4) % 4] for r in range(R)], np.int32)
    return dict(q=q, k=k, key_pad=key_pad.reshape(-1), mem_row=mem_row, length=length, H=H, dh=dh, T=T, Ls=Ls, scale=float(scale))


class _Out:
    """The three outputs inside sentinel-filled buffers with guard margins; ``shift`` floats move the bases off 16 bytes."""

    def __init__(self, R, H, T, Ls, want=("heads", "mean", "align"), shift=0):
        self.shapes = {"heads": (R, H, T, Ls), "mean": (R, T, Ls), "align": (R, T)}
        self.dtypes = {"heads": torch.float32, "mean": torch.float32, "align": torch.int32}
        self.lo = GUARD + shift
        self.buf, self.view = {}, {}
        for name in want:
            n = int(np.prod(self.shapes[name]))
            fill = U.sentinel_array((self.lo + n + GUARD,), self.dtypes[name])
            self.buf[name] = torch.from_numpy(fill.copy()).cuda()
            self.view[name] = self.buf[name][self.lo:self.lo + n].view(self.shapes[name])

    def ptr(self, name):
        return self.view.get(name)

    def result(self) -> dict:
        out = {}
        for name, buf in self.buf.items():
            raw = buf.cpu().numpy()
            n = int(np.prod(self.shapes[name]))
            fill = U.sentinel_array(raw.shape, self.dtypes[name])
            as_bits = (lambda a: a.view(np.int32))
            assert np.array_equal(as_bits(raw[:self.lo]), as_bits(fill[:self.lo])), f"{name}: guard in front overwritten"
            assert np.array_equal(as_bits(raw[self.lo + n:]), as_bits(fill[self.lo + n:])), f"{name}: guard behind overwritten"
            body = raw[self.lo:self.lo + n]
            assert not (as_bits(body) == as_bits(fill[:n])).any(), f"{name}: elements left unwritten"
            out[name] = body.reshape(self.shapes[name])
        return out


def _launch(model, o, want=("heads", "mean", "align"), shift=0, rows=None):
    """One ttx_debug_attn_probs launch on the operands ``o`` (``rows``: only these query rows) -> result dict."""
    T, Ls, H, dh = o["T"], o["Ls"], o["H"], o["dh"]
    q, mem_row, length = o["q"], o["mem_row"], o["length"]
    if rows is not None:
        q = q.reshape(-1, T, q.shape[1])[rows].reshape(-1, q.shape[1])
        mem_row, length = mem_row[rows], length[rows]
    out = _Out(len(length), H, T, Ls, want, shift)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q, o["k"], o["key_pad"], mem_row, length)]
    model.debug_attn_probs(dev[0], dev[1], dev[2], dev[4], H, dh, T, Ls, o["scale"], mem_row=dev[3], out_heads=out.ptr("heads"),
                           out_mean=out.ptr("mean"), out_align=out.ptr("align"))
    torch.cuda.synchronize()
    return out.result()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("idx", range(len(KERNEL_CASES)))
def test_kernel_against_float64(tiny, idx):
    dh, H, T, Ls, N = KERNEL_CASES[idx]
    o = _operands(dh, H, T, Ls, N, seed=100 + idx, ragged_ld=idx % 3 == 1)
    ref = A.np_attn_probs(**o, dtype=np.float64)["heads"]
    e_np = np.abs(A.np_attn_probs(**o, dtype=np.float32)["heads"].astype(np.float64) - ref).max()
    shift = 1 if idx % 2 else 0                                           # odd cases: bases off 16 bytes
    got = _launch(tiny, o, shift=shift)
    err = np.abs(got["heads"].astype(np.float64) - ref).max()
    pad_rows = (o["key_pad"].reshape(-1, Ls) != 0)[o["mem_row"]]
    live = A.live_mask(o["length"], T)
    sums = got["heads"].astype(np.float64).sum(-1)
    sum_err = np.abs(sums - 1)[np.broadcast_to((live & ~pad_rows.all(-1)[:, None])[:, None, :], sums.shape)]
    print(f"dh {dh} H {H} T {T} Ls {Ls} N {N}: max |P - float64| {err:.3e}, NumPy fp32 {e_np:.3e} (bound {4 * e_np:.3e}); "
          f"max |row sum - 1| {sum_err.max() if sum_err.size else 0:.3e} (bound {Ls * A.EPS32:.3e})")
    assert A.check_result(got, ref, pad_rows, o["length"], 4 * e_np) == []
    assert set(o["length"].tolist()) >= {0, 1, T} and pad_rows.all(-1).any()
    # every combination of requested outputs gives the same bits for those it writes
    for r in (1, 2):
        for want in itertools.combinations(("heads", "mean", "align"), r):
            part = _launch(tiny, o, want=want, shift=1 - shift)
            assert set(part) == set(want) and all(_same_bits(part[n], got[n]) for n in want), want
    # a row computed alone is bit-equal to the same row inside the batch
    for r in {0, len(o["length"]) - 1, 3 % len(o["length"])}:
        alone = _launch(tiny, o, rows=np.array([r]))
        assert all(_same_bits(alone[n], got[n][r:r + 1]) for n in got), r
    # key columns appended as PAD change no bit of the other columns
    for extra in (3, 64):
        if Ls + extra > 1024:
            continue
        Rm = o["key_pad"].size // Ls
        k2 = np.zeros((Rm, Ls + extra, o["k"].shape[1]), np.float32)
        k2[:, :Ls] = o["k"].reshape(Rm, Ls, -1)
        k2[:, Ls:] = 9.0
        pad2 = np.ones((Rm, Ls + extra), np.uint8)
        pad2[:, :Ls] = o["key_pad"].reshape(Rm, Ls)
        wide = _launch(tiny, {**o, "k": k2.reshape(Rm * (Ls + extra), -1), "key_pad": pad2.reshape(-1), "Ls": Ls + extra})
        assert _same_bits(wide["heads"][..., :Ls], got["heads"]) and (wide["heads"][..., Ls:] == 0).all()
        assert _same_bits(wide["mean"][..., :Ls], got["mean"]) and (wide["mean"][..., Ls:] == 0).all()
        assert np.array_equal(wide["align"], got["align"])


def test_kernel_refuses_what_it_cannot_take(tta, tiny):
    N = tta._native
    o = _operands(32, 1, 2, 8, 1, seed=1, ragged_ld=False)
    out = _Out(4, 1, 2, 8)
    dev = {n: torch.from_numpy(np.ascontiguousarray(o[n])).cuda() for n in ("q", "k", "key_pad", "mem_row", "length")}

    def call(**kw):
        a = dict(H=1, dh=32, T=2, Ls=8, heads=out.ptr("heads"), mean=out.ptr("mean"), align=out.ptr("align"))
        a.update(kw)
        p = lambda t: None if t is None else t.data_ptr()                 # noqa: E731
        return tiny._lib.ttx_debug_attn_probs(tiny._session, dev["q"].data_ptr(), 32, dev["k"].data_ptr(), 64, dev["key_pad"].data_ptr(),
                                              dev["mem_row"].data_ptr(), dev["length"].data_ptr(), 4, 4, a["H"], a["dh"], a["T"],
                                              a["Ls"], 1.0, p(a["heads"]), p(a["mean"]), p(a["align"]), tiny._stream())

    assert call(Ls=1025) == N.TTX_ERR_INVALID and b"1024" in tiny._lib.ttx_last_error()
    assert call(dh=48) == N.TTX_ERR_INVALID
    assert call(heads=None, mean=None, align=None) == N.TTX_ERR_INVALID
    assert call(T=0) == N.TTX_ERR_INVALID and call(H=2) == N.TTX_ERR_INVALID      # ldq < H * head_dim
    torch.cuda.synchronize()
    for name, buf in out.buf.items():                                      # nothing was launched: all sentinel
        assert np.array_equal(buf.cpu().numpy().view(np.int32), U.sentinel_array(buf.shape, out.dtypes[name]).view(np.int32))
    assert call() == N.TTX_OK
    torch.cuda.synchronize()
    out.result()


# -- 2. the tiny model against the reference's maps --------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_refs():
    """Per (case, layer): the float64 restatement and e_ref = max |reference fp32 - float64|, computed once."""
    st, cfg = tiny_state()
    out = {}
    for name, c in A.golden_cases().items():
        for layer in (0, 1):
            ref = A.oracle_maps(st, cfg["num_heads"], c["src"], c["hyp"], layer, PAD, EOS)
            out[name, layer] = (ref, float(np.abs(c[f"heads_l{layer}"].astype(np.float64) - ref).max()))
    return out


def _np(t):
    return None if t is None else t.cpu().numpy()


@pytest.mark.parametrize("layer", [0, 1])
def test_tiny_model_against_the_reference(tiny, fixture_refs, layer):
    c = A.golden_cases()["targets"]
    ref, e_ref = fixture_refs["targets", layer]
    src, hyp = torch.from_numpy(c["src"]).cuda(), torch.from_numpy(c["hyp"]).cuda()
    B, K, W = hyp.shape
    alls = tiny.attention_maps(src, hyp, layer=layer, heads="all")
    mean = tiny.attention_maps(src, hyp, layer=layer, heads="mean")
    assert alls.attn.shape == (B, K, 2, W - 1, src.shape[1]) and mean.attn.shape == (B, K, W - 1, src.shape[1])
    assert alls.attn.dtype == torch.float32 and alls.alignment.dtype == torch.int32 and alls.length.dtype == torch.int32
    assert np.array_equal(_np(alls.length), c["length"]) and torch.equal(alls.length, mean.length)
    got = {"heads": _np(alls.attn).reshape(ref.shape), "mean": _np(mean.attn).reshape(B * K, W - 1, -1),
           "align": _np(mean.alignment).reshape(B * K, W - 1)}
    err = np.abs(got["heads"].astype(np.float64) - ref).max()
    print(f"layer {layer}: max |GPU - float64| {err:.3e}; e_ref {e_ref:.3e}; bound 4 e_ref {4 * e_ref:.3e}; ratio {err / e_ref:.2f}")
    pad_rows = np.repeat(c["src"] == PAD, K, axis=0)
    assert A.check_result(got, ref, pad_rows, c["length"], 4 * e_ref) == []
    assert torch.equal(alls.alignment, mean.alignment)
    if layer == 1:                                                         # -1 is the last layer
        assert torch.equal(tiny.attention_maps(src, hyp, heads="mean").attn, mean.attn)
    # the alignment against the reference's, where the reference's two largest values are clearly apart
    miss, compared, live = A.align_agreement(got["align"], c[f"heads_l{layer}"], c["length"], 2 * 4 * e_ref)
    print(f"layer {layer}: alignment compared at {compared} of {live} live positions, {miss} differ")
    assert live - compared <= 0.02 * live and miss == 0


@pytest.mark.parametrize("layer", [0, 1])
def test_rule_rows(tiny, fixture_refs, layer):
    c = A.golden_cases()["rule"]
    ref, e_ref = fixture_refs["rule", layer]
    src, hyp = torch.from_numpy(c["src"]).cuda(), torch.from_numpy(c["hyp"]).cuda()
    B, K, W = hyp.shape
    for trim in (True, False):
        m = tiny.attention_maps(src, hyp, layer=layer, heads="all", trim=trim)
        assert _np(m.length).reshape(-1).tolist() == [1, 4, 11, 0, 6, 3]
        heads = _np(m.attn).reshape(ref.shape)
        got = {"heads": heads, "align": _np(m.alignment).reshape(B * K, W - 1)}
        assert A.check_result(got, ref, np.repeat(c["src"] == PAD, K, axis=0), c["length"], 4 * e_ref) == []
        assert (heads[3] == 0).all() and (got["align"][3] == -1).all()     # the all-PAD hypothesis
        assert c["hyp"].reshape(-1, W)[4, 3] == PAD and heads[4, :, 3].sum() > 1.9 and got["align"][4, 3] >= 0   # PAD before the EOS: live


# -- 3. invariance on the bits ------------------------------------------------------------------------------------------
def test_maps_do_not_depend_on_the_call(tiny):
    src, tgt, _, _ = fixture_tokens()
    src, tgt = src.cuda(), tgt.cuda()
    B, W = tgt.shape
    hyp5 = torch.stack([tgt.roll(i, 0) for i in range(5)], dim=1)        # [B, 5, W]: hypothesis 0 of source b is its own target
    for heads in ("all", "mean"):
        whole = tiny.attention_maps(src, hyp5, heads=heads)
        again = tiny.attention_maps(src, hyp5, heads=heads)
        assert all(torch.equal(a, b) for a, b in zip(whole, again))
        for kw in (dict(max_rows=1), dict(max_rows=3 * 5 * (W - 1)), dict(trim=False), dict(trim=False, max_rows=2 * 5 * (W - 1))):
            other = tiny.attention_maps(src, hyp5, heads=heads, **kw)
            assert all(torch.equal(a, b) for a, b in zip(whole, other)), kw
        one_by_one = [tiny.attention_maps(src[b:b + 1], hyp5[b:b + 1], heads=heads) for b in range(B)]
        for i, name in enumerate(("attn", "alignment", "length")):
            assert torch.equal(torch.cat([m[i] for m in one_by_one]), whole[i]), name
        n1 = tiny.attention_maps(src, hyp5[:, :1].contiguous(), heads=heads)
        assert torch.equal(n1.attn[:, 0], whole.attn[:, 0]) and torch.equal(n1.alignment[:, 0], whole.alignment[:, 0])
    none = tiny.attention_maps(src, hyp5, return_alignment=False)
    assert none.alignment is None and torch.equal(none.attn, whole.attn)


# -- 4. other models: head dimension 64, four heads ---------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hd64", "h4"])
def test_other_models_against_float64(tta, which):
    if which == "hd64":
        from util_hd64 import hd64_state
        st, cfg = hd64_state()
    else:
        from util_draft_select import h4_state
        st, cfg = h4_state()
    H = cfg["num_heads"]
    model = tta.NativeTransformer(st, H, 0, device=0)
    src, tgt, _, _ = fixture_tokens()
    src, tgt = src[[1, 5, 8]], tgt[[1, 5, 8]]
    hyp = torch.stack([tgt, tgt.roll(1, 0)], dim=1)
    length = A.lengths_of(hyp.reshape(-1, hyp.shape[-1]), PAD, EOS)
    pad_rows = np.repeat(src.numpy() == PAD, 2, axis=0)
    for layer in (0, 1):
        ref = A.oracle_maps(st, H, src, hyp, layer, PAD, EOS)
        # no reference maps for these models: the yardstick is what plain fp32 tensor algebra makes of the same definition
        e32 = np.abs(A.oracle_maps(st, H, src, hyp, layer, PAD, EOS, dtype=torch.float32).astype(np.float64) - ref).max()
        alls = model.attention_maps(src.cuda(), hyp.cuda(), layer=layer, heads="all")
        mean = model.attention_maps(src.cuda(), hyp.cuda(), layer=layer, heads="mean")
        got = {"heads": _np(alls.attn).reshape(ref.shape), "mean": _np(mean.attn).reshape(6, -1, src.shape[1]),
               "align": _np(mean.alignment).reshape(6, -1)}
        err = np.abs(got["heads"].astype(np.float64) - ref).max()
        print(f"{which} (H {H}, head dim {cfg['embedding_dim'] // H}) layer {layer}: max |GPU - float64| {err:.3e}; fp32 oracle {e32:.3e}")
        assert A.check_result(got, ref, pad_rows, length, 4 * e32) == []
    model.close()


# -- 5. the surface -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["greedy", "beam_search", "greedy_speculative", "beam_search_speculative"])
def test_generators_attention(tta, tiny, kind):
    g = _generators(tta, tiny)[kind]()
    src = fixture_tokens()[0][:4].cuda()
    pred = g.generate(src)
    calls = g.model_calls_num
    m = g.attention(src, pred)
    B, K, L = pred.shape
    assert isinstance(m, tta.AttentionMaps) and g.model_calls_num == calls
    assert m.attn.shape == (B, K, L - 1, src.shape[1]) and m.attn.dtype == torch.float32
    assert m.alignment.shape == (B, K, L - 1) and m.alignment.dtype == torch.int32
    assert m.length.dtype == torch.int32 and torch.equal(m.length, g.score(src, pred).length)
    live = torch.arange(L - 1, device="cuda").expand(B, K, -1) < m.length.unsqueeze(-1)
    assert (m.alignment[~live] == -1).all() and (m.alignment[live] >= 0).all()
    assert (m.alignment[live] < (src != PAD).sum(1)[:, None, None].expand(B, K, L - 1)[live]).all()
    a = g.attention(src, pred, heads="all", layer=0, return_alignment=False)
    assert a.attn.shape == (B, K, 2, L - 1, src.shape[1]) and a.alignment is None


@pytest.mark.parametrize("generation", ["greedy_speculative", "beam_search"])
def test_predict_with_attention(tta, tmp_path, generation, monkeypatch):
    monkeypatch.delenv("TTX_PREDICT_ATTENTION", raising=False)
    monkeypatch.delenv("TTX_PREDICT_SCORES", raising=False)
    src, tgt, _, _ = fixture_tokens()
    batches = []
    for i, j in ((0, 3), (3, 4), (4, 8)):
        s_ = src[i:j]
        batches.append({"src_tokens": s_[:, :int((s_ != PAD).sum(1).max())].cuda(), "tgt_tokens": tgt[i:j].cuda()})
    kw = dict(beam_size=3, smart_drafts_mode=False) if generation == "beam_search" else {}
    today = {"algorithm", "batch_size", "tgt_test_path", "max_len", "total_seconds", "model_calls", "seconds_per_model_call"}
    if "speculative" in generation:
        today |= {"n_drafts", "draft_len"}
    res = {}
    for schedule in ("rows", "batches"):                                   # served from the look-ahead window | decoded on the spot
        for on in (False, True):
            rf = tmp_path / f"r_{schedule}_{on}.txt"
            mod = _module(tta, generation, rf, **kw)
            mod.predict_with_attention = on
            outs = tta.run_predict(mod, batches, schedule=schedule, window=3, in_flight=2)
            rep = json.loads(rf.read_text().strip().split("\n")[-1])
            res[schedule, on] = (outs, rep, mod)
        (off_outs, off_rep, off_mod), (on_outs, on_rep, mod) = res[schedule, False], res[schedule, True]
        assert set(off_rep) == today and off_mod.predict_alignments == {}
        assert all(torch.equal(a, b) for a, b in zip(off_outs, on_outs)) and on_rep["model_calls"] == off_rep["model_calls"]
        assert set(on_rep) == today | {"attention_seconds"} and on_rep["attention_seconds"] > 0
        assert sorted(mod.predict_alignments) == list(range(len(batches)))
        for i, (b, p) in enumerate(zip(batches, on_outs)):
            al, ln = mod.predict_alignments[i]
            want = mod.generator.attention(b["src_tokens"], p)
            assert torch.equal(al, want.alignment) and torch.equal(ln, want.length) and al.shape == p.shape[:2] + (p.shape[2] - 1,)
        if schedule == "rows" and generation != "beam_search":
            assert mod._ahead is not None and mod._ahead.served == len(batches)
    monkeypatch.setenv("TTX_PREDICT_ATTENTION", "1")
    mod = _module(tta, generation, tmp_path / "r_env.txt", **kw)
    tta.run_predict(mod, batches, schedule="batches")
    assert sorted(mod.predict_alignments) == list(range(len(batches)))
    assert all(torch.equal(mod.predict_alignments[i][0], res["batches", True][2].predict_alignments[i][0]) for i in range(len(batches)))


def test_rejects_bad_inputs(tta, tiny):
    N = tta._native
    c = A.golden_cases()["rule"]
    src, hyp = torch.from_numpy(c["src"]).cuda(), torch.from_numpy(c["hyp"]).cuda()
    with pytest.raises(ValueError):
        tiny.attention_maps(src, hyp, heads="some")
    with pytest.raises(ValueError):
        tiny.attention_maps(src, hyp[:, :, :1])
    with pytest.raises(ValueError):
        tiny.attention_maps(src[:2], hyp)
    bad = hyp.clone()
    bad[1, 1, 2] = tiny.tgt_vocab_size
    with pytest.raises(IndexError):
        tiny.attention_maps(src, bad)
    for layer in (2, -2):
        with pytest.raises(tta.TtxError):
            tiny.attention_maps(src, hyp, layer=layer)
    # the C boundary refuses before any launch: the outputs keep their poison
    B, K, W = hyp.shape
    Ls = src.shape[1]
    lib, sess, stream = tiny._lib, tiny._scoring_session(), tiny._stream()
    mean = torch.full((B * K, W - 1, Ls), 7.0, device="cuda")
    align = torch.full((B * K, W - 1), 7, dtype=torch.int32, device="cuda")
    length = torch.full((B * K,), 7, dtype=torch.int32, device="cuda")
    wide = torch.zeros((1, 1025), dtype=torch.int64, device="cuda")

    def am(B_=B, Ls_=Ls, ld=W, N_=K, W_=W, layer=-1, outs=True, s=src):
        return lib.ttx_attention_maps(sess, s.data_ptr(), B_, Ls_, hyp.data_ptr(), ld, N_, W_, EOS, layer, None,
                                      mean.data_ptr() if outs else None, align.data_ptr() if outs else None, length.data_ptr(), stream)

    assert am(outs=False) == N.TTX_ERR_INVALID and b"no output" in lib.ttx_last_error()
    assert am(layer=2) == N.TTX_ERR_INVALID and am(layer=-2) == N.TTX_ERR_INVALID
    assert am(B_=1, Ls_=1025, s=wide) == N.TTX_ERR_INVALID and b"1024" in lib.ttx_last_error()
    assert am(W_=1) == N.TTX_ERR_INVALID and am(ld=W - 1) == N.TTX_ERR_INVALID
    assert am(W_=5002, ld=5002) == N.TTX_ERR_INVALID
    assert am(B_=0) == N.TTX_ERR_INVALID and am(N_=0) == N.TTX_ERR_INVALID
    assert am(B_=1 << 12, N_=1 << 6, W_=65, ld=65) == N.TTX_ERR_INVALID            # 2^24 positions
    torch.cuda.synchronize()
    assert (mean == 7.0).all() and (align == 7).all() and (length == 7).all()
    # the vocabulary limit of scoring does not apply, and the session is still usable
    assert am() == N.TTX_OK
    torch.cuda.synchronize()
    assert np.array_equal(length.cpu().numpy(), c["length"].reshape(-1))
    assert torch.equal(mean.view(B, K, W - 1, Ls), tiny.attention_maps(src, hyp, trim=False).attn)
