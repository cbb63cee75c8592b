"""Every exported form of a sampling, beam or scoring call, given arguments that say the same thing, is the same call (include/ttx.h:
"a NULL or zeroed option makes the call the plain one, launch for launch").  Through ctypes, on the tiny golden model, the first four
fixture sources, max_len 16, num_samples 2, temperature 2.0, one seed; speculative forms with draft_len 3 and n_drafts 2, the pool
with capacity 8 on one session, stochastic and standard beam search with beam_size 3.

Each form of a comparison runs on a session of its own that has served no call, so that the three launch counters of the session
(k_logit_bias, k_syntax_mask, k_beam_step_masked: launches enqueued or captured, a replayed graph adds none) start from the same
history and must move by the same amount.  Outputs are allocated filled with a sentinel and compared whole with ``torch.equal``.
No tolerance appears anywhere: everything is equality."""
import ctypes as C
from typing import NamedTuple

import pytest
import torch

from test_gpu_sampling import states
from util_models import fixture_tokens, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
SEED = 20261021
MAX_LEN, N_SAMPLES, T = 16, 2, 2.0
DRAFT_LEN, N_DRAFTS, CAPACITY, BEAM = 3, 2, 8, 3
PREFIX_LEN = [0, 1, 3, 5]
SENTINEL = -7
ALWAYS = [EOS, 4, 6, 7, 8]                    # frequent structure tokens of the fixture vocabulary (tests/test_gpu_logit_bias.py)


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def native(tta):
    st, cfg = states("tiny")
    return tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0)


class Inputs(NamedTuple):
    src: torch.Tensor           # Long[4, Ls] on the device, longest source first (the order a pool takes its list in)
    h_len: object               # the sources' lengths, host int32
    keys: torch.Tensor          # Long[4] on the device: 0..3, what a null d_row_keys stands for
    pre: torch.Tensor           # Long[4, 5] on the device: the forced prefixes, PAD beyond PREFIX_LEN
    h_plen: object              # PREFIX_LEN, host int32
    bias: torch.Tensor          # Float[4, V] on the device: 0 on the source's allow-list, -inf elsewhere
    c_token: int


@pytest.fixture(scope="module")
def inp(native):
    src, tgt, c_token, V = fixture_tokens()
    src = src[:4]
    lengths = ((src != PAD) * torch.arange(1, src.shape[1] + 1)).amax(1)
    order = torch.argsort(lengths, descending=True, stable=True)
    src, tgt, lengths = src[order][:, :int(lengths.max())].contiguous(), tgt[:4][order], lengths[order]
    pre = torch.full((4, max(PREFIX_LEN)), PAD, dtype=torch.int64)
    for b, n in enumerate(PREFIX_LEN):
        pre[b, :n] = tgt[b, 1:1 + n]
        assert not bool(torch.isin(pre[b, :n], torch.tensor([PAD, BOS, EOS])).any()), "the fixture target is shorter than its prefix"
    from translation_transformer_amd.scoring import allowlist_from_source, bias_from_allowed
    allowed = allowlist_from_source(src, ALWAYS, V, PAD)
    allowed[:, BOS] = False                   # every source row begins with BOS; no target holds one after column 0
    bias = bias_from_allowed(allowed).to(torch.float32)
    assert bool(torch.isinf(bias).any(1).all()) and bool((bias == 0).any(1).all())
    i32 = lambda xs: (C.c_int32 * len(xs))(*[int(x) for x in xs])
    return Inputs(src.cuda(), i32(lengths), torch.arange(4, dtype=torch.int64).cuda(), pre.cuda(), i32(PREFIX_LEN),
                  bias.cuda().contiguous(), c_token)


class Opt(NamedTuple):
    """The options of one sampling call as device tensors and host length arrays; all None: the plain call."""
    pre: object = None
    plen: object = None
    prop: object = None
    qlen: object = None
    bias: object = None


def ptr(t):
    return None if t is None else t.data_ptr()


def ld(t):
    return 0 if t is None else int(t.stride(0))


def counters(lib, sess) -> tuple:
    return (lib.ttx_debug_logit_bias_launches(sess), lib.ttx_debug_syntax_launches(sess), lib.ttx_debug_beam_step_masked_launches(sess))


def on_fresh_session(native, call):
    """``call(session) -> tuple`` on a session that has served no call: ``(what it returned, the counters' movement)``."""
    lib, sess = native._lib, native.new_session()
    try:
        assert counters(lib, sess) == (0, 0, 0)
        got = call(sess)
        torch.cuda.synchronize()
        return got, counters(lib, sess)
    finally:
        lib.ttx_session_destroy(sess)


def assert_same(native, calls: dict, moved=None) -> tuple:
    """Every call of ``calls`` (label -> call) returns the first one's values, bit for bit, and moves the counters as it does
    (``moved``: by exactly that).  Returns the first call's values."""
    first = None
    for label, call in calls.items():
        got, cnt = on_fresh_session(native, call)
        if first is None:
            first, first_label = (got, cnt), label
            assert moved is None or cnt == moved, f"{label}: the launch counters moved by {cnt}, expected {moved}"
            continue
        assert cnt == first[1], f"{label}: the launch counters moved by {cnt}, {first_label}'s by {first[1]}"
        assert len(got) == len(first[0])
        for i, (a, b) in enumerate(zip(got, first[0])):
            assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b, f"{label}: output {i} differs from {first_label}'s"
    return first[0]


# -- the sampling families ------------------------------------------------------------------------------------------------------
def sample_params(N_):
    return N_.SampleParams(MAX_LEN, N_SAMPLES, T, 0, 1.0, PAD, BOS, EOS, SEED)


def family(tta, native, inp, name: str):
    """``form(suffix, *mid) -> call``: the call ``ttx_sample_<name>generate<suffix>`` with ``mid`` between the parameters and the
    outputs; it returns ``(d_out, model_calls)`` and leaves the call's accepted draft tokens in ``form.accepted``."""
    N_, lib = tta._native, native._lib
    B, Ls = inp.src.shape
    if name == "plain":
        base, p = "ttx_sample_generate", sample_params(N_)
    else:
        base, p = "ttx_sample_speculative_generate", N_.SampleSpecParams(sample_params(N_), DRAFT_LEN, N_DRAFTS, inp.c_token, 0)
        if name == "pool":
            base += "_pool"

    def form(suffix, *mid):
        def call(sess):
            out = torch.full((B, N_SAMPLES, MAX_LEN), SENTINEL, dtype=torch.int64, device="cuda")
            st = N_.GenStats()
            if name == "pool":
                head = ((C.c_void_p * 1)(sess.value), 1, inp.src.data_ptr(), B, Ls, inp.h_len, inp.keys.data_ptr(), CAPACITY, C.byref(p))
            else:
                head = (sess, inp.src.data_ptr(), B, Ls, inp.keys.data_ptr(), C.byref(p))
            N_.check(getattr(lib, base + suffix)(*head, *mid, out.data_ptr(), C.byref(st), native._stream()))
            form.accepted = int(st.accepted_tokens)
            return out, int(st.model_calls)
        return call
    return form


def option_forms(tta, form, o: Opt, speculative: bool) -> dict:
    """The forms that can state the options ``o``, each stating exactly them."""
    N_ = tta._native
    opts = lambda: C.byref(N_.SampleOpts.of(ptr(o.pre), ld(o.pre), o.plen, ptr(o.prop), ld(o.prop), o.qlen, o.bias))
    calls = {}
    if o.bias is None and o.prop is None:
        calls["_prefix"] = form("_prefix", ptr(o.pre), ld(o.pre), o.plen)
    if o.bias is None and speculative:
        calls["_proposal"] = form("_proposal", ptr(o.pre), ld(o.pre), o.plen, ptr(o.prop), ld(o.prop), o.qlen)
    calls["_ex"] = form("_ex", opts())
    calls["_syntax, NULL syntax"] = form("_syntax", opts(), None)
    return calls


def unconstrained_forms(tta, form, speculative: bool) -> dict:
    N_ = tta._native
    calls = {"plain": form("")}
    calls.update(option_forms(tta, form, Opt(), speculative))             # NULL / 0 / NULL and zeroed opts
    calls["_ex, NULL opts"] = form("_ex", None)
    calls["_syntax, NULL opts and NULL syntax"] = form("_syntax", None, None)
    calls["_syntax, d_cls NULL"] = form("_syntax", C.byref(N_.SampleOpts()), C.byref(N_.Syntax(None, 0)))
    return calls


@pytest.fixture(scope="module")
def plain_rows(tta, native, inp):
    """The plain sampler's rows [4, 2, 16] (every unconstrained form gives them; the bias and syntax counters stay 0)."""
    return assert_same(native, unconstrained_forms(tta, family(tta, native, inp, "plain"), False), moved=(0, 0, 0))[0]


def proposal_of(rows: torch.Tensor) -> Opt:
    """Sample 0 of every source without its BOS, up to and including its first EOS: a proposal some of whose drafts are accepted
    (sample 0 accepts all of them, sample 1 diverges)."""
    q = rows[:, 0, 1:].cpu()
    ends = ((q == EOS) | (q == PAD)).int()
    qlen = [int(e.argmax()) + int(q[b, int(e.argmax())] == EOS) if bool(e.any()) else q.shape[1] for b, e in enumerate(ends)]
    assert min(qlen) >= 1
    return Opt(prop=q.cuda().contiguous(), qlen=(C.c_int32 * len(qlen))(*qlen))


def test_plain_sampler_unconstrained(plain_rows):
    assert plain_rows.shape == (4, N_SAMPLES, MAX_LEN) and bool((plain_rows[:, :, 0] == BOS).all()) and not bool((plain_rows == SENTINEL).any())
    assert not torch.equal(plain_rows[:, 0], plain_rows[:, 1]), "both samples of every source are equal: temperature 2 shows nothing"


def test_plain_sampler_prompted_and_biased(tta, native, inp, plain_rows):
    form = family(tta, native, inp, "plain")
    rows = assert_same(native, option_forms(tta, form, Opt(pre=inp.pre, plen=inp.h_plen), False), moved=(0, 0, 0))[0]
    for b, n in enumerate(PREFIX_LEN):
        assert torch.equal(rows[b, :, 1:1 + n], inp.pre[b, :n].expand(N_SAMPLES, n)), "a row does not begin with its prefix"
    assert torch.equal(rows[0], plain_rows[0]), "the source with the empty prefix"
    biased, cnt = on_fresh_session(native, form("_ex", C.byref(tta._native.SampleOpts.of(bias=inp.bias))))
    assert cnt[0] > 0 and cnt[1:] == (0, 0) and not torch.equal(biased[0], plain_rows)
    assert_same(native, option_forms(tta, form, Opt(bias=inp.bias), False), moved=cnt)


@pytest.mark.parametrize("name", ["speculative", "pool"])
def test_speculative_sampler(tta, native, inp, plain_rows, name):
    form = family(tta, native, inp, name)
    rows = assert_same(native, unconstrained_forms(tta, form, True), moved=(0, 0, 0))[0]
    accepted = form.accepted
    assert torch.equal(rows, plain_rows), "the speculative loop's rows are the plain sampler's"
    assert_same(native, option_forms(tta, form, Opt(pre=inp.pre, plen=inp.h_plen), True), moved=(0, 0, 0))
    assert_same(native, option_forms(tta, form, Opt(bias=inp.bias), True))
    proposed = assert_same(native, option_forms(tta, form, proposal_of(plain_rows), True), moved=(0, 0, 0))[0]
    assert torch.equal(proposed, plain_rows), "a proposal changes no row"
    # accepted_tokens itself is not compared between the forms: two identical proposed calls on fresh sessions can differ in it
    assert form.accepted > accepted, "no draft of the proposal was accepted: the proposed forms show nothing"


# -- stochastic beam search -----------------------------------------------------------------------------------------------------
def sbs_forms(tta, native, inp, filt, o: Opt, with_plain: bool) -> dict:
    N_, lib = tta._native, native._lib
    B, Ls = inp.src.shape
    p = N_.SbsParams(MAX_LEN, BEAM, T, PAD, BOS, EOS, SEED)
    f_arg = None if filt is None else C.byref(filt)

    def form(suffix, *mid):
        def call(sess):
            out = torch.full((B, BEAM, MAX_LEN), SENTINEL, dtype=torch.int64, device="cuda")
            logp = torch.full((B, BEAM), float(SENTINEL), dtype=torch.float32, device="cuda")
            gumbel = torch.full((B, BEAM), float(SENTINEL), dtype=torch.float32, device="cuda")
            st = N_.BeamSearchStats()
            N_.check(getattr(lib, "ttx_sbs_generate" + suffix)(sess, inp.src.data_ptr(), B, Ls, inp.keys.data_ptr(), C.byref(p), *mid,
                                                                out.data_ptr(), logp.data_ptr(), gumbel.data_ptr(), None, C.byref(st),
                                                                native._stream()))
            return out, logp, gumbel, int(st.model_calls)
        return call
    calls = {"plain": form("")} if with_plain else {}
    calls["_ex"] = form("_ex", f_arg, ptr(o.pre), ld(o.pre), o.plen)
    calls["_bias, NULL bias"] = form("_bias", f_arg, ptr(o.pre), ld(o.pre), o.plen, None, 0)
    return calls


def test_stochastic_beam_search(tta, native, inp):
    free = assert_same(native, sbs_forms(tta, native, inp, None, Opt(), True), moved=(0, 0, 0))
    masked = assert_same(native, sbs_forms(tta, native, inp, tta._native.SbsFilter(5, 1.0), Opt(pre=inp.pre, plen=inp.h_plen), False),
                         moved=(0, 0, 0))
    for b, n in enumerate(PREFIX_LEN):
        live = torch.isfinite(masked[2][b])
        assert bool(live.any()) and torch.equal(masked[0][b, live, 1:1 + n], inp.pre[b, :n].expand(int(live.sum()), n))
    assert not torch.equal(free[0], masked[0])


# -- standard beam search -------------------------------------------------------------------------------------------------------
def test_beam_search(tta, native, inp):
    N_, lib = tta._native, native._lib
    B, Ls = inp.src.shape
    p = N_.BeamSearchParams(MAX_LEN, BEAM, PAD, BOS, EOS)

    def form(constrained: bool, scores: bool):
        def call(sess):
            out = torch.full((B, BEAM, MAX_LEN), SENTINEL, dtype=torch.int64, device="cuda")
            score = torch.full((B, BEAM), float("nan"), dtype=torch.float32, device="cuda")
            st = N_.BeamSearchStats()
            if constrained:
                N_.check(lib.ttx_beam_generate_constrained(sess, inp.src.data_ptr(), B, Ls, C.byref(p), None, 0, None, None, 0, None,
                                                           out.data_ptr(), score.data_ptr() if scores else None, C.byref(st),
                                                           native._stream()))
            else:
                N_.check(lib.ttx_beam_generate(sess, inp.src.data_ptr(), B, Ls, C.byref(p), out.data_ptr(), C.byref(st), native._stream()))
            assert scores != bool(torch.isnan(score).all()), "d_score is written exactly when it is given"
            return out, int(st.model_calls), int(st.out_width)
        return call
    assert_same(native, {"ttx_beam_generate": form(False, False), "_constrained, all NULL": form(True, False),
                         "_constrained, all NULL, d_score": form(True, True)}, moved=(0, 0, 0))


# -- scoring --------------------------------------------------------------------------------------------------------------------
def score_outputs(R: int, W: int, V: int, logits: bool):
    """Every output array of a scoring call, filled with the sentinel; with ``logits`` those of ttx_score_proposal, ``logits`` eighth."""
    full = lambda shape, dtype: torch.full(shape, SENTINEL & 0xFF if dtype == torch.uint8 else SENTINEL, dtype=dtype, device="cuda")
    o = dict(tok_logq=full((R, W - 1), torch.float32), logq=full((R,), torch.float32), first_outside=full((R,), torch.int32),
             rank=full((R, W - 1), torch.int32), n_kept=full((R, W - 1), torch.int32), length=full((R,), torch.int32),
             finished=full((R,), torch.uint8))
    if logits:
        o.update(logits=full((R, W - 1, V), torch.float32), tok_logp=full((R, W - 1), torch.float32), score=full((R,), torch.float32))
    return o


@pytest.mark.parametrize("temperature", [T, 1.0])       # 1.0 without a filter: the branch that copies ttx_score_hypotheses' values
def test_scoring(tta, native, inp, plain_rows, temperature):
    N_, lib = tta._native, native._lib
    (B, Ls), W, V = inp.src.shape, MAX_LEN, native.tgt_vocab_size
    R = B * N_SAMPLES
    hyp = plain_rows.reshape(R, W).contiguous()
    dist = N_.Dist(temperature, 0, 1.0)

    def proposal(suffix, *mid):
        def call(sess):
            o = score_outputs(R, W, V, True)
            N_.check(getattr(lib, "ttx_score_proposal" + suffix)(
                sess, inp.src.data_ptr(), B, Ls, hyp.data_ptr(), W, N_SAMPLES, W, EOS, C.byref(dist), None, *mid, o["logits"].data_ptr(),
                o["tok_logp"].data_ptr(), o["score"].data_ptr(), o["tok_logq"].data_ptr(), o["logq"].data_ptr(),
                o["first_outside"].data_ptr(), o["rank"].data_ptr(), o["n_kept"].data_ptr(), o["length"].data_ptr(),
                o["finished"].data_ptr(), native._stream()))
            return tuple(o.values())
        return call
    got = assert_same(native, {"ttx_score_proposal": proposal(""), "_bias, NULL bias": proposal("_bias", None, 0),
                               "_syntax, NULL bias and NULL syntax": proposal("_syntax", None, 0, None)}, moved=(0, 0, 0))
    logits = got[7]
    assert logits.shape == (R, W - 1, V) and not bool((logits == SENTINEL).any())

    def logq(suffix, *mid):
        def call(sess):
            o = score_outputs(R, W, V, False)
            N_.check(getattr(lib, "ttx_hypothesis_logq" + suffix)(
                sess, logits.data_ptr(), hyp.data_ptr(), R, W, V, PAD, EOS, C.byref(dist), None, *mid, o["tok_logq"].data_ptr(),
                o["logq"].data_ptr(), o["first_outside"].data_ptr(), o["rank"].data_ptr(), o["n_kept"].data_ptr(),
                o["length"].data_ptr(), o["finished"].data_ptr(), native._stream()))
            return tuple(o.values())
        return call
    assert_same(native, {"ttx_hypothesis_logq": logq(""), "_bias, NULL bias": logq("_bias", None, 0, N_SAMPLES),
                         "_syntax, NULL bias and NULL syntax": logq("_syntax", None, 0, N_SAMPLES, None)}, moved=(0, 0, 0))
