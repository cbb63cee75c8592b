"""k_sbs_step (csrc/ttx_sbs.hip.h) one launch at a time through ttx_debug_sbs_step, on the consistent operands of
util_sbs_checks.kernel_case, against the float64 restatement of tests/util_sbs_checks.py with its checker ``check_step``
(tests/test_sbs_checks_host.py shows that the checker can fail, and that these inputs keep float64 alone under the cap).

The margin: max |G'_fp32 - G'_float64| over the selected, well-conditioned children of these very inputs, NumPy restatement in
float32 against float64 on the CPU, is 3.9e-6 (FP32_GAP = 4.0e-6 bounds it); ten times that, MARGIN = 4.0e-5, for the device's
own expf / logf / log1pf.  A rank is excused where a neighbouring rank's float64 G' is within MARGIN or a child is ill-conditioned
(0 < Z - g < 1e-2); at most 5 % of the ranks of a parametrisation.  Exact beside that: every integer output given the selected
(parent, token) pairs, gumbel[rank 0] == G[0] on the bits, finished parents carried bit for bit, sentinels in everything the rule
does not write, guard margins, inputs untouched, a source alone against the same source among others, two launches, the trace
records, nothing written on a refusal; and one chi-square frequency check of the ordered first two draws on 4 096 workgroups.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import util_beam_checks as B
import util_sbs_checks as S
from util_sbs_checks import LEVEL, chi2_p

pytestmark = pytest.mark.gpu
DEV = "cuda"
IN = ["logits", "slot_of", "finished", "phi", "g", "gen", "key"]
OUT = ["new_cand", "new_phi", "new_g", "parent", "new_len", "new_finished", "parent_draft", "summary"]
TRACE = ["tr_parent", "tr_token", "tr_phi", "tr_g"]
I32, I64, F32, U8 = np.int32, np.int64, np.float32, np.uint8
SUMMARY0 = [7, 8, 7, 6, 5]


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def arrays_of(c: S.Case, trace: bool = False) -> dict:
    n = c.B * c.K
    a = dict(logits=c.logits, slot_of=c.slot_of, finished=c.finished.astype(U8), phi=c.phi, g=c.G, gen=c.gen, key=c.keys,
             new_cand=B.sent((n, c.ld), I64), new_phi=B.sent(n, F32), new_g=B.sent(n, F32), parent=B.sent(n, I32),
             new_len=B.sent(n, I32), new_finished=B.sent(n, U8), parent_draft=B.sent(n, I32), summary=np.array(SUMMARY0, I32))
    if trace:
        a.update(tr_parent=B.sent(n, I32), tr_token=B.sent(n, I32), tr_phi=B.sent(n, F32), tr_g=B.sent(n, F32))
    return a


def launch(native, c: S.Case, trace: bool = False, **over) -> dict:
    """Upload, one launch, margins and inputs checked, the outputs back."""
    arrays = arrays_of(c, trace)
    names = IN + OUT + (TRACE if trace else [])
    bufs = B.upload({k: arrays[k] for k in names}, DEV)
    kw = dict(V=c.V, ld=c.ld, width=c.width, B=c.B, beam=c.beam, K=c.K, pad=c.pad, eos=c.eos, pos=c.pos, seed=c.seed,
              inv_T=float(np.float32(1.0) / np.float32(c.temperature)))
    kw.update(over)
    native.debug_sbs_step(**kw, **{k: B.dev(bufs[k]) for k in names})
    torch.cuda.synchronize()
    B.check_margins(bufs)
    B.check_inputs(bufs, arrays, IN)
    return B.download(bufs, OUT + (TRACE if trace else []))


def sub_case(c: S.Case, b: int) -> S.Case:
    """Source b of a case alone: its candidates, its logits rows compacted in their order, its key."""
    cs = slice(b * c.beam, (b + 1) * c.beam)
    live = np.nonzero(c.slot_of[cs] >= 0)[0]
    slot_of = np.full(c.beam, -1, dtype=I32)
    slot_of[live] = np.arange(len(live), dtype=I32)
    logits = np.zeros((max(len(live), 1), c.V), dtype=F32)
    logits[:len(live)] = c.logits[c.slot_of[cs][live]]
    return c._replace(B=1, logits=logits, slot_of=slot_of, phi=c.phi[cs], G=c.G[cs], finished=c.finished[cs], gen=c.gen[cs],
                      keys=c.keys[b:b + 1])


def check_against_float64(c: S.Case, got: dict, what: str) -> int:
    """The integers exactly given the selection, the selection and values through check_step.  Returns the excused count."""
    excused = 0
    n_fin = 0
    for b in range(c.B):
        cs, ks = slice(b * c.beam, (b + 1) * c.beam), slice(b * c.K, (b + 1) * c.K)
        par_c = got["parent"][ks]
        assert ((par_c >= b * c.beam) & (par_c < (b + 1) * c.beam)).all(), f"{what}: parent outside source {b}: {par_c}"
        tok = got["new_cand"][ks, c.width]
        dev = SimpleNamespace(parent=par_c - b * c.beam, token=tok, phi=got["new_phi"][ks], g=got["new_g"][ks], finished=got["new_finished"][ks])
        bad, ex = S.check_step(dev, S.case_reference(c, b), c.G[cs], c.phi[cs], c.finished[cs], c.K, c.pad, c.eos, S.MARGIN)
        assert not bad, f"{what}, source {b}: " + "; ".join(bad[:4])
        excused += ex
        # rows: the parent's tokens, the new token, PAD up to ld
        want = np.full((c.K, c.ld), c.pad, dtype=I64)
        want[:, :c.width] = c.gen[par_c, :c.width]
        want[:, c.width] = tok
        B.same(got["new_cand"][ks], want, f"{what}: new_cand of source {b}")
        if np.isfinite(c.G[cs][0]):
            assert got["new_g"][ks][0].tobytes() == c.G[cs][0].tobytes(), f"{what}: gumbel of rank 0 is not the first parent's G"
        n_fin += int(got["new_finished"][ks].sum())
    n = c.B * c.K
    B.same(got["new_len"], np.full(n, c.width + 1, I32), f"{what}: new_len")
    B.same(got["parent_draft"], np.zeros(n, I32), f"{what}: parent_draft")
    B.same(got["summary"], np.array([SUMMARY0[0] + n_fin] + SUMMARY0[1:], I32), f"{what}: summary")
    assert set(np.unique(got["new_finished"]).tolist()) <= {0, 1}
    return excused


CASES = [(V, beam, K, t) for V in S.KERNEL_V for beam, K in S.KERNEL_BEAM_K for t in S.KERNEL_T]


@pytest.mark.parametrize("V,beam,K,t", CASES, ids=[f"V{v}-beam{b}-K{k}-T{t}" for v, b, k, t in CASES])
def test_sbs_step(native, V, beam, K, t):
    """B = 3 sources in one launch against float64, then source 1 alone (B = 1): the same bits."""
    c = S.kernel_case(V, beam, K, t)
    got = launch(native, c)
    excused = check_against_float64(c, got, "B = 3")
    assert excused <= S.EXCUSED_CAP * c.B * c.K, f"{excused} of {c.B * c.K} ranks excused"
    alone = launch(native, sub_case(c, 1))
    check_against_float64(sub_case(c, 1), alone, "alone")
    ks = slice(K, 2 * K)
    for name in ("new_cand", "new_phi", "new_g", "new_len", "new_finished", "parent_draft"):
        B.same(alone[name], got[name][ks], f"source 1 alone against among others: {name}")
    B.same(alone["parent"], got["parent"][ks] - beam, "source 1 alone against among others: parent")


def test_two_launches_agree_and_the_trace_records_the_selection(native):
    c = S.kernel_case(65, 5, 5, 1.0)
    first, second = launch(native, c, trace=True), launch(native, c)
    for name in OUT:
        B.same(first[name], second[name], f"two launches: {name}")
    B.same(first["tr_parent"], first["parent"] - (np.arange(c.B * c.K, dtype=I32) // c.K) * c.beam, "trace: parent rank")
    B.same(first["tr_token"], first["new_cand"][:, c.width].astype(I32), "trace: token")
    B.same(first["tr_phi"], first["new_phi"], "trace: phi")
    B.same(first["tr_g"], first["new_g"], "trace: g")


def test_default_keys_are_the_source_indices(native):
    c = S.kernel_case(64, 2, 2, 1.0)
    c = c._replace(keys=np.arange(c.B, dtype=I64))
    with_keys = launch(native, c)
    arrays = arrays_of(c)
    names = [k for k in IN + OUT if k != "key"]
    bufs = B.upload({k: arrays[k] for k in names}, DEV)
    native.debug_sbs_step(V=c.V, ld=c.ld, width=c.width, B=c.B, beam=c.beam, K=c.K, pad=c.pad, eos=c.eos, pos=c.pos, seed=c.seed,
                          inv_T=1.0 / c.temperature, **{k: B.dev(bufs[k]) for k in names})
    torch.cuda.synchronize()
    B.check_margins(bufs)
    got = B.download(bufs, OUT)
    for name in OUT:
        B.same(got[name], with_keys[name], f"keys absent: {name}")


def test_fewer_finite_children_than_k(native):
    """A root step with three finite logits and K = 5: the finite children first, then the -inf children by ascending token, finished,
    with phi' and G' -inf."""
    c = S.kernel_case(7, 1, 5, 1.0, B=1)
    x = c.logits.copy()
    x[0, [1, 3, 4, 6]] = -np.inf
    x[0, [0, 2, 5]] = [0.5, -0.25, 1.0]
    c = c._replace(logits=x)
    got = launch(native, c)
    check_against_float64(c, got, "few finite")
    assert sorted(got["new_cand"][:3, c.width].tolist()) == [0, 2, 5] and got["new_cand"][3:, c.width].tolist() == [1, 3]
    assert np.isneginf(got["new_g"][3:]).all() and np.isneginf(got["new_phi"][3:]).all() and got["new_finished"][3:].tolist() == [1, 1]


REFUSED = [dict(K=33), dict(beam=33), dict(V=1025), dict(V=0), dict(B=0), dict(K=8, beam=1, V=7), dict(width=99), dict(pos=0),
           dict(inv_T=0.0), dict(inv_T=float("inf")), dict(inv_T=float("nan")), dict(inv_T=-1.0)]


@pytest.mark.parametrize("over", REFUSED, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_refusals_write_nothing(native, over):
    import translation_transformer_amd as t
    c = S.kernel_case(7, 2, 2, 1.0)
    arrays = arrays_of(c)
    bufs = B.upload(arrays, DEV)
    kw = dict(V=c.V, ld=c.ld, width=c.width, B=c.B, beam=c.beam, K=c.K, pad=c.pad, eos=c.eos, pos=c.pos, seed=c.seed, inv_T=1.0)
    kw.update(over)
    with pytest.raises(t.TtxError) as e:
        native.debug_sbs_step(**kw, **{k: B.dev(bufs[k]) for k in arrays})
    assert e.value.code == -1
    torch.cuda.synchronize()
    B.check_margins(bufs)
    B.check_inputs(bufs, arrays, list(arrays))


def test_refuses_an_lds_image_beyond_150_kb_and_a_missing_array(native):
    import translation_transformer_amd as t
    c = S.kernel_case(7, 2, 2, 1.0)
    arrays = arrays_of(c)
    bufs = B.upload(arrays, DEV)
    kw = dict(ld=c.ld, width=c.width, B=c.B, pad=c.pad, eos=c.eos, pos=c.pos, seed=c.seed, inv_T=1.0)
    assert 32 * 1024 * 4 <= 150 * 1024                               # the largest (beam, V) the entry admits fits the image
    with pytest.raises(t.TtxError):
        native.debug_sbs_step(V=c.V, beam=c.beam, K=c.K, **kw, **{k: B.dev(bufs[k]) for k in arrays if k != "new_g"})
    with pytest.raises(t.TtxError):
        native.debug_sbs_step(V=c.V, beam=c.beam, K=c.K, **kw, **{k: B.dev(bufs[k]) for k in arrays},
                              tr_parent=B.dev(bufs["parent"]))           # one trace array without the others
    torch.cuda.synchronize()
    B.check_inputs(bufs, arrays, list(arrays))


def test_ordered_pairs_follow_sampling_without_replacement(native):
    """One launch of 4 096 workgroups with distinct keys on the same V = 4 logits, beam 1, K = 2: the ordered pair (first, second)
    has probability p_a p_b / (1 - p_a).  Chi-square at the 1e-4 level with the fixed seed for which the float64 restatement
    passes on the CPU (checked here on the same keys)."""
    n, V, seed = 4096, 4, 20190611
    x = np.array([[0.3, -0.4, 1.0, 0.1]], dtype=F32)
    p = np.exp(x[0].astype(np.float64))
    p /= p.sum()
    probs = (p[:, None] * p[None, :] / (1 - p[:, None]))[~np.eye(V, dtype=bool)]
    c = S.Case(V, 1, 2, n, 1.0, np.repeat(x, n, 0), np.arange(n, dtype=I32), np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, U8),
               np.full((n, 4), 1, I32), np.arange(1000, 1000 + n, dtype=I64), 1, 4, 1, seed, pad=-1, eos=-1)
    got = launch(native, c)
    tok = got["new_cand"][:, 1].reshape(n, 2)
    assert (tok[:, 0] != tok[:, 1]).all() and (got["new_g"].reshape(n, 2)[:, 0] == 0).all()

    def pairs(t):
        return np.bincount(t[:, 0] * V + t[:, 1], minlength=V * V).astype(np.float64).reshape(V, V)[~np.eye(V, dtype=bool)]
    ref = np.array([S.case_reference(c, b).token for b in range(n)])
    assert chi2_p(pairs(ref), probs) > LEVEL, "the float64 restatement fails the chi-square on these keys: pick another seed"
    assert chi2_p(pairs(tok), probs) > LEVEL
    assert (tok == ref).mean() > 0.99                                 # and the device draws what the restatement draws
