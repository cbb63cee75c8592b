"""tests/util_beam_mask_checks.py on the CPU: the restatement of k_beam_step_masked by hand on small cases, the stand-in fp32
evaluation inside the checker's bound on every kind of case, the checker against planted defects of the stand-in (each must be
caught, and named by source, rank and field), and the argument checks of TranslationInferenceBeamSearchConstrained, which come before
it touches the model.  No GPU."""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import util_beam_mask_checks as M

NEG = -np.inf
F32, I32, U8 = np.float32, np.int32, np.uint8


def hand_case(logits, finished, score, *, beam, K, width=2, pfx=None):
    n_cand, V = len(finished), np.asarray(logits).shape[1]
    fin = np.asarray(finished, U8)
    run = np.flatnonzero(fin == 0)
    slot_of = np.full(n_cand, -1, I32)
    slot_of[run] = np.arange(len(run))
    c = NS(B=n_cand // beam, beam=beam, K=K, V=V, pad=M.PAD, eos=M.EOS, width=width, ld=width + 2, finished=fin, slot_of=slot_of,
           logits=np.asarray(logits, F32), score=np.asarray(score, F32), gen=(np.arange(n_cand * (width + 2)).reshape(n_cand, -1) % 50 + 3).astype(I32),
           summary=np.array([3, 0x7FFFFFFF, 0, 0, 0], I32), pfx_tok=None, pfx_len=None, pfx_src=None)
    if pfx is not None:
        c.pfx_tok, c.pfx_len, c.pfx_src = (np.asarray(x, I32) for x in pfx)
    return c


def test_by_hand_masked_row():
    # one source, two live parents, V = 4.  Parent 0 keeps tokens 1 and 3 (p = 1/4, 3/4 after renormalisation), parent 1 keeps none.
    ln = math.log
    c = hand_case([[NEG, ln(1.0), NEG, ln(3.0)], [NEG] * 4], [0, 0], [-1.0, -0.5], beam=2, K=4)
    tot, bnd = M.totals(c)
    assert np.allclose(tot[0, [1, 3]], [-1.0 + ln(0.25), -1.0 + ln(0.75)], rtol=0, atol=2e-7)   # the logits are fp32
    assert (tot[0, [0, 2]] == NEG).all() and (tot[1] == NEG).all() and not np.isnan(tot).any()
    assert (bnd[0, [1, 3]] > 0).all() and (bnd[0, [1, 3]] < 1e-5).all()
    picks = M.exact_order(c)
    assert picks == [[(0, 3), (0, 1), (0, 0), (0, 2)]]              # the finite ones best first, then -inf by ascending flat index
    o = M.standin(c)
    assert o["new_cand"][:, c.width].tolist() == [3, 1, M.PAD, M.PAD]   # a dead row carries PAD, not the forbidden token
    assert o["new_score"][2:].tolist() == [NEG, NEG] and o["new_finished"].tolist() == [0, 0, 1, 1]
    assert o["parent"].tolist() == [0, 0, 0, 0] and o["summary"][0] == 3 + 2
    assert (o["new_cand"][2, :c.width] == c.gen[0, :c.width]).all() and (o["new_cand"][2, c.width:] == M.PAD).all()
    M.check(o, c, "hand")


def test_by_hand_finished_dead_forced():
    # source 0: a finished parent (score -2) and a dead one; source 1: forced to token 3 with a live and a finished parent
    z = 1.0 + 3.0 * math.exp(-35.0)
    c = hand_case([[0.5, 1.5, 2.5, 3.5]], [1, 1, 0, 1], [-2.0, NEG, -0.25, -4.0], beam=2, K=2,
                  pfx=([[9, 3, 9], [9, 9, 9]], [0, 2], [1, 0]))
    assert M.forced_token(c, 0) is None and M.forced_token(c, 1) == 3
    tot, bnd = M.totals(c)
    assert abs(tot[0, M.PAD] - (-2.0 - math.log(z))) < 1e-12 and (tot[0, 1:] == NEG).all()    # PAD is a finished parent's one child
    assert (tot[1] == NEG).all()                                      # the dead parent
    assert tot[2].tolist() == [NEG, NEG, NEG, -0.25] and bnd[2, 3] == 0.0   # forced: the score itself, nothing added
    assert abs(tot[3, M.PAD] - (-4.0 - math.log(z))) < 1e-12              # a finished parent ignores the table
    assert M.exact_order(c) == [[(0, 0), (0, 1)], [(0, 3), (1, 0)]]
    o = M.standin(c)
    assert o["new_score"][2] == F32(-0.25) and o["new_finished"].tolist() == [1, 1, 0, 1] and o["new_score"][1] == NEG
    M.check(o, c, "hand")
    c.pfx_tok[0, 1] = 77                                               # an id outside [0, V) is read as 0
    assert M.forced_token(c, 1) == 0


KINDS = [("finite", 3, 3, 65), ("tenth", 5, 5, 64), ("tenth", 1, 3, 7), ("few", 3, 3, 65), ("few0", 5, 5, 7), ("few", 1, 3, 256),
         ("forced", 5, 5, 65), ("forced", 1, 3, 7), ("tie", 5, 5, 64)]


@pytest.mark.parametrize("kind,beam,K,V", KINDS)
@pytest.mark.parametrize("width", [1, 10])
def test_standin_inside_the_bound(kind, beam, K, V, width):
    c = M.case(beam=beam, K=K, V=V, kind=kind, width=width, ld=12, seed=V + beam)
    worst = M.check(M.standin(c), c, f"{kind} beam {beam} V {V}")
    assert worst <= 1.0
    if kind in ("few", "few0"):
        tot, _ = M.totals(c)
        counts = [int(np.isfinite(tot[b * beam:(b + 1) * beam]).sum()) for b in range(c.B)]
        assert counts == list((K, K - 1, 1) if kind == "few" else (0, 1, K - 1))
    if kind == "forced":
        assert [M.forced_token(c, b) is not None for b in range(3)] == [True, False, True]
        assert M.forced_token(c, 0) == 0                              # the id outside the vocabulary


# defect -> the case that shows it and the field the checker must name
PLANTED = {"inf_twice": ("few", "parent|token|new_finished"), "inf_first": ("few", "parent|token"), "dead_token": ("few", "token"),
           "dead_unfinished": ("few0", "new_finished"), "nan_row": ("few0", "parent|token|new_score"), "forced_logp": ("forced", "parent|token|new_score"),
           "forced_other_source": ("forced", "parent|token"), "tie_high": ("tie", "parent|token")}


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_checker_catches(defect):
    kind, field = PLANTED[defect]
    c = M.case(beam=5, K=5, V=65, kind=kind, width=3, ld=6, seed=11)
    M.check(M.standin(c), c, "clean")
    with pytest.raises(AssertionError, match=rf"source \d+ rank \d+ field ({field})"):
        M.check(M.standin(c, defect), c, defect)


def test_checker_names_the_first_difference():
    c = M.case(beam=5, K=5, V=65, kind="tenth", width=3, ld=6, seed=5)
    o = M.standin(c)
    o["new_len"][1 * c.K + 2] += 1
    with pytest.raises(AssertionError, match="source 1 rank 2 field new_len"):
        M.check(o, c, "planted")
    o = M.standin(c)
    o["new_cand"][7, c.width + 1] = 9                                    # beyond the new token: PAD
    with pytest.raises(AssertionError, match="source 1 rank 2 field new_cand"):
        M.check(o, c, "planted")
    o = M.standin(c)
    o["summary"][0] += 1
    with pytest.raises(AssertionError, match="summary"):
        M.check(o, c, "planted")
    o = M.standin(c)
    tot, bnd = M.totals(c)
    k, t = M.exact_order(c)[0][0]
    o["new_score"][0] = F32(o["new_score"][0] + 4 * bnd[k, t] + 2e-6)
    with pytest.raises(AssertionError, match="source 0 rank 0 field new_score"):
        M.check(o, c, "planted")


def test_refuses_malformed_arguments_before_the_model():
    import translation_transformer_amd as tta
    from translation_transformer_amd.syntax import SmilesSyntax
    assert tta.TranslationInferenceBeamSearchConstrained is tta.decoding.TranslationInferenceBeamSearchConstrained
    g = object.__new__(tta.TranslationInferenceBeamSearchConstrained)
    g.model = NS(device="cpu", tgt_vocab_size=12, src_pad_token_i=0, tgt_pad_token_i=0, check_tokens=lambda s: None)
    g.beam_size, g.max_len, g.pad_token, g.bos_token, g.eos_token = 3, 8, 0, 1, 2
    src = torch.tensor([[5, 6, 7], [5, 6, 0]])
    cls = torch.zeros(12, dtype=torch.int8)
    cls[4], cls[5] = 1, 2                                                # OPEN, CLOSE
    bad_calls = [dict(logit_bias=torch.zeros(2, 11)), dict(logit_bias=torch.zeros(3, 12)), dict(logit_bias=torch.zeros(2, 12, dtype=torch.int64)),
                 dict(logit_bias=torch.full((2, 12), float("nan"))), dict(allowed=torch.ones(2, 11, dtype=torch.bool)),
                 dict(syntax=torch.zeros(12, dtype=torch.int64)), dict(syntax=torch.zeros(30, dtype=torch.int8)),
                 dict(syntax=SmilesSyntax(cls), prefix=torch.tensor([[5, 4], [4, 5]])),           # the depth goes negative
                 dict(prefix=torch.tensor([[3, 4, 5]])), dict(prefix=torch.tensor([[3, 0, 5], [3, 4, 0]])),
                 dict(prefix=torch.tensor([[3, 12], [3, 4]])), dict(prefix=torch.full((2, 8), 3)), dict(prefix=torch.zeros(2, 3))]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            g.generate(src, **kw)
    # the unconstrained beam search keeps refusing, and points at the class that does not
    plain = object.__new__(tta.TranslationInferenceBeamSearch)
    with pytest.raises(ValueError, match="TranslationInferenceBeamSearchConstrained"):
        plain.generate(None, allowed=torch.ones(2, 12, dtype=torch.bool))
    with pytest.raises(ValueError, match="TranslationInferenceBeamSearchConstrained"):
        plain.generate(None, syntax=SmilesSyntax(cls))
