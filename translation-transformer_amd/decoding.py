"""Generators with the reference's constructor keywords, counters and ``generate`` contract
(src/model/lightning_model.py:92-137 shows how they are built), running on the
HIP library.  ``model`` must be a ``NativeTransformer``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _native as N
from .model import AttentionMaps, FoldedHypotheses, HypothesisScores, NativeTransformer, ProposalScores
from .scoring import combine_bias
from .syntax import as_syntax


def _refuse_bias(who: str, logit_bias, allowed) -> None:
    """The generators that take no logit bias say so, rather than decode unconstrained."""
    if logit_bias is not None or allowed is not None:
        raise ValueError(f"{who} takes no logit_bias / allowed: the per-source logit bias is implemented for TranslationInferenceSampling, "
                         "TranslationInferenceSamplingSpeculative (generate and generate_many) and "
                         "TranslationInferenceStochasticBeamSearch.generate; temperature=0 on the samplers is constrained greedy decoding, "
                         "and TranslationInferenceBeamSearchConstrained is beam search under a bias")


def _refuse_syntax(who: str, syntax) -> None:
    """The generators that take no syntax constraint say so, rather than decode unconstrained."""
    if syntax is not None:
        raise ValueError(f"{who} takes no syntax: the syntax constraint is implemented for TranslationInferenceSampling and "
                         "TranslationInferenceSamplingSpeculative (generate and generate_many); temperature=0 on the samplers is "
                         "greedy decoding that cannot emit an unbalanced row, and TranslationInferenceBeamSearchConstrained is beam search "
                         "under the constraint")


def _need_native(model) -> NativeTransformer:
    if not isinstance(model, NativeTransformer):
        raise TypeError("the native generators run on a NativeTransformer (no eager/PyTorch fallback exists)")
    return model


class _ScoresHypotheses:
    """``score`` for every generator: the model's log-likelihood of each returned hypothesis, by one teacher-forced pass over the
    finished rows (NativeTransformer.score_hypotheses) — the same scale for all four classes.  Scoring is no part of the
    reference's loops and leaves the counters (``model_calls_num`` and the rest) alone."""

    def _pad_eos(self) -> tuple:
        return self.pad_token, self.eos_token

    def score(self, src: torch.Tensor, pred: torch.Tensor, **kw) -> HypothesisScores:
        """``pred``: Long[B, N, L] as ``generate(src)`` returned it.  Keywords go to ``score_hypotheses``."""
        pad, eos = self._pad_eos()
        if pad != self.model.tgt_pad_token_i:
            raise ValueError("the generator's pad token differs from the model's")
        return self.model.score_hypotheses(src, pred, eos_token_idx=eos, **kw)

    def score_many(self, batches: list, preds: list, **kw) -> list:
        """``score`` for a list: ``preds[i]`` as ``generate_many(batches)`` returned it (None for a batch that came back None), one
        ``HypothesisScores`` or None per batch, in list order.  The whole list is scored in length buckets with one
        synchronisation (NativeTransformer.score_hypotheses_many, which takes the keywords)."""
        pad, eos = self._pad_eos()
        if pad != self.model.tgt_pad_token_i:
            raise ValueError("the generator's pad token differs from the model's")
        return self.model.score_hypotheses_many(batches, preds, eos_token_idx=eos, **kw)

    def attention(self, src: torch.Tensor, pred: torch.Tensor, **kw) -> AttentionMaps:
        """Cross-attention maps and source alignments of the hypotheses ``pred`` (Long[B, N, L] as ``generate(src)`` returned
        it), from the same teacher-forced pass as ``score``.  Keywords go to ``attention_maps``."""
        pad, eos = self._pad_eos()
        if pad != self.model.tgt_pad_token_i:
            raise ValueError("the generator's pad token differs from the model's")
        return self.model.attention_maps(src, pred, eos_token_idx=eos, **kw)

    def alternatives(self, src: torch.Tensor, pred: torch.Tensor, k: int = 5, **kw):
        """What the model considered at every position of the hypotheses ``pred`` (Long[B, N, L] as ``generate(src)`` returned
        it): an ``Alternatives`` (with ``with_scores=True`` also the ``HypothesisScores``), from the same teacher-forced pass
        as ``score``.  Keywords go to ``NativeTransformer.alternatives``."""
        pad, eos = self._pad_eos()
        if pad != self.model.tgt_pad_token_i:
            raise ValueError("the generator's pad token differs from the model's")
        return self.model.alternatives(src, pred, k=k, eos_token_idx=eos, **kw)

    def logq(self, src: torch.Tensor, pred: torch.Tensor, prefix=None, logit_bias=None, allowed=None, syntax=None,
             **kw) -> ProposalScores:
        """The log-probability of the hypotheses ``pred`` (Long[B, N, L] as ``generate(src)`` returned it) under a SAMPLING
        distribution, beside ``score`` (which gives it under the model): by default the generator's own ``temperature``,
        ``top_k`` and ``top_p`` where it has them (the two samplers, stochastic beam search), temperature 1 without a filter on
        the deterministic generators.  ``prefix``: the forced prefix the rows were generated with (``check_prefix``'s form);
        its positions cost nothing (``forced_len`` = the prefix lengths).  ``logit_bias`` (Float[B, V]) and / or ``allowed``
        (Bool[B, V]): the per-source bias the rows were generated under (``generate``'s keywords): ``logq`` is then the
        log-probability under the biased distribution, ``-inf`` with ``first_outside`` at the first forbidden token for a row the
        biased sampler cannot emit, while ``with_scores=True`` keeps ``scores`` the raw model's.  ``syntax``: the ``SmilesSyntax``
        the rows were generated under (``generate``'s keyword): ``logq`` is the log-probability under the constrained sampler, with
        the generator's ``max_len`` as the rule's, and ``first_outside`` names the first position the constrained sampler could not
        have emitted (an unmatched ``)``, an EOS with a branch or ring open, a token the column budget excludes).  Other keywords go
        to ``NativeTransformer.proposal_scores``."""
        pad, eos = self._pad_eos()
        if pad != self.model.tgt_pad_token_i:
            raise ValueError("the generator's pad token differs from the model's")
        for name, default in (("temperature", 1.0), ("top_k", 0), ("top_p", 1.0)):
            kw.setdefault(name, getattr(self, name, default))
        if prefix is not None:
            if kw.get("forced_len") is not None:
                raise ValueError("a call takes a prefix or forced_len, not both")
            _, lengths = check_prefix(prefix, int(pred.shape[0]), int(pred.shape[-1]), pad, self.model.tgt_vocab_size)
            kw["forced_len"] = torch.tensor(lengths, dtype=torch.int32)
        bias = combine_bias(logit_bias, allowed, int(pred.shape[0]), self.model.tgt_vocab_size)
        if bias is not None:
            kw["logit_bias"] = bias
        if syntax is not None:
            kw["syntax"] = as_syntax(syntax)
            kw["syntax"].check_prefix(prefix, pad)
            kw.setdefault("syntax_max_len", int(getattr(self, "max_len", 0)) or int(pred.shape[-1]))
        return self.model.proposal_scores(src, pred, eos_token_idx=eos, **kw)

    def fold(self, src: torch.Tensor, pred: torch.Tensor, scores=None, order: str = "score", unfinished: str = "last",
             **kw) -> FoldedHypotheses:
        """The distinct hypotheses among ``pred`` (Long[B, N, L] as ``generate(src)`` returned it), counted and ranked on the
        device: a ``FoldedHypotheses`` whose ``pred`` holds each source's distinct rows best first and all-PAD rows after,
        ``count`` how often each was drawn and ``logmass`` the log of the probability mass they cover (finished hypotheses exclude
        each other; an unfinished row's score is that of its prefix, which overlaps with its continuations).  ``scores`` (Float[B, N] or
        a HypothesisScores of the same rows) default to ``self.score(src, pred)``.  Candidates of several calls or of several
        generators are merged before the call, by ``torch.cat([pred_a, pred_b], dim=1)`` (and the same on their scores): rows
        that two of them share fold into one with the summed count.  Other keywords go to
        ``NativeTransformer.fold_hypotheses``."""
        pad, eos = self._pad_eos()
        if pad != self.model.tgt_pad_token_i:
            raise ValueError("the generator's pad token differs from the model's")
        if scores is None:
            scores = self.score(src, pred)
        return self.model.fold_hypotheses(pred, scores, order=order, unfinished=unfinished, pad=pad, eos=eos, **kw)

    def _scored(self, src: torch.Tensor, pred: torch.Tensor, return_scores: bool, return_logq: bool = False, prefix=None,
                logit_bias=None, syntax=None):
        """``pred``; with ``return_scores`` and / or ``return_logq`` the tuple ``(pred[, HypothesisScores][, ProposalScores])``.
        Both flags: ONE decoder pass (``with_scores=True``), the ProposalScores' ``scores`` being the HypothesisScores."""
        if not return_logq:
            return (pred, self.score(src, pred)) if return_scores else pred
        q = self.logq(src, pred, prefix=prefix, logit_bias=logit_bias, syntax=syntax, with_scores=return_scores)
        return (pred, q.scores, q) if return_scores else (pred, q)

    def _scored_many(self, batches: list, preds: list, return_scores: bool = True, return_logq: bool = False, prefixes=None,
                     biases=None, syntax=None) -> list:
        if return_scores and not return_logq and os.environ.get("TTX_SCORE_LIST", "1") != "0":
            # scores alone: the whole list in length buckets, the per-batch values on the bits (TTX_SCORE_LIST=0: batch by batch)
            return [(p, s) for p, s in zip(preds, self.score_many(batches, preds))]
        pres = prefixes if prefixes is not None else [None] * len(batches)
        bs = biases if biases is not None else [None] * len(batches)
        return [(p,) + (None,) * (int(return_scores) + int(return_logq)) if p is None
                else self._scored(b, p, return_scores, return_logq, q, lb, syntax) for b, p, q, lb in zip(batches, preds, pres, bs)]


def _slot_pool_plan(rows: int, in_flight: int, capacity: int | None) -> tuple:
    """(slots per pool, sessions) of a slot-pool call over ``rows`` decoder rows: 1 024 slots x 3 pools for lists that fill them, else
    512 slots x 5 pools (measured; profiles/r08_sweep_c2_pools.txt, profiles/r03_sweep_c2_pools.txt); a given
    ``capacity`` or TTX_POOL_CAPACITY sets the slots, TTX_POOL_SESSIONS the sessions (experiments).  One rule for the
    greedy pool and the sampling pool."""
    by_default = not (capacity or os.environ.get("TTX_POOL_CAPACITY"))
    cap = int(capacity or os.environ.get("TTX_POOL_CAPACITY") or (1024 if rows >= 3 * 1024 else 512))
    n_pools = 3 if (by_default and cap == 1024) else max(1, 2560 // cap)
    n_sess = max(1, min(in_flight, n_pools, -(-rows // 32)))
    if os.environ.get("TTX_POOL_SESSIONS"):
        n_sess = max(1, int(os.environ["TTX_POOL_SESSIONS"]))
    return cap, n_sess


class TranslationInferenceGreedySpeculative(_ScoresHypotheses):
    """Drop-in for src/decoding/speculative_decoding.py:8-174: copy-drafts, one parallel verify pass per
    step, longest accepted prefix + 1 bonus token — the whole loop runs in ttx_greedy_speculative_generate."""

    def __init__(self, model, max_len: int, draft_len: int, n_drafts: int, pad_token: int, bos_token: int,
                 eos_token: int, replace_token: int) -> None:
        self.model = _need_native(model)
        self.max_len = max_len
        self.pad_token, self.bos_token, self.eos_token = pad_token, bos_token, eos_token
        self.replace_token = replace_token
        self.draft_len = draft_len
        self.n_drafts = n_drafts
        self.accepted_tokens_num = 0   # left at 0 by the reference's greedy-speculative loop as well
        self.model_calls_num = 0
        self.stats_total = {"accepted_tokens": 0, "produced_tokens": 0, "verified_positions": 0,
                            "kv_prefix_positions": 0, "src_positions": 0, "encode_ms": 0.0, "decode_ms": 0.0,
                            "src_tokens_padded": 0, "batches": 0}
        self.last_stats: N.GenStats | None = None
        self.last_failed_batches: list = []    # generate_many(on_error="skip"): batches on which the reference raises
        self.last_batch_counters: list = []    # generate_many: what each batch added to the counter attributes (None: failed)
        self.record_step = 0           # parity tests: k > 0 keeps the logits of verify step k (see step_snapshot)

    def step_snapshot(self) -> dict:
        """The verify step recorded through ``record_step`` during the last ``generate``: numpy arrays
        logits [n_active, rps, V], rows [n_active] (batch row of every slot), front [B], gen [B, gen_ld]."""
        import numpy as np
        m = self.model
        info = (C.c_int32 * 6)()
        N.check(m._lib.ttx_debug_step_snapshot(m.session, info, None, None, None, None))
        n_act, rps, B, gen_ld, V, step = list(info)
        logits = np.empty((n_act, rps, V), dtype=np.float32)
        act = np.empty(n_act, dtype=np.int32)
        front = np.empty(B, dtype=np.int32)
        gen = np.empty((B, gen_ld), dtype=np.int32)
        N.check(m._lib.ttx_debug_step_snapshot(m.session, info, logits.ctypes.data, act.ctypes.data, front.ctypes.data,
                                               gen.ctypes.data))
        return {"logits": logits, "rows": act, "front": front, "gen": gen, "step": step}

    def __str__(self):
        return (f"Greedy speculative decoding (draft_len={self.draft_len}, n_drafts={self.n_drafts}, "
                f"max_len={self.max_len})")

    def generate(self, src: torch.Tensor, return_scores: bool = False, logit_bias=None, allowed=None, syntax=None):
        """``return_scores=True``: ``(pred, HypothesisScores)`` instead of ``pred`` (see ``score``).  ``logit_bias`` / ``allowed``
        are refused (ValueError): the samplers at ``temperature=0`` decode greedily under a bias."""
        _refuse_bias("TranslationInferenceGreedySpeculative", logit_bias, allowed)
        _refuse_syntax("TranslationInferenceGreedySpeculative", syntax)
        m = self.model
        src = src.to(m.device, torch.int64).contiguous()
        m.check_tokens(src)
        B, Ls = src.shape
        out = torch.empty((B, 1, self.max_len), dtype=torch.int64, device=m.device)
        p = N.GenParams(self.max_len, self.draft_len, self.n_drafts, self.pad_token, self.bos_token, self.eos_token,
                        self.replace_token, int(self.record_step))
        st = N.GenStats()
        N.check(m._lib.ttx_greedy_speculative_generate(m.session, src.data_ptr(), B, Ls, C.byref(p), out.data_ptr(),
                                                       C.byref(st), m._stream()))
        self.model_calls_num += int(st.model_calls)
        t = self.stats_total
        for k in ("accepted_tokens", "produced_tokens", "verified_positions", "kv_prefix_positions", "src_positions",
                  "encode_ms", "decode_ms"):
            t[k] += getattr(st, k)
        t["src_tokens_padded"] += B * Ls
        t["batches"] += 1
        self.last_stats = st
        return self._scored(src, out, return_scores)

    def generate_many(self, batches: list, in_flight: int = 4, reorder: bool = False, group_size: int | None = None,
                      on_error: str = "raise", pool: bool | None = None, return_scores: bool = False, logit_biases=None,
                      allowed=None, syntax=None) -> list:
        """Decode several batches with up to `in_flight` of them on the GPU at once (one session + stream each;
        ttx_greedy_speculative_generate_many).  Returns one [B,1,max_len] tensor per batch, each identical to what
        ``generate`` returns for that batch; counters accumulate as if ``generate`` had been called per batch.

        ``reorder=True`` decodes the rows in groups sorted by source length (less padding, rows of similar length
        finish together) through ttx_greedy_speculative_generate_rows and then replays the reference's width rule
        over the batches as passed (scheduling.replay_batch): outputs, ``model_calls_num`` and the error behaviour
        stay those of per-batch ``generate`` calls.

        ``on_error="skip"``: a batch on which the reference raises (a row finishing at a width beyond max_len,
        speculative_decoding.py:158) yields ``None`` in the returned list instead of ending the call; the indices are
        kept in ``self.last_failed_batches``.

        ``return_scores=True``: a list of ``(pred, HypothesisScores)`` pairs; a batch that came back ``None`` has ``None``
        scores.  ``logit_biases`` / ``allowed`` are refused (ValueError), as in ``generate``."""
        _refuse_bias("TranslationInferenceGreedySpeculative.generate_many", logit_biases, allowed)
        _refuse_syntax("TranslationInferenceGreedySpeculative.generate_many", syntax)
        if return_scores:
            return self._scored_many(batches, self.generate_many(batches, in_flight, reorder, group_size, on_error, pool))
        m = self.model
        if on_error not in ("raise", "skip"):
            raise ValueError("on_error must be 'raise' or 'skip'")
        self.last_failed_batches = []
        self.last_batch_counters = [None] * len(batches)
        if not batches:
            return []
        if reorder:
            try:
                if pool is None:
                    pool = True
                return self._generate_reordered(batches, in_flight, group_size, on_error, pool)
            except N.TtxError as e:
                if e.code != N.TTX_ERR_ROW_REPLAY:
                    raise            # otherwise: a PAD inside a sequence; decode the batches as given
        srcs = [b.to(m.device, torch.int64).contiguous() for b in batches]
        for b in srcs:
            m.check_tokens(b)
        outs = [torch.empty((s.shape[0], 1, self.max_len), dtype=torch.int64, device=m.device) for s in srcs]
        n = len(srcs)
        pool = m.session_pool(max(1, min(in_flight, n)))
        sess = (C.c_void_p * len(pool))(*[p.value for p in pool])
        src_p = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
        out_p = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        Bs = (C.c_int * n)(*[s.shape[0] for s in srcs])
        Ls = (C.c_int * n)(*[s.shape[1] for s in srcs])
        p = N.GenParams(self.max_len, self.draft_len, self.n_drafts, self.pad_token, self.bos_token, self.eos_token,
                        self.replace_token, 0)
        stats = (N.GenStats * n)()
        rc = m._lib.ttx_greedy_speculative_generate_many(sess, len(pool), n, src_p, Bs, Ls, C.byref(p), out_p, stats, m._stream())
        if not (rc == N.TTX_ERR_REFERENCE and on_error == "skip"):
            N.check(rc)
        t = self.stats_total
        for i, st in enumerate(stats):
            if st.status != N.TTX_OK:                  # only reachable in skip mode: every batch was decoded, this one raises
                if st.status != N.TTX_ERR_REFERENCE:
                    N.check(int(st.status))
                outs[i] = None
                self.last_failed_batches.append(i)
                continue
            self.model_calls_num += int(st.model_calls)
            self.last_batch_counters[i] = {"model_calls_num": int(st.model_calls)}
            for k in ("accepted_tokens", "produced_tokens", "verified_positions", "kv_prefix_positions", "src_positions",
                      "encode_ms", "decode_ms"):
                t[k] += getattr(st, k)
            t["src_tokens_padded"] += srcs[i].shape[0] * srcs[i].shape[1]
            t["batches"] += 1
        return outs

    def _generate_reordered(self, batches: list, in_flight: int, group_size: int | None, on_error: str = "raise",
                            pool: bool = True) -> list:
        from .scheduling import plan_row_groups, replay_batch
        m = self.model
        L, T = self.max_len, self.max_len + 1
        srcs = [b.to(m.device, torch.int64) for b in batches]
        sizes = [int(s.shape[0]) for s in srcs]
        R = sum(sizes)
        # device group size: the given batch size is not binding any more; larger groups run the GEMMs at better MFMA
        # occupancy, but at least `in_flight` groups should exist so that tails overlap
        if pool:      # slot pool: 1 024 slots x 3 pools for lists that fill them, else 512 slots x 5 pools (measured, DESIGN.md
            # §6); lists that fit the pools at once are split evenly
            gsz, pool_sessions = _slot_pool_plan(R, in_flight, group_size)
        else:
            gsz = int(group_size or min(256, max(max(sizes), -(-R // max(1, in_flight)))))
        self.last_group_size = gsz
        # all rows in one right-padded matrix; a row's length is the position after its last non-PAD token
        Lmax = max(int(s.shape[1]) for s in srcs)
        allsrc = torch.full((R, Lmax), self.pad_token, dtype=torch.int64, device=m.device)
        r0 = 0
        for s in srcs:
            allsrc[r0:r0 + s.shape[0], :s.shape[1]] = s
            r0 += s.shape[0]
        m.check_tokens(allsrc)
        pos = torch.arange(1, Lmax + 1, device=m.device)
        lengths = ((allsrc != self.pad_token) * pos).amax(dim=1)
        order, groups = plan_row_groups(lengths.cpu().numpy(), gsz)
        order_t = torch.from_numpy(order).to(m.device)
        sorted_src = allsrc[order_t]
        sorted_len = lengths[order_t].cpu().numpy()
        out_sorted = torch.empty((R, L), dtype=torch.int64, device=m.device)
        traj_sorted = torch.empty((R, T), dtype=torch.int16, device=m.device)
        fin_sorted = torch.empty((R,), dtype=torch.int32, device=m.device)
        p = N.GenParams(L, self.draft_len, self.n_drafts, self.pad_token, self.bos_token, self.eos_token, self.replace_token, 0)
        if pool:
            # continuous batching: every session keeps `gsz` slots filled from the sorted work list
            # (ttx_greedy_speculative_generate_pool)
            # the default of a list that fills them is three pools of 1 024 slots since the verify step runs in two phases
            # (profiles/r08_sweep_c2_pools.txt); every other case keeps the rule it had (five pools of 512:
            # profiles/r03_sweep_c2_pools.txt)
            sessions = m.session_pool(pool_sessions)
            sess = (C.c_void_p * len(sessions))(*[q.value for q in sessions])
            width = max(2, int(sorted_len.max()))
            src_mat = sorted_src[:, :width].contiguous() if width <= sorted_src.shape[1] else torch.nn.functional.pad(
                sorted_src, (0, width - sorted_src.shape[1]), value=self.pad_token).contiguous()
            h_len = (C.c_int32 * R)(*[int(x) for x in sorted_len])
            one = N.GenStats()
            N.check(m._lib.ttx_greedy_speculative_generate_pool(sess, len(sessions), src_mat.data_ptr(), R, width, h_len, gsz,
                                                                C.byref(p), out_sorted.data_ptr(), traj_sorted.data_ptr(),
                                                                fin_sorted.data_ptr(), C.byref(one), m._stream()))
            stats, gsrc = [one], [src_mat]
        else:
            gsrc = [sorted_src[g, :max(2, int(sorted_len[g].max()))].contiguous() for g in groups]
            n = len(gsrc)
            sessions = m.session_pool(max(1, min(in_flight, n)))
            sess = (C.c_void_p * len(sessions))(*[q.value for q in sessions])
            src_p = (C.c_void_p * n)(*[s.data_ptr() for s in gsrc])
            out_p = (C.c_void_p * n)(*[out_sorted[g].data_ptr() for g in groups])
            traj_p = (C.c_void_p * n)(*[traj_sorted[g].data_ptr() for g in groups])
            fin_p = (C.c_void_p * n)(*[fin_sorted[g].data_ptr() for g in groups])
            Bs = (C.c_int * n)(*[s.shape[0] for s in gsrc])
            Ls = (C.c_int * n)(*[s.shape[1] for s in gsrc])
            stats = (N.GenStats * n)()
            N.check(m._lib.ttx_greedy_speculative_generate_rows(sess, len(sessions), n, src_p, Bs, Ls, C.byref(p), out_p, traj_p, fin_p,
                                                                stats, m._stream()))
        # back to the caller's row order, then the reference's per-batch loop over the traces
        inv = torch.empty_like(order_t)
        inv[order_t] = torch.arange(R, device=m.device)
        out_rows = out_sorted[inv]
        traj = traj_sorted[inv].cpu().numpy()
        fin = fin_sorted[inv].cpu().numpy()
        keep = torch.zeros(R, dtype=torch.bool)
        t = self.stats_total
        failed = None
        r0 = 0
        for bi, B in enumerate(sizes):
            rep = replay_batch(traj[r0:r0 + B], fin[r0:r0 + B], L, self.draft_len, self.n_drafts)
            if rep.error:
                if on_error == "skip":
                    self.last_failed_batches.append(bi)
                    r0 += B
                    continue
                failed = bi
                break
            keep[r0:r0 + B] = torch.from_numpy(rep.finished)
            self.model_calls_num += rep.model_calls
            self.last_batch_counters[bi] = {"model_calls_num": rep.model_calls}
            t["accepted_tokens"] += rep.accepted_tokens
            t["produced_tokens"] += rep.produced_tokens
            t["verified_positions"] += rep.verified_positions
            t["kv_prefix_positions"] += rep.kv_prefix_positions
            t["src_positions"] += rep.rows_iterations * int(srcs[bi].shape[1])
            t["src_tokens_padded"] += B * int(srcs[bi].shape[1])
            t["batches"] += 1
            r0 += B
        for st in stats:
            t["encode_ms"] += st.encode_ms
            t["decode_ms"] += st.decode_ms
        # what the device actually executed (row groups), beside the reference-equivalent per-batch counters above
        dv = t.setdefault("device", {"model_calls": 0, "accepted_tokens": 0, "produced_tokens": 0, "verified_positions": 0,
                                     "kv_prefix_positions": 0, "src_positions": 0, "src_tokens_padded": 0, "batches": 0})
        for st, gs in zip(stats, gsrc):
            for k in ("model_calls", "accepted_tokens", "produced_tokens", "verified_positions", "kv_prefix_positions",
                      "src_positions"):
                dv[k] += int(getattr(st, k))
            dv["src_tokens_padded"] += int(st.src_tokens_padded) if pool else int(gs.numel())
            dv["batches"] += 1
        t["device_model_calls"] = dv["model_calls"]
        if failed is not None:
            raise N.ReferenceError_(f"batch {failed}: a row finished at a width beyond max_len: shape mismatch in the reference "
                                    "(speculative_decoding.py:158)")
        out_rows = torch.where(keep.to(m.device)[:, None], out_rows, torch.full_like(out_rows, self.pad_token))
        outs, r0 = [], 0
        skipped = set(self.last_failed_batches)
        for bi, B in enumerate(sizes):
            outs.append(None if bi in skipped else out_rows[r0:r0 + B].unsqueeze(1).contiguous())
            r0 += B
        return outs


class TranslationInferenceGreedy(_ScoresHypotheses):
    """Drop-in for src/decoding/standard_decoding.py:4-55; the loop runs in ttx_greedy_generate (KV cache)."""

    def __init__(self, model, max_len: int, pad_token: int, bos_token: int, eos_token: int) -> None:
        self.model = _need_native(model)
        self.max_len = max_len
        self.pad_token, self.bos_token, self.eos_token = pad_token, bos_token, eos_token
        self.model_calls_num = 0
        self.given_tokens = 0

    def __str__(self):
        return f"Greedy decoding (max_len={self.max_len})"

    def generate(self, src: torch.Tensor, return_scores: bool = False, logit_bias=None, allowed=None, syntax=None):
        """``return_scores=True``: ``(pred, HypothesisScores)`` instead of ``pred`` (see ``score``).  ``logit_bias`` / ``allowed``
        are refused (ValueError): ``TranslationInferenceSampling`` at ``temperature=0`` is this loop under a bias."""
        _refuse_bias("TranslationInferenceGreedy", logit_bias, allowed)
        _refuse_syntax("TranslationInferenceGreedy", syntax)
        m = self.model
        src = src.to(m.device, torch.int64).contiguous()
        m.check_tokens(src)
        B, Ls = src.shape
        out = torch.empty((B, 1, self.max_len), dtype=torch.int64, device=m.device)
        p = N.GenParams(self.max_len, 0, 1, self.pad_token, self.bos_token, self.eos_token, self.pad_token, 0)
        st = N.GenStats()
        N.check(m._lib.ttx_greedy_generate(m.session, src.data_ptr(), B, Ls, C.byref(p), out.data_ptr(), C.byref(st),
                                           m._stream()))
        self.model_calls_num += int(st.model_calls)
        self.given_tokens += int((src != m.src_pad_token_i).sum())
        return self._scored(src, out, return_scores)


def check_prefix(prefix, B: int, max_len: int, pad_token: int, vocab_size: int):
    """The forced target prefixes of a sampling call: ``prefix`` Long[B, Lp] without BOS, right-padded with PAD, a row's
    length the number of tokens before its first PAD.  Returns ``(Long[B, Lp] on the CPU, [length per source])``, or
    ``(None, None)`` for ``prefix=None``.  ValueError: a shape that is not [B, Lp], a non-PAD token after a PAD, an id
    outside the vocabulary, a length above ``max_len - 1``.  Needs no device."""
    if prefix is None:
        return None, None
    p = torch.as_tensor(prefix)
    if p.dim() != 2 or p.dtype.is_floating_point or p.dtype == torch.bool:
        raise ValueError(f"prefix must be an integer tensor [B, Lp], got {tuple(p.shape)} {p.dtype}")
    if p.shape[0] != B:
        raise ValueError(f"prefix must hold one row per source ({B}), got {p.shape[0]}")
    p = p.detach().to("cpu", torch.int64).contiguous()
    is_pad = p == pad_token
    lengths = (~is_pad).to(torch.int64).cumprod(dim=1).sum(dim=1)            # tokens before the first PAD
    if bool(((~is_pad).sum(dim=1) != lengths).any()):
        raise ValueError("prefix holds a non-PAD token after a PAD: prefixes are right-padded")
    if p.numel() and (int(p.min()) < 0 or int(p.max()) >= vocab_size):
        raise ValueError(f"prefix holds an id outside the vocabulary [0, {vocab_size})")
    if p.shape[0] and int(lengths.max()) > max_len - 1:
        raise ValueError(f"a prefix of {int(lengths.max())} tokens does not fit max_len - 1 = {max_len - 1}")
    return p, [int(x) for x in lengths]


class TranslationInferenceSampling(_ScoresHypotheses):
    """Seeded ancestral sampling: ``num_samples`` draws per source from the model's distribution under ``temperature``,
    ``top_k`` and ``top_p``.  The whole loop runs in ttx_sample_generate: the greedy loop (KV cache, one graph per step) with
    k_sample choosing each token, the encoder once per source.  The reference has the seam for it
    (TranslationInferenceGreedy.sample, src/decoding/standard_decoding.py:27-28) and no sampler of its own.

    ``temperature=0`` is greedy.  ``top_k`` is 0 (off) or 1..32; ``top_p`` is in (0, 1] (1: off); a ``top_p < 1`` with
    ``top_k=0`` runs with ``top_k=32``, so a filtered kept set never holds more than 32 tokens.  Vocabularies up to 1 024.
    Sample ``j`` of a source depends on (seed, the source's row key, j, position) and on the source alone: not on the batch
    size, ``num_samples`` or the other rows of the batch.  A sampled PAD ends a row as EOS does."""

    def __init__(self, model, max_len: int, pad_token: int, bos_token: int, eos_token: int, temperature: float = 1.0,
                 top_k: int = 0, top_p: float = 1.0, num_samples: int = 1, seed: int = 0) -> None:
        self.model = _need_native(model)
        self.max_len = max_len
        self.pad_token, self.bos_token, self.eos_token = pad_token, bos_token, eos_token
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        self.num_samples, self.seed = int(num_samples), int(seed)
        self.model_calls_num = 0
        self.given_tokens = 0
        self.last_stats: N.GenStats | None = None

    def __str__(self):
        return (f"Sampling (temperature={self.temperature}, top_k={self.top_k}, top_p={self.top_p}, "
                f"num_samples={self.num_samples}, seed={self.seed}, max_len={self.max_len})")

    def _prefix_args(self, prefix, B: int):
        """``(device tensor or None, its pointer, its row length, host lengths)`` of a call's ``prefix`` (``check_prefix``)."""
        m = self.model
        p, lengths = check_prefix(prefix, B, self.max_len, self.pad_token, m.tgt_vocab_size)
        if p is None:
            return None, None, 0, None
        d = p.to(m.device)
        return d, (d.data_ptr() if d.numel() else None), int(d.shape[1]), (C.c_int32 * max(B, 1))(*lengths)

    def _bias_arg(self, logit_bias, allowed, B: int):
        """The call's ``logit_bias`` / ``allowed`` as one contiguous float32 device tensor [B, V], or None for neither."""
        m = self.model
        bias = combine_bias(logit_bias, allowed, B, m.tgt_vocab_size)
        return None if bias is None else bias.to(m.device).contiguous()

    def _syntax_arg(self, syntax, prefix=None):
        """``(SmilesSyntax, device table, byref(ttx_syntax))`` of a call's ``syntax`` after its checks, or three ``None``."""
        syn = as_syntax(syntax)
        if syn is None:
            return None, None, None
        m = self.model
        d_cls = syn.table(m.tgt_vocab_size, m.device)
        for q in (prefix if isinstance(prefix, (list, tuple)) else [prefix]):
            syn.check_prefix(q, self.pad_token)
        return syn, d_cls, N.Syntax.arg(d_cls, self.max_len)

    def generate(self, src: torch.Tensor, row_keys=None, return_scores: bool = False, prefix=None, return_logq: bool = False,
                 logit_bias=None, allowed=None, syntax=None):
        """Long[B, num_samples, max_len].  ``row_keys``: one integer per source (default 0..B-1), the source's identity for
        the random stream: the same (source, key) gives the same samples in any batch.  ``return_scores=True``:
        ``(pred, HypothesisScores)`` instead of ``pred`` (see ``score``).  ``return_logq=True``: ``(pred, ProposalScores)``, the
        rows' log-probability under the distribution they were drawn from (see ``logq``; what ``logq(src, pred, prefix=prefix)``
        returns); both flags: ``(pred, HypothesisScores, ProposalScores)`` from one decoder pass.

        ``prefix``: Long[B, Lp] without BOS, right-padded with PAD: the forced beginning of every sample of a source.  A
        row is BOS, its prefix, the sampled completion, PAD; a position inside the prefix holds the prefix token whatever the
        logits say and consumes no random number, so the completion's draws are those of its positions.  A forced EOS ends
        the row.  One decoder step per forced token.  An empty prefix (zero width, all PAD, ``None``) is the unprompted call.

        ``logit_bias``: Float[B, V], one row per source, added to the logits of every row of that source at every position before
        temperature and filter (one rounded fp32 add; an entry that is exactly zero leaves the logit's bits alone; ``-inf`` forbids
        the token; ``NaN`` and ``+inf`` are refused: ``scoring.check_logit_bias``).  ``allowed``: Bool[B, V], sugar for a bias of
        0 / ``-inf`` (``scoring.allowlist_from_source`` builds the "tokens of the source" list); both together: the allow-list is
        added onto the bias.  A forced prefix position ignores the bias.  A row depends on its source, key, sample id, prefix and
        its source's bias row alone.  ``temperature=0`` is constrained greedy decoding.  ``return_logq=True`` scores under the
        call's bias.  ``None`` for both is the call without the keywords, launch for launch.

        ``syntax``: a ``SmilesSyntax`` (or its raw int8 table [V]): the row can only hold tokens after which it can still end
        balanced inside ``max_len``: every OPEN closed, every ring label used an even number of times, EOS at the end (the rule:
        include/ttx.h; k_syntax_mask writes ``-inf`` over the other tokens after the bias and before temperature and filter, an
        allowed logit keeps its bits).  Unprompted, every row ends in EOS at or before the last column, balanced and without a
        FORBID token.  A necessary condition for a parseable SMILES string, not validity.  A forced prefix position ignores the
        mask, yet its tokens count in the state; a prefix whose running depth goes negative is refused (ValueError), one that
        already needs more columns than remain is accepted: closers only, and the row may end unfinished.  With a bias the allowed
        set is the intersection.  ``temperature=0`` is greedy decoding over the allowed set.  ``return_logq=True`` scores under
        the call's table.  ``None`` is the call without the keyword, launch for launch."""
        m, n = self.model, self.num_samples
        src = src.to(m.device, torch.int64).contiguous()
        m.check_tokens(src)
        B, Ls = src.shape
        # d_prefix is bound only to keep the device tensor alive until the call returns: prefix_ptr points into it
        d_prefix, prefix_ptr, ld_prefix, h_plen = self._prefix_args(prefix, B)
        bias = self._bias_arg(logit_bias, allowed, B)
        syn, d_cls, syn_arg = self._syntax_arg(syntax, prefix)      # d_cls keeps the device table alive until the call returns
        keys = None
        if row_keys is not None:
            keys = torch.as_tensor(row_keys, dtype=torch.int64).to(m.device).contiguous()
            if keys.shape != (B,):
                raise ValueError(f"row_keys must hold one key per source ({B}), got shape {tuple(keys.shape)}")
        p = N.SampleParams(self.max_len, n, self.temperature, self.top_k, self.top_p, self.pad_token, self.bos_token,
                           self.eos_token, self.seed & 0xFFFFFFFFFFFFFFFF)
        out = torch.empty((B, max(n, 1), max(self.max_len, 1)), dtype=torch.int64, device=m.device)
        st = N.GenStats()
        opts = N.SampleOpts.of(prefix_ptr, ld_prefix, h_plen, bias=bias)        # the general form: zeroed fields and a NULL syntax
        N.check(m._lib.ttx_sample_generate_syntax(m.session, src.data_ptr(), B, Ls, None if keys is None else keys.data_ptr(),
                                                  C.byref(p), C.byref(opts), syn_arg, out.data_ptr(), C.byref(st), m._stream()))
        self.model_calls_num += int(st.model_calls)
        self.given_tokens += int((src != m.src_pad_token_i).sum())
        self.last_stats = st
        return self._scored(src, out, return_scores, return_logq, prefix, bias, syn)


class TranslationInferenceSamplingSpeculative(TranslationInferenceSampling):
    """``TranslationInferenceSampling``'s samples from the greedy-speculative loop: copy drafts of the source are verified
    ``1 + n_drafts * draft_len`` positions per decoder pass, and a draft token is accepted iff it is the token the plain sampler
    emits at its position (the sampler is counter-based, so that token is defined for every row of a verify step).  The
    committed rows are therefore the plain sampler's, under the same seeding contract: sample ``j`` of a source depends on
    (seed, the source's row key, j, position) and on the source alone.  The whole loop runs in
    ttx_sample_speculative_generate.  A row can differ from the plain sampler's only where its uniform falls within fp32
    rounding of a CDF boundary (the two loops form a position's logits in passes over different row counts)."""

    def __init__(self, model, max_len: int, draft_len: int, n_drafts: int, pad_token: int, bos_token: int, eos_token: int,
                 replace_token: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, num_samples: int = 1,
                 seed: int = 0) -> None:
        super().__init__(model, max_len, pad_token, bos_token, eos_token, temperature, top_k, top_p, num_samples, seed)
        self.draft_len, self.n_drafts, self.replace_token = int(draft_len), int(n_drafts), int(replace_token)
        self.accepted_tokens_num = 0
        self.stats_total = {"accepted_tokens": 0, "produced_tokens": 0, "verified_positions": 0, "kv_prefix_positions": 0,
                            "src_positions": 0, "encode_ms": 0.0, "decode_ms": 0.0, "src_tokens_padded": 0, "batches": 0}
        self.last_stats: N.GenStats | None = None

    def __str__(self):
        return (f"Speculative sampling (draft_len={self.draft_len}, n_drafts={self.n_drafts}, temperature={self.temperature}, "
                f"top_k={self.top_k}, top_p={self.top_p}, num_samples={self.num_samples}, seed={self.seed}, max_len={self.max_len})")

    def generate(self, src: torch.Tensor, row_keys=None, return_scores: bool = False, prefix=None, proposal=None,
                 return_logq: bool = False, logit_bias=None, allowed=None, syntax=None):
        """Long[B, num_samples, max_len]; ``row_keys``, ``return_scores``, ``return_logq``, ``prefix``, ``logit_bias``,
        ``allowed`` and ``syntax`` as for ``TranslationInferenceSampling.generate`` (the rows under a bias or a syntax constraint
        are the plain sampler's under the same; a draft, prefix-as-draft or proposal token the constrained sampler cannot emit is
        never accepted: the draw of a draft position comes from the row masked for the prefix that includes the earlier draft
        tokens).  A prefix rides in as the first draft of its rows, which is certain to be
        accepted: ``P`` forced tokens take ``ceil(P / (draft_len + 1))`` verify steps.

        ``proposal``: Long[B, Lq] without BOS, right-padded with PAD, may end in EOS: a draft the caller brings for every sample
        of a source (a cheaper model's output, an earlier prediction, the source's own greedy answer).  It is offered, never
        forced: a draft token is accepted iff it is the token of its position, so the returned rows are those of the call
        without ``proposal`` whatever the proposal holds (under the class's one caveat: a uniform within fp32 rounding of a CDF
        boundary); only the number of decoder passes changes.  Before every
        verify step the proposal is aligned with the row so far (up to 32 tokens to the left, 31 to the right, by the last few
        tokens) and replaces the first draft from there on, so a row finds its place again after a substitution, an insertion
        or a deletion.  A proposal equal to the row takes ``ceil(L / (draft_len + 1))`` passes for ``L`` emitted tokens.
        ``temperature=0`` is the greedy use: the tokens are the greedy-speculative generator's and the proposal is a draft for
        them.  An empty proposal (zero width, all PAD, ``None``) is the call without one.  ``prefix`` together with
        ``proposal`` raises ValueError."""
        if prefix is not None and proposal is not None:
            raise ValueError("a call takes a forced prefix or a proposal, not both")
        m, n = self.model, self.num_samples
        src = src.to(m.device, torch.int64).contiguous()
        m.check_tokens(src)
        B, Ls = src.shape
        # d_prefix is bound only to keep the device tensor alive until the call returns: prefix_ptr points into it
        d_prefix, prefix_ptr, ld_prefix, h_plen = self._prefix_args(prefix, B)
        d_prop, prop_ptr, ld_prop, h_qlen = self._prefix_args(proposal, B)          # the same checks and limits
        bias = self._bias_arg(logit_bias, allowed, B)
        syn, d_cls, syn_arg = self._syntax_arg(syntax, prefix)      # d_cls keeps the device table alive until the call returns
        keys = None
        if row_keys is not None:
            keys = torch.as_tensor(row_keys, dtype=torch.int64).to(m.device).contiguous()
            if keys.shape != (B,):
                raise ValueError(f"row_keys must hold one key per source ({B}), got shape {tuple(keys.shape)}")
        p = N.SampleSpecParams(N.SampleParams(self.max_len, n, self.temperature, self.top_k, self.top_p, self.pad_token,
                                              self.bos_token, self.eos_token, self.seed & 0xFFFFFFFFFFFFFFFF),
                               self.draft_len, self.n_drafts, self.replace_token, 0)
        out = torch.empty((B, max(n, 1), max(self.max_len, 1)), dtype=torch.int64, device=m.device)
        st = N.GenStats()
        opts = N.SampleOpts.of(prefix_ptr, ld_prefix, h_plen, prop_ptr, ld_prop, h_qlen, bias)
        N.check(m._lib.ttx_sample_speculative_generate_syntax(m.session, src.data_ptr(), B, Ls, None if keys is None else keys.data_ptr(),
                                                              C.byref(p), C.byref(opts), syn_arg, out.data_ptr(), C.byref(st), m._stream()))
        self.model_calls_num += int(st.model_calls)
        self.accepted_tokens_num += int(st.accepted_tokens)
        self.given_tokens += int((src != m.src_pad_token_i).sum())
        t = self.stats_total
        for k in ("accepted_tokens", "produced_tokens", "verified_positions", "kv_prefix_positions", "src_positions", "encode_ms",
                  "decode_ms"):
            t[k] += getattr(st, k)
        t["src_tokens_padded"] += B * Ls
        t["batches"] += 1
        self.last_stats = st
        return self._scored(src, out, return_scores, return_logq, prefix, bias, syn)

    def generate_many(self, batches: list, row_keys=None, in_flight: int = 4, capacity: int | None = None,
                      return_scores: bool = False, prefixes=None, proposals=None, return_logq: bool = False,
                      logit_biases=None, allowed=None, syntax=None) -> list:
        """The samples of all batches from slot pools (ttx_sample_speculative_generate_pool: continuous batching over the sources
        of the whole list, sorted by length; the ``num_samples`` rows of a source are admitted together).  Returns one
        Long[B_i, num_samples, max_len] per batch.

        ``row_keys``: one sequence of integers per batch; by default the running index over the concatenated batches, so that
        ``generate_many(batches)[i]`` holds the rows of ``generate(batches[i], row_keys=arange(off_i, off_i + B_i))``.  A row does
        not depend on its slot, on the capacity or on what shares the pool.  ``capacity`` (slots, i.e. decoder rows, per pool;
        ``TTX_POOL_CAPACITY``) and the pool count follow the greedy generator's rule over the ``S * num_samples`` decoder rows and
        are never below ``num_samples``.  ``model_calls_num`` counts the verify steps the device executed.
        ``return_scores=True``: a list of ``(pred, HypothesisScores)`` pairs; ``return_logq=True``: of ``(pred, ProposalScores)``
        pairs (what ``logq(batches[i], pred_i, prefix=prefixes[i])`` returns); both: of triples, one decoder pass per batch.
        ``prefixes``: a list aligned with ``batches``, each entry a ``prefix`` tensor for that batch (see ``generate``) or
        ``None``; ``generate_many(batches, prefixes=ps)[i]`` holds the rows of ``generate(batches[i], prefix=ps[i],
        row_keys=arange(off_i, off_i + B_i))``.
        ``proposals``: the same for ``generate``'s ``proposal``: offered drafts, which change no row.  A call takes ``prefixes``
        or ``proposals``, not both (ValueError).
        ``logit_biases`` and ``allowed``: lists aligned with ``batches``, each entry a ``logit_bias`` / ``allowed`` tensor for that
        batch (see ``generate``) or ``None``: ``generate_many(batches, logit_biases=bs)[i]`` holds the rows of
        ``generate(batches[i], logit_bias=bs[i], row_keys=arange(off_i, off_i + B_i))``.  Every pool holds the call's table
        [S, V]; a slot gets its source's row at admission and a reused slot carries nothing over.  ``return_logq=True`` scores
        each batch under its own bias.
        ``syntax``: ONE ``SmilesSyntax`` for the whole call (see ``generate``): every row of every batch is generated under it,
        and ``generate_many(batches, syntax=t)[i]`` holds the rows of ``generate(batches[i], syntax=t, row_keys=...)``.  The
        state is recomputed from the slot's row, so a reused slot carries nothing over."""
        for name, tabs in (("logit_biases", logit_biases), ("allowed", allowed)):
            if tabs is not None and len(tabs) != len(batches):
                raise ValueError(f"{name} must hold one entry per batch ({len(batches)}), got {len(tabs)}")
        biases = None
        if logit_biases is not None or allowed is not None:
            V = self.model.tgt_vocab_size
            lbs = logit_biases if logit_biases is not None else [None] * len(batches)
            als = allowed if allowed is not None else [None] * len(batches)
            biases = [combine_bias(lb, al, int(b.shape[0]), V) for lb, al, b in zip(lbs, als, batches)]
            if all(b is None for b in biases):
                biases = None
        if return_scores or return_logq:
            return self._scored_many(batches, self.generate_many(batches, row_keys, in_flight, capacity, prefixes=prefixes,
                                                                 proposals=proposals, logit_biases=biases, syntax=syntax),
                                     return_scores, return_logq, prefixes, biases, as_syntax(syntax))
        from .scheduling import plan_row_groups
        if prefixes is not None and proposals is not None:
            raise ValueError("a call takes forced prefixes or proposals, not both")
        for name, tabs in (("prefixes", prefixes), ("proposals", proposals)):
            if tabs is not None and len(tabs) != len(batches):
                raise ValueError(f"{name} must hold one entry per batch ({len(batches)}), got {len(tabs)}")
        if not batches:
            return []
        m, n, L = self.model, self.num_samples, self.max_len
        syn, d_cls, syn_arg = self._syntax_arg(syntax, prefixes)    # d_cls keeps the device table alive until the call returns
        sizes = [int(b.shape[0]) for b in batches]
        S = sum(sizes)

        def stacked(tabs):
            """Every source's prefix (proposal) in one right-padded matrix beside the sources and the lengths, or (None, None)
            when no batch carries a non-empty one: the plain call, with nothing to sort or upload."""
            if tabs is None or all(q is None for q in tabs):
                return None, None
            checked = [check_prefix(q, B, L, self.pad_token, m.tgt_vocab_size) for q, B in zip(tabs, sizes)]
            Lp = max([int(c[0].shape[1]) for c in checked if c[0] is not None] or [0])
            mat = torch.full((S, Lp), self.pad_token, dtype=torch.int64)
            lens_all = torch.zeros(S, dtype=torch.int64)
            r0 = 0
            for (q, lens), B in zip(checked, sizes):
                if q is not None:
                    mat[r0:r0 + B, :q.shape[1]] = q
                    lens_all[r0:r0 + B] = torch.tensor(lens, dtype=torch.int64)
                r0 += B
            return (mat, lens_all) if bool(lens_all.any()) else (None, None)

        allpre, plen = stacked(prefixes)
        allprop, qlen = stacked(proposals)
        allbias = None                  # every source's bias row, zeros (no bias) for the batches that carry none
        if biases is not None:
            allbias = torch.cat([torch.zeros((B, V), dtype=torch.float32, device=m.device) if b is None else b.to(m.device)
                                 for b, B in zip(biases, sizes)])
        srcs = [b.to(m.device, torch.int64) for b in batches]
        if row_keys is None:
            keys = torch.arange(S, dtype=torch.int64)
        else:
            if len(row_keys) != len(srcs):
                raise ValueError(f"row_keys must hold one sequence per batch ({len(srcs)}), got {len(row_keys)}")
            per = [torch.as_tensor(k, dtype=torch.int64).reshape(-1).cpu() for k in row_keys]
            for i, (k, B) in enumerate(zip(per, sizes)):
                if k.shape != (B,):
                    raise ValueError(f"row_keys[{i}] must hold one key per source ({B}), got shape {tuple(k.shape)}")
            keys = torch.cat(per) if per else torch.zeros(0, dtype=torch.int64)
        p = N.SampleSpecParams(N.SampleParams(L, n, self.temperature, self.top_k, self.top_p, self.pad_token, self.bos_token,
                                              self.eos_token, self.seed & 0xFFFFFFFFFFFFFFFF),
                               self.draft_len, self.n_drafts, self.replace_token, 0)
        R = S * max(n, 1)
        cap, n_sess = _slot_pool_plan(R, in_flight, capacity)
        cap = max(cap, n)
        self.last_group_size, self.last_pool_sessions = cap, n_sess
        # all sources in one right-padded matrix, sorted by length (longest first) with their keys
        Lmax = max([int(s.shape[1]) for s in srcs if s.shape[0]] or [2])
        allsrc = torch.full((S, Lmax), self.pad_token, dtype=torch.int64, device=m.device)
        r0 = 0
        for s in srcs:
            allsrc[r0:r0 + s.shape[0], :s.shape[1]] = s
            r0 += s.shape[0]
        m.check_tokens(allsrc)
        out_sorted = torch.empty((S, max(n, 1), max(L, 1)), dtype=torch.int64, device=m.device)
        st = N.GenStats()
        if S:
            pos = torch.arange(1, Lmax + 1, device=m.device)
            lengths = ((allsrc != self.pad_token) * pos).amax(dim=1)
            order, _ = plan_row_groups(lengths.cpu().numpy(), cap)
            order_t = torch.from_numpy(order).to(m.device)
            sorted_len = lengths[order_t].cpu().numpy()
            width = max(2, int(sorted_len.max()))
            sorted_src = allsrc[order_t]
            src_mat = sorted_src[:, :width].contiguous() if width <= Lmax else torch.nn.functional.pad(
                sorted_src, (0, width - Lmax), value=self.pad_token).contiguous()
            keys_sorted = keys.to(m.device)[order_t].contiguous()
            h_len = (C.c_int32 * S)(*[int(x) for x in sorted_len])
            sessions = m.session_pool(n_sess)
            sess = (C.c_void_p * len(sessions))(*[q.value for q in sessions])
            order_cpu = torch.from_numpy(order).to(torch.int64)

            def table_args(mat, lens_all):
                """``(sorted device matrix kept alive, its pointer, its row length, host lengths)`` in the pool's order."""
                if mat is None:
                    return None, None, 0, None
                d = mat[order_cpu].contiguous().to(m.device)
                return d, (d.data_ptr() if d.numel() else None), int(d.shape[1]), (C.c_int32 * S)(*[int(x) for x in lens_all[order_cpu]])

            pre_sorted, pre_ptr, ld_prefix, h_plen = table_args(allpre, plen)
            prop_sorted, prop_ptr, ld_prop, h_qlen = table_args(allprop, qlen)
            bias_sorted = None if allbias is None else allbias[order_t].contiguous()      # kept alive until the call returns
            opts = N.SampleOpts.of(pre_ptr, ld_prefix, h_plen, prop_ptr, ld_prop, h_qlen, bias_sorted)
            N.check(m._lib.ttx_sample_speculative_generate_pool_syntax(sess, len(sessions), src_mat.data_ptr(), S, width, h_len,
                                                                       keys_sorted.data_ptr(), cap, C.byref(p), C.byref(opts), syn_arg,
                                                                       out_sorted.data_ptr(), C.byref(st), m._stream()))
            inv = torch.empty_like(order_t)
            inv[order_t] = torch.arange(S, device=m.device)
            out_rows = out_sorted[inv]
            self.given_tokens += int((allsrc != m.src_pad_token_i).sum())
        else:
            out_rows = out_sorted
        self.model_calls_num += int(st.model_calls)
        self.accepted_tokens_num += int(st.accepted_tokens)
        t = self.stats_total
        for k in ("accepted_tokens", "produced_tokens", "verified_positions", "kv_prefix_positions", "src_positions", "encode_ms",
                  "decode_ms", "src_tokens_padded"):
            t[k] += getattr(st, k)
        t["batches"] += len(srcs)
        t["pool_calls"] = t.get("pool_calls", 0) + 1
        self.last_stats = st
        outs, r0 = [], 0
        for B in sizes:
            outs.append(out_rows[r0:r0 + B].contiguous())
            r0 += B
        return outs


class TranslationInferenceBeamSearch(_ScoresHypotheses):
    """Drop-in for src/decoding/standard_decoding.py:58-174:the whole loop runs in ttx_beam_generate (per-hypothesis KV
    cache, encoder and cross K/V once per source, log-softmax + top-beam + row assembly in one kernel per step)."""

    def __init__(self, model, beam_size: int, max_len: int, pad_token: int, bos_token: int, eos_token: int):
        assert max_len > 1
        assert beam_size > 0
        self.model = _need_native(model)
        self.beam_size, self.max_len = beam_size, max_len
        self.pad_token, self.bos_token, self.eos_token = pad_token, bos_token, eos_token
        self.model_calls_num = 0
        self.given_tokens = 0
        self.b_sz = 0

    def __str__(self):
        return f"Beam search decoding (beam_size={self.beam_size}, max_len={self.max_len})"

    def generate(self, src: torch.Tensor, return_scores: bool = False, logit_bias=None, allowed=None, syntax=None):
        """``return_scores=True``: ``(pred, HypothesisScores)`` instead of ``pred`` (see ``score``).  ``logit_bias`` / ``allowed``
        are refused (ValueError)."""
        _refuse_bias("TranslationInferenceBeamSearch", logit_bias, allowed)
        _refuse_syntax("TranslationInferenceBeamSearch", syntax)
        m, K = self.model, self.beam_size
        src = src.to(m.device, torch.int64).contiguous()
        m.check_tokens(src)
        B, Ls = src.shape
        out = torch.empty((B, K, self.max_len), dtype=torch.int64, device=m.device)
        p = N.BeamSearchParams(self.max_len, K, self.pad_token, self.bos_token, self.eos_token)
        st = N.BeamSearchStats()
        N.check(m._lib.ttx_beam_generate(m.session, src.data_ptr(), B, Ls, C.byref(p), out.data_ptr(), C.byref(st), m._stream()))
        self.model_calls_num += int(st.model_calls)
        self.b_sz += int(st.running_rows)
        self.given_tokens += int((src != m.src_pad_token_i).sum())
        return self._scored(src, out[:, :, :int(st.out_width)].contiguous(), return_scores)


class ConstrainedBeamDetails(NamedTuple):
    """What constrained beam search knows about its rows: ``logp`` Float[B, K] the cumulative log-probability of each hypothesis
    under the constrained, renormalised distribution (a forced prefix position costs nothing; ``-inf`` for a dead row),
    ``finished`` Bool[B, K] the loop's flag (the row holds EOS, or it is dead) and ``alive`` Bool[B, K] (``logp`` is finite)."""
    logp: torch.Tensor
    finished: torch.Tensor
    alive: torch.Tensor


class TranslationInferenceBeamSearchConstrained(_ScoresHypotheses):
    """``TranslationInferenceBeamSearch`` under a per-source logit bias or allow-list, a syntax constraint and forced target
    prefixes: "the K best answers that use only the reactants' tokens", "the K best balanced strings", "the K best completions
    of this scaffold" as one call.  The whole loop runs in ttx_beam_generate_constrained: the standard beam loop with
    k_logit_bias and k_syntax_mask on every level's logits and k_beam_step_masked where that loop launches k_beam_step
    (include/ttx.h states the rule).  A forbidden or masked token is a -inf logit, the scores are log-probabilities under the
    constrained, renormalised distribution, and a source with fewer than K possible rows returns the missing ranks as DEAD rows
    (BOS then PAD, ``logp = -inf``), last.  Without a keyword ``generate`` is ``TranslationInferenceBeamSearch.generate``, launch
    for launch."""

    def __init__(self, model, beam_size: int, max_len: int, pad_token: int, bos_token: int, eos_token: int):
        assert max_len > 1
        assert beam_size > 0
        self.model = _need_native(model)
        self.beam_size, self.max_len = beam_size, max_len
        self.pad_token, self.bos_token, self.eos_token = pad_token, bos_token, eos_token
        self.model_calls_num = 0
        self.given_tokens = 0
        self.b_sz = 0

    def __str__(self):
        return f"Constrained beam search decoding (beam_size={self.beam_size}, max_len={self.max_len})"

    _prefix_args = TranslationInferenceSampling._prefix_args
    _bias_arg = TranslationInferenceSampling._bias_arg
    _syntax_arg = TranslationInferenceSampling._syntax_arg

    def generate(self, src: torch.Tensor, logit_bias=None, allowed=None, syntax=None, prefix=None, return_scores: bool = False,
                 return_details: bool = False):
        """Long[B, K, width], hypotheses best first; ``return_scores=True`` appends the ``HypothesisScores`` of the returned
        rows (the raw model's, see ``score``) and ``return_details=True`` a ``ConstrainedBeamDetails``, in that order, as a tuple.

        ``logit_bias`` (Float[B, V]) and ``allowed`` (Bool[B, V], sugar for 0 / ``-inf``) as for
        ``TranslationInferenceSampling.generate`` (``scoring.check_logit_bias``; ``scoring.allowlist_from_source`` builds the
        "tokens of the source" list): the bias is added to every level's logits before the log-softmax.  ``syntax``: a
        ``SmilesSyntax`` (or its raw int8 table [V]) with the generator's ``max_len`` as the rule's: a row can only hold tokens
        after which it can still end balanced inside ``max_len``, so every live row ends in EOS by the last column.  ``prefix``:
        Long[B, Lp] without BOS, right-padded with PAD (``check_prefix``): the forced beginning of every row of a source; a forced
        position ignores bias and mask, reads no logits and costs nothing in ``logp``; a forced EOS ends the row (one live row).
        One decoder step per forced token.  A prefix whose running depth goes negative under ``syntax`` is refused (ValueError).

        ``logp`` agrees with ``logq(src, pred, logit_bias=.., allowed=.., syntax=.., prefix=..).logq`` at temperature 1.  Dead
        rows come back as BOS followed by PAD only, ``logp = -inf``, ``alive = False``."""
        m, K = self.model, self.beam_size
        src = src.to(m.device, torch.int64).contiguous()
        m.check_tokens(src)
        B, Ls = src.shape
        # d_prefix and d_cls are bound only to keep the device tensors alive until the call returns
        d_prefix, prefix_ptr, ld_prefix, h_plen = self._prefix_args(prefix, B)
        bias = self._bias_arg(logit_bias, allowed, B)
        syn, d_cls, syn_arg = self._syntax_arg(syntax, prefix)
        out = torch.empty((B, K, self.max_len), dtype=torch.int64, device=m.device)
        logp = torch.empty((B, K), dtype=torch.float32, device=m.device)
        p = N.BeamSearchParams(self.max_len, K, self.pad_token, self.bos_token, self.eos_token)
        st = N.BeamSearchStats()
        N.check(m._lib.ttx_beam_generate_constrained(m.session, src.data_ptr(), B, Ls, C.byref(p),
                                                     None if bias is None else bias.data_ptr(),
                                                     0 if bias is None else int(bias.stride(0)), syn_arg, prefix_ptr, ld_prefix,
                                                     h_plen, out.data_ptr(), logp.data_ptr(), C.byref(st), m._stream()))
        self.model_calls_num += int(st.model_calls)
        self.b_sz += int(st.running_rows)
        self.given_tokens += int((src != m.src_pad_token_i).sum())
        out = out[:, :, :int(st.out_width)].contiguous()
        alive = torch.isfinite(logp)
        blank = torch.full_like(out, self.pad_token)
        blank[:, :, 0] = self.bos_token
        out = torch.where(alive[:, :, None], out, blank)
        res = [out]
        if return_scores:
            res.append(self.score(src, out))
        if return_details:
            finished = (out[:, :, 1:] == self.eos_token).any(-1) | ~alive
            res.append(ConstrainedBeamDetails(logp, finished, alive))
        return res[0] if len(res) == 1 else tuple(res)


class SbsTrace(NamedTuple):
    """Every level of a stochastic beam search, in selection order: tensors [levels, B, K] of the parent's rank in the previous
    level, the token, the child's log-probability ``phi`` and its perturbed log-probability ``g``."""
    parent: torch.Tensor
    token: torch.Tensor
    phi: torch.Tensor
    g: torch.Tensor


class SbsDetails(NamedTuple):
    """What stochastic beam search knows about its rows: ``logp`` Float[B, K] the model's log-probability of each hypothesis at
    the generator's temperature (under ``top_k`` / ``top_p`` the log-probability under the filtered, renormalised distribution;
    under a ``prefix`` that of the completion given source and prefix: forced tokens cost nothing), ``gumbel`` Float[B, K] its perturbed log-probability (the sampling order: non-increasing, 0 for
    the first row), ``finished`` Bool[B, K], and the ``trace`` when one was asked for (always in sampling order)."""
    logp: torch.Tensor
    gumbel: torch.Tensor
    finished: torch.Tensor
    trace: SbsTrace | None = None


class TranslationInferenceStochasticBeamSearch(_ScoresHypotheses):
    """Stochastic beam search (Kool, van Hoof & Welling, ICML 2019): ``beam_size`` = K pairwise distinct hypotheses per source
    that are an exact sample without replacement from the model's sequence distribution under ``temperature``.  The whole loop
    runs in ttx_sbs_generate: the standard beam loop with k_sbs_step, which perturbs the children's log-probabilities with
    Gumbel noise keyed by (seed, the source's row key, the parent's rank, token, position) and keeps the K largest conditional
    maxima (include/ttx.h states the rule).  The rows of a source depend on the source, its key, the seed, the temperature and
    K only, and the call with K returns the first K rows of the call with a larger K.  A sampled PAD ends a row as EOS does.

    ``top_k`` (0: off, or 1..32) and ``top_p`` (in (0, 1]; 1: off; a ``top_p < 1`` alone runs with ``top_k=32``) are
    ``TranslationInferenceSampling``'s filter: at every free position the kept set is the sampler's, on the bits, every other token
    counts as a -inf logit, and the log-probabilities are renormalised over the kept set.  The K rows are then a sample without
    replacement from the sequence distribution the filtered sampler draws from; fewer than K rows may exist (``top_k=1`` has one:
    the greedy row), and the missing ranks come back finished with ``logp = gumbel = -inf``.  A filter or a ``prefix`` runs
    ttx_sbs_generate_ex (k_sbs_step_masked); a call with neither is ttx_sbs_generate, launch for launch.
    ``generate_many`` decodes a whole list of batches on a pool of source slots (ttx_sbs_generate_pool) and returns, bit for bit,
    the rows of the per-batch calls.  ``scoring.sbs_weights`` turns ``logp`` and ``gumbel`` of a K + 1 call into importance weights, of the
    filtered / conditional distribution when a filter / prefix is on."""

    def __init__(self, model, beam_size: int, max_len: int, pad_token: int, bos_token: int, eos_token: int,
                 temperature: float = 1.0, seed: int = 0, top_k: int = 0, top_p: float = 1.0) -> None:
        self.model = _need_native(model)
        self.beam_size, self.max_len = int(beam_size), int(max_len)
        self.pad_token, self.bos_token, self.eos_token = pad_token, bos_token, eos_token
        self.temperature, self.seed = float(temperature), int(seed)
        self.top_k, self.top_p = int(top_k), float(top_p)
        self.model_calls_num = 0
        self.given_tokens = 0
        self.b_sz = 0
        self.last_stats: N.SbsPoolStats | None = None       # of the most recent generate_many
        self.last_batch_counters: list = []                 # generate_many: what each batch added to the counter attributes

    def __str__(self):
        return (f"Stochastic beam search (beam_size={self.beam_size}, temperature={self.temperature}, top_k={self.top_k}, "
                f"top_p={self.top_p}, seed={self.seed}, max_len={self.max_len})")

    def generate(self, src: torch.Tensor, row_keys=None, return_scores: bool = False, return_details: bool = False,
                 order: str = "sample", trace: bool = False, prefix=None, logit_bias=None, allowed=None, syntax=None):
        """Long[B, K, max_len]: BOS, the tokens up to and including the first EOS or PAD, PAD after.  ``row_keys``: one integer
        per source (default 0..B-1), the source's identity for the random stream.  ``order="sample"``: rows in sampling order
        (``gumbel`` descending); ``order="logp"``: re-sorted by ``logp``, best first (equal values keep their sampling order).
        ``return_scores=True`` appends the ``HypothesisScores`` of the returned rows and ``return_details=True`` an
        ``SbsDetails`` (with ``trace=True`` including the ``SbsTrace``), in that order, as a tuple.

        ``prefix``: Long[B, Lp] without BOS, right-padded with PAD, validated as the samplers validate theirs
        (``check_prefix``): the forced beginning of every row of a source.  A finite row is BOS, the prefix, a completion, PAD;
        the rows are K distinct completions, a sample without replacement from the model's distribution given source and prefix,
        and ``logp`` is the completion's conditional log-probability.  A forced position reads no logits and spends no noise; a
        forced EOS ends the row (one finite row).  One decoder step per forced token.  An empty prefix (zero width, all PAD,
        ``None``) is the unprompted call.

        ``logit_bias`` (Float[B, V]) and ``allowed`` (Bool[B, V]) as for ``TranslationInferenceSampling.generate``: the bias is
        added to every level's logits before temperature and filter (ttx_sbs_generate_bias), so the K rows are a sample without
        replacement from what the biased sampler draws from and ``logp`` is the log-probability under it; under a narrow
        allow-list fewer than K rows may exist (the missing ranks come back as under a filter).  ``None`` for both is the call
        without the keywords.  ``syntax`` is refused (ValueError): the beam layouts take no syntax constraint yet."""
        _refuse_syntax("TranslationInferenceStochasticBeamSearch", syntax)
        if order not in ("sample", "logp"):
            raise ValueError(f"order must be 'sample' or 'logp', got {order!r}")
        m, K = self.model, self.beam_size
        src = src.to(m.device, torch.int64).contiguous()
        m.check_tokens(src)
        B, Ls = src.shape
        pre, plen = check_prefix(prefix, B, self.max_len, self.pad_token, m.tgt_vocab_size)
        d_prefix = prefix_ptr = h_plen = None            # d_prefix keeps the device tensor alive until the call returns
        ld_prefix = 0
        if pre is not None:
            d_prefix = pre.to(m.device)
            prefix_ptr, ld_prefix = (d_prefix.data_ptr() if d_prefix.numel() else None), int(d_prefix.shape[1])
            h_plen = (C.c_int32 * max(B, 1))(*plen)
        keys = None
        if row_keys is not None:
            keys = torch.as_tensor(row_keys, dtype=torch.int64).to(m.device).contiguous()
            if keys.shape != (B,):
                raise ValueError(f"row_keys must hold one key per source ({B}), got shape {tuple(keys.shape)}")
        p = N.SbsParams(self.max_len, K, self.temperature, self.pad_token, self.bos_token, self.eos_token,
                        self.seed & 0xFFFFFFFFFFFFFFFF)
        Kc, Lc = max(K, 1), max(self.max_len, 2)
        out = torch.empty((B, Kc, Lc), dtype=torch.int64, device=m.device)
        logp = torch.empty((B, Kc), dtype=torch.float32, device=m.device)
        gumbel = torch.empty((B, Kc), dtype=torch.float32, device=m.device)
        tr = tr_arg = None
        if trace:
            shape = (Lc - 1, B, Kc)
            tr = SbsTrace(torch.zeros(shape, dtype=torch.int32, device=m.device), torch.zeros(shape, dtype=torch.int32, device=m.device),
                          torch.zeros(shape, dtype=torch.float32, device=m.device), torch.zeros(shape, dtype=torch.float32, device=m.device))
            tr_arg = C.byref(N.SbsTrace(*(t.data_ptr() for t in tr)))
        st = N.BeamSearchStats()
        filt = N.SbsFilter(self.top_k, self.top_p)
        bias = combine_bias(logit_bias, allowed, B, m.tgt_vocab_size)
        if bias is not None:
            bias = bias.to(m.device).contiguous()        # bound until the call returns; a NULL d_bias is the unbiased call
        N.check(m._lib.ttx_sbs_generate_bias(m.session, src.data_ptr(), B, Ls, None if keys is None else keys.data_ptr(), C.byref(p),
                                             C.byref(filt), prefix_ptr, ld_prefix, h_plen, None if bias is None else bias.data_ptr(),
                                             0 if bias is None else int(bias.stride(0)), out.data_ptr(), logp.data_ptr(),
                                             gumbel.data_ptr(), tr_arg, C.byref(st), m._stream()))
        self.model_calls_num += int(st.model_calls)
        self.b_sz += int(st.running_rows)
        self.given_tokens += int((src != m.src_pad_token_i).sum())
        if order == "logp":
            idx = torch.argsort(logp, dim=1, descending=True, stable=True)
            out = torch.gather(out, 1, idx[:, :, None].expand_as(out))
            logp, gumbel = torch.gather(logp, 1, idx), torch.gather(gumbel, 1, idx)
        res = [out]
        if return_scores:
            res.append(self.score(src, out))
        if return_details:
            ended = ((out[:, :, 1:] == self.eos_token) | (out[:, :, 1:] == self.pad_token)).any(-1) | torch.isinf(gumbel)
            if tr is not None:
                tr = SbsTrace(*(t[:int(st.model_calls)] for t in tr))
            res.append(SbsDetails(logp, gumbel, ended, tr))
        return res[0] if len(res) == 1 else tuple(res)

    def _pool_plan(self, S: int, in_flight: int, capacity: int | None) -> tuple:
        """(source slots per pool, sessions): a given ``capacity`` or TTX_POOL_CAPACITY counts sources; the default is the greedy
        pool's row plan for the ``S * K`` decoder rows, divided by K (DESIGN.md §24 has the sweep behind it)."""
        K = max(self.beam_size, 1)
        given = capacity if capacity is not None else (os.environ.get("TTX_POOL_CAPACITY") or None)
        if given is not None and not 1 <= int(given) <= 1024:
            raise ValueError(f"capacity (source slots per pool) must lie in [1, 1024], got {given}")
        # the pool count follows the decoder rows a pool holds, whichever way the capacity was given
        rows_cap, n_sess = _slot_pool_plan(S * K, in_flight, None if given is None else int(given) * K)
        return (int(given) if given is not None else min(1024, max(1, rows_cap // K))), n_sess

    def generate_many(self, batches: list, row_keys=None, in_flight: int = 4, capacity: int | None = None,
                      return_scores: bool = False, return_details: bool = False, order: str = "sample", prefixes=None,
                      logit_biases=None, allowed=None, syntax=None) -> list:
        """``generate`` over a whole list of batches on pools of source slots (ttx_sbs_generate_pool: continuous batching over the
        sources of the list, sorted by length).  A source leaves the pool as soon as its K rows are finished and the next one
        takes its slot, so a decoder pass serves unfinished candidates only.  Returns one entry per batch, shaped as ``generate``
        returns it (a tensor, or a tuple with ``HypothesisScores`` and / or ``SbsDetails``, whose ``trace`` is ``None``: the pool
        keeps none).

        ``generate_many(batches, row_keys=ks, prefixes=ps)[i]`` equals ``generate(batches[i], row_keys=ks[i], prefix=ps[i])`` bit
        for bit: tokens, ``logp`` and ``gumbel``, whatever the capacity, ``in_flight``, the order of the list or the batching
        (include/ttx.h states the contract and its range).  ``row_keys``: one sequence of integers per batch; by default the
        running index over the concatenated batches.  ``prefixes``: a list aligned with ``batches``, each entry a ``prefix`` for
        that batch or ``None``.  ``capacity``: source slots per pool (``TTX_POOL_CAPACITY``), at most 1 024; ``in_flight``: pools
        at once.  ``model_calls_num`` counts the decoder passes the device executed, ``b_sz`` the unfinished candidates they
        served; ``last_batch_counters`` holds each batch's share of the counters (``b_sz`` and ``given_tokens`` as ``generate`` counts
        them for that batch, the decoder passes apportioned by candidates)."""
        from .scheduling import plan_row_groups
        _refuse_bias("TranslationInferenceStochasticBeamSearch.generate_many (the source-slot pool)", logit_biases, allowed)
        _refuse_syntax("TranslationInferenceStochasticBeamSearch.generate_many (the source-slot pool)", syntax)
        if order not in ("sample", "logp"):
            raise ValueError(f"order must be 'sample' or 'logp', got {order!r}")
        self._pool_plan(1, in_flight, capacity)               # refuses a capacity outside [1, 1024] before anything else
        if prefixes is not None and len(prefixes) != len(batches):
            raise ValueError(f"prefixes must hold one entry per batch ({len(batches)}), got {len(prefixes)}")
        if row_keys is not None and len(row_keys) != len(batches):
            raise ValueError(f"row_keys must hold one sequence per batch ({len(batches)}), got {len(row_keys)}")
        if not batches:
            return []
        m, K, L = self.model, self.beam_size, self.max_len
        sizes = [int(b.shape[0]) for b in batches]
        S = sum(sizes)
        if row_keys is None:
            keys = torch.arange(S, dtype=torch.int64)
        else:
            per = [torch.as_tensor(k, dtype=torch.int64).reshape(-1).cpu() for k in row_keys]
            for i, (k, B) in enumerate(zip(per, sizes)):
                if k.shape != (B,):
                    raise ValueError(f"row_keys[{i}] must hold one key per source ({B}), got shape {tuple(k.shape)}")
            keys = torch.cat(per) if per else torch.zeros(0, dtype=torch.int64)
        allpre = plen = None
        if prefixes is not None and any(q is not None for q in prefixes):
            checked = [check_prefix(q, B, L, self.pad_token, m.tgt_vocab_size) for q, B in zip(prefixes, sizes)]
            Lp = max([int(c[0].shape[1]) for c in checked if c[0] is not None] or [0])
            allpre = torch.full((S, Lp), self.pad_token, dtype=torch.int64)
            plen = torch.zeros(S, dtype=torch.int64)
            r0 = 0
            for (q, lens), B in zip(checked, sizes):
                if q is not None:
                    allpre[r0:r0 + B, :q.shape[1]] = q
                    plen[r0:r0 + B] = torch.tensor(lens, dtype=torch.int64)
                r0 += B
            if not bool(plen.any()):
                allpre = plen = None
        srcs = [b.to(m.device, torch.int64) for b in batches]
        Lmax = max([int(s.shape[1]) for s in srcs if s.shape[0]] or [2])
        allsrc = torch.full((S, Lmax), self.pad_token, dtype=torch.int64, device=m.device)
        r0 = 0
        for s in srcs:
            allsrc[r0:r0 + s.shape[0], :s.shape[1]] = s
            r0 += s.shape[0]
        m.check_tokens(allsrc)
        cap, n_sess = self._pool_plan(S, in_flight, capacity)
        self.last_group_size, self.last_pool_sessions = cap, n_sess
        p = N.SbsParams(L, K, self.temperature, self.pad_token, self.bos_token, self.eos_token, self.seed & 0xFFFFFFFFFFFFFFFF)
        filt = N.SbsFilter(self.top_k, self.top_p)
        Kc, Lc = max(K, 1), max(L, 2)
        out_sorted = torch.empty((S, Kc, Lc), dtype=torch.int64, device=m.device)
        logp_sorted = torch.empty((S, Kc), dtype=torch.float32, device=m.device)
        gumbel_sorted = torch.empty((S, Kc), dtype=torch.float32, device=m.device)
        st = N.SbsPoolStats()
        per_src = torch.zeros(max(S, 1), dtype=torch.int32, device=m.device)     # candidates decoded per source, in the pool's order
        st.d_src_running_rows = per_src.data_ptr()
        if S:
            pos = torch.arange(1, Lmax + 1, device=m.device)
            lengths = ((allsrc != self.pad_token) * pos).amax(dim=1)
            order_np, _ = plan_row_groups(lengths.cpu().numpy(), cap * Kc)
            order_t = torch.from_numpy(order_np).to(m.device)
            sorted_len = lengths[order_t].cpu().numpy()
            width = max(2, int(sorted_len.max()))
            sorted_src = allsrc[order_t]
            src_mat = sorted_src[:, :width].contiguous() if width <= Lmax else torch.nn.functional.pad(
                sorted_src, (0, width - Lmax), value=self.pad_token).contiguous()
            keys_sorted = keys.to(m.device)[order_t].contiguous()
            h_len = (C.c_int32 * S)(*[max(2, int(x)) for x in sorted_len])
            sessions = m.session_pool(n_sess)
            sess = (C.c_void_p * len(sessions))(*[q.value for q in sessions])
            d_prefix = prefix_ptr = h_plen = None            # d_prefix keeps the device tensor alive until the call returns
            ld_prefix = 0
            if allpre is not None:
                order_cpu = torch.from_numpy(order_np).to(torch.int64)
                d_prefix = allpre[order_cpu].contiguous().to(m.device)
                prefix_ptr, ld_prefix = (d_prefix.data_ptr() if d_prefix.numel() else None), int(d_prefix.shape[1])
                h_plen = (C.c_int32 * S)(*[int(x) for x in plen[order_cpu]])
            N.check(m._lib.ttx_sbs_generate_pool(sess, len(sessions), src_mat.data_ptr(), S, width, h_len, keys_sorted.data_ptr(), cap,
                                                 C.byref(p), C.byref(filt), prefix_ptr, ld_prefix, h_plen, out_sorted.data_ptr(),
                                                 logp_sorted.data_ptr(), gumbel_sorted.data_ptr(), C.byref(st), m._stream()))
            inv = torch.empty_like(order_t)
            inv[order_t] = torch.arange(S, device=m.device)
            out_rows, logp_rows, gumbel_rows = out_sorted[inv], logp_sorted[inv], gumbel_sorted[inv]
            per_src = per_src[inv]
            self.given_tokens += int((allsrc != m.src_pad_token_i).sum())
        else:
            out_rows, logp_rows, gumbel_rows = out_sorted, logp_sorted, gumbel_sorted
        self.model_calls_num += int(st.model_calls)
        self.b_sz += int(st.running_rows)
        self.last_stats = st
        # what each batch added to the counters (a look-ahead that falls back takes them back): its sources' tokens, the candidates
        # decoded for its sources (exactly what generate(batch) counts), and the call's decoder passes apportioned by those
        # candidates (largest remainder: the shares sum to the call's count, which serves every batch at once)
        rows_of = [int(x) for x in torch.stack([c.sum() for c in torch.split(per_src[:S].long(), sizes)]).cpu()] if S else [0] * len(sizes)
        total_rows, calls = max(1, sum(rows_of)), int(st.model_calls)
        quota = [calls * r // total_rows for r in rows_of]
        for i in sorted(range(len(sizes)), key=lambda i: -(calls * rows_of[i] % total_rows))[:calls - sum(quota)]:
            quota[i] += 1
        self.last_batch_counters = [{"model_calls_num": q, "b_sz": r, "given_tokens": int((b != m.src_pad_token_i).sum())}
                                    for q, r, b in zip(quota, rows_of, srcs)]
        res, r0 = [], 0
        for src, B in zip(srcs, sizes):
            out, logp, gumbel = out_rows[r0:r0 + B].contiguous(), logp_rows[r0:r0 + B].contiguous(), gumbel_rows[r0:r0 + B].contiguous()
            r0 += B
            if order == "logp":
                idx = torch.argsort(logp, dim=1, descending=True, stable=True)
                out = torch.gather(out, 1, idx[:, :, None].expand_as(out))
                logp, gumbel = torch.gather(logp, 1, idx), torch.gather(gumbel, 1, idx)
            entry = [out]
            if return_scores:
                entry.append(self.score(src, out) if B else None)
            if return_details:
                ended = ((out[:, :, 1:] == self.eos_token) | (out[:, :, 1:] == self.pad_token)).any(-1) | torch.isinf(gumbel)
                entry.append(SbsDetails(logp, gumbel, ended, None))
            res.append(entry[0] if len(entry) == 1 else tuple(entry))
        return res


class TranslationInferenceBeamSearchSpeculative(_ScoresHypotheses):
    """Drop-in for src/decoding/speculative_decoding.py:241-869 (both draft modes): the whole loop — candidate rows, draft
    slots, KV-cached verify step, accepted lengths, best draft, leaf enumeration and scoring, per-source selection,
    termination — runs in ttx_beam_speculative_generate; Python allocates the output tensor and keeps the counters."""

    def __init__(self, model, max_len: int, n_best: int, draft_len: int, n_drafts: int, vocab_size: int,
                 smart_drafts_mode: bool, pad_token: int, bos_token: int, eos_token: int, C_token: int,
                 max_steps: int | None = None) -> None:
        self.model = _need_native(model)
        self.max_len, self.vocab_size = max_len, vocab_size
        self.smart_drafts_mode = smart_drafts_mode
        self.pad_token_idx, self.bos_token_idx, self.eos_token_idx, self.C_token_idx = pad_token, bos_token, eos_token, C_token
        self.n_best = n_best
        self.accepted_tokens_num = 0
        self.model_calls_num = 0
        self.model_input_lines_num = 0
        self.max_drafts_num = n_drafts
        self.n_drafts = 0
        self.requested_drafts_num = n_drafts
        self.produced_non_pad_tokens = 0
        self.max_draft_len, self.min_draft_len = 200, 5
        clamped = min(max(self.min_draft_len, draft_len), self.max_draft_len)
        if clamped != draft_len:
            print(f"The draft length should be in range [{self.min_draft_len}: {self.max_draft_len}], so it was changed to {clamped}")
        self.draft_len = clamped
        self.b_sz = 0
        # Safety valve absent from the reference, whose loop never ends when a candidate keeps emitting PAD before any
        # EOS; None = reference behaviour.
        self.max_steps = max_steps
        self.last_failed_batches: list = []    # generate_many(on_error="skip"): batches on which the reference raises / the guard trips
        self.last_batch_counters: list = []    # generate_many: what each batch added to the counter attributes (None: failed)
        # work the device executed, for bench.py's roofline
        self.stats_total = {"verified_positions": 0, "executed_positions": 0, "kv_prefix_positions": 0, "running_candidates": 0,
                            "src_tokens_padded": 0, "src_positions": 0, "encode_ms": 0.0, "decode_ms": 0.0, "batches": 0}
        if vocab_size != self.model.tgt_vocab_size:
            raise ValueError("vocab_size differs from the model's target vocabulary")

    def __str__(self):
        return (f"SpeculativeSampling decoding (n_best={self.n_best}, max_len={self.max_len}, "
                f"max_num_of_drafts={self.max_drafts_num}, draft_len={self.draft_len})")

    def _params(self) -> N.BeamParams:
        return N.BeamParams(self.max_len, self.n_best, self.draft_len, self.requested_drafts_num, int(bool(self.smart_drafts_mode)),
                            self.pad_token_idx, self.bos_token_idx, self.eos_token_idx, self.C_token_idx, int(self.max_steps or 0))

    def _pad_eos(self) -> tuple:
        return self.pad_token_idx, self.eos_token_idx

    _COUNTERS = ("model_calls_num", "accepted_tokens_num", "produced_non_pad_tokens", "model_input_lines_num", "b_sz", "n_drafts")

    def _counter_values(self) -> dict:
        return {k: getattr(self, k) for k in self._COUNTERS}

    def _account(self, st: N.BeamStats, B: int) -> None:
        t = self.stats_total
        for k in ("verified_positions", "executed_positions", "kv_prefix_positions", "running_candidates", "src_tokens_padded",
                  "encode_ms", "decode_ms"):
            t[k] += getattr(st, k)
        t["src_positions"] += int(st.running_candidates) * (int(st.src_tokens_padded) // max(1, B))
        t["batches"] += 1
        self.model_calls_num += int(st.model_calls)
        if self.smart_drafts_mode:                                               # only the smart-drafts loop counts these (:741, :760)
            self.model_input_lines_num += int(st.input_lines)
            self.b_sz += int(st.running_rows)
        self.accepted_tokens_num += int(st.accepted_tokens)
        self.produced_non_pad_tokens += int(st.produced_non_pad_tokens)
        if not self.smart_drafts_mode:
            self.n_drafts += B * self.requested_drafts_num                       # :434

    def generate(self, src: torch.Tensor, return_scores: bool = False, logit_bias=None, allowed=None, syntax=None):
        """``return_scores=True``: ``(pred, HypothesisScores)`` instead of ``pred`` (see ``score``).  ``logit_bias`` / ``allowed``
        are refused (ValueError)."""
        _refuse_bias("TranslationInferenceBeamSearchSpeculative", logit_bias, allowed)
        _refuse_syntax("TranslationInferenceBeamSearchSpeculative", syntax)
        m = self.model
        src = src.to(m.device, torch.int64).contiguous()
        m.check_tokens(src)
        B, Ls = src.shape
        out = torch.empty((B, self.n_best, self.max_len), dtype=torch.int64, device=m.device)
        p, st = self._params(), N.BeamStats()
        N.check(m._lib.ttx_beam_speculative_generate(m.session, src.data_ptr(), B, Ls, C.byref(p), out.data_ptr(), C.byref(st),
                                                     m._stream()))
        self._account(st, B)
        return self._scored(src, out[:, :, :int(st.out_width)].contiguous(), return_scores)

    def generate_many(self, batches: list, in_flight: int = 4, pool: bool | None = None, on_error: str = "raise",
                      capacity: int | None = None, return_scores: bool = False, logit_biases=None, allowed=None, syntax=None) -> list:
        """Several batches on the GPU at once; every returned tensor and the counters are those of per-batch ``generate`` calls.

        ``pool`` (default: on for two or more batches, ``TTX_BEAM_POOL=0`` turns it off): the given batches are decoded in slot
        pools — continuous batching: whole batches are admitted as slots free up, one verify step per iteration serves a few
        hundred candidates of many batches, and the reference's batch-wide loop scalars (draft length, stop rule, smart-mode
        table width) are kept per batch on the device (ttx_beam_speculative_generate_pool); result width, model calls and
        counters per given batch come from per-source traces (scheduling.replay_beam_batch).  Otherwise the batches run as
        given, ``in_flight`` of them at once, one session + stream each (ttx_beam_speculative_generate_many).

        ``on_error="skip"``: a batch on which the reference raises (or the ``max_steps`` guard trips) yields ``None`` instead of
        ending the call; the indices are kept in ``self.last_failed_batches`` — ``generate`` on that batch raises the error.

        ``return_scores=True``: a list of ``(pred, HypothesisScores)`` pairs; a batch that came back ``None`` has ``None``
        scores.  ``logit_biases`` / ``allowed`` are refused (ValueError), as in ``generate``."""
        _refuse_bias("TranslationInferenceBeamSearchSpeculative.generate_many", logit_biases, allowed)
        _refuse_syntax("TranslationInferenceBeamSearchSpeculative.generate_many", syntax)
        if return_scores:
            return self._scored_many(batches, self.generate_many(batches, in_flight, pool, on_error, capacity))
        m = self.model
        if on_error not in ("raise", "skip"):
            raise ValueError("on_error must be 'raise' or 'skip'")
        self.last_failed_batches = []
        self.last_batch_counters = [None] * len(batches)
        if not batches:
            return []
        srcs = [b.to(m.device, torch.int64).contiguous() for b in batches]
        for b in srcs:
            m.check_tokens(b)
        if pool is None:
            pool = len(srcs) > 1
        # smart mode needs a window library for every batch (Ls - 5 > 0, drafting.py:39); max_len < 3 never enters the loop
        d0 = self.draft_len if not self.smart_drafts_mode else min(max(5, self.draft_len + 1), 200) - 1
        if pool and self.max_len >= 3 and all(int(b.shape[1]) >= 2 and (not self.smart_drafts_mode or int(b.shape[1]) > 5) for b in srcs):
            return self._generate_pooled(srcs, in_flight, on_error, capacity, d0)
        return self._generate_as_given(srcs, list(range(len(srcs))), in_flight, on_error)

    def _generate_as_given(self, srcs: list, index: list, in_flight: int, on_error: str) -> list:
        m = self.model
        n = len(srcs)
        outs = [torch.empty((s.shape[0], self.n_best, self.max_len), dtype=torch.int64, device=m.device) for s in srcs]
        sessions = m.session_pool(max(1, min(in_flight, n)))
        sess = (C.c_void_p * len(sessions))(*[q.value for q in sessions])
        src_p = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
        out_p = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        Bs = (C.c_int * n)(*[s.shape[0] for s in srcs])
        Ls = (C.c_int * n)(*[s.shape[1] for s in srcs])
        p = self._params()
        stats = (N.BeamStats * n)()
        rc = m._lib.ttx_beam_speculative_generate_many(sess, len(sessions), n, src_p, Bs, Ls, C.byref(p), out_p, stats, m._stream())
        if rc not in (N.TTX_OK, N.TTX_ERR_REFERENCE, N.TTX_ERR_MAX_STEPS):
            N.check(rc)                            # not a per-batch outcome: the call itself failed
        res = []
        for i, (s, o, st) in enumerate(zip(srcs, outs, stats)):
            if int(st.status) != N.TTX_OK:         # every batch was decoded; this one raises in the reference / trips the guard
                if on_error == "raise" or int(st.status) not in (N.TTX_ERR_REFERENCE, N.TTX_ERR_MAX_STEPS):
                    if int(st.status) == N.TTX_ERR_MAX_STEPS:
                        raise RuntimeError("beam-speculative loop exceeded max_steps (non-terminating input)")
                    if int(st.status) == N.TTX_ERR_REFERENCE:
                        raise N.ReferenceError_(f"batch {index[i]}: fewer candidate leaves than n_best for a source (the reference "
                                                "asserts here, speculative_decoding.py:195)")
                    N.check(int(st.status))
                self.last_failed_batches.append(index[i])
                res.append(None)
                continue
            before = self._counter_values()
            self._account(st, s.shape[0])
            self.last_batch_counters[index[i]] = {k: v - before[k] for k, v in self._counter_values().items()}
            res.append(o[:, :, :int(st.out_width)].contiguous())
        return res

    def _generate_pooled(self, srcs: list, in_flight: int, on_error: str, capacity: int | None, d0: int) -> list:
        from .scheduling import replay_beam_batch
        m, K, L = self.model, self.n_best, self.max_len
        n = len(srcs)
        sizes = np.array([int(s.shape[0]) for s in srcs])
        widths = np.array([int(s.shape[1]) for s in srcs], dtype=np.int32)
        R = int(sizes.sum())
        Lmax = int(widths.max())
        allsrc = torch.full((R, Lmax), self.pad_token_idx, dtype=torch.int64, device=m.device)
        starts = np.concatenate([[0], np.cumsum(sizes)])
        for s, r0 in zip(srcs, starts):
            allsrc[r0:r0 + s.shape[0], :s.shape[1]] = s
        pos = torch.arange(1, Lmax + 1, device=m.device)
        lengths = ((allsrc != self.pad_token_idx) * pos).amax(dim=1).clamp(min=2).cpu().numpy().astype(np.int32)
        # work list: whole batches, the one with the longest source first (a chunk is encoded at its longest row's width)
        batch_long = np.array([lengths[starts[i]:starts[i + 1]].max() for i in range(n)])
        border = np.argsort(-batch_long, kind="stable")
        order = np.concatenate([np.arange(starts[b], starts[b + 1]) for b in border])
        order_t = torch.from_numpy(order).to(m.device)
        width = int(lengths.max())
        src_mat = allsrc[order_t][:, :width].contiguous()
        h_len = np.ascontiguousarray(lengths[order])
        h_batch = np.ascontiguousarray(np.repeat(np.arange(n, dtype=np.int32), sizes[border]))
        h_given = np.ascontiguousarray(widths[border])
        # pool size: about 16 k step rows per iteration (where the step GEMMs run on their large tilings); a few pools in flight
        rps = 1 + self.requested_drafts_num * d0
        cap = int(capacity or os.environ.get("TTX_BEAM_POOL_CAPACITY") or max(4, min(512, 16384 // max(1, K * rps))))
        cap = max(cap, int(sizes.max()))
        n_sess = max(1, min(in_flight, 4, -(-R // cap)))
        if os.environ.get("TTX_POOL_SESSIONS"):
            n_sess = max(1, int(os.environ["TTX_POOL_SESSIONS"]))
        sessions = m.session_pool(n_sess)
        sess = (C.c_void_p * len(sessions))(*[q.value for q in sessions])
        T_cap = L + 8
        out_sorted = torch.empty((R, K, L), dtype=torch.int64, device=m.device)
        tlen = torch.empty((R, T_cap), dtype=torch.int16, device=m.device)
        summ = torch.empty((R, 8), dtype=torch.int32, device=m.device)
        st = N.BeamStats()
        p = self._params()
        i32 = C.POINTER(C.c_int32)
        N.check(m._lib.ttx_beam_speculative_generate_pool(
            sess, len(sessions), src_mat.data_ptr(), R, width, h_len.ctypes.data_as(i32), h_batch.ctypes.data_as(i32), n,
            h_given.ctypes.data_as(i32), cap, C.byref(p), out_sorted.data_ptr(), tlen.data_ptr(), summ.data_ptr(), T_cap, C.byref(st),
            m._stream()))
        inv = torch.empty_like(order_t)
        inv[order_t] = torch.arange(R, device=m.device)
        out_rows = out_sorted[inv]
        tlen_h, summ_h = tlen[inv].cpu().numpy(), summ[inv].cpu().numpy()
        # what the device executed (for bench.py's roofline), once for the whole call
        t = self.stats_total
        for k in ("verified_positions", "executed_positions", "kv_prefix_positions", "running_candidates", "src_tokens_padded",
                  "encode_ms", "decode_ms"):
            t[k] += getattr(st, k)
        t["src_positions"] += int((summ_h[:, 7].astype(np.int64) * lengths.astype(np.int64)).sum())   # cross-attention keys read
        t["device_model_calls"] = t.get("device_model_calls", 0) + int(st.model_calls)
        t["pool_calls"] = t.get("pool_calls", 0) + 1
        res: list = [None] * n
        for bi in range(n):
            r0, r1 = int(starts[bi]), int(starts[bi + 1])
            rep = replay_beam_batch(tlen_h[r0:r1], summ_h[r0:r1], L, d0, K)
            if rep.error is not None:
                if on_error == "raise":
                    if rep.error == "max_steps":
                        raise RuntimeError("beam-speculative loop exceeded max_steps (non-terminating input)")
                    raise N.ReferenceError_(f"batch {bi}: fewer candidate leaves than n_best for a source (the reference asserts here, "
                                            "speculative_decoding.py:195)")
                self.last_failed_batches.append(bi)
                continue
            res[bi] = out_rows[r0:r1, :, :rep.out_width].contiguous()
            before = self._counter_values()
            self.model_calls_num += rep.model_calls
            self.accepted_tokens_num += rep.accepted_tokens
            self.produced_non_pad_tokens += rep.produced_non_pad_tokens
            if self.smart_drafts_mode:
                self.model_input_lines_num += rep.input_lines
                self.b_sz += rep.running_rows
            else:
                self.n_drafts += (r1 - r0) * self.requested_drafts_num
            self.last_batch_counters[bi] = {k: v - before[k] for k, v in self._counter_values().items()}
            t["batches"] += 1
        return res
