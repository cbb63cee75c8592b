"""Host-side mirror of the reference model protocol over the HIP library.

``NativeTransformer`` offers what the reference's generators call on ``VanillaTransformer``
(src/model/modules.py:86-138): ``src_pad_token_i``, ``encode_src(src, src_pad_mask)``,
``decode_tgt(tgt, memory, memory_pad_mask=...)`` and ``model(src, tgt)`` — same argument meaning, same
tensor shapes/dtypes out — so the reference's own generator classes can drive it unchanged, and it owns
the ``ttx_session`` the native generators of decoding.py run on.  torch is used for device memory and
the current stream only; every FLOP happens in libttx_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _native as N
from .scheduling import score_plan


def reference_pe_table(emb: int, max_len: int = 5000) -> torch.Tensor:
    """The non-persistent ``pe`` buffer of the reference (src/model/embeddings.py:38-45), rebuilt with the
    same torch ops so the table handed to the library is bit-identical to the one the reference adds."""
    pe = torch.zeros(max_len, emb)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, emb, 2).float() * (-math.log(10000.0) / emb))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return torch.vstack((torch.zeros(1, emb), pe)).contiguous()


def _strip(state: dict) -> dict:
    if any(k.startswith("model.") for k in state):
        return {k[len("model."):]: v for k, v in state.items() if k.startswith("model.")}
    return dict(state)


def shape_of_state(state_dict: dict) -> dict:
    """Model dimensions read off a reference state dict (SURVEY.md §8(b) B6 names)."""
    st = _strip(state_dict)
    emb = st["src_token_featurizer.embedding.weight"]
    return {"emb_dim": int(emb.shape[1]), "src_vocab_size": int(emb.shape[0]),
            "tgt_vocab_size": int(st["next_token_classifier.weight"].shape[0]),
            "ff_dim": int(st["transformer.encoder.layers.0.linear1.weight"].shape[0]),
            "num_enc_layers": 1 + max(int(k.split(".")[3]) for k in st if k.startswith("transformer.encoder.layers.")),
            "num_dec_layers": 1 + max(int(k.split(".")[3]) for k in st if k.startswith("transformer.decoder.layers."))}


class _DeviceSpan:
    """Exposes a device allocation of the library to torch (``torch.as_tensor``) without copying it."""

    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": "<f4", "data": (ptr, False), "version": 2}


class TeacherForced(NamedTuple):
    """Result of ``NativeTransformer.teacher_forced``: device tensors, nothing copied to the host."""
    loss: torch.Tensor            # 0-d fp32: nn.CrossEntropyLoss (mean over all B*(Lt-1) positions, PAD targets included)
    token_acc: torch.Tensor       # 0-d fp32: calc_token_acc
    seq_acc: torch.Tensor         # 0-d fp32: calc_sequence_acc (NaN when no target holds an EOS)
    pred_tokens: torch.Tensor     # int64 [B, Lt-1]: argmax of the logits (first maximum)
    token_nll: torch.Tensor       # fp32 [B, Lt-1]: per-position cross-entropy
    logits: torch.Tensor | None   # fp32 [B, Lt-1, V] when asked for


class HypothesisScores(NamedTuple):
    """Result of ``NativeTransformer.score_hypotheses`` / ``hypothesis_logprobs``: device tensors, nothing copied to the host.
    For hypothesis ``h = hyp[b, k]`` (column 0, the BOS, is never scored): ``length`` n is the column of the first EOS at a
    column >= 1 (``finished``), else the last column >= 1 holding a non-PAD token, else 0; ``token_logp[t-1]`` is
    ``log_softmax(decode_tgt(h[:-1])[t-1])[h[t]]`` for t = 1..n and exactly 0 beyond; ``score`` is their sum."""
    score: torch.Tensor              # fp32 [B, N]: log-likelihood of the hypothesis under the model (0.0 for an all-PAD row)
    length: torch.Tensor             # int32 [B, N]: scored tokens, the EOS included
    finished: torch.Tensor           # bool [B, N]: the hypothesis holds an EOS
    token_logp: torch.Tensor | None  # fp32 [B, N, W-1] when asked for


class AttentionMaps(NamedTuple):
    """Result of ``NativeTransformer.attention_maps``: device tensors, nothing copied to the host.  Query position ``t`` of
    hypothesis ``hyp[b, k]`` (the one that predicts ``hyp[b, k, t+1]``) is live iff ``t + 1 <= length[b, k]``; ``attn`` is the
    cross-attention of one decoder layer over the source positions, exactly 0.0 at PAD keys and at positions that are not
    live; ``alignment[b, k, t]`` is the source position of the first maximum of the head-mean map, -1 where not live."""
    attn: torch.Tensor               # fp32 [B, N, W-1, Ls] (heads="mean") or [B, N, H, W-1, Ls] (heads="all")
    alignment: torch.Tensor | None   # int32 [B, N, W-1] when asked for
    length: torch.Tensor             # int32 [B, N]: as HypothesisScores.length


class Alternatives(NamedTuple):
    """Result of ``NativeTransformer.alternatives`` / ``hypothesis_alternatives``: device tensors, nothing copied to the host.
    Position ``p`` of hypothesis ``h`` (the one that predicts ``h[p+1]``) is live iff ``p < length``.  Where not live:
    ``top_id`` = -1, ``rank`` = -1, the rest exactly 0."""
    top_id: torch.Tensor             # int32 [..., T, k]: the k most probable ids, best first, equal logits by ascending id
    top_logp: torch.Tensor           # fp32 [..., T, k]: their log-probabilities
    chosen_logp: torch.Tensor        # fp32 [..., T]: log-probability of the emitted token (HypothesisScores.token_logp, bit for bit)
    rank: torch.Tensor               # int32 [..., T]: tokens the model preferred to the emitted one (0: it was the first maximum)
    entropy: torch.Tensor            # fp32 [..., T]: entropy of the distribution, nats
    length: torch.Tensor             # int32 [...]: as HypothesisScores.length

    @property
    def margin(self) -> torch.Tensor:
        """fp32 [..., T]: log-probability of the best id minus that of the runner-up (needs k >= 2); exactly 0 where not live."""
        if self.top_logp.shape[-1] < 2:
            raise ValueError("margin needs k >= 2")
        return self.top_logp[..., 0] - self.top_logp[..., 1]


class ProposalScores(NamedTuple):
    """Result of ``NativeTransformer.proposal_scores`` / ``hypothesis_logq``: device tensors, nothing copied to the host.  The
    log-probability of hypothesis ``hyp[b, k]`` under the SAMPLING distribution q (temperature, top-k, top-p) where
    ``HypothesisScores.score`` is its log-probability under the model p.  Position ``p`` (the one that predicts ``h[p+1]``) is
    live iff ``p < length``; forced positions and positions that are not live hold ``token_logq`` = 0, ``rank`` = -1 and
    ``n_kept`` = 0."""
    logq: torch.Tensor                # fp32 [B, N]: log q of the hypothesis; -inf when the sampler cannot emit it
    length: torch.Tensor              # int32 [B, N]: as HypothesisScores.length
    finished: torch.Tensor            # bool [B, N]: as HypothesisScores.finished
    first_outside: torch.Tensor       # int32 [B, N]: the first live position whose token is outside q's support, else -1
    token_logq: torch.Tensor | None   # fp32 [B, N, W-1] when asked for
    rank: torch.Tensor | None         # int32 [B, N, W-1] when asked for: tokens ranked above the emitted one under q's scaling
    n_kept: torch.Tensor | None       # int32 [B, N, W-1] when asked for: size of the kept set (rank == n_kept: just outside it)
    scores: HypothesisScores | None   # with_scores=True: score_hypotheses' result (with token_logp), from the same decoder pass


class FoldedHypotheses(NamedTuple):
    """Result of ``fold_hypotheses`` / ``fold`` / ``scoring.fold_samples``: the distinct hypotheses of every source, counted and
    ranked (ttx_fold_hypotheses); device tensors, nothing copied to the host.  ``U = n_unique[b]`` ranks of source ``b`` are
    live."""
    pred: torch.Tensor | None      # int64 [B, N, L] by rank: the representatives' rows as they stood, all-PAD rows beyond U (gather=True)
    perm: torch.Tensor             # int32 [B, N]: rank -> sample index of the representative, -1 beyond U
    count: torch.Tensor            # int32 [B, N] by rank: how many of the N rows are this hypothesis, 0 beyond U
    n_unique: torch.Tensor         # int32 [B]: U
    first: torch.Tensor            # int32 [B, N] by sample: the first row equal to this one
    rank_of: torch.Tensor          # int32 [B, N] by sample: the rank of the hypothesis the row belongs to
    score: torch.Tensor            # fp32 [B, N] by rank: the representative's own score (NaN read as -inf), -inf beyond U or unscored
    logmass: torch.Tensor | None   # fp32 [B]: log sum exp of the representatives' scores (with scores = log p: the mass covered)


def fold_on_device(lib, session, hyp, scores=None, order: str = "score", unfinished: str = "keep", gather: bool = True,
                   with_logmass=None, pad: int = 0, eos: int = 2, debug_no_filter: bool = False) -> FoldedHypotheses:
    """One ttx_fold_hypotheses call on ``hyp`` Long[B, N, L] (a device tensor, or a view of one whose last-dimension stride is 1:
    it is folded in place through its row stride) and ``scores`` Float[B, N] (or anything with ``.score``, or None).
    ``session``: a ttx_session or None (the kernel needs no workspace).  ``lib``: the loaded library, or None to load it after
    the arguments have been checked.  Every argument is checked before the library or the device is touched."""
    if not isinstance(hyp, torch.Tensor) or hyp.dim() != 3 or hyp.dtype.is_floating_point or hyp.dtype == torch.bool:
        raise ValueError(f"fold needs hyp as an integer tensor [B, N, L], got {getattr(hyp, 'dtype', type(hyp))} "
                         f"{tuple(getattr(hyp, 'shape', ()))}")
    B, K, L = (int(v) for v in hyp.shape)
    if B < 1 or K < 1 or L < 1:
        raise ValueError(f"fold needs hyp [B >= 1, N >= 1, L >= 1], got {tuple(hyp.shape)}")
    if K > 1024:
        raise ValueError(f"fold takes at most 1024 rows per source, got N = {K}")
    if order not in N.FOLD_ORDERS:
        raise ValueError(f"order must be 'score', 'count' or 'first', got {order!r}")
    if unfinished not in ("keep", "last"):
        raise ValueError(f"unfinished must be 'keep' or 'last', got {unfinished!r}")
    sc = getattr(scores, "score", scores)
    if sc is not None:
        if not isinstance(sc, torch.Tensor) or not sc.dtype.is_floating_point or tuple(sc.shape) != (B, K):
            raise ValueError(f"scores must be a floating-point tensor [B, N] = [{B}, {K}], got "
                             f"{getattr(sc, 'dtype', type(sc))} {tuple(getattr(sc, 'shape', ()))}")
    elif order == "score":
        raise ValueError("order='score' needs scores (pass scores, or order='count' / 'first')")
    if with_logmass is None:
        with_logmass = sc is not None
    if with_logmass and sc is None:
        raise ValueError("with_logmass needs scores")
    if not hyp.is_cuda:
        raise ValueError("fold runs on the GPU and has no CPU fallback: pass device tensors (scoring.unique_samples folds host "
                         "tensors)")
    if sc is not None and sc.device != hyp.device:
        raise ValueError(f"scores are on {sc.device}, hyp on {hyp.device}")
    dev = hyp.device
    if hyp.dtype != torch.int64:
        hyp = hyp.to(torch.int64)
    ld = int(hyp.stride(1)) if K > 1 else (int(hyp.stride(0)) if B > 1 else L)
    if not ((L == 1 or hyp.stride(2) == 1) and ld >= L and (B == 1 or hyp.stride(0) == K * ld) and (K == 1 or hyp.stride(1) == ld)):
        hyp, ld = hyp.contiguous(), L
    if sc is not None:
        sc = sc.detach().to(torch.float32).contiguous()
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    first, rank_of, perm, count, n_unique = i32(B, K), i32(B, K), i32(B, K), i32(B, K), i32(B)
    out_score = torch.empty((B, K), dtype=torch.float32, device=dev)
    pred = torch.empty((B, K, L), dtype=torch.int64, device=dev) if gather else None
    logmass = torch.empty((B,), dtype=torch.float32, device=dev) if with_logmass else None
    flags = (N.TTX_FOLD_UNFINISHED_LAST if unfinished == "last" else 0) | (N.TTX_FOLD_DEBUG_NO_FILTER if debug_no_filter else 0)
    ptr = lambda t: None if t is None else t.data_ptr()
    lib = lib or N.lib()
    with torch.cuda.device(dev):
        N.check(lib.ttx_fold_hypotheses(session, hyp.data_ptr(), B, K, L, ld, int(pad), int(eos), ptr(sc), N.FOLD_ORDERS[order], flags,
                                        first.data_ptr(), rank_of.data_ptr(), n_unique.data_ptr(), perm.data_ptr(), count.data_ptr(),
                                        out_score.data_ptr(), ptr(pred), ptr(logmass),
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return FoldedHypotheses(pred, perm, count, n_unique, first, rank_of, out_score, logmass)


class NativeTransformer:
    # score_hypotheses: decoder positions (rows x columns) of one call; the widest activation buffer takes ff_dim floats per
    # position (256 MiB at ff_dim 2048), and a bench batch of 32 rows x 199 columns still fits one call
    SCORE_MAX_ROWS = 32768

    def __init__(self, state_dict: dict | None, num_heads: int, pad_token_idx: int = 0, device: int | str | torch.device = 0,
                 max_positions: int = 5000, layer_norm_eps: float = 1e-5, shape: dict | None = None, activation: str = "relu"):
        """``state_dict``: the reference's state dict (weights are packed into one HBM blob).  ``state_dict=None`` with
        ``shape`` (see shape_of_state): an EMPTY model of those dimensions whose blob is filled afterwards — the receiving side
        of the one-off weight broadcast (dist.broadcast_model).  ``activation``: the reference's init_arg,
        "relu" or "gelu" (the exact erf GELU); the state dict does not carry it, so it has to be given with the weights."""
        act = N.activation_code(activation)         # ValueError before any GPU call
        self.activation = activation
        if not torch.cuda.is_available():
            raise RuntimeError("NativeTransformer needs an MI355X: the HIP path has no CPU fallback")
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        self.device = dev
        st = _strip(state_dict) if state_dict is not None else None
        dims = shape_of_state(st) if st is not None else dict(shape)
        self.emb_dim, self.src_vocab_size, self.tgt_vocab_size = dims["emb_dim"], dims["src_vocab_size"], dims["tgt_vocab_size"]
        self.ff_dim, self.num_enc_layers, self.num_dec_layers = dims["ff_dim"], dims["num_enc_layers"], dims["num_dec_layers"]
        self.num_heads = int(num_heads)
        self.src_pad_token_i = int(pad_token_idx)
        self.tgt_pad_token_i = int(pad_token_idx)
        self.cfg = N.Config(self.tgt_vocab_size, self.src_vocab_size, self.emb_dim, self.num_heads, self.ff_dim,
                            self.num_enc_layers, self.num_dec_layers, self.src_pad_token_i, int(max_positions),
                            float(layer_norm_eps))
        self._lib = N.lib()
        self._model = C.c_void_p()
        self._session = C.c_void_p()
        # TTX_PROFILE_GEMM=1 at construction makes EVERY session of this model a profiling one (new_session below), not only the
        # first: the slot pools' later sessions are created long after the caller dropped the variable again
        self._profile_sessions = os.environ.get("TTX_PROFILE_GEMM") == "1"
        if st is None:
            N.check(self._lib.ttx_model_create_empty(C.byref(self.cfg), dev.index or 0, C.byref(self._model)))
            N.check(self._lib.ttx_model_set_activation(self._model, act))      # before the first session: sessions bake it in
            N.check(self._lib.ttx_session_create(self._model, C.byref(self._session)))
            return
        host = {k: torch.as_tensor(v).detach().to("cpu", torch.float32).contiguous() for k, v in st.items()}
        host["positional_encoding.pe"] = reference_pe_table(self.emb_dim, max_positions)
        arr = (N.Tensor * len(host))()
        keep = []
        for i, (k, v) in enumerate(host.items()):
            name = k.encode()
            keep.append((name, v))
            arr[i] = N.Tensor(name, C.cast(v.data_ptr(), C.POINTER(C.c_float)), v.numel())
        N.check(self._lib.ttx_model_create(C.byref(self.cfg), arr, len(host), dev.index or 0, C.byref(self._model)))
        N.check(self._lib.ttx_model_set_activation(self._model, act))
        N.check(self._lib.ttx_session_create(self._model, C.byref(self._session)))

    def blob_tensor(self) -> torch.Tensor:
        """The packed weight blob in HBM as a flat fp32 torch tensor sharing the library's memory (ttx_model_blob): every
        tensor of the state dict plus the derived ones (sinusoid table, packed cross-attention K/V projection).  Writing
        the blob of another model of the same shape into it (one RCCL broadcast) makes this model that model."""
        ptr, nbytes = C.c_void_p(), C.c_int64()
        N.check(self._lib.ttx_model_blob(self._model, C.byref(ptr), C.byref(nbytes)))
        with torch.cuda.device(self.device):
            t = torch.as_tensor(_DeviceSpan(int(ptr.value), int(nbytes.value)), device=self.device)
        t._ttx_owner = self              # the tensor borrows the allocation: keep the model alive with it
        return t

    # -- plumbing ------------------------------------------------------------------------------
    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def session(self) -> C.c_void_p:
        return self._session

    def new_session(self) -> C.c_void_p:
        s = C.c_void_p()
        had = os.environ.get("TTX_PROFILE_GEMM")
        if self._profile_sessions:
            os.environ["TTX_PROFILE_GEMM"] = "1"
        try:
            N.check(self._lib.ttx_session_create(self._model, C.byref(s)))
        finally:
            if self._profile_sessions:
                if had is None:
                    os.environ.pop("TTX_PROFILE_GEMM", None)
                else:
                    os.environ["TTX_PROFILE_GEMM"] = had
        return s

    def session_pool(self, n: int) -> list:
        """`n` sessions (the default one first) for several batches in flight; created once, reused."""
        pool = getattr(self, "_pool", None)
        if pool is None:
            pool = self._pool = [self._session]
        while len(pool) < n:
            pool.append(self.new_session())
        return pool[:n]

    def kernel_profile(self) -> dict:
        """GEMM event-pair sums of every session of this model since the last read (ttx_last_kernel_profile; sessions created
        under TTX_PROFILE_GEMM=1): {"gemm_ms", "launches", "pair_overhead_ms"}, and "logit_bias_launches": the k_logit_bias
        launches the sessions have enqueued since they were created (not reset by a read; 0 unless a biased call ran), and
        "syntax_launches": the same count of k_syntax_mask launches (0 unless a syntax-constrained call ran)."""
        ms, n, e = C.c_double(), C.c_int64(), C.c_double()
        tot_ms, tot_n, over, lb, sy = 0.0, 0, [], 0, 0
        for sess in (getattr(self, "_pool", None) or [self._session]):
            lb += int(self._lib.ttx_debug_logit_bias_launches(sess))
            sy += int(self._lib.ttx_debug_syntax_launches(sess))
            N.check(self._lib.ttx_last_kernel_profile(sess, C.byref(ms), C.byref(n), C.byref(e)))
            tot_ms += ms.value
            tot_n += n.value
            if n.value and e.value > 0:
                over.append(e.value)
        return {"gemm_ms": tot_ms, "launches": tot_n, "pair_overhead_ms": float(np.median(over)) if over else 0.0,
                "logit_bias_launches": lb, "syntax_launches": sy}

    # -- kernel-level test entry points --------------------------------------------------------
    @staticmethod
    def _ptr(t: torch.Tensor | None):
        return None if t is None else t.data_ptr()

    def debug_gemm(self, x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, y: torch.Tensor, n: int, k: int,
                   m_max: int, m_live: torch.Tensor | None = None, relu: bool = False, splits: int = 0, slab_stride: int = 0,
                   variant: int = 0, tiling: int = 0, activation: int | None = None) -> int:
        """One GEMM launch on the caller's device tensors (ttx_debug_gemm): ``x`` / ``w`` / ``y`` are 2-D fp32 views whose
        row strides are the leading dimensions (``y``: the first slab), ``m_live`` an int32 device scalar or None.  Returns
        the kernel id the launch dispatched; arguments a kernel cannot take raise TtxError (TTX_ERR_INVALID).  ``activation``
        (0 none, 1 ReLU, 2 exact GELU) goes through ttx_debug_gemm_act and then replaces ``relu``."""
        kid = C.c_int32(0)
        if activation is not None:
            N.check(self._lib.ttx_debug_gemm_act(self._session, x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), self._ptr(bias),
                                                 y.data_ptr(), y.stride(0), self._ptr(m_live), int(m_max), int(n), int(k),
                                                 int(activation), int(splits), int(slab_stride), int(variant), int(tiling),
                                                 C.byref(kid), self._stream()))
            return int(kid.value)
        N.check(self._lib.ttx_debug_gemm(self._session, x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), self._ptr(bias),
                                         y.data_ptr(), y.stride(0), self._ptr(m_live), int(m_max), int(n), int(k), int(relu),
                                         int(splits), int(slab_stride), int(variant), int(tiling), C.byref(kid), self._stream()))
        return int(kid.value)

    def debug_finish_ln(self, slabs: torch.Tensor, n_slabs: int, slab_stride: int, bias: torch.Tensor, resid: torch.Tensor,
                        g1: torch.Tensor, b1: torch.Tensor, g2: torch.Tensor | None, b2: torch.Tensor | None,
                        row_valid: torch.Tensor | None, y: torch.Tensor, m_max: int, d: int, eps: float = 1e-5,
                        m_live: torch.Tensor | None = None) -> None:
        """One finisher launch on the caller's device tensors (ttx_debug_finish_ln): rows are contiguous, ``d`` wide."""
        N.check(self._lib.ttx_debug_finish_ln(self._session, slabs.data_ptr(), int(n_slabs), int(slab_stride), bias.data_ptr(),
                                              resid.data_ptr(), g1.data_ptr(), b1.data_ptr(), self._ptr(g2), self._ptr(b2),
                                              self._ptr(row_valid), y.data_ptr(), self._ptr(m_live), int(m_max), int(d),
                                              float(eps), self._stream()))

    def debug_attn(self, mode: int, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int, scale: float,
                   groups: int, max_keys: int, L: int = 0, Lk: int = 0, tok: torch.Tensor | None = None, pad: int = 0,
                   key_pad: torch.Tensor | None = None, mem_row: torch.Tensor | None = None, act_idx: torch.Tensor | None = None,
                   front: torch.Tensor | None = None, src_of: torch.Tensor | None = None, src_len: torch.Tensor | None = None,
                   kcache: torch.Tensor | None = None, vcache: torch.Tensor | None = None, cache_seq_stride: int = 0,
                   cache_slot: torch.Tensor | None = None, gen_ld: int = 0, n: int = 1, d: int = 0, n_active: int = 0,
                   kernel: int = 0, head_dim: int = 32, choose_as: tuple | None = None) -> int:
        """One attention launch on the caller's device tensors (ttx_debug_attn_hd): ``q`` / ``k`` / ``v`` are 2-D fp32 views whose
        row strides are the leading dimensions (``k`` and ``v`` share theirs), ``out`` has rows of ``head_dim`` * ``heads`` floats
        (``head_dim`` 32 or 64); index and token tensors are int32, ``key_pad`` uint8.  ``kernel``: 0 the production choice,
        1 k_attn, 2 k_attn2, 3 k_attn3, 4 k_attn3s, 5 k_attn1.  Returns the kernel that ran; arguments a kernel cannot take raise TtxError
        (TTX_ERR_INVALID).  ``choose_as`` = (n, d): a step launch that chooses between k_attn2 and k_attn as a launch in that
        layout does (ttx_debug_attn_as: the probe of the two-phase verify step)."""
        kid = C.c_int32(0)
        assert k.stride(0) == v.stride(0)
        if choose_as is not None:
            N.check(self._lib.ttx_debug_attn_as(self._session, q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0),
                                                out.data_ptr(), int(heads), int(head_dim), float(scale), int(L), int(Lk), self._ptr(tok),
                                                int(pad), self._ptr(key_pad), self._ptr(mem_row), self._ptr(act_idx), self._ptr(front),
                                                self._ptr(src_of), self._ptr(src_len), self._ptr(kcache), self._ptr(vcache),
                                                int(cache_seq_stride), self._ptr(cache_slot), int(gen_ld), int(n), int(d), int(mode),
                                                int(groups), int(n_active), int(max_keys), int(kernel), C.byref(kid),
                                                int(choose_as[0]), int(choose_as[1]), self._stream()))
            return int(kid.value)
        N.check(self._lib.ttx_debug_attn_hd(self._session, q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0),
                                            out.data_ptr(), int(heads), int(head_dim), float(scale), int(L), int(Lk), self._ptr(tok),
                                            int(pad), self._ptr(key_pad), self._ptr(mem_row), self._ptr(act_idx), self._ptr(front),
                                            self._ptr(src_of), self._ptr(src_len), self._ptr(kcache), self._ptr(vcache),
                                            int(cache_seq_stride), self._ptr(cache_slot), int(gen_ld), int(n), int(d), int(mode),
                                            int(groups), int(n_active), int(max_keys), int(kernel), C.byref(kid), self._stream()))
        return int(kid.value)

    def debug_attn_probs(self, q: torch.Tensor, k: torch.Tensor, key_pad: torch.Tensor, length: torch.Tensor, heads: int,
                         head_dim: int, T: int, Ls: int, scale: float, mem_row: torch.Tensor | None = None,
                         out_heads: torch.Tensor | None = None, out_mean: torch.Tensor | None = None,
                         out_align: torch.Tensor | None = None) -> None:
        """One k_attn_probs launch on the caller's device tensors (ttx_debug_attn_probs): ``q`` [R*T, >= heads*head_dim] and
        ``k`` [Rm*Ls, >= heads*head_dim] are 2-D fp32 views whose row strides are the leading dimensions, ``key_pad`` uint8
        [Rm*Ls], ``length`` int32 [R], ``mem_row`` int32 [R] or None; the outputs are written in place: ``out_heads``
        fp32 [R, heads, T, Ls], ``out_mean`` fp32 [R, T, Ls], ``out_align`` int32 [R, T], each optional."""
        R, Rm = int(length.numel()), int(key_pad.numel()) // int(Ls)
        N.check(self._lib.ttx_debug_attn_probs(self._session, q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), key_pad.data_ptr(),
                                               self._ptr(mem_row), length.data_ptr(), R, Rm, int(heads), int(head_dim), int(T), int(Ls),
                                               float(scale), self._ptr(out_heads), self._ptr(out_mean), self._ptr(out_align),
                                               self._stream()))

    @staticmethod
    def score_batch_table(batches: list):
        """The ttx_score_batch array of ``batches``: (src, hyp, N, W) per batch with ``src`` int64 [B, Ls] contiguous and ``hyp``
        int64 [B*N, >= W] whose row stride is ld_hyp (a view is fine); device tensors, borrowed."""
        table = (N.ScoreBatch * len(batches))()
        for i, (src, hyp, K, W) in enumerate(batches):
            assert src.is_contiguous() and hyp.stride(1) == 1 and hyp.shape[0] == src.shape[0] * K
            table[i] = N.ScoreBatch(src.data_ptr(), hyp.data_ptr(), int(src.shape[0]), int(src.shape[1]), int(K), int(W), int(hyp.stride(0)))
        return table

    def debug_score_list(self, op: str, batches: list, sel=None, tok_off=None, n: int = 0, w: int = 0, ls: int = 0, eos: int = 2,
                         **arrays) -> None:
        """ONE launch of k_sl_extents / k_sl_pack / k_sl_unpack (``op``: "extents", "pack", "unpack") on the caller's device
        tensors (ttx_debug_score_list).  ``batches`` as ``score_batch_table`` takes them; ``sel``: the chunk's sources (indices in
        list order), ``n`` / ``w`` / ``ls`` the chunk's rows per source and widths; ``tok_off``: per batch its offset into
        ``d_tok_logp``, in floats; ``arrays``: the fields of ttx_debug_score_list_args by name (``d_e=...``), tensors or None."""
        a = N.DebugScoreListArgs(N=int(n), W=int(w), Ls=int(ls), eos=int(eos), **{k: self._ptr(v) for k, v in arrays.items()})
        h_sel = None if sel is None else (C.c_int32 * len(sel))(*[int(x) for x in sel])
        h_off = None if tok_off is None else (C.c_int64 * len(tok_off))(*[int(x) for x in tok_off])
        N.check(self._lib.ttx_debug_score_list(self._scoring_session(), N.DEBUG_SCORE_LIST_OPS.index(op), self.score_batch_table(batches),
                                               len(batches), h_sel, 0 if sel is None else len(sel), h_off, C.byref(a), self._stream()))

    @staticmethod
    def attn_probs_key_limit(head_dim: int) -> int:
        """The longest source ``attention_maps`` takes at ``head_dim`` (ttx_attn_probs_key_limit; a host query)."""
        return int(N.lib().ttx_attn_probs_key_limit(int(head_dim)))

    def debug_argmax(self, logits: torch.Tensor, pred: torch.Tensor, m_max: int, m_live: torch.Tensor | None = None) -> None:
        """One k_argmax launch (ttx_debug_argmax): ``logits`` fp32 [m_max, V] contiguous, ``pred`` int32 [m_max], ``m_live`` an
        int32 device scalar or None."""
        N.check(self._lib.ttx_debug_argmax(self._session, logits.data_ptr(), int(logits.shape[1]), pred.data_ptr(),
                                           self._ptr(m_live), int(m_max), self._stream()))

    def debug_logit_bias(self, logits: torch.Tensor, bias: torch.Tensor, src: torch.Tensor | None = None, m_live: torch.Tensor | None = None,
                         rows_per_src: int = 1, act_idx: torch.Tensor | None = None, row_map: torch.Tensor | None = None, n: int = 1,
                         d: int = 0) -> None:
        """ONE launch of k_logit_bias, in place on ``logits`` (a float32 device tensor [M, V] whose rows are contiguous; a view
        with a 4-byte aligned base is fine) with ``bias`` float32 [sources, ld >= V] (row stride ``bias.stride(0)``).  Plain mapping
        (``act_idx`` None): ``src`` int32 [M] or ``rows_per_src``; step layout: ``act_idx``, ``src`` by decoder row, ``row_map`` or
        None, ``n`` drafts of ``d`` tokens.  ``m_live``: int32 [1] on the device, the live rows."""
        M, V = logits.shape
        assert logits.stride(1) == 1 and logits.stride(0) == V and bias.stride(1) == 1
        N.check(self._lib.ttx_debug_logit_bias(self.session, logits.data_ptr(), V, M, self._ptr(m_live), bias.data_ptr(),
                                               int(bias.stride(0)), self._ptr(src), rows_per_src, self._ptr(act_idx), self._ptr(row_map),
                                               n, d, self._stream()))

    def debug_syntax_mask(self, logits: torch.Tensor, cls: torch.Tensor, max_len: int, eos: int, tok: torch.Tensor,
                          front: torch.Tensor | None = None, m_live: torch.Tensor | None = None, act_idx: torch.Tensor | None = None,
                          row_map: torch.Tensor | None = None, drafts: torch.Tensor | None = None, n: int = 1, d: int = 0,
                          t: int = 0) -> None:
        """ONE launch of k_syntax_mask, in place on ``logits`` (a float32 device tensor [M, V] whose rows are contiguous) with the
        int8 class table ``cls`` [V].  Plain mapping (``act_idx`` None, ``t`` 0): ``tok`` int32 [M, ld], ``front`` int32 [1].  Step
        layout (``act_idx`` set): ``tok`` int32 [B, ld], ``front`` int32 [B], ``row_map`` or None, ``drafts`` int32 [B, n, d].
        Teacher-forced (``t`` > 0): ``tok`` int64 [M / t, ld].  ``m_live``: int32 [1] on the device, the live rows."""
        M, V = logits.shape
        assert logits.stride(1) == 1 and logits.stride(0) == V and tok.stride(1) == 1 and cls.dtype == torch.int8 and cls.numel() >= V
        mode = 2 if t > 0 else 1 if act_idx is not None else 0
        assert tok.dtype == (torch.int64 if mode == 2 else torch.int32)
        N.check(self._lib.ttx_debug_syntax_mask(self.session, mode, logits.data_ptr(), V, M, self._ptr(m_live), cls.data_ptr(),
                                                int(max_len), int(eos), tok.data_ptr(), int(tok.stride(0)), self._ptr(front),
                                                self._ptr(act_idx), self._ptr(row_map), self._ptr(drafts), int(n), int(d), int(t),
                                                self._stream()))

    def debug_sample(self, logits: torch.Tensor, key: torch.Tensor, sample: torch.Tensor, done: torch.Tensor, front: torch.Tensor,
                     pred: torch.Tensor, m_max: int, m_live: torch.Tensor | None = None, *, temperature: float = 1.0, top_k: int = 0,
                     top_p: float = 1.0, pad: int = 0, eos: int = 2, seed: int = 0) -> None:
        """One k_sample launch (ttx_debug_sample): ``logits`` fp32 [m_max, V] contiguous, ``key`` int64 [m_max] (read as
        uint64), ``sample`` int32 [m_max] (read as uint32), ``done`` int32 [m_max] (read and written), ``front`` int32 [1],
        ``pred`` int32 [m_max], ``m_live`` an int32 device scalar or None."""
        p = N.SampleParams(1, 1, float(temperature), int(top_k), float(top_p), int(pad), 0, int(eos), int(seed) & 0xFFFFFFFFFFFFFFFF)
        N.check(self._lib.ttx_debug_sample(self._session, logits.data_ptr(), int(logits.shape[1]), key.data_ptr(), sample.data_ptr(),
                                           done.data_ptr(), front.data_ptr(), pred.data_ptr(), self._ptr(m_live), int(m_max),
                                           C.byref(p), self._stream()))

    def debug_sample_step(self, logits: torch.Tensor, key: torch.Tensor, sample: torch.Tensor, act_idx: torch.Tensor,
                          front: torch.Tensor, pred: torch.Tensor, *, B: int, n: int, d: int, n_active: int,
                          m_live: torch.Tensor | None = None, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                          pad: int = 0, eos: int = 2, seed: int = 0) -> None:
        """One k_sample_step launch (ttx_debug_sample_step): ``logits`` fp32 [B * (1 + n*d), V] contiguous in the step-row layout,
        ``key`` int64 [B] (read as uint64) and ``sample`` int32 [B] (read as uint32) by decoder row, ``act_idx`` / ``front`` int32
        [B], ``pred`` int32 [B * (1 + n*d)], ``m_live`` an int32 device scalar or None."""
        p = N.SampleParams(1, 1, float(temperature), int(top_k), float(top_p), int(pad), 0, int(eos), int(seed) & 0xFFFFFFFFFFFFFFFF)
        N.check(self._lib.ttx_debug_sample_step(self._session, logits.data_ptr(), int(logits.shape[1]), key.data_ptr(),
                                                sample.data_ptr(), act_idx.data_ptr(), front.data_ptr(), int(B), int(n), int(d),
                                                int(n_active), pred.data_ptr(), self._ptr(m_live), C.byref(p), self._stream()))

    def debug_embed(self, table: torch.Tensor, pe: torch.Tensor, x: torch.Tensor, tok: torch.Tensor | None = None, rows: int = 0,
                    L: int = 0, act_idx: torch.Tensor | None = None, front: torch.Tensor | None = None,
                    gen: torch.Tensor | None = None, drafts: torch.Tensor | None = None, B: int = 0, n: int = 1, d: int = 0,
                    n_active: int = 0, step: bool = False) -> None:
        """One k_embed launch (ttx_debug_embed) on the caller's tables: full mode takes ``tok`` int32 [rows] and ``L``, step mode
        ``act_idx`` / ``front`` int32 [B], ``gen`` int32 [B, gen_ld], ``drafts`` int32 [B, n, d] and ``n_active``."""
        N.check(self._lib.ttx_debug_embed(self._session, table.data_ptr(), int(table.shape[0]), pe.data_ptr(), int(pe.shape[0]),
                                          int(table.shape[1]), x.data_ptr(), self._ptr(tok), int(rows), int(L), self._ptr(act_idx),
                                          self._ptr(front), self._ptr(gen), 0 if gen is None else int(gen.stride(0)),
                                          self._ptr(drafts), int(B), int(n), int(d), int(n_active), int(bool(step)), self._stream()))

    def debug_accept(self, state, *, B: int, n: int, d: int, Ls: int, max_len: int, pad: int, bos: int, eos: int, gen_ld: int,
                     greedy: bool = False, threads: int = 0, row_rule: bool = False, pool: bool = False, traj_ld: int = 0,
                     pool_rows: int = 0, _entry: str = "ttx_debug_accept", **arrays) -> list:
        """One k_accept (``greedy``: k_greedy_accept) launch (ttx_debug_accept).  ``state``: the 13 entry words of the DecState
        (include/ttx.h); ``arrays``: device tensors named as the fields of ttx_debug_accept_args without the ``d_`` prefix.
        Returns the 17 exit words: the DecState the kernel left and the four words it published for the host."""
        a = N.DebugAcceptArgs()
        for name, _ in N.DebugAcceptArgs._fields_[:15]:
            t = arrays.pop(name[2:], None)
            setattr(a, name, None if t is None else t.data_ptr())
        assert not arrays, f"unknown operands {sorted(arrays)}"
        a.gen_ld, a.traj_ld, a.pool_rows, a.row_rule, a.pool = int(gen_ld), int(traj_ld), int(pool_rows), int(row_rule), int(pool)
        a.B, a.N, a.D, a.Ls, a.max_len, a.pad, a.bos, a.eos = int(B), int(n), int(d), int(Ls), int(max_len), int(pad), int(bos), int(eos)
        a.greedy, a.threads = int(greedy), int(threads)
        words = (C.c_int64 * N.DEBUG_ACCEPT_STATE_WORDS)(*[int(v) for v in state], *([0] * (N.DEBUG_ACCEPT_STATE_WORDS - len(state))))
        N.check(getattr(self._lib, _entry)(self._session, C.byref(a), words, self._stream()))
        return [int(v) for v in words]

    def debug_sample_accept(self, state, *, B: int, n: int, d: int, Ls: int, max_len: int, pad: int, bos: int, eos: int, gen_ld: int,
                            threads: int = 0, **arrays) -> list:
        """One k_sample_accept launch (ttx_debug_sample_accept), the accept step of speculative sampling: ``debug_accept``'s
        ``state``, exit words and ``arrays`` (act_idx, front, gen, drafts, pred, rec, out, and haspad holding zeros)."""
        return self.debug_accept(state, B=B, n=n, d=d, Ls=Ls, max_len=max_len, pad=pad, bos=bos, eos=eos, gen_ld=gen_ld,
                                 threads=threads, _entry="ttx_debug_sample_accept", **arrays)

    def debug_sample_step_select(self, logits: torch.Tensor, key: torch.Tensor, sample: torch.Tensor, act_idx: torch.Tensor,
                                 front: torch.Tensor, pred: torch.Tensor, *, B: int, n: int, d: int, n_active: int, n_rows: int,
                                 row_map: torch.Tensor | None = None, m_live: torch.Tensor | None = None, temperature: float = 1.0,
                                 top_k: int = 0, top_p: float = 1.0, pad: int = 0, eos: int = 2, seed: int = 0) -> None:
        """One k_sample_step launch as a pass of the slot pool runs it (ttx_debug_sample_step_select): ``debug_sample_step``'s
        operands with ``logits`` [n_rows, V] and ``pred`` [n_rows] stored compacted and ``row_map`` int32 [n_rows] (None: the
        identity); the probe layout n = 1, d = 0 is accepted."""
        p = N.SampleParams(1, 1, float(temperature), int(top_k), float(top_p), int(pad), 0, int(eos), int(seed) & 0xFFFFFFFFFFFFFFFF)
        N.check(self._lib.ttx_debug_sample_step_select(self._session, logits.data_ptr(), int(logits.shape[1]), key.data_ptr(),
                                                       sample.data_ptr(), act_idx.data_ptr(), front.data_ptr(), int(B), int(n), int(d),
                                                       int(n_active), pred.data_ptr(), self._ptr(m_live), C.byref(p),
                                                       self._ptr(row_map), int(n_rows), self._stream()))

    @staticmethod
    def _debug_prefix(tok: torch.Tensor, length: torch.Tensor, src: torch.Tensor) -> N.DebugPrefix:
        """ttx_debug_prefix of the forced prefixes ``tok`` int32 [sources, ld], ``length`` int32 [rows], ``src`` int32 [rows]."""
        return N.DebugPrefix(tok.data_ptr(), int(tok.shape[1]), int(tok.shape[0]), length.data_ptr(), src.data_ptr())

    def debug_prefix_drafts(self, act_idx: torch.Tensor, front: torch.Tensor, drafts: torch.Tensor, draft0: torch.Tensor, *,
                            prefix_tok: torch.Tensor, prefix_len: torch.Tensor, prefix_src: torch.Tensor, n_active: int,
                            eos: int = 2, pad: int = 0, replace: int = 3) -> None:
        """One k_prefix_drafts launch (ttx_debug_prefix_drafts): ``act_idx`` / ``front`` int32 [B], ``drafts`` int32 [B, n, d]
        (draft 0 of the active rows is rewritten), ``draft0`` int32 [B, d], the prefix table int32 [sources, ld] with the rows'
        lengths and sources int32 [B]."""
        B, n, d = drafts.shape
        x = self._debug_prefix(prefix_tok, prefix_len, prefix_src)
        N.check(self._lib.ttx_debug_prefix_drafts(self._session, act_idx.data_ptr(), front.data_ptr(), int(B), int(n), int(d),
                                                  int(n_active), drafts.data_ptr(), draft0.data_ptr(), C.byref(x), int(eos), int(pad),
                                                  int(replace), self._stream()))

    def debug_proposal_drafts(self, act_idx: torch.Tensor, front: torch.Tensor, gen: torch.Tensor, drafts: torch.Tensor,
                              draft0: torch.Tensor, *, proposal_tok: torch.Tensor, proposal_len: torch.Tensor,
                              proposal_src: torch.Tensor, n_active: int, ctx: int = 2, bos: int = 1, eos: int = 2, pad: int = 0,
                              replace: int = 3) -> None:
        """One k_proposal_drafts launch (ttx_debug_proposal_drafts): ``act_idx`` / ``front`` int32 [B], ``gen`` int32 [B, gen_ld]
        the rows' tokens, ``drafts`` int32 [B, n, d] (draft 0 of the active rows is rewritten), ``draft0`` int32 [B, d], the
        proposal table int32 [sources, ld] with the rows' lengths and sources int32 [B]."""
        B, n, d = drafts.shape
        x = self._debug_prefix(proposal_tok, proposal_len, proposal_src)
        N.check(self._lib.ttx_debug_proposal_drafts(self._session, act_idx.data_ptr(), front.data_ptr(), gen.data_ptr(),
                                                    int(gen.shape[1]), int(B), int(n), int(d), int(n_active), drafts.data_ptr(),
                                                    draft0.data_ptr(), C.byref(x), int(ctx), int(bos), int(eos), int(pad),
                                                    int(replace), self._stream()))

    def debug_sample_prefix(self, logits: torch.Tensor, key: torch.Tensor, sample: torch.Tensor, done: torch.Tensor,
                            front: torch.Tensor, pred: torch.Tensor, m_max: int, m_live: torch.Tensor | None = None, *,
                            prefix_tok: torch.Tensor, prefix_len: torch.Tensor, prefix_src: torch.Tensor, temperature: float = 1.0,
                            top_k: int = 0, top_p: float = 1.0, pad: int = 0, eos: int = 2, seed: int = 0) -> None:
        """``debug_sample`` with forced prefixes (ttx_debug_sample_prefix): the table and the rows' lengths and sources [m_max]."""
        p = N.SampleParams(1, 1, float(temperature), int(top_k), float(top_p), int(pad), 0, int(eos), int(seed) & 0xFFFFFFFFFFFFFFFF)
        x = self._debug_prefix(prefix_tok, prefix_len, prefix_src)
        N.check(self._lib.ttx_debug_sample_prefix(self._session, logits.data_ptr(), int(logits.shape[1]), key.data_ptr(),
                                                  sample.data_ptr(), done.data_ptr(), front.data_ptr(), pred.data_ptr(),
                                                  self._ptr(m_live), int(m_max), C.byref(p), C.byref(x), self._stream()))

    def debug_sample_step_prefix(self, logits: torch.Tensor, key: torch.Tensor, sample: torch.Tensor, act_idx: torch.Tensor,
                                 front: torch.Tensor, pred: torch.Tensor, *, B: int, n: int, d: int, n_active: int, n_rows: int,
                                 prefix_tok: torch.Tensor, prefix_len: torch.Tensor, prefix_src: torch.Tensor,
                                 row_map: torch.Tensor | None = None, m_live: torch.Tensor | None = None, temperature: float = 1.0,
                                 top_k: int = 0, top_p: float = 1.0, pad: int = 0, eos: int = 2, seed: int = 0) -> None:
        """``debug_sample_step_select`` with forced prefixes (ttx_debug_sample_step_prefix): the table and the decoder rows' lengths
        and sources [B]."""
        p = N.SampleParams(1, 1, float(temperature), int(top_k), float(top_p), int(pad), 0, int(eos), int(seed) & 0xFFFFFFFFFFFFFFFF)
        x = self._debug_prefix(prefix_tok, prefix_len, prefix_src)
        N.check(self._lib.ttx_debug_sample_step_prefix(self._session, logits.data_ptr(), int(logits.shape[1]), key.data_ptr(),
                                                       sample.data_ptr(), act_idx.data_ptr(), front.data_ptr(), int(B), int(n), int(d),
                                                       int(n_active), pred.data_ptr(), self._ptr(m_live), C.byref(p),
                                                       self._ptr(row_map), int(n_rows), C.byref(x), self._stream()))

    def debug_sample_accept_pool(self, state, *, B: int, n: int, d: int, Ls: int, max_len: int, pad: int, bos: int, eos: int,
                                 gen_ld: int, pool_rows: int, traj_ld: int = 1, threads: int = 0, spread: bool = False,
                                 exec_rows: torch.Tensor | None = None, **arrays) -> list:
        """The accept step of the sampling pool (ttx_debug_sample_accept_pool): ``debug_accept``'s ``state`` and exit words;
        ``arrays``: act_idx, front, gen, drafts, pred, rec, haspad (zeros), row_of and pool_out.  ``spread``: the pair
        k_sample_accept_slots + k_accept_finish instead of one k_sample_accept launch; ``exec_rows``: an int32 device scalar."""
        a = N.DebugAcceptArgs()
        for name, _ in N.DebugAcceptArgs._fields_[:15]:
            t = arrays.pop(name[2:], None)
            setattr(a, name, None if t is None else t.data_ptr())
        assert not arrays, f"unknown operands {sorted(arrays)}"
        a.gen_ld, a.traj_ld, a.pool_rows, a.row_rule, a.pool = int(gen_ld), int(traj_ld), int(pool_rows), 1, 1
        a.B, a.N, a.D, a.Ls, a.max_len, a.pad, a.bos, a.eos = int(B), int(n), int(d), int(Ls), int(max_len), int(pad), int(bos), int(eos)
        a.greedy, a.threads = 0, int(threads)
        words = (C.c_int64 * N.DEBUG_ACCEPT_STATE_WORDS)(*[int(v) for v in state], *([0] * (N.DEBUG_ACCEPT_STATE_WORDS - len(state))))
        N.check(self._lib.ttx_debug_sample_accept_pool(self._session, C.byref(a), words, self._ptr(exec_rows), int(bool(spread)),
                                                       self._stream()))
        return [int(v) for v in words]

    def debug_pool_fill_sample(self, *, B: int, n: int, d: int, n_active: int, n_sources: int, per_src: int, first_src: int, Ls_new: int,
                               Ls_cap: int, gen_ld: int, kv_row: int, max_len: int, out_rows: int, bos: int, pad: int, **arrays) -> dict:
        """One admission of the sampling pool (ttx_debug_pool_fill_sample); ``arrays``: device tensors named as the pointer fields
        of ttx_debug_pool_fill_args without the ``d_`` prefix (row_keys may be absent).  Returns n_active, m_rows, error and the
        n_active word published for the host."""
        a = N.DebugPoolFillArgs()
        for name in N.DebugPoolFillArgs.POINTERS:
            t = arrays.pop(name[2:], None)
            setattr(a, name, None if t is None else t.data_ptr())
        assert not arrays, f"unknown operands {sorted(arrays)}"
        for name, v in dict(B=B, N=n, D=d, n_active=n_active, n_sources=n_sources, per_src=per_src, first_src=first_src, Ls_new=Ls_new,
                            Ls_cap=Ls_cap, gen_ld=gen_ld, kv_row=kv_row, max_len=max_len, out_rows=out_rows, bos=bos, pad=pad).items():
            setattr(a, name, int(v))
        res = (C.c_int32 * 4)()
        N.check(self._lib.ttx_debug_pool_fill_sample(self._session, C.byref(a), res, self._stream()))
        return dict(zip(("n_active", "m_rows", "error", "host_n_active"), (int(v) for v in res)))

    def debug_accept_block(self) -> list:
        """The int32 words of the session's AcceptBlk (ttx_debug_accept_block): all zero between accept steps."""
        words = (C.c_int32 * N.DEBUG_ACCEPT_BLOCK_WORDS)()
        N.check(self._lib.ttx_debug_accept_block(self._session, words, N.DEBUG_ACCEPT_BLOCK_WORDS, self._stream()))
        return [int(v) for v in words]

    # the beam family, one launch each (include/ttx.h: ttx_debug_bs_prep .. ttx_debug_tree_cache)
    def _debug_beam(self, struct, entry, scalars: dict, arrays: dict, *extra):
        """Fill ``struct`` (a ttx_debug_*_args of _native.py) from int scalars and device tensors named as its fields without
        the ``d_`` prefix (None or absent: a null pointer), and call ``entry``."""
        a = struct()
        for name in struct.POINTERS:
            t = arrays.pop(name[2:], None)
            setattr(a, name, None if t is None else t.data_ptr())
        assert not arrays, f"unknown operands {sorted(arrays)}"
        for name, v in scalars.items():
            setattr(a, name, int(v))
        N.check(entry(self._session, C.byref(a), *extra, self._stream()))

    def debug_bs_prep(self, *, ld: int, max_cand: int, n_cand: int, beam: int, dl: int, n: int, pad: int, smart: bool = False,
                      n_lib: int = 0, lib_ld: int = 0, D0: int = 0, **arrays) -> None:
        """One k_bs_prep launch (ttx_debug_bs_prep)."""
        self._debug_beam(N.DebugBsPrepArgs, self._lib.ttx_debug_bs_prep,
                         dict(ld=ld, max_cand=max_cand, n_cand=n_cand, beam=beam, dl=dl, N=n, pad=pad, smart=smart, n_lib=n_lib,
                              lib_ld=lib_ld, D0=D0), arrays)

    def debug_bs_list(self, counters, *, n_cand: int, n: int, dl: int, **arrays) -> list:
        """One k_bs_list launch (ttx_debug_bs_list) on the 8 entry words of the BeamCounters image.  Returns 21 words: the
        counters as the kernel left them, then the DecState it wrote."""
        words = (C.c_int64 * N.DEBUG_BS_LIST_WORDS)(*[int(v) for v in counters], *([0] * (N.DEBUG_BS_LIST_WORDS - len(counters))))
        self._debug_beam(N.DebugBsListArgs, self._lib.ttx_debug_bs_list, dict(n_cand=n_cand, N=n, dl=dl), arrays, words)
        return [int(v) for v in words]

    def debug_bs_hits(self, *, V: int, max_cand: int, n_cand: int, n: int, dl: int, K: int, vpl: int = 0, **arrays) -> None:
        """One k_bs_hits launch (ttx_debug_bs_hits); ``vpl`` 0 is the production choice by V."""
        self._debug_beam(N.DebugBsHitsArgs, self._lib.ttx_debug_bs_hits,
                         dict(V=V, max_cand=max_cand, n_cand=n_cand, N=n, dl=dl, K=K, vpl=vpl), arrays)

    def debug_bs_leaves(self, *, V: int, max_cand: int, n_cand: int, n: int, dl: int, K: int, bos: int, pad: int, smart: bool = False,
                        max_group: int = 0, vpl: int = 0, **arrays) -> None:
        """One k_bs_leaves launch (ttx_debug_bs_leaves)."""
        self._debug_beam(N.DebugBsLeavesArgs, self._lib.ttx_debug_bs_leaves,
                         dict(V=V, max_cand=max_cand, n_cand=n_cand, N=n, dl=dl, K=K, bos=bos, pad=pad, smart=smart,
                              max_group=max_group, vpl=vpl), arrays)

    def debug_beam_select(self, *, width: int, ld_in: int, ld_out: int, B: int, beam: int, dl: int, K: int, pad: int, eos: int,
                          **arrays) -> None:
        """One k_beam_select<int> launch (ttx_debug_beam_select)."""
        self._debug_beam(N.DebugBeamSelectArgs, self._lib.ttx_debug_beam_select,
                         dict(width=width, ld_in=ld_in, ld_out=ld_out, B=B, beam=beam, dl=dl, K=K, pad=pad, eos=eos), arrays)

    def debug_beam_step(self, *, V: int, ld: int, width: int, B: int, beam: int, K: int, pad: int, eos: int, **arrays) -> None:
        """One k_beam_step launch (ttx_debug_beam_step)."""
        self._debug_beam(N.DebugBeamStepArgs, self._lib.ttx_debug_beam_step,
                         dict(V=V, ld=ld, width=width, B=B, beam=beam, K=K, pad=pad, eos=eos), arrays)

    def debug_beam_step_masked(self, *, V: int, ld: int, width: int, B: int, beam: int, K: int, pad: int, eos: int, pfx_tok=None,
                               pfx_len=None, pfx_src=None, pfx_ld: int = 0, pfx_sources: int = 0, **arrays) -> None:
        """One k_beam_step_masked launch (ttx_debug_beam_step_masked): debug_beam_step's operands and optionally the prefix table by
        source (``pfx_tok`` int32 [pfx_sources, pfx_ld], ``pfx_len`` / ``pfx_src`` int32 [B])."""
        pfx = None
        if pfx_tok is not None or pfx_len is not None or pfx_src is not None:
            pfx = C.byref(N.DebugPrefix(self._ptr(pfx_tok), int(pfx_ld), int(pfx_sources), self._ptr(pfx_len), self._ptr(pfx_src)))
        self._debug_beam(N.DebugBeamStepArgs, self._lib.ttx_debug_beam_step_masked,
                         dict(V=V, ld=ld, width=width, B=B, beam=beam, K=K, pad=pad, eos=eos), arrays, pfx)

    def debug_beam_step_masked_launches(self) -> int:
        """k_beam_step_masked launches this model's session has enqueued from the beam loop (ttx_debug_beam_step_masked_launches)."""
        return int(self._lib.ttx_debug_beam_step_masked_launches(self._session))

    def debug_sbs_step(self, *, V: int, ld: int, width: int, B: int, beam: int, K: int, pad: int, eos: int, pos: int, seed: int,
                       inv_T: float, **arrays) -> None:
        """One k_sbs_step launch (ttx_debug_sbs_step): the operands of debug_beam_step with ``phi``, ``g``, ``key`` (absent: keys
        0..B-1), ``new_phi``, ``new_g`` and optionally the four ``tr_*`` trace arrays."""
        a = self._sbs_step_args(arrays, dict(V=V, ld=ld, width=width, B=B, beam=beam, K=K, pad=pad, eos=eos, pos=pos), seed, inv_T)
        N.check(self._lib.ttx_debug_sbs_step(self._session, C.byref(a), self._stream()))

    @staticmethod
    def _sbs_step_args(arrays: dict, scalars: dict, seed: int, inv_T: float):
        a = N.DebugSbsStepArgs()
        for name in a.POINTERS:
            t = arrays.pop(name[2:], None)
            setattr(a, name, None if t is None else t.data_ptr())
        assert not arrays, f"unknown operands {sorted(arrays)}"
        for name, v in scalars.items():
            setattr(a, name, int(v))
        a.seed, a.inv_T = int(seed) & 0xFFFFFFFFFFFFFFFF, float(inv_T)
        return a

    def debug_sbs_step_ex(self, *, V: int, ld: int, width: int, B: int, beam: int, K: int, pad: int, eos: int, pos: int, seed: int,
                          inv_T: float, top_k: int = 0, top_p: float = 1.0, waves: int = 0, pfx_tok=None, pfx_len=None, pfx_src=None,
                          pfx_ld: int = 0, pfx_sources: int = 0, **arrays) -> None:
        """One k_sbs_step_masked launch (ttx_debug_sbs_step_ex): debug_sbs_step's operands, the filter, ``waves`` (0: the production
        choice) and optionally the prefix table by source (``pfx_tok`` int32 [pfx_sources, pfx_ld], ``pfx_len`` / ``pfx_src`` int32 [B])."""
        a = self._sbs_step_args(arrays, dict(V=V, ld=ld, width=width, B=B, beam=beam, K=K, pad=pad, eos=eos, pos=pos), seed, inv_T)
        pfx = None
        if pfx_tok is not None or pfx_len is not None or pfx_src is not None:
            pfx = C.byref(N.DebugPrefix(self._ptr(pfx_tok), int(pfx_ld), int(pfx_sources), self._ptr(pfx_len), self._ptr(pfx_src)))
        N.check(self._lib.ttx_debug_sbs_step_ex(self._session, C.byref(a), int(top_k), float(top_p), pfx, int(waves), self._stream()))

    def debug_tree_cache(self, *, max_cand: int, layers: int, prev_n: int, prev_d: int, d: int, cache_layer_stride: int,
                         cache_seq_stride: int, qkv_layer_stride: int, **arrays) -> None:
        """One k_tree_cache launch (ttx_debug_tree_cache); ``slot_parent`` / ``slot_self`` absent: two buffers."""
        self._debug_beam(N.DebugTreeCacheArgs, self._lib.ttx_debug_tree_cache,
                         dict(max_cand=max_cand, layers=layers, prev_N=prev_n, prev_D=prev_d, d=d, cache_layer_stride=cache_layer_stride,
                              cache_seq_stride=cache_seq_stride, qkv_layer_stride=qkv_layer_stride), arrays)

    def debug_bsp(self, op: str, words, *, C_: int, K: int, n: int, D0: int, Ls_cap: int, max_len: int, ld: int, smart: bool, lib_ld: int,
                  pad: int, bos: int, eos: int, repl: int, max_steps: int, T_cap: int, R: int = 0, first_row: int = 0, kv_row: int = 0,
                  Ls_new: int = 0, **arrays) -> list:
        """One launch of a bookkeeping kernel of the beam-speculative batch pool (ttx_debug_bsp); ``op`` one of
        _native.DEBUG_BSP_OPS, ``C_`` the pool's source slots.  ``words``: the 8 BeamCounters words and the 4 BeamPoolHost words
        on entry; returns the 12 as the kernel left them."""
        w = (C.c_int64 * N.DEBUG_BSP_WORDS)(*[int(v) for v in words])
        scalars = dict(C=C_, K=K, N=n, D0=D0, Ls_cap=Ls_cap, max_len=max_len, ld=ld, smart=smart, lib_ld=lib_ld, pad=pad, bos=bos, eos=eos,
                       repl=repl, max_steps=max_steps, T_cap=T_cap, R=R, first_row=first_row, kv_row=kv_row, Ls_new=Ls_new)
        a = N.DebugBspArgs()
        for name in N.DebugBspArgs.POINTERS:
            t = arrays.pop(name[2:], None)
            setattr(a, name, None if t is None else t.data_ptr())
        assert not arrays, f"unknown operands {sorted(arrays)}"
        for name, v in scalars.items():
            setattr(a, name, int(v))
        code = op if isinstance(op, int) else N.DEBUG_BSP_OPS.index(op)
        N.check(self._lib.ttx_debug_bsp(self._session, code, C.byref(a), w, self._stream()))
        return [int(v) for v in w]

    def debug_sbs_step_pool(self, *, V: int, ld: int, C_: int, K: int, pad: int, eos: int, seed: int, inv_T: float, masked: bool = False,
                            top_k: int = 0, top_p: float = 1.0, pfx_tok=None, pfx_len=None, pfx_src=None, pfx_ld: int = 0,
                            pfx_sources: int = 0, **arrays) -> None:
        """One k_sbs_step_pool (``masked`` false) or k_sbs_step_pool_masked launch (ttx_debug_sbs_step_pool) over ``C_`` slots:
        candidate arrays [C_ * K], slot arrays ``row_of``, ``level``, ``nlive``, ``key``, ``nfin`` [C_]; the prefix table by slot."""
        a = N.DebugSbsStepPoolArgs()
        for name in a.POINTERS:
            t = arrays.pop(name[2:], None)
            setattr(a, name, None if t is None else t.data_ptr())
        assert not arrays, f"unknown operands {sorted(arrays)}"
        for name, v in dict(V=V, ld=ld, C=C_, K=K, pad=pad, eos=eos).items():
            setattr(a, name, int(v))
        a.seed, a.inv_T = int(seed) & 0xFFFFFFFFFFFFFFFF, float(inv_T)
        pfx = None
        if pfx_tok is not None or pfx_len is not None or pfx_src is not None:
            pfx = C.byref(N.DebugPrefix(self._ptr(pfx_tok), int(pfx_ld), int(pfx_sources), self._ptr(pfx_len), self._ptr(pfx_src)))
        N.check(self._lib.ttx_debug_sbs_step_pool(self._session, C.byref(a), int(bool(masked)), int(top_k), float(top_p), pfx,
                                                  self._stream()))

    def debug_sbs_pool(self, op: str, words, *, C_: int, K: int, max_len: int, ld: int, Ls_cap: int, pad: int, bos: int, R: int = 0,
                       first_row: int = 0, kv_row: int = 0, Ls_new: int = 0, **arrays) -> list:
        """One launch of a bookkeeping kernel of the stochastic beam pool (ttx_debug_sbs_pool); ``op`` one of
        _native.DEBUG_SBS_POOL_OPS.  ``words`` as for ``debug_bsp``; returns the 12 as the kernel left them."""
        w = (C.c_int64 * N.DEBUG_BSP_WORDS)(*[int(v) for v in words])
        a = N.DebugSbsPoolArgs()
        for name in a.POINTERS:
            t = arrays.pop(name[2:], None)
            setattr(a, name, None if t is None else t.data_ptr())
        assert not arrays, f"unknown operands {sorted(arrays)}"
        for name, v in dict(C=C_, K=K, max_len=max_len, ld=ld, Ls_cap=Ls_cap, pad=pad, bos=bos, R=R, first_row=first_row, kv_row=kv_row,
                            Ls_new=Ls_new).items():
            setattr(a, name, int(v))
        code = op if isinstance(op, int) else N.DEBUG_SBS_POOL_OPS.index(op)
        N.check(self._lib.ttx_debug_sbs_pool(self._session, code, C.byref(a), w, self._stream()))
        return [int(v) for v in w]

    def debug_kvcopy(self, rec: torch.Tensor, n_copy: int, qkv: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor,
                     n: int, d: int, width: int, B: int) -> None:
        """One k_kvcopy launch (ttx_debug_kvcopy): ``rec`` int32 [B, 5], ``qkv`` fp32 [Ld, B * (1 + n*d), 3 * width], the caches
        fp32 [Ld, B, Lc, width]; all contiguous in their last dimensions."""
        assert kcache.stride() == vcache.stride()
        N.check(self._lib.ttx_debug_kvcopy(self._session, rec.data_ptr(), int(n_copy), qkv.data_ptr(), int(qkv.stride(0)),
                                           kcache.data_ptr(), vcache.data_ptr(), int(kcache.stride(0)), int(kcache.stride(1)),
                                           int(n), int(d), int(width), int(B), int(qkv.shape[0]), self._stream()))

    def debug_kvcopy_split(self, rec: torch.Tensor, n_copy: int, qkv: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor,
                           n: int, d: int, width: int, B: int, pos2: torch.Tensor | None = None,
                           qkv_probe: torch.Tensor | None = None) -> None:
        """debug_kvcopy with the two-phase indirection (ttx_debug_kvcopy_split): ``pos2`` int32 [n_copy] (slot -> position of its
        rows in ``qkv``, -1: the slot's single row of ``qkv_probe`` fp32 [Ld, B, 3 * width]); both None: debug_kvcopy."""
        assert kcache.stride() == vcache.stride()
        N.check(self._lib.ttx_debug_kvcopy_split(self._session, rec.data_ptr(), int(n_copy), qkv.data_ptr(), int(qkv.stride(0)),
                                                 kcache.data_ptr(), vcache.data_ptr(), int(kcache.stride(0)), int(kcache.stride(1)),
                                                 int(n), int(d), int(width), int(B), int(qkv.shape[0]), self._ptr(pos2),
                                                 self._ptr(qkv_probe), 0 if qkv_probe is None else int(qkv_probe.stride(0)),
                                                 self._stream()))

    def debug_probe_split(self, act_idx: torch.Tensor, pred_probe: torch.Tensor, drafts: torch.Tensor, n_active: int,
                          act2: torch.Tensor, pos2: torch.Tensor, probes_before: int = 0) -> list:
        """One k_probe_split launch (ttx_debug_probe_split): ``act_idx`` / ``pred_probe`` / ``act2`` / ``pos2`` int32 [B],
        ``drafts`` int32 [B, n, d].  Returns the 7 result words of include/ttx.h."""
        B, n, d = drafts.shape
        words = (C.c_int32 * 7)(0, 0, 0, 0, int(probes_before), 0, 0)
        N.check(self._lib.ttx_debug_probe_split(self._session, act_idx.data_ptr(), pred_probe.data_ptr(), drafts.data_ptr(), int(B),
                                                int(n), int(d), int(n_active), act2.data_ptr(), pos2.data_ptr(), words,
                                                self._stream()))
        return [int(v) for v in words]

    def debug_merge_pred(self, pos2: torch.Tensor, pred_probe: torch.Tensor, pred2: torch.Tensor, pred: torch.Tensor, B: int,
                         n: int, d: int, n_active: int) -> None:
        """One k_merge_pred launch (ttx_debug_merge_pred): ``pred`` int32 [B * (1 + n*d)] in k_accept's layout."""
        N.check(self._lib.ttx_debug_merge_pred(self._session, pos2.data_ptr(), pred_probe.data_ptr(), pred2.data_ptr(),
                                               pred.data_ptr(), int(B), int(n), int(d), int(n_active), self._stream()))

    # draft select (DESIGN.md "Two-phase verify step"): the same launches on the compacted rows of a draft pass
    def debug_probe_split_select(self, act_idx: torch.Tensor, pred_probe: torch.Tensor, drafts: torch.Tensor, n_active: int,
                                 act2: torch.Tensor, pos2: torch.Tensor, draft_mask: torch.Tensor, row_base: torch.Tensor,
                                 row_map: torch.Tensor, probes_before: int = 0) -> list:
        """debug_probe_split that also writes ``draft_mask`` / ``row_base`` int32 [B] and ``row_map`` int32 [B * (1 + n*d)]
        (ttx_debug_probe_split_select).  Returns the 8 result words of include/ttx.h."""
        B, n, d = drafts.shape
        words = (C.c_int32 * 8)(0, 0, 0, 0, int(probes_before), 0, 0, 0)
        N.check(self._lib.ttx_debug_probe_split_select(self._session, act_idx.data_ptr(), pred_probe.data_ptr(), drafts.data_ptr(),
                                                       int(B), int(n), int(d), int(n_active), act2.data_ptr(), pos2.data_ptr(),
                                                       self._ptr(draft_mask), self._ptr(row_base), self._ptr(row_map), words,
                                                       self._stream()))
        return [int(v) for v in words]

    def debug_merge_pred_select(self, pos2: torch.Tensor, pred_probe: torch.Tensor, pred2: torch.Tensor, pred: torch.Tensor, B: int,
                                n: int, d: int, n_active: int, row_base: torch.Tensor | None, draft_mask: torch.Tensor | None) -> None:
        """debug_merge_pred on compacted draft-pass predictions (ttx_debug_merge_pred_select)."""
        N.check(self._lib.ttx_debug_merge_pred_select(self._session, pos2.data_ptr(), pred_probe.data_ptr(), pred2.data_ptr(),
                                                      pred.data_ptr(), int(B), int(n), int(d), int(n_active), self._ptr(row_base),
                                                      self._ptr(draft_mask), self._stream()))

    def debug_kvcopy_select(self, rec: torch.Tensor, n_copy: int, qkv: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor,
                            n: int, d: int, width: int, B: int, pos2: torch.Tensor | None, qkv_probe: torch.Tensor | None,
                            row_base: torch.Tensor | None, draft_mask: torch.Tensor | None) -> None:
        """debug_kvcopy_split on a compacted ``qkv`` (ttx_debug_kvcopy_select)."""
        assert kcache.stride() == vcache.stride()
        N.check(self._lib.ttx_debug_kvcopy_select(self._session, rec.data_ptr(), int(n_copy), qkv.data_ptr(), int(qkv.stride(0)),
                                                  kcache.data_ptr(), vcache.data_ptr(), int(kcache.stride(0)), int(kcache.stride(1)),
                                                  int(n), int(d), int(width), int(B), int(qkv.shape[0]), self._ptr(pos2),
                                                  self._ptr(qkv_probe), 0 if qkv_probe is None else int(qkv_probe.stride(0)),
                                                  self._ptr(row_base), self._ptr(draft_mask), self._stream()))

    def debug_embed_select(self, table: torch.Tensor, pe: torch.Tensor, x: torch.Tensor, act_idx: torch.Tensor, front: torch.Tensor,
                           gen: torch.Tensor, drafts: torch.Tensor, B: int, n: int, d: int, n_active: int,
                           row_map: torch.Tensor | None, m_rows: int) -> None:
        """The step mode of debug_embed writing ``m_rows`` rows, row i that of layout row ``row_map[i]`` (ttx_debug_embed_select)."""
        N.check(self._lib.ttx_debug_embed_select(self._session, table.data_ptr(), int(table.shape[0]), pe.data_ptr(), int(pe.shape[0]),
                                                 int(table.shape[1]), x.data_ptr(), act_idx.data_ptr(), front.data_ptr(),
                                                 gen.data_ptr(), int(gen.stride(0)), drafts.data_ptr(), int(B), int(n), int(d),
                                                 int(n_active), self._ptr(row_map), int(m_rows), self._stream()))

    def debug_attn_select(self, mode: int, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int,
                          scale: float, groups: int, max_keys: int, row_base: torch.Tensor | None, draft_mask: torch.Tensor | None,
                          Lk: int = 0, tok: torch.Tensor | None = None, pad: int = 0, key_pad: torch.Tensor | None = None,
                          act_idx: torch.Tensor | None = None, front: torch.Tensor | None = None, src_of: torch.Tensor | None = None,
                          src_len: torch.Tensor | None = None, kcache: torch.Tensor | None = None, vcache: torch.Tensor | None = None,
                          cache_seq_stride: int = 0, cache_slot: torch.Tensor | None = None, gen_ld: int = 0, n: int = 1, d: int = 0,
                          n_active: int = 0, kernel: int = 0, **unused) -> int:
        """A step-mode debug_attn at head dimension 32 on compacted rows (ttx_debug_attn_select); takes debug_attn's keywords."""
        kid = C.c_int32(0)
        assert k.stride(0) == v.stride(0)
        N.check(self._lib.ttx_debug_attn_select(self._session, q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0),
                                                out.data_ptr(), int(heads), float(scale), int(Lk), self._ptr(tok), int(pad),
                                                self._ptr(key_pad), self._ptr(act_idx), self._ptr(front), self._ptr(src_of),
                                                self._ptr(src_len), self._ptr(kcache), self._ptr(vcache), int(cache_seq_stride),
                                                self._ptr(cache_slot), int(gen_ld), int(n), int(d), int(mode), int(groups),
                                                int(n_active), int(max_keys), int(kernel), C.byref(kid), self._ptr(row_base),
                                                self._ptr(draft_mask), self._stream()))
        return int(kid.value)

    def attn_kernels_seen(self, session=None) -> set:
        """Ids of the attention kernels ``session`` (default: this model's own) has dispatched so far (ttx_debug_attn_kernels_seen)."""
        mask = int(self._lib.ttx_debug_attn_kernels_seen(self._session if session is None else session))
        if mask < 0:
            N.check(mask)
        return {k for k in range(1, 32) if mask >> k & 1}

    POOL_COUNTERS = ("steps", "split_steps", "slot_steps_probed", "slots_matched", "drafts_matched", "rows_executed", "draft_select")

    def pool_last_counters(self, session=None) -> dict:
        """Counters of the last slot-pool call whose first session was ``session`` (default: this model's own), summed over its
        pools (ttx_pool_last_counters)."""
        words = (C.c_int64 * 7)()
        N.check(self._lib.ttx_pool_last_counters(self._session if session is None else session, words))
        return dict(zip(self.POOL_COUNTERS, (int(v) for v in words)))

    @staticmethod
    def attn_staged_key_limit(head_dim: int, q_per_group: int) -> int:
        """Keys one k_attn2 workgroup can stage at ``head_dim`` for groups of ``q_per_group`` query rows
        (ttx_attn_staged_key_limit; a host query)."""
        return int(N.lib().ttx_attn_staged_key_limit(int(head_dim), int(q_per_group)))

    def close(self) -> None:
        if getattr(self, "_score_session", None):
            self._lib.ttx_session_destroy(self._score_session)
            self._score_session = None
        for extra in getattr(self, "_pool", [])[1:]:
            self._lib.ttx_session_destroy(extra)
        self._pool = None
        if getattr(self, "_session", None):
            self._lib.ttx_session_destroy(self._session)
            self._session = None
        if getattr(self, "_model", None):
            self._lib.ttx_model_destroy(self._model)
            self._model = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _tokens(self, t: torch.Tensor) -> torch.Tensor:
        return t.to(self.device, torch.int64).contiguous()

    def check_tokens(self, t: torch.Tensor, vocab: int | None = None) -> None:
        """torch.nn.Embedding raises IndexError on ids outside the table (the reference's first op on `src`); so do the
        generators here, before the ids reach a kernel (which would otherwise look them up as id 0)."""
        if t.numel() == 0:
            return
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= (vocab or self.src_vocab_size):
            raise IndexError("index out of range in self")

    # -- B5 ------------------------------------------------------------------------------------
    def encode_src(self, src: torch.Tensor, src_pad_mask: torch.Tensor | None = None) -> torch.Tensor:
        """modules.py:110-116.  The mask argument is accepted for signature parity; the library derives
        it as ``src == pad`` exactly as every reference call site does (speculative_decoding.py:60)."""
        src = self._tokens(src)
        self.check_tokens(src)
        B, Ls = src.shape
        mem = torch.empty((B, Ls, self.emb_dim), dtype=torch.float32, device=self.device)
        N.check(self._lib.ttx_encode_src(self._session, src.data_ptr(), B, Ls, mem.data_ptr(), self._stream()))
        return mem

    def decode_tgt(self, tgt: torch.Tensor, memory: torch.Tensor, memory_pad_mask: torch.Tensor,
                   memory_row: torch.Tensor | None = None) -> torch.Tensor:
        """modules.py:118-138.  ``memory_row`` (int32 [R], optional) lets R decoder rows share fewer
        memory rows instead of the reference's repeat_interleave'd copy."""
        tgt = self._tokens(tgt)
        R, Lt = tgt.shape
        memory = memory.to(self.device, torch.float32).contiguous()
        Rm, Ls, _ = memory.shape
        pad = memory_pad_mask.to(self.device, torch.uint8).contiguous()
        row_ptr = None
        if memory_row is not None:
            memory_row = memory_row.to(self.device, torch.int32).contiguous()
            row_ptr = memory_row.data_ptr()
        logits = torch.empty((R, Lt, self.tgt_vocab_size), dtype=torch.float32, device=self.device)
        N.check(self._lib.ttx_decode_tgt(self._session, tgt.data_ptr(), R, Lt, memory.data_ptr(), pad.data_ptr(),
                                         row_ptr, Rm, Ls, logits.data_ptr(), self._stream()))
        return logits

    def __call__(self, src: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
        """modules.py:86-108."""
        src, tgt = self._tokens(src), self._tokens(tgt)
        B, Ls = src.shape
        Lt = tgt.shape[1]
        logits = torch.empty((B, Lt, self.tgt_vocab_size), dtype=torch.float32, device=self.device)
        N.check(self._lib.ttx_forward(self._session, src.data_ptr(), B, Ls, tgt.data_ptr(), Lt, logits.data_ptr(),
                                      self._stream()))
        return logits

    forward = __call__

    # -- teacher-forced evaluation -------------------------------------------------------------
    def teacher_forced(self, src: torch.Tensor, tgt: torch.Tensor, return_logits: bool = False,
                       eos_token_idx: int = 2) -> TeacherForced:
        """What validation_step / test_step compute (src/model/lightning_model.py:174-207, src/utils/metrics.py): the forward
        pass on ``tgt[:, :-1]`` followed by the loss and accuracy stage against ``tgt[:, 1:]``, all on the device
        (ttx_teacher_forced_eval).  The logits are materialised only with ``return_logits=True``."""
        src, tgt = self._tokens(src), self._tokens(tgt)
        self.check_tokens(src)
        self.check_tokens(tgt, self.tgt_vocab_size)       # the reference's embedding / cross-entropy raise on these
        B, Ls = src.shape
        Lt = tgt.shape[1]
        if tgt.shape[0] != B or Lt < 2:
            raise ValueError(f"teacher_forced needs tgt [B, Lt >= 2] for src [B, Ls]; got {tuple(tgt.shape)} for {tuple(src.shape)}")
        T = Lt - 1
        logits = (torch.empty((B, T, self.tgt_vocab_size), dtype=torch.float32, device=self.device) if return_logits else None)
        pred = torch.empty((B, T), dtype=torch.int64, device=self.device)
        nll = torch.empty((B, T), dtype=torch.float32, device=self.device)
        out = torch.empty(3, dtype=torch.float32, device=self.device)
        N.check(self._lib.ttx_teacher_forced_eval(self._session, src.data_ptr(), B, Ls, tgt.data_ptr(), Lt, int(eos_token_idx),
                                                  logits.data_ptr() if logits is not None else None, pred.data_ptr(),
                                                  nll.data_ptr(), out.data_ptr(), self._stream()))
        return TeacherForced(out[0], out[1], out[2], pred, nll, logits)

    def token_metrics(self, logits: torch.Tensor, tgt: torch.Tensor, eos_token_idx: int = 2) -> TeacherForced:
        """The metric stage alone over given logits [B, Lt-1, V] (ttx_token_metrics)."""
        x = logits.to(self.device, torch.float32).contiguous()
        tgt = self._tokens(tgt)
        B, T, V = x.shape
        if tgt.shape != (B, T + 1):
            raise ValueError(f"token_metrics needs tgt [B, T+1] for logits [B, T, V]; got {tuple(tgt.shape)} for {tuple(x.shape)}")
        self.check_tokens(tgt, V)
        pred = torch.empty((B, T), dtype=torch.int64, device=self.device)
        nll = torch.empty((B, T), dtype=torch.float32, device=self.device)
        out = torch.empty(3, dtype=torch.float32, device=self.device)
        N.check(self._lib.ttx_token_metrics(self._session, x.data_ptr(), tgt.data_ptr(), B, T + 1, V, int(eos_token_idx),
                                            pred.data_ptr(), nll.data_ptr(), out.data_ptr(), self._stream()))
        return TeacherForced(out[0], out[1], out[2], pred, nll, x)

    # -- log-likelihood scores of hypotheses ----------------------------------------------------
    def _scoring_session(self) -> C.c_void_p:
        """Scoring runs on a session of its own: its activation buffers are sized by whole hypotheses, and growing a buffer of
        a decoding session would drop that session's captured graphs."""
        if getattr(self, "_score_session", None) is None:
            self._score_session = self.new_session()
        return self._score_session

    def _trim_and_chunk(self, hyp: torch.Tensor, eos: int, trim: bool, max_rows: int | None) -> tuple:
        """(Wt, chunk) of one teacher-forced pass over ``hyp`` Long[B, N, W]: the columns that are run (``trim``: the longest
        non-PAD extent of the batch, one scalar device-to-host read) and the sources per library call, so that one call runs at
        most ``max_rows`` decoder positions (a single source is never split)."""
        _, K, W = hyp.shape
        Wt = W
        if trim:
            cols = torch.arange(1, W + 1, device=self.device)
            Wt = min(W, max(2, int((((hyp != self.tgt_pad_token_i) | (hyp == eos)) * cols).amax())))
        limit = min(int(max_rows or self.SCORE_MAX_ROWS), (1 << 24) - 1)
        return Wt, max(1, limit // (K * (Wt - 1)))

    def hypothesis_logprobs(self, logits: torch.Tensor, hyp: torch.Tensor, pad: int, eos: int) -> HypothesisScores:
        """The scoring stage alone (ttx_hypothesis_logprobs): ``logits`` fp32 [..., W-1, V] as ``decode_tgt(hyp[..., :-1])``
        gives them, ``hyp`` Long[..., W] with the same leading shape.  Nothing is synchronised."""
        x = logits.to(self.device, torch.float32).contiguous()
        hyp = self._tokens(hyp)
        lead, W = tuple(hyp.shape[:-1]), int(hyp.shape[-1])
        if hyp.dim() < 2 or W < 2 or tuple(x.shape[:-1]) != lead + (W - 1,):
            raise ValueError(f"hypothesis_logprobs needs hyp [..., W >= 2] for logits [..., W-1, V]; got {tuple(hyp.shape)} for "
                             f"{tuple(x.shape)}")
        V = int(x.shape[-1])
        self.check_tokens(hyp, V)
        R = hyp.numel() // W
        tok = torch.empty(lead + (W - 1,), dtype=torch.float32, device=self.device)
        score = torch.empty(lead, dtype=torch.float32, device=self.device)
        length = torch.empty(lead, dtype=torch.int32, device=self.device)
        fin = torch.empty(lead, dtype=torch.bool, device=self.device)
        N.check(self._lib.ttx_hypothesis_logprobs(self._scoring_session(), x.data_ptr(), hyp.data_ptr(), R, W, V, int(pad), int(eos),
                                                  tok.data_ptr(), score.data_ptr(), length.data_ptr(), fin.data_ptr(),
                                                  self._stream()))
        return HypothesisScores(score, length, fin, tok)

    def score_hypotheses(self, src: torch.Tensor, hyp: torch.Tensor, eos_token_idx: int = 2, return_token_logp: bool = False,
                         max_rows: int | None = None, trim: bool = True, logits_out: torch.Tensor | None = None) -> HypothesisScores:
        """Log-likelihood of every hypothesis ``hyp[b, k]`` (Long[B, N, W], as the generators return them) of source ``src[b]``
        under the model: the encoder once per source, ONE teacher-forced decoder pass over the B*N rows and the scoring stage
        (ttx_score_hypotheses).  The same scale for the output of every generator.

        ``trim=True`` (default) reads the longest non-PAD extent of the batch and scores only that many columns: generator
        outputs are PAD-filled to ``max_len`` and the decoder pass would pay for every PAD column.  This is ONE scalar
        device-to-host read, i.e. one synchronisation; ``trim=False`` never synchronises.  ``token_logp`` keeps the full
        [B, N, W-1] shape either way, zeros beyond a hypothesis' length.

        ``max_rows`` (default ``SCORE_MAX_ROWS`` = 32768) bounds the decoder positions ``B_chunk * N * (W-1)`` of one library
        call: whole sources are scored in chunks, so that a look-ahead window of many batches does not size the activation
        buffers by the whole window.  A single source is never split.

        ``logits_out`` (fp32 [B*N, W-1, V], needs ``trim=False`` and one chunk) receives the decoder's logits."""
        src, hyp = self._tokens(src), self._tokens(hyp)
        if src.dim() != 2 or hyp.dim() != 3 or hyp.shape[0] != src.shape[0] or hyp.shape[1] < 1 or hyp.shape[2] < 2:
            raise ValueError(f"score_hypotheses needs hyp [B, N >= 1, W >= 2] for src [B, Ls]; got {tuple(hyp.shape)} for "
                             f"{tuple(src.shape)}")
        self.check_tokens(src)
        self.check_tokens(hyp, self.tgt_vocab_size)
        (B, Ls), (_, K, W) = src.shape, hyp.shape
        eos = int(eos_token_idx)
        Wt, chunk = self._trim_and_chunk(hyp, eos, trim, max_rows)
        if logits_out is not None:
            if Wt != W or chunk < B or tuple(logits_out.shape) != (B * K, W - 1, self.tgt_vocab_size) \
                    or logits_out.dtype != torch.float32 or not logits_out.is_contiguous() or logits_out.device != self.device:
                raise ValueError("logits_out needs trim=False, one chunk and a contiguous fp32 [B*N, W-1, V] device tensor")
        score = torch.empty((B, K), dtype=torch.float32, device=self.device)
        length = torch.empty((B, K), dtype=torch.int32, device=self.device)
        fin = torch.empty((B, K), dtype=torch.bool, device=self.device)
        tok = None
        if return_token_logp:
            tok = (torch.empty if Wt == W else torch.zeros)((B, K, W - 1), dtype=torch.float32, device=self.device)
        sess, stream = self._scoring_session(), self._stream()
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            part = None
            if tok is not None:
                part = tok[b0:b1] if Wt == W else torch.empty((b1 - b0, K, Wt - 1), dtype=torch.float32, device=self.device)
            N.check(self._lib.ttx_score_hypotheses(sess, src[b0:b1].data_ptr(), b1 - b0, Ls, hyp[b0:b1].data_ptr(), W, K, Wt, eos,
                                                   self._ptr(logits_out), self._ptr(part), score[b0:b1].data_ptr(),
                                                   length[b0:b1].data_ptr(), fin[b0:b1].data_ptr(), stream))
            if part is not None and Wt != W:
                tok[b0:b1, :, :Wt - 1] = part
        return HypothesisScores(score, length, fin, tok)

    def score_hypotheses_many(self, srcs: list, hyps: list, eos_token_idx: int = 2, return_token_logp: bool = False,
                              max_rows: int | None = None) -> list:
        """``score_hypotheses(srcs[i], hyps[i], eos_token_idx, return_token_logp)`` for every batch of a list, in list order, in
        length buckets (ttx_score_list_extents / ttx_score_list_run): the sources of the whole list are sorted by their
        hypotheses' and their own non-PAD extent (``scheduling.score_plan``) and scored in chunks of at most ``max_rows``
        decoder positions (default ``SCORE_MAX_ROWS``; swept in DESIGN.md §30), each chunk at the widths of its own longest member, so that neither
        hypothesis nor source columns that are PAD in almost every row are run.  Shapes may differ from batch to batch; an entry
        whose ``hyp`` is None gives None.  The values are those of the per-batch calls bit for bit while sources and hypotheses
        stay within the attention kernels' staged key range (384 positions, 320 at head dimension 64).  ONE device-to-host read
        (the extents, with the token-id check riding on it) is the call's only synchronisation; the results of a call share one
        allocation per field."""
        if len(srcs) != len(hyps):
            raise ValueError(f"score_hypotheses_many needs one hyp (or None) per src, got {len(hyps)} for {len(srcs)}")
        out = [None] * len(hyps)
        live = [i for i, h in enumerate(hyps) if h is not None]
        if not live:
            return out
        eos = int(eos_token_idx)
        keep, shapes = [], []                                  # the converted tensors stay alive until the call has been enqueued
        table = (N.ScoreBatch * len(live))()
        for j, i in enumerate(live):
            src, hyp = self._tokens(srcs[i]), self._tokens(hyps[i])
            if src.dim() != 2 or hyp.dim() != 3 or hyp.shape[0] != src.shape[0] or hyp.shape[1] < 1 or hyp.shape[2] < 2 \
                    or src.shape[0] < 1 or src.shape[1] < 1:
                raise ValueError(f"score_hypotheses_many needs hyp [B, N >= 1, W >= 2] for src [B >= 1, Ls >= 1]; batch {i} has "
                                 f"{tuple(hyp.shape)} for {tuple(src.shape)}")
            (B, Ls), (_, K, W) = src.shape, hyp.shape
            keep.append((src, hyp))
            shapes.append((B, K, W))
            table[j] = N.ScoreBatch(src.data_ptr(), hyp.data_ptr(), B, Ls, K, W, W)
        S = sum(B for B, _, _ in shapes)
        rows = np.cumsum([0] + [B * K for B, K, _ in shapes])
        toks = np.cumsum([0] + [B * K * (W - 1) for B, K, W in shapes])
        R = int(rows[-1])
        sess, stream = self._scoring_session(), self._stream()
        ext = torch.empty(2 * S + 1, dtype=torch.int32, device=self.device)          # e, ls, the token-id flags
        N.check(self._lib.ttx_score_list_extents(sess, table, len(live), eos, ext.data_ptr(), ext[S:].data_ptr(), None,
                                                 ext[2 * S:].data_ptr(), stream))
        host = ext.cpu().numpy()                                                     # the call's one synchronisation
        if host[2 * S]:
            raise IndexError("index out of range in self")
        limit = min(int(max_rows or self.SCORE_MAX_ROWS), (1 << 24) - 1)
        if limit < 1:
            raise ValueError(f"max_rows must be at least 1, got {max_rows}")
        plan = score_plan(np.repeat([K for _, K, _ in shapes], [B for B, _, _ in shapes]), host[:S], host[S:2 * S], limit)
        order = np.ascontiguousarray(np.concatenate([c.sources for c in plan]), dtype=np.int32)
        chunks, first = (N.ScoreChunk * len(plan))(), 0
        for c, ch in enumerate(plan):
            chunks[c] = N.ScoreChunk(first, len(ch.sources), ch.N, ch.W, ch.Ls)
            first += len(ch.sources)
        score = torch.empty(R, dtype=torch.float32, device=self.device)
        length = torch.empty(R, dtype=torch.int32, device=self.device)
        fin = torch.empty(R, dtype=torch.bool, device=self.device)
        tok = torch.empty(int(toks[-1]), dtype=torch.float32, device=self.device) if return_token_logp else None
        tok_off = (C.c_int64 * len(live))(*[int(t) for t in toks[:-1]])
        N.check(self._lib.ttx_score_list_run(sess, table, len(live), order.ctypes.data_as(C.POINTER(C.c_int32)), S, chunks, len(plan),
                                             eos, score.data_ptr(), length.data_ptr(), fin.data_ptr(), self._ptr(tok),
                                             tok_off if tok is not None else None, stream))
        self.last_score_plan = plan                            # for tools and tests: the chunks the last call ran
        for j, i in enumerate(live):
            (B, K, W), r0, r1 = shapes[j], int(rows[j]), int(rows[j + 1])
            out[i] = HypothesisScores(score[r0:r1].view(B, K), length[r0:r1].view(B, K), fin[r0:r1].view(B, K),
                                      None if tok is None else tok[int(toks[j]):int(toks[j + 1])].view(B, K, W - 1))
        return out

    # -- folding hypotheses into their distinct ones ---------------------------------------------
    def fold_hypotheses(self, hyp: torch.Tensor, scores=None, order: str = "score", unfinished: str = "keep", gather: bool = True,
                        with_logmass: bool | None = None, pad: int | None = None, eos: int = 2,
                        debug_no_filter: bool = False) -> FoldedHypotheses:
        """The distinct hypotheses among each source's rows, counted and ranked on the device (ttx_fold_hypotheses; the rule
        is ``scoring.unique_samples``', stated in include/ttx.h).  ``hyp`` Long[B, N, L] with N <= 1024, or a view whose
        last-dimension stride is 1 (folded in place through its row stride); ``scores`` Float[B, N] or anything with ``.score``.
        ``order``: "score" (descending score, equal scores by first occurrence; needs scores), "count" (the most frequent first,
        then by score when given), "first" (by first occurrence).  ``unfinished="last"`` puts the hypotheses without an EOS behind
        the finished ones.  ``gather=False`` skips the gathered rows (``pred`` is None); ``with_logmass`` defaults to whether
        scores were given.  ``pad`` (default: the model's) fills the rows beyond ``n_unique``.  Nothing is synchronised."""
        hyp = hyp.to(self.device) if isinstance(hyp, torch.Tensor) else hyp
        sc = getattr(scores, "score", scores)
        sc = sc.to(self.device) if isinstance(sc, torch.Tensor) else sc
        return fold_on_device(self._lib, self._session, hyp, sc, order, unfinished, gather, with_logmass,
                              self.tgt_pad_token_i if pad is None else pad, eos, debug_no_filter)

    # -- per-position alternatives of hypotheses -------------------------------------------------
    def _alt_buffers(self, lead: tuple, T: int, k: int, fill: bool) -> Alternatives:
        """Output tensors of the alternatives stage; ``fill``: pre-set to the not-live values (columns a trimmed pass leaves)."""
        dev = self.device

        def make(shape, dtype, value):
            return torch.full(shape, value, dtype=dtype, device=dev) if fill else torch.empty(shape, dtype=dtype, device=dev)

        return Alternatives(make(lead + (T, k), torch.int32, -1), make(lead + (T, k), torch.float32, 0.0),
                            make(lead + (T,), torch.float32, 0.0), make(lead + (T,), torch.int32, -1),
                            make(lead + (T,), torch.float32, 0.0), torch.empty(lead, dtype=torch.int32, device=dev))

    def hypothesis_alternatives(self, logits: torch.Tensor, hyp: torch.Tensor, pad: int, eos: int, k: int = 5) -> Alternatives:
        """The alternatives stage alone (ttx_hypothesis_alternatives): ``logits`` fp32 [..., W-1, V] as
        ``decode_tgt(hyp[..., :-1])`` gives them, ``hyp`` Long[..., W] with the same leading shape.  A ``logits`` tensor that is
        already a contiguous fp32 device tensor is read in place.  Nothing is synchronised."""
        x = logits.to(self.device, torch.float32)
        if not x.is_contiguous():
            x = x.contiguous()
        hyp = self._tokens(hyp)
        lead, W = tuple(hyp.shape[:-1]), int(hyp.shape[-1])
        if hyp.dim() < 2 or W < 2 or tuple(x.shape[:-1]) != lead + (W - 1,):
            raise ValueError(f"hypothesis_alternatives needs hyp [..., W >= 2] for logits [..., W-1, V]; got {tuple(hyp.shape)} "
                             f"for {tuple(x.shape)}")
        V, k = int(x.shape[-1]), int(k)
        if not 1 <= k <= min(32, V):
            raise ValueError(f"k must be in [1, min(32, V)], got {k} for V = {V}")
        self.check_tokens(hyp, V)
        out = self._alt_buffers(lead, W - 1, k, fill=False)
        N.check(self._lib.ttx_hypothesis_alternatives(self._scoring_session(), x.data_ptr(), hyp.data_ptr(), hyp.numel() // W, W, V,
                                                      int(pad), int(eos), k, *(t.data_ptr() for t in out), self._stream()))
        return out

    def alternatives(self, src: torch.Tensor, hyp: torch.Tensor, k: int = 5, eos_token_idx: int = 2, max_rows: int | None = None,
                     trim: bool = True, with_scores: bool = False):
        """What the model considered at every position of hypothesis ``hyp[b, n]`` (Long[B, N, W]) of source ``src[b]``: the
        ``k`` most probable tokens with their log-probabilities, the log-probability and rank of the emitted token and the
        entropy, from the teacher-forced pass ``score_hypotheses`` runs (ttx_score_alternatives).

        ``trim`` and ``max_rows`` behave as in ``score_hypotheses``: one scalar device-to-host read or none, whole sources per
        chunk.  Results keep the full ``W-1``; columns cut by ``trim`` hold the not-live values.

        ``with_scores=True`` returns ``(Alternatives, HypothesisScores)`` (the scores with ``token_logp``), both from the same
        decoder pass: the chunk's logits stay in a device buffer and the scoring stage runs on them."""
        src, hyp = self._tokens(src), self._tokens(hyp)
        if src.dim() != 2 or hyp.dim() != 3 or hyp.shape[0] != src.shape[0] or hyp.shape[1] < 1 or hyp.shape[2] < 2:
            raise ValueError(f"alternatives needs hyp [B, N >= 1, W >= 2] for src [B, Ls]; got {tuple(hyp.shape)} for "
                             f"{tuple(src.shape)}")
        k, V = int(k), self.tgt_vocab_size
        if not 1 <= k <= min(32, V):
            raise ValueError(f"k must be in [1, min(32, V)], got {k} for V = {V}")
        self.check_tokens(src)
        self.check_tokens(hyp, V)
        (B, Ls), (_, K, W) = src.shape, hyp.shape
        eos = int(eos_token_idx)
        Wt, chunk = self._trim_and_chunk(hyp, eos, trim, max_rows)
        T, Tt = W - 1, Wt - 1
        out = self._alt_buffers((B, K), T, k, fill=Wt != W)
        sc = None
        if with_scores:
            sc = HypothesisScores(torch.empty((B, K), dtype=torch.float32, device=self.device), out.length,
                                  torch.empty((B, K), dtype=torch.bool, device=self.device),
                                  (torch.empty if Wt == W else torch.zeros)((B, K, T), dtype=torch.float32, device=self.device))
            buf = torch.empty((min(B, chunk) * K, Tt, V), dtype=torch.float32, device=self.device)   # one chunk's logits, reused
        sess, stream = self._scoring_session(), self._stream()
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            nb = b1 - b0
            part = Alternatives(*(t[b0:b1] for t in out)) if Wt == W else self._alt_buffers((nb, K), Tt, k, fill=False)
            logits = buf[:nb * K] if with_scores else None
            N.check(self._lib.ttx_score_alternatives(sess, src[b0:b1].data_ptr(), nb, Ls, hyp[b0:b1].data_ptr(), W, K, Wt, eos, k,
                                                     self._ptr(logits), *(t.data_ptr() for t in part[:5]),
                                                     out.length[b0:b1].data_ptr(), stream))
            if Wt != W:
                for full, cut in zip(out[:5], part[:5]):
                    full[b0:b1, :, :Tt] = cut
            if with_scores:
                rows = hyp[b0:b1] if Wt == W else hyp[b0:b1, :, :Wt].contiguous()
                tok = sc.token_logp[b0:b1] if Wt == W else torch.empty((nb, K, Tt), dtype=torch.float32, device=self.device)
                N.check(self._lib.ttx_hypothesis_logprobs(sess, logits.data_ptr(), rows.data_ptr(), nb * K, Wt, V,
                                                          self.tgt_pad_token_i, eos, tok.data_ptr(), sc.score[b0:b1].data_ptr(),
                                                          out.length[b0:b1].data_ptr(), sc.finished[b0:b1].data_ptr(), stream))
                if Wt != W:
                    sc.token_logp[b0:b1, :, :Tt] = tok
        return (out, sc) if with_scores else out

    # -- log-probability of hypotheses under the sampling distribution ---------------------------
    @staticmethod
    def _dist(temperature: float, top_k: int, top_p: float) -> N.Dist:
        """The ``ttx_dist`` of a call; ValueError for what the sampler refuses (the library checks again before any launch)."""
        t, k, p = float(temperature), int(top_k), float(top_p)
        if not (t >= 0.0 and t != float("inf")):
            raise ValueError(f"temperature must be finite and >= 0, got {temperature!r}")
        if not 0 <= k <= 32:
            raise ValueError(f"top_k must be 0 or in [1, 32], got {top_k!r}")
        if not 0.0 < p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
        return N.Dist(t, k, p)

    def _forced_rows(self, forced_len, lead: tuple) -> torch.Tensor | None:
        """``forced_len`` as the int32 device tensor of shape ``lead`` the kernel reads: given per hypothesis (``lead``) or, for
        ``lead = (B, N)``, per source ([B]).  ValueError: another shape, a non-integer dtype, or (for a host tensor, where it
        costs no synchronisation) a negative entry; the kernel clamps to [0, length]."""
        if forced_len is None:
            return None
        f = torch.as_tensor(forced_len)
        if f.dtype.is_floating_point or f.dtype == torch.bool:
            raise ValueError(f"forced_len must be an integer tensor, got {f.dtype}")
        if tuple(f.shape) == lead[:1] and len(lead) == 2:
            f = f[:, None].expand(lead)
        elif tuple(f.shape) != lead:
            raise ValueError(f"forced_len must have shape {lead[:1] if len(lead) == 2 else lead} or {lead}, got {tuple(f.shape)}")
        if f.device.type == "cpu" and f.numel() and int(f.min()) < 0:
            raise ValueError("forced_len holds a negative entry")
        return f.to(self.device, torch.int32).contiguous()

    def hypothesis_logq(self, logits: torch.Tensor, hyp: torch.Tensor, pad: int, eos: int, temperature: float = 1.0, top_k: int = 0,
                        top_p: float = 1.0, forced_len=None, check_ids: bool = True, logit_bias=None, syntax=None,
                        syntax_max_len: int = 0) -> ProposalScores:
        """The stage alone (ttx_hypothesis_logq): ``logits`` fp32 [..., W-1, V] as ``decode_tgt(hyp[..., :-1])`` gives them,
        ``hyp`` Long[..., W] with the same leading shape, ``forced_len`` integers of that leading shape.  A ``logits`` tensor
        that is already a contiguous fp32 device tensor is read in place.  Every output is returned.  Nothing is synchronised
        (``check_ids=False`` skips the IndexError check of the token ids, which reads their range back).
        ``logit_bias``: Float[S, V] with ``S`` the first leading dimension (the sources; ``scoring.check_logit_bias``'s form): the
        stage runs on a biased copy of the logits (ttx_hypothesis_logq_bias), ``logits`` itself is not written.
        ``syntax``: a ``syntax.SmilesSyntax``: the copy is also masked by k_syntax_mask under the rule's ``syntax_max_len``
        (0: W), after the bias (ttx_hypothesis_logq_syntax)."""
        x = logits.to(self.device, torch.float32)
        if not x.is_contiguous():
            x = x.contiguous()
        hyp = self._tokens(hyp)
        lead, W = tuple(hyp.shape[:-1]), int(hyp.shape[-1])
        if hyp.dim() < 2 or W < 2 or tuple(x.shape[:-1]) != lead + (W - 1,):
            raise ValueError(f"hypothesis_logq needs hyp [..., W >= 2] for logits [..., W-1, V]; got {tuple(hyp.shape)} for "
                             f"{tuple(x.shape)}")
        V = int(x.shape[-1])
        dist = self._dist(temperature, top_k, top_p)
        forced = self._forced_rows(forced_len, lead)
        if check_ids:
            self.check_tokens(hyp, V)
        dev = self.device
        out = ProposalScores(torch.empty(lead, dtype=torch.float32, device=dev), torch.empty(lead, dtype=torch.int32, device=dev),
                             torch.empty(lead, dtype=torch.bool, device=dev), torch.empty(lead, dtype=torch.int32, device=dev),
                             torch.empty(lead + (W - 1,), dtype=torch.float32, device=dev),
                             torch.empty(lead + (W - 1,), dtype=torch.int32, device=dev),
                             torch.empty(lead + (W - 1,), dtype=torch.int32, device=dev), None)
        bias = d_cls = None                      # both bound until the call returns
        if logit_bias is not None:
            from .scoring import check_logit_bias
            bias = check_logit_bias(logit_bias, int(lead[0]), V).to(dev).contiguous()
        if syntax is not None:
            from .syntax import as_syntax
            d_cls = as_syntax(syntax).table(V, dev)
        R = hyp.numel() // W
        # the general form: a NULL d_bias and a NULL syntax are the plain call
        N.check(self._lib.ttx_hypothesis_logq_syntax(self._scoring_session(), x.data_ptr(), hyp.data_ptr(), R, W, V, int(pad), int(eos),
                                                     C.byref(dist), self._ptr(forced), self._ptr(bias), V, R // max(int(lead[0]), 1),
                                                     N.Syntax.arg(d_cls, syntax_max_len), out.token_logq.data_ptr(), out.logq.data_ptr(),
                                                     out.first_outside.data_ptr(), out.rank.data_ptr(), out.n_kept.data_ptr(),
                                                     out.length.data_ptr(), out.finished.data_ptr(), self._stream()))
        if syntax is not None:
            out.logq.masked_fill_(out.first_outside >= 0, float("-inf"))     # see proposal_scores
        return out

    def proposal_scores(self, src: torch.Tensor, hyp: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                        forced_len=None, with_scores: bool = False, return_token_logq: bool = False, return_rank: bool = False,
                        trim: bool = True, max_rows: int | None = None, eos_token_idx: int = 2, logit_bias=None, syntax=None,
                        syntax_max_len: int = 0) -> ProposalScores:
        """Log-probability of every hypothesis ``hyp[b, k]`` (Long[B, N, W]) of source ``src[b]`` under the distribution a sampler
        with (``temperature``, ``top_k``, ``top_p``) draws from: the teacher-forced pass of ``score_hypotheses`` and the stage
        that evaluates the sampler's own rule at every emitted token (ttx_score_proposal; include/ttx.h defines the quantity).
        ``logq = -inf`` means the sampler cannot emit the row (``first_outside`` names the position).  A row that was SAMPLED at
        these settings can still get ``-inf`` when one of its tokens sat on the nucleus boundary: decode-time and teacher-forced
        logits agree to rounding only.  ``return_rank=True`` returns ``rank`` and ``n_kept``, which show that case
        (``rank == n_kept`` at ``first_outside``).

        ``forced_len``: integers [B] (per source) or [B, N]: the first ``forced_len`` positions of a row were forced (a prefix),
        cost nothing and are inside the support.  ``with_scores=True`` fills ``scores`` with ``score_hypotheses``' result (with
        ``token_logp``) from the same decoder pass.  With temperature 1, no filter and no ``forced_len``, ``logq`` is
        ``score_hypotheses``' ``score`` bit for bit.  ``trim`` and ``max_rows`` behave as in ``score_hypotheses``; results keep the
        full ``W-1``, columns cut by ``trim`` hold the not-live values.

        ``logit_bias``: Float[B, V], the per-source bias the rows were (or would be) sampled under (``scoring.check_logit_bias``'s
        form; ``-inf`` forbids a token).  The log q stage then reads the biased logits (k_logit_bias on the teacher-forced logits,
        ttx_score_proposal_bias), so ``logq`` is the log-probability under the biased sampler's distribution, ``first_outside`` names
        the first forbidden token and ``logq = -inf`` means "cannot be emitted".  ``scores`` (``with_scores=True``) stay the RAW
        model's log p, from the logits before the bias, in the same pass: ``scoring.importance_weights`` stays ``p / q``.

        ``syntax``: the ``syntax.SmilesSyntax`` the rows were (or would be) sampled under, with ``syntax_max_len`` the sampler's
        ``max_len`` (0: W).  k_syntax_mask then masks the teacher-forced logits after the bias (ttx_score_proposal_syntax):
        ``first_outside`` names the first position the constrained sampler could not have emitted; ``scores`` stay the raw log p.
        After an unmatched CLOSE (depth below zero, which no constrained row reaches) the rule can leave a later position no token
        at all: ``token_logq`` is NaN there, ``logq`` is ``-inf`` as for every row with a ``first_outside``."""
        src, hyp = self._tokens(src), self._tokens(hyp)
        if src.dim() != 2 or hyp.dim() != 3 or hyp.shape[0] != src.shape[0] or hyp.shape[1] < 1 or hyp.shape[2] < 2:
            raise ValueError(f"proposal_scores needs hyp [B, N >= 1, W >= 2] for src [B, Ls]; got {tuple(hyp.shape)} for "
                             f"{tuple(src.shape)}")
        V = self.tgt_vocab_size                   # above 1024: refused by the library from the model's config, before any launch
        dist = self._dist(temperature, top_k, top_p)
        (B, Ls), (_, K, W) = src.shape, hyp.shape
        forced = self._forced_rows(forced_len, (B, K))
        self.check_tokens(src)
        self.check_tokens(hyp, V)
        eos, dev = int(eos_token_idx), self.device
        bias = None
        if logit_bias is not None:
            from .scoring import check_logit_bias
            bias = check_logit_bias(logit_bias, B, V).to(dev).contiguous()
        d_cls = syn_arg = None
        if syntax is not None:
            from .syntax import as_syntax
            d_cls = as_syntax(syntax).table(V, dev)
            syn_arg = N.Syntax.arg(d_cls, int(syntax_max_len) or W)
        Wt, chunk = self._trim_and_chunk(hyp, eos, trim, max_rows)
        T, Tt = W - 1, Wt - 1
        cut = Wt != W

        def per_pos(dtype, value, wanted=True):
            if not wanted:
                return None
            return torch.full((B, K, T), value, dtype=dtype, device=dev) if cut else torch.empty((B, K, T), dtype=dtype, device=dev)

        sc = None
        if with_scores:
            sc = HypothesisScores(torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.int32, device=dev),
                                  torch.empty((B, K), dtype=torch.bool, device=dev), per_pos(torch.float32, 0.0))
        out = ProposalScores(torch.empty((B, K), dtype=torch.float32, device=dev), sc.length if sc else torch.empty((B, K), dtype=torch.int32, device=dev),
                             sc.finished if sc else torch.empty((B, K), dtype=torch.bool, device=dev),
                             torch.empty((B, K), dtype=torch.int32, device=dev), per_pos(torch.float32, 0.0, return_token_logq),
                             per_pos(torch.int32, -1, return_rank), per_pos(torch.int32, 0, return_rank), sc)
        full = [out.token_logq, out.rank, out.n_kept, sc.token_logp if sc else None]
        sess, stream = self._scoring_session(), self._stream()
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            nb = b1 - b0
            part = [None if t is None else (t[b0:b1] if not cut else torch.empty((nb, K, Tt), dtype=t.dtype, device=dev)) for t in full]
            tail = (None, self._ptr(part[3]), sc.score[b0:b1].data_ptr() if sc else None,
                    self._ptr(part[0]), out.logq[b0:b1].data_ptr(), out.first_outside[b0:b1].data_ptr(),
                    self._ptr(part[1]), self._ptr(part[2]), out.length[b0:b1].data_ptr(), out.finished[b0:b1].data_ptr(), stream)
            head = (sess, src[b0:b1].data_ptr(), nb, Ls, hyp[b0:b1].data_ptr(), W, K, Wt, eos, C.byref(dist),
                    None if forced is None else forced[b0:b1].data_ptr())
            N.check(self._lib.ttx_score_proposal_syntax(*head, None if bias is None else bias[b0:b1].data_ptr(), V, syn_arg, *tail))
            if cut:
                for t, c in zip(full, part):
                    if t is not None:
                        t[b0:b1, :, :Tt] = c
        if syn_arg is not None:
            # a hypothesis whose depth has gone negative (an unmatched CLOSE: outside the support from there on) can later meet a
            # position at which the rule leaves no token at all; its token_logq is NaN there, and the row is -inf all the same
            out.logq.masked_fill_(out.first_outside >= 0, float("-inf"))
        return out

    # -- cross-attention maps of hypotheses -----------------------------------------------------
    def attention_maps(self, src: torch.Tensor, hyp: torch.Tensor, eos_token_idx: int = 2, layer: int = -1, heads: str = "mean",
                       return_alignment: bool = True, max_rows: int | None = None, trim: bool = True) -> AttentionMaps:
        """Which source positions every token of hypothesis ``hyp[b, k]`` (Long[B, N, W]) attended to: the cross-attention
        probabilities of decoder layer ``layer`` (-1: the last) in the model's own teacher-forced pass on the hypothesis
        (ttx_attention_maps).  ``heads="mean"`` gives the head average fp32 [B, N, W-1, Ls] (what ``nn.MultiheadAttention``
        returns with ``average_attn_weights=True``), ``heads="all"`` every head, fp32 [B, N, H, W-1, Ls].  The pass ends at the
        tapped layer: no later layer, no logits.

        ``trim`` and ``max_rows`` behave as in ``score_hypotheses``: one scalar device-to-host read or none, whole sources per
        chunk of at most ``max_rows`` decoder positions, which also bounds the map bytes one library call writes
        (``positions * Ls * 4``, times H for ``"all"``).  Results keep the full ``W-1``: zeros / -1 past the trimmed width."""
        if heads not in ("mean", "all"):
            raise ValueError(f"heads must be 'mean' or 'all', got {heads!r}")
        src, hyp = self._tokens(src), self._tokens(hyp)
        if src.dim() != 2 or hyp.dim() != 3 or hyp.shape[0] != src.shape[0] or hyp.shape[1] < 1 or hyp.shape[2] < 2:
            raise ValueError(f"attention_maps needs hyp [B, N >= 1, W >= 2] for src [B, Ls]; got {tuple(hyp.shape)} for "
                             f"{tuple(src.shape)}")
        self.check_tokens(src)
        self.check_tokens(hyp, self.tgt_vocab_size)
        (B, Ls), (_, K, W) = src.shape, hyp.shape
        eos, H = int(eos_token_idx), self.num_heads
        Wt, chunk = self._trim_and_chunk(hyp, eos, trim, max_rows)
        T, Tt = W - 1, Wt - 1
        shape = (B, K, H, T, Ls) if heads == "all" else (B, K, T, Ls)
        attn = (torch.empty if Wt == W else torch.zeros)(shape, dtype=torch.float32, device=self.device)
        align = torch.full((B, K, T), -1, dtype=torch.int32, device=self.device) if return_alignment else None
        length = torch.empty((B, K), dtype=torch.int32, device=self.device)
        sess, stream = self._scoring_session(), self._stream()
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            if Wt == W:
                a_part, al_part = attn[b0:b1], (align[b0:b1] if align is not None else None)
            else:
                a_part = torch.empty((b1 - b0,) + shape[1:-2] + (Tt, Ls), dtype=torch.float32, device=self.device)
                al_part = torch.empty((b1 - b0, K, Tt), dtype=torch.int32, device=self.device) if align is not None else None
            N.check(self._lib.ttx_attention_maps(sess, src[b0:b1].data_ptr(), b1 - b0, Ls, hyp[b0:b1].data_ptr(), W, K, Wt, eos,
                                                 int(layer), a_part.data_ptr() if heads == "all" else None,
                                                 a_part.data_ptr() if heads == "mean" else None, self._ptr(al_part),
                                                 length[b0:b1].data_ptr(), stream))
            if Wt != W:
                attn[b0:b1, ..., :Tt, :] = a_part
                if align is not None:
                    align[b0:b1, :, :Tt] = al_part
        return AttentionMaps(attn, align, length)

    # -- beam-speculative bookkeeping kernels --------------------------------------------------
    def nucleus_mask(self, logits: torch.Tensor, nucleus: float, max_kept: int, fill: float) -> torch.Tensor:
        """mask_with_num_logits_according_nucleus (speculative_decoding.py:871-904) on the device."""
        shape = logits.shape
        x = logits.to(self.device, torch.float32).contiguous().reshape(-1, shape[-1])
        out = torch.empty_like(x)
        N.check(self._lib.ttx_nucleus_mask(self._session, x.data_ptr(), x.shape[0], x.shape[1], float(nucleus), int(max_kept),
                                           float(fill), out.data_ptr(), self._stream()))
        return out.reshape(shape)

    def accepted_lengths(self, logits: torch.Tensor, drafts: torch.Tensor, nucleus: float, max_kept: int) -> torch.Tensor:
        """Leading draft tokens that survive the nucleus mask of their position (speculative_decoding.py:539-548, :847-869).
        logits [R,D+1,V], drafts Long[R,D] -> Long[R]."""
        R, D1, V = logits.shape
        x = logits.to(self.device, torch.float32).contiguous()
        d = drafts.to(self.device, torch.int64).contiguous()
        out = torch.empty(R, dtype=torch.int32, device=self.device)
        N.check(self._lib.ttx_accepted_lengths(self._session, x.data_ptr(), d.data_ptr(), R, D1 - 1, V, float(nucleus),
                                               int(max_kept), out.data_ptr(), self._stream()))
        return out.long()

    def ragged_topk(self, score: torch.Tensor, counts: torch.Tensor, k: int):
        """topk_in_each_group (speculative_decoding.py:177-238): (values [G,k], flat indices [G*k])."""
        sc = score.to(self.device, torch.float32).contiguous().reshape(-1)
        counts = counts.to(self.device)
        offs = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=self.device)
        offs[1:] = counts.cumsum(0)
        G = counts.numel()
        top = torch.empty((G, k), dtype=torch.float32, device=self.device)
        idx = torch.empty((G, k), dtype=torch.int64, device=self.device)
        N.check(self._lib.ttx_ragged_topk(self._session, sc.data_ptr(), offs.data_ptr(), G, int(counts.max()), int(k),
                                          top.data_ptr(), idx.data_ptr(), self._stream()))
        return top, idx.reshape(-1)

    def make_drafts(self, src: torch.Tensor, draft_len: int, n_drafts: int, min_draft_len: int, max_draft_len: int,
                    eos_token_idx: int, pad_token_idx: int, replace_token_idx: int) -> torch.Tensor:
        """src/utils/drafting.py:5-67 on the device."""
        src = self._tokens(src)
        B, L = src.shape
        D = min(max(min_draft_len, draft_len), max_draft_len)
        out = torch.empty((B, n_drafts, D), dtype=torch.int64, device=self.device)
        N.check(self._lib.ttx_make_drafts(self._session, src.data_ptr(), B, L, draft_len, n_drafts, min_draft_len,
                                          max_draft_len, eos_token_idx, pad_token_idx, replace_token_idx,
                                          out.data_ptr(), self._stream()))
        return out
