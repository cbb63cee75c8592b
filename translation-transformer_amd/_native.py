"""ctypes binding of libttx_hip.so (include/ttx.h) + the in-tree build recipe.

The shared library is the product; this module only loads it and marshals pointers.  There is no
fallback: if the library is missing, cannot be loaded, or finds no gfx950 device, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
CSRC = PKG_DIR / "csrc"
INCLUDE = PKG_DIR.parent / "include"
LIB_PATH = PKG_DIR / "libttx_hip.so"
# translation units (compiled in parallel, linked into one shared library) and the headers every one of them depends on
UNITS = [CSRC / "ttx_api.hip", CSRC / "ttx_gemm.hip", CSRC / "ttx_attn.hip"]
HEADERS = [CSRC / "ttx_internal.h", CSRC / "ttx_common.hip.h", CSRC / "ttx_loop_kernels.hip.h", CSRC / "ttx_metrics.hip.h",
           CSRC / "ttx_score.hip.h", CSRC / "ttx_score_list.hip.h", CSRC / "ttx_fold.hip.h", CSRC / "ttx_alternatives.hip.h", CSRC / "ttx_attn_probs.hip.h", CSRC / "ttx_sample.hip.h", CSRC / "ttx_logq.hip.h", CSRC / "ttx_sbs.hip.h", CSRC / "ttx_sbs_pool.hip.h",
           CSRC / "ttx_proposal.hip.h", CSRC / "ttx_logit_bias.hip.h", CSRC / "ttx_syntax.hip.h", CSRC / "ttx_beam_mask.hip.h",
           CSRC / "ttx_select.h", CSRC / "ttx_tokenizer.h", CSRC / "ttx_drive.h", CSRC / "ttx_admit.h", INCLUDE / "ttx.h"]
SOURCES = UNITS + HEADERS
OBJ_DIR = CSRC / "build"

TTX_OK, TTX_ERR_INVALID, TTX_ERR_HIP, TTX_ERR_NO_DEVICE, TTX_ERR_REFERENCE, TTX_ERR_NOMEM = 0, -1, -2, -3, -4, -5
TTX_ERR_ROW_REPLAY = -6
TTX_ERR_MAX_STEPS = -7
# enum ttx_fold_order and the flag bits of ttx_fold_hypotheses
TTX_FOLD_FIRST, TTX_FOLD_SCORE, TTX_FOLD_COUNT = 0, 1, 2
TTX_FOLD_UNFINISHED_LAST, TTX_FOLD_DEBUG_NO_FILTER = 1, 2
FOLD_ORDERS = {"first": TTX_FOLD_FIRST, "score": TTX_FOLD_SCORE, "count": TTX_FOLD_COUNT}
# enum ttx_activation; the strings are the reference's `activation` init_arg
TTX_ACT_NONE, TTX_ACT_RELU, TTX_ACT_GELU = 0, 1, 2
ACTIVATIONS = {"relu": TTX_ACT_RELU, "gelu": TTX_ACT_GELU}


def activation_code(activation: str) -> int:
    """The ttx_activation of the reference's `activation` string; ValueError for anything but the two it can be here."""
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be 'relu' or 'gelu' (the exact erf GELU), got {activation!r}")
    return ACTIVATIONS[activation]


class TtxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libttx_hip error {code}: {msg}")
        self.code = code


class ReferenceError_(RuntimeError):
    """Raised where the reference implementation itself raises on the same input."""


class Config(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("src_vocab_size", C.c_int32), ("embedding_dim", C.c_int32),
                ("num_heads", C.c_int32), ("feedforward_dim", C.c_int32), ("num_encoder_layers", C.c_int32),
                ("num_decoder_layers", C.c_int32), ("pad_token", C.c_int32), ("max_positions", C.c_int32),
                ("layer_norm_eps", C.c_float)]


class Tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("numel", C.c_int64)]


class GenParams(C.Structure):
    _fields_ = [("max_len", C.c_int32), ("draft_len", C.c_int32), ("n_drafts", C.c_int32), ("pad_token", C.c_int32),
                ("bos_token", C.c_int32), ("eos_token", C.c_int32), ("replace_token", C.c_int32),
                ("want_logits", C.c_int32)]


class BeamParams(C.Structure):
    _fields_ = [("max_len", C.c_int32), ("n_best", C.c_int32), ("draft_len", C.c_int32), ("n_drafts", C.c_int32),
                ("smart_drafts_mode", C.c_int32), ("pad_token", C.c_int32), ("bos_token", C.c_int32),
                ("eos_token", C.c_int32), ("replace_token", C.c_int32), ("max_steps", C.c_int32)]


class BeamStats(C.Structure):
    _fields_ = [("model_calls", C.c_int64), ("input_lines", C.c_int64), ("running_rows", C.c_int64),
                ("accepted_tokens", C.c_int64), ("produced_non_pad_tokens", C.c_int64), ("verified_positions", C.c_int64),
                ("executed_positions", C.c_int64), ("kv_prefix_positions", C.c_int64), ("running_candidates", C.c_int64),
                ("src_tokens_padded", C.c_int64), ("encode_ms", C.c_double), ("decode_ms", C.c_double),
                ("out_width", C.c_int32), ("status", C.c_int32)]


class BeamSearchParams(C.Structure):
    _fields_ = [("max_len", C.c_int32), ("beam_size", C.c_int32), ("pad_token", C.c_int32), ("bos_token", C.c_int32),
                ("eos_token", C.c_int32)]


class BeamSearchStats(C.Structure):
    _fields_ = [("model_calls", C.c_int64), ("running_rows", C.c_int64), ("out_width", C.c_int32), ("pad_", C.c_int32)]


class SbsParams(C.Structure):
    """ttx_sbs_params: stochastic beam search; beam_size is K, the temperature is finite and > 0."""
    _fields_ = [("max_len", C.c_int32), ("beam_size", C.c_int32), ("temperature", C.c_float), ("pad_token", C.c_int32),
                ("bos_token", C.c_int32), ("eos_token", C.c_int32), ("seed", C.c_uint64)]


class SbsFilter(C.Structure):
    """ttx_sbs_filter: top_k 0 and top_p 1 are off."""
    _fields_ = [("top_k", C.c_int32), ("top_p", C.c_float)]


class SbsTrace(C.Structure):
    """ttx_sbs_trace: device arrays [max_len - 1, B, K] of parent rank, token, phi' and G' per level."""
    _fields_ = [(n, C.c_void_p) for n in ("d_parent", "d_token", "d_phi", "d_g")]


class DebugSbsStepArgs(C.Structure):
    """ttx_debug_sbs_step_args: one k_sbs_step launch's operands."""
    POINTERS = ("d_logits", "d_slot_of", "d_finished", "d_phi", "d_g", "d_gen", "d_key", "d_new_cand", "d_new_phi", "d_new_g",
                "d_parent", "d_new_len", "d_new_finished", "d_parent_draft", "d_summary", "d_tr_parent", "d_tr_token", "d_tr_phi",
                "d_tr_g")
    _fields_ = [(n, C.c_void_p) for n in POINTERS] + [("seed", C.c_uint64)] + \
               [(n, C.c_int32) for n in ("V", "ld", "width", "B", "beam", "K", "pad", "eos", "pos")] + [("inv_T", C.c_float)]


class SbsPoolStats(C.Structure):
    """ttx_sbs_pool_stats: sums over the pools of one ttx_sbs_generate_pool call."""
    _fields_ = [("model_calls", C.c_int64), ("running_rows", C.c_int64), ("src_tokens_padded", C.c_int64), ("live_slots", C.c_int64),
                ("decode_ms", C.c_double), ("status", C.c_int32), ("pad_", C.c_int32), ("d_src_running_rows", C.c_void_p)]


class DebugSbsStepPoolArgs(C.Structure):
    """ttx_debug_sbs_step_pool_args: one k_sbs_step_pool / k_sbs_step_pool_masked launch's operands."""
    POINTERS = ("d_logits", "d_slot_of", "d_finished", "d_phi", "d_g", "d_gen", "d_row_of", "d_level", "d_nlive", "d_key", "d_new_cand",
                "d_new_phi", "d_new_g", "d_parent", "d_new_len", "d_new_finished", "d_parent_draft", "d_nfin")
    _fields_ = [(n, C.c_void_p) for n in POINTERS] + [("seed", C.c_uint64)] + \
               [(n, C.c_int32) for n in ("V", "ld", "C", "K", "pad", "eos")] + [("inv_T", C.c_float)]


class DebugSbsPoolArgs(C.Structure):
    """ttx_debug_sbs_pool_args: the operands of one bookkeeping launch of the stochastic beam pool."""
    POINTERS = ("d_row_of", "d_level", "d_nlive", "d_nfin", "d_key", "d_pfx_len", "d_pfx_src", "d_run_acc", "d_cand_next", "d_len_next", "d_fin_next",
                "d_phi_next", "d_parent", "d_parent_draft", "d_cand_src_len", "d_g_in", "d_g_out", "d_len_all", "d_row_keys",
                "d_pfx_len_src", "d_out", "d_out_logp", "d_out_gumbel", "d_src_running", "d_dev_summary", "d_src_of", "d_new_slot", "d_valid_new",
                "d_src_valid", "d_memkv", "d_memkv_new")
    _fields_ = [(n, C.c_void_p) for n in POINTERS] + \
               [(n, C.c_int32) for n in ("C", "K", "max_len", "ld", "Ls_cap", "pad", "bos", "R", "first_row", "kv_row", "Ls_new")]


class GenStats(C.Structure):
    _fields_ = [("model_calls", C.c_int64), ("accepted_tokens", C.c_int64), ("produced_tokens", C.c_int64),
                ("verified_positions", C.c_int64), ("kv_prefix_positions", C.c_int64), ("src_positions", C.c_int64),
                ("encode_ms", C.c_double), ("decode_ms", C.c_double), ("src_tokens_padded", C.c_int64),
                ("status", C.c_int64)]


class SampleParams(C.Structure):
    """ttx_sample_params: temperature 0 is greedy, top_k 0 and top_p 1 are off."""
    _fields_ = [("max_len", C.c_int32), ("num_samples", C.c_int32), ("temperature", C.c_float), ("top_k", C.c_int32),
                ("top_p", C.c_float), ("pad_token", C.c_int32), ("bos_token", C.c_int32), ("eos_token", C.c_int32),
                ("seed", C.c_uint64)]


class Dist(C.Structure):
    """ttx_dist: a sampling distribution; temperature 0 is greedy, top_k 0 and top_p 1 are off."""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float)]


class SampleSpecParams(C.Structure):
    """ttx_sample_spec_params: the sampler's parameters and the copy drafts of the speculative form."""
    _fields_ = [("sample", SampleParams), ("draft_len", C.c_int32), ("n_drafts", C.c_int32), ("replace_token", C.c_int32),
                ("reserved", C.c_int32)]


class SampleOpts(C.Structure):
    """ttx_sample_opts: every option of a sampling call (prefix, proposal, logit bias); a zeroed struct is the plain call."""
    _fields_ = [("d_prefix", C.c_void_p), ("ld_prefix", C.c_int32), ("h_prefix_len", C.c_void_p),
                ("d_proposal", C.c_void_p), ("ld_proposal", C.c_int32), ("h_proposal_len", C.c_void_p),
                ("d_bias", C.c_void_p), ("ld_bias", C.c_int32)]

    @classmethod
    def of(cls, prefix_ptr=None, ld_prefix=0, h_prefix_len=None, proposal_ptr=None, ld_proposal=0, h_proposal_len=None, bias=None):
        """From the device pointers, the HOST length arrays (ctypes int32 arrays, which the caller keeps alive) and a contiguous
        float32 device tensor ``bias`` [sources, V] (or None)."""
        host = lambda a: None if a is None else C.cast(a, C.c_void_p)
        return cls(prefix_ptr, ld_prefix, host(h_prefix_len), proposal_ptr, ld_proposal, host(h_proposal_len),
                   None if bias is None else bias.data_ptr(), 0 if bias is None else int(bias.stride(0)))


class Syntax(C.Structure):
    """ttx_syntax: the class table (int8 [V] on the device) and the maximal length of the rule."""
    _fields_ = [("d_cls", C.c_void_p), ("max_len", C.c_int32)]

    @classmethod
    def arg(cls, d_cls=None, max_len: int = 0):
        """The ``syntax`` argument of a call: a reference to the struct for the int8 device tensor ``d_cls`` [V] (which the caller
        keeps alive until the call returns), or ``None`` (a NULL pointer: the unconstrained call) without a table."""
        return None if d_cls is None else C.byref(cls(d_cls.data_ptr(), int(max_len)))


class ScoreBatch(C.Structure):
    """ttx_score_batch: one (src, hyp) batch of a list scored by ttx_score_list_*; device pointers, then the shape."""
    _fields_ = [("d_src", C.c_void_p), ("d_hyp", C.c_void_p)] + [(n, C.c_int32) for n in ("B", "Ls", "N", "W", "ld_hyp")]


class ScoreChunk(C.Structure):
    """ttx_score_chunk: the sources order[first : first + count] in one pass of W hypothesis and Ls source columns."""
    _fields_ = [(n, C.c_int32) for n in ("first", "count", "N", "W", "Ls")]


class DebugScoreListArgs(C.Structure):
    """ttx_debug_score_list_args: the operands of one k_sl_extents / k_sl_pack / k_sl_unpack launch."""
    POINTERS = ("d_e", "d_ls", "d_n", "d_bad", "d_src_c", "d_hyp_c", "d_score_c", "d_length_c", "d_fin_c", "d_tok_c", "d_score",
                "d_length", "d_finished", "d_tok_logp")
    _fields_ = [(n, C.c_void_p) for n in POINTERS] + [(n, C.c_int32) for n in ("N", "W", "Ls", "eos")]


DEBUG_SCORE_LIST_OPS = ("extents", "pack", "unpack")     # ttx_debug_score_list's op, in order


class DebugPrefix(C.Structure):
    """ttx_debug_prefix: the forced prefixes of a debug launch (table, row length, sources; per-row length and table row)."""
    _fields_ = [("d_tok", C.c_void_p), ("ld", C.c_int32), ("n_sources", C.c_int32), ("d_len", C.c_void_p), ("d_src", C.c_void_p)]


class DebugAcceptArgs(C.Structure):
    """ttx_debug_accept_args: the device arrays and scalars of one k_accept / k_greedy_accept launch."""
    _fields_ = [(n, C.c_void_p) for n in ("d_act_idx", "d_front", "d_gen", "d_drafts", "d_pred", "d_rec", "d_out", "d_haspad",
                                          "d_traj", "d_fin_step", "d_rstep", "d_row_of", "d_pool_out", "d_pool_traj",
                                          "d_pool_fin_step")] + \
               [(n, C.c_int32) for n in ("gen_ld", "traj_ld", "pool_rows", "row_rule", "pool", "B", "N", "D", "Ls", "max_len",
                                         "pad", "bos", "eos", "greedy", "threads")]


class DebugPoolFillArgs(C.Structure):
    """ttx_debug_pool_fill_args: the device arrays and scalars of one admission of the sampling pool."""
    POINTERS = ("d_act_idx", "d_front", "d_haspad", "d_rstep", "d_row_of", "d_src_len", "d_key", "d_sample", "d_row_keys", "d_gen",
                "d_drafts", "d_drafts_new", "d_src_valid", "d_valid_new", "d_memkv", "d_memkv_new", "d_out")
    _fields_ = [(n, C.c_void_p) for n in POINTERS] + \
               [(n, C.c_int32) for n in ("B", "N", "D", "n_active", "n_sources", "per_src", "first_src", "Ls_new", "Ls_cap", "gen_ld",
                                         "kv_row", "max_len", "out_rows", "bos", "pad")]


def _debug_args(name: str, pointers, ints, int64s=()):
    """A ttx_debug_*_args struct of include/ttx.h: device pointers, then int64 strides, then int32 scalars."""
    fields = [(n, C.c_void_p) for n in pointers] + [(n, C.c_int64) for n in int64s] + [(n, C.c_int32) for n in ints]
    return type(name, (C.Structure,), {"_fields_": fields, "POINTERS": tuple(pointers), "__doc__": f"ttx_{name}: one launch's operands."})


# the beam family (csrc/ttx_loop_kernels.hip.h), one struct per kernel
DebugBsPrepArgs = _debug_args("debug_bs_prep_args",
                              ("d_cand_next", "d_len_next", "d_fin_next", "d_logp_next", "d_drafts_all", "d_lib", "d_gen", "d_front",
                               "d_len", "d_active", "d_finished", "d_logp", "d_per_cand", "d_drafts32"),
                              ("ld", "max_cand", "n_cand", "beam", "dl", "N", "pad", "smart", "n_lib", "lib_ld", "D0"))
DebugBsListArgs = _debug_args("debug_bs_list_args",
                              ("d_active", "d_per_cand", "d_len", "d_act_idx", "d_slot_of", "d_prev_len", "d_summary"), ("n_cand", "N", "dl"))
DebugBsHitsArgs = _debug_args("debug_bs_hits_args",
                              ("d_logits", "d_finished", "d_slot_of", "d_per_cand", "d_drafts32", "d_hit", "d_dl_of"),
                              ("V", "max_cand", "n_cand", "N", "dl", "K", "vpl"))
DebugBsLeavesArgs = _debug_args("debug_bs_leaves_args",
                                ("d_logits", "d_finished", "d_slot_of", "d_per_cand", "d_drafts32", "d_logp", "d_hit", "d_best_n",
                                 "d_best_slot", "d_chosen", "d_leaf_score", "d_leaf_tok", "d_leaf_cnt", "d_live", "d_dl_of", "d_grp_of",
                                 "d_cand_batch"),
                                ("V", "max_cand", "n_cand", "N", "dl", "K", "bos", "pad", "smart", "max_group", "vpl"))
DebugBeamSelectArgs = _debug_args("debug_beam_select_args",
                                  ("d_leaf_score", "d_leaf_tok", "d_leaf_cnt", "d_cand", "d_len", "d_chosen", "d_chosen_slot",
                                   "d_finished", "d_new_cand", "d_new_logp", "d_parent", "d_parent_draft", "d_mark", "d_summary",
                                   "d_new_len", "d_new_finished"),
                                  ("width", "ld_in", "ld_out", "B", "beam", "dl", "K", "pad", "eos"))
DebugBeamStepArgs = _debug_args("debug_beam_step_args",
                                ("d_logits", "d_slot_of", "d_finished", "d_score", "d_gen", "d_new_cand", "d_new_score", "d_parent",
                                 "d_new_len", "d_new_finished", "d_parent_draft", "d_summary"),
                                ("V", "ld", "width", "B", "beam", "K", "pad", "eos"))
DebugTreeCacheArgs = _debug_args("debug_tree_cache_args",
                                 ("d_len", "d_parent", "d_parent_draft", "d_prev_len", "d_active", "d_k_old", "d_v_old", "d_k_new",
                                  "d_v_new", "d_qkv_prev", "d_prev_slot_of", "d_slot_parent", "d_slot_self"),
                                 ("max_cand", "layers", "prev_N", "prev_D", "d"),
                                 ("cache_layer_stride", "cache_seq_stride", "qkv_layer_stride"))
# the pool's bookkeeping kernels (k_bsp_init .. k_bsp_publish): one struct for the eight of them
DebugBspArgs = _debug_args("debug_bsp_args",
                           ("d_row_of", "d_slot_batch", "d_src_acc", "d_src_state", "d_tok", "d_drafts_all", "d_bat_id", "d_bat_iter",
                            "d_bat_dl", "d_bat_grp", "d_bat_live", "d_bat_nfin", "d_bat_longest_fin", "d_bat_longest_cur", "d_bat_state",
                            "d_bat_given", "d_cand_next", "d_len_next", "d_fin_next", "d_logp_next", "d_parent", "d_parent_draft",
                            "d_gen", "d_front", "d_len", "d_active", "d_finished", "d_live", "d_logp", "d_per_cand", "d_drafts32",
                            "d_cand_dl", "d_cand_batch", "d_cache_slot", "d_cache_slot_parent", "d_chosen_slot", "d_chosen",
                            "d_leaf_score", "d_leaf_tok", "d_leaf_cnt", "d_dev_summary", "d_out", "d_trace_len", "d_summary",
                            "d_len_all", "d_batch_all", "d_given_all", "d_src_of", "d_cand_src_len", "d_new_slot", "d_tok_new",
                            "d_valid_new", "d_src_valid", "d_drafts_new", "d_memkv", "d_memkv_new"),
                           ("C", "K", "N", "D0", "Ls_cap", "max_len", "ld", "smart", "lib_ld", "pad", "bos", "eos", "repl", "max_steps",
                            "T_cap", "R", "first_row", "kv_row", "Ls_new"))
DEBUG_BSP_OPS = ("init", "admit", "fill", "prep", "select", "batches", "retire", "publish")     # ttx_debug_bsp's op, in order
DEBUG_SBS_POOL_OPS = ("init", "admit", "fill", "retire", "publish")     # ttx_debug_sbs_pool's op, in order (words: DEBUG_BSP_WORDS)
DEBUG_BSP_WORDS = 12              # int64 words of ttx_debug_bsp's host array: 8 of the BeamCounters, 4 of the BeamPoolHost
DEBUG_BS_LIST_WORDS = 21          # int64 words of ttx_debug_bs_list's host array: 8 of the BeamCounters, 13 of the DecState

DEBUG_ACCEPT_BLOCK_WORDS = 264   # int32 words of the AcceptBlk between k_accept_slots and k_accept_finish (ttx_debug_accept_block)
DEBUG_ACCEPT_STATE_WORDS = 17     # int64 words of ttx_debug_accept's host `state` array (include/ttx.h)


# every symbol include/ttx.h declares: (name, restype, argtypes)
_VP, _I, _I64P = C.c_void_p, C.c_int, C.c_void_p
SYMBOLS = {
    "ttx_abi_version": (C.c_int, []),
    "ttx_last_error": (C.c_char_p, []),
    "ttx_device_count": (C.c_int, []),
    "ttx_model_create": (C.c_int, [C.POINTER(Config), C.POINTER(Tensor), _I, _I, C.POINTER(_VP)]),
    "ttx_model_destroy": (None, [_VP]),
    "ttx_model_create_empty": (C.c_int, [C.POINTER(Config), _I, C.POINTER(_VP)]),
    "ttx_model_blob": (C.c_int, [_VP, C.POINTER(_VP), C.POINTER(C.c_int64)]),
    "ttx_model_set_activation": (C.c_int, [_VP, _I]),
    "ttx_model_activation": (C.c_int, [_VP]),
    "ttx_session_create": (C.c_int, [_VP, C.POINTER(_VP)]),
    "ttx_session_destroy": (None, [_VP]),
    "ttx_encode_src": (C.c_int, [_VP, _VP, _I, _I, _VP, _VP]),
    "ttx_decode_tgt": (C.c_int, [_VP, _VP, _I, _I, _VP, _VP, _VP, _I, _I, _VP, _VP]),
    "ttx_forward": (C.c_int, [_VP, _VP, _I, _I, _VP, _I, _VP, _VP]),
    "ttx_token_metrics": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "ttx_teacher_forced_eval": (C.c_int, [_VP, _VP, _I, _I, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "ttx_hypothesis_logprobs": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "ttx_score_hypotheses": (C.c_int, [_VP, _VP, _I, _I, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ttx_score_list_extents": (C.c_int, [_VP, C.POINTER(ScoreBatch), _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "ttx_score_list_run": (C.c_int, [_VP, C.POINTER(ScoreBatch), _I, C.POINTER(C.c_int32), _I, C.POINTER(ScoreChunk), _I, _I, _VP, _VP,
                                     _VP, _VP, C.POINTER(C.c_int64), _VP]),
    "ttx_debug_score_list": (C.c_int, [_VP, _I, C.POINTER(ScoreBatch), _I, C.POINTER(C.c_int32), _I, C.POINTER(C.c_int64),
                                       C.POINTER(DebugScoreListArgs), _VP]),
    "ttx_fold_hypotheses": (C.c_int, [_VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ttx_hypothesis_alternatives": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ttx_score_alternatives": (C.c_int, [_VP, _VP, _I, _I, _VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ttx_hypothesis_logq": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _I, _I, C.POINTER(Dist), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ttx_score_proposal": (C.c_int, [_VP, _VP, _I, _I, _VP, _I, _I, _I, _I, C.POINTER(Dist), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                    _VP, _VP, _VP, _VP]),
    "ttx_attention_maps": (C.c_int, [_VP, _VP, _I, _I, _VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "ttx_attn_probs_key_limit": (C.c_int, [_I]),
    "ttx_debug_attn_probs": (C.c_int, [_VP, _VP, _I, _VP, _I, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, C.c_float, _VP, _VP, _VP, _VP]),
    "ttx_make_drafts": (C.c_int, [_VP, _VP, _I, _I, _I, _I, _I, _I, _I, _I, _I, _VP, _VP]),
    "ttx_greedy_speculative_generate": (C.c_int, [_VP, _VP, _I, _I, C.POINTER(GenParams), _VP, C.POINTER(GenStats), _VP]),
    "ttx_greedy_generate": (C.c_int, [_VP, _VP, _I, _I, C.POINTER(GenParams), _VP, C.POINTER(GenStats), _VP]),
    "ttx_sample_generate": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SampleParams), _VP, C.POINTER(GenStats), _VP]),
    "ttx_sample_speculative_generate": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SampleSpecParams), _VP, C.POINTER(GenStats), _VP]),
    "ttx_sample_generate_prefix": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SampleParams), _VP, _I, C.POINTER(C.c_int32), _VP,
                                            C.POINTER(GenStats), _VP]),
    "ttx_sample_speculative_generate_prefix": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SampleSpecParams), _VP, _I,
                                                        C.POINTER(C.c_int32), _VP, C.POINTER(GenStats), _VP]),
    "ttx_sample_speculative_generate_pool_prefix": (C.c_int, [C.POINTER(_VP), _I, _VP, _I, _I, C.POINTER(C.c_int32), _VP, _I,
                                                             C.POINTER(SampleSpecParams), _VP, _I, C.POINTER(C.c_int32), _VP,
                                                             C.POINTER(GenStats), _VP]),
    "ttx_sample_speculative_generate_proposal": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SampleSpecParams), _VP, _I,
                                                          C.POINTER(C.c_int32), _VP, _I, C.POINTER(C.c_int32), _VP,
                                                          C.POINTER(GenStats), _VP]),
    "ttx_sample_speculative_generate_pool_proposal": (C.c_int, [C.POINTER(_VP), _I, _VP, _I, _I, C.POINTER(C.c_int32), _VP, _I,
                                                               C.POINTER(SampleSpecParams), _VP, _I, C.POINTER(C.c_int32), _VP, _I,
                                                               C.POINTER(C.c_int32), _VP, C.POINTER(GenStats), _VP]),
    "ttx_sample_generate_ex": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SampleParams), C.POINTER(SampleOpts), _VP, C.POINTER(GenStats), _VP]),
    "ttx_sample_speculative_generate_ex": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SampleSpecParams), C.POINTER(SampleOpts), _VP,
                                                    C.POINTER(GenStats), _VP]),
    "ttx_sample_speculative_generate_pool_ex": (C.c_int, [C.POINTER(_VP), _I, _VP, _I, _I, C.POINTER(C.c_int32), _VP, _I,
                                                         C.POINTER(SampleSpecParams), C.POINTER(SampleOpts), _VP, C.POINTER(GenStats), _VP]),
    "ttx_hypothesis_logq_bias": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _I, _I, C.POINTER(Dist), _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP,
                                          _VP, _VP, _VP]),
    "ttx_score_proposal_bias": (C.c_int, [_VP, _VP, _I, _I, _VP, _I, _I, _I, _I, C.POINTER(Dist), _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP,
                                         _VP, _VP, _VP, _VP, _VP, _VP]),
    "ttx_sbs_generate_bias": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SbsParams), C.POINTER(SbsFilter), _VP, _I, _VP, _VP, _I, _VP, _VP,
                                       _VP, C.POINTER(SbsTrace), C.POINTER(BeamSearchStats), _VP]),
    "ttx_debug_logit_bias_launches": (C.c_int, [_VP]),
    "ttx_sample_generate_syntax": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SampleParams), C.POINTER(SampleOpts), C.POINTER(Syntax), _VP,
                                            C.POINTER(GenStats), _VP]),
    "ttx_sample_speculative_generate_syntax": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SampleSpecParams), C.POINTER(SampleOpts),
                                                        C.POINTER(Syntax), _VP, C.POINTER(GenStats), _VP]),
    "ttx_sample_speculative_generate_pool_syntax": (C.c_int, [C.POINTER(_VP), _I, _VP, _I, _I, C.POINTER(C.c_int32), _VP, _I,
                                                             C.POINTER(SampleSpecParams), C.POINTER(SampleOpts), C.POINTER(Syntax), _VP,
                                                             C.POINTER(GenStats), _VP]),
    "ttx_hypothesis_logq_syntax": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _I, _I, C.POINTER(Dist), _VP, _VP, _I, _I, C.POINTER(Syntax), _VP, _VP,
                                            _VP, _VP, _VP, _VP, _VP, _VP]),
    "ttx_score_proposal_syntax": (C.c_int, [_VP, _VP, _I, _I, _VP, _I, _I, _I, _I, C.POINTER(Dist), _VP, _VP, _I, C.POINTER(Syntax), _VP, _VP,
                                           _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ttx_debug_syntax_mask": (C.c_int, [_VP, _I, _VP, _I, _I, _VP, _VP, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "ttx_debug_syntax_launches": (C.c_int, [_VP]),
    "ttx_debug_logit_bias": (C.c_int, [_VP, _VP, _I, _I, _VP, _VP, _I, _VP, _I, _VP, _VP, _I, _I, _VP]),
    "ttx_greedy_speculative_generate_many": (C.c_int, [C.POINTER(_VP), _I, _I, C.POINTER(_VP), C.POINTER(C.c_int),
                                                      C.POINTER(C.c_int), C.POINTER(GenParams), C.POINTER(_VP),
                                                      C.POINTER(GenStats), _VP]),
    "ttx_greedy_speculative_generate_rows": (C.c_int, [C.POINTER(_VP), _I, _I, C.POINTER(_VP), C.POINTER(C.c_int),
                                                      C.POINTER(C.c_int), C.POINTER(GenParams), C.POINTER(_VP),
                                                      C.POINTER(_VP), C.POINTER(_VP), C.POINTER(GenStats), _VP]),
    "ttx_greedy_speculative_generate_pool": (C.c_int, [C.POINTER(_VP), _I, _VP, _I, _I, C.POINTER(C.c_int32), _I,
                                                      C.POINTER(GenParams), _VP, _VP, _VP, C.POINTER(GenStats), _VP]),
    "ttx_sample_speculative_generate_pool": (C.c_int, [C.POINTER(_VP), _I, _VP, _I, _I, C.POINTER(C.c_int32), _VP, _I,
                                                      C.POINTER(SampleSpecParams), _VP, C.POINTER(GenStats), _VP]),
    "ttx_beam_speculative_generate": (C.c_int, [_VP, _VP, _I, _I, C.POINTER(BeamParams), _VP, C.POINTER(BeamStats), _VP]),
    "ttx_beam_speculative_generate_many": (C.c_int, [C.POINTER(_VP), _I, _I, C.POINTER(_VP), C.POINTER(C.c_int),
                                                    C.POINTER(C.c_int), C.POINTER(BeamParams), C.POINTER(_VP),
                                                    C.POINTER(BeamStats), _VP]),
    "ttx_beam_speculative_generate_pool": (C.c_int, [C.POINTER(_VP), _I, _VP, _I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I,
                                                    C.POINTER(C.c_int32), _I, C.POINTER(BeamParams), _VP, _VP, _VP, _I,
                                                    C.POINTER(BeamStats), _VP]),
    "ttx_beam_generate": (C.c_int, [_VP, _VP, _I, _I, C.POINTER(BeamSearchParams), _VP, C.POINTER(BeamSearchStats), _VP]),
    "ttx_beam_generate_constrained": (C.c_int, [_VP, _VP, _I, _I, C.POINTER(BeamSearchParams), _VP, _I, C.POINTER(Syntax), _VP, _I, _VP,
                                                _VP, _VP, C.POINTER(BeamSearchStats), _VP]),
    "ttx_sbs_generate": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SbsParams), _VP, _VP, _VP, C.POINTER(SbsTrace),
                                  C.POINTER(BeamSearchStats), _VP]),
    "ttx_sbs_generate_ex": (C.c_int, [_VP, _VP, _I, _I, _VP, C.POINTER(SbsParams), C.POINTER(SbsFilter), _VP, _I, _VP, _VP, _VP, _VP,
                                     C.POINTER(SbsTrace), C.POINTER(BeamSearchStats), _VP]),
    "ttx_sbs_generate_pool": (C.c_int, [_VP, _I, _VP, _I, _I, C.POINTER(C.c_int32), _VP, _I, C.POINTER(SbsParams), C.POINTER(SbsFilter),
                                       _VP, _I, _VP, _VP, _VP, _VP, C.POINTER(SbsPoolStats), _VP]),
    "ttx_nucleus_mask": (C.c_int, [_VP, _VP, _I, _I, C.c_float, _I, C.c_float, _VP, _VP]),
    "ttx_accepted_lengths": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, C.c_float, _I, _VP, _VP]),
    "ttx_ragged_topk": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP]),
    "ttx_tokenizer_create": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_int32), _I, C.POINTER(_VP)]),
    "ttx_tokenizer_destroy": (None, [_VP]),
    "ttx_tokenizer_encode": (C.c_int, [_VP, C.c_char_p, _VP, _I]),
    "ttx_tokenizer_encode_batch": (C.c_int, [_VP, C.POINTER(C.c_char_p), _I, _VP, _I]),
    "ttx_tokenizer_decode": (C.c_int, [_VP, _VP, _I, _VP, _I]),
    "ttx_debug_step_snapshot": (C.c_int, [_VP, C.POINTER(C.c_int32), _VP, _VP, _VP, _VP]),
    "ttx_debug_gemm_bench": (C.c_int, [_VP, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ttx_debug_gemm": (C.c_int, [_VP, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _I, _I, _I, _I, _I, C.c_int64, _I, _I,
                                 C.POINTER(C.c_int32), _VP]),
    "ttx_debug_gemm_act": (C.c_int, [_VP, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _I, _I, _I, _I, _I, C.c_int64, _I, _I,
                                     C.POINTER(C.c_int32), _VP]),
    "ttx_debug_finish_ln": (C.c_int, [_VP, _VP, _I, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, C.c_float, _VP]),
    "ttx_debug_attn": (C.c_int, [_VP, _VP, _I, _VP, _VP, _I, _VP, _I, C.c_float, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                 C.c_int64, _VP, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int32), _VP]),
    "ttx_debug_attn_hd": (C.c_int, [_VP, _VP, _I, _VP, _VP, _I, _VP, _I, _I, C.c_float, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                    _VP, C.c_int64, _VP, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int32), _VP]),
    "ttx_debug_attn_as": (C.c_int, [_VP, _VP, _I, _VP, _VP, _I, _VP, _I, _I, C.c_float, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                    _VP, C.c_int64, _VP, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int32), _I, _I, _VP]),
    "ttx_debug_argmax": (C.c_int, [_VP, _VP, _I, _VP, _VP, _I, _VP]),
    "ttx_debug_sample": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _I, C.POINTER(SampleParams), _VP]),
    "ttx_debug_sample_step": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, C.POINTER(SampleParams), _VP]),
    "ttx_debug_sample_accept": (C.c_int, [_VP, C.POINTER(DebugAcceptArgs), C.POINTER(C.c_int64), _VP]),
    "ttx_debug_sample_step_select": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, C.POINTER(SampleParams),
                                              _VP, _I, _VP]),
    "ttx_debug_prefix_drafts": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, C.POINTER(DebugPrefix), _I, _I, _I, _VP]),
    "ttx_debug_proposal_drafts": (C.c_int, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _I, _VP, _VP, C.POINTER(DebugPrefix), _I, _I, _I, _I,
                                            _I, _VP]),
    "ttx_debug_sample_prefix": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _I, C.POINTER(SampleParams),
                                         C.POINTER(DebugPrefix), _VP]),
    "ttx_debug_sample_step_prefix": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, C.POINTER(SampleParams),
                                              _VP, _I, C.POINTER(DebugPrefix), _VP]),
    "ttx_debug_sample_accept_pool": (C.c_int, [_VP, C.POINTER(DebugAcceptArgs), C.POINTER(C.c_int64), _VP, _I, _VP]),
    "ttx_debug_pool_fill_sample": (C.c_int, [_VP, C.POINTER(DebugPoolFillArgs), C.POINTER(C.c_int32), _VP]),
    "ttx_debug_embed": (C.c_int, [_VP, _VP, _I, _VP, _I, _I, _VP, _VP, _I, _I, _VP, _VP, _VP, _I, _VP, _I, _I, _I, _I, _I, _VP]),
    "ttx_debug_accept": (C.c_int, [_VP, C.POINTER(DebugAcceptArgs), C.POINTER(C.c_int64), _VP]),
    "ttx_debug_accept_block": (C.c_int, [_VP, C.POINTER(C.c_int32), _I, _VP]),
    "ttx_debug_bs_prep": (C.c_int, [_VP, C.POINTER(DebugBsPrepArgs), _VP]),
    "ttx_debug_bs_list": (C.c_int, [_VP, C.POINTER(DebugBsListArgs), C.POINTER(C.c_int64), _VP]),
    "ttx_debug_bs_hits": (C.c_int, [_VP, C.POINTER(DebugBsHitsArgs), _VP]),
    "ttx_debug_bs_leaves": (C.c_int, [_VP, C.POINTER(DebugBsLeavesArgs), _VP]),
    "ttx_debug_beam_select": (C.c_int, [_VP, C.POINTER(DebugBeamSelectArgs), _VP]),
    "ttx_debug_beam_step": (C.c_int, [_VP, C.POINTER(DebugBeamStepArgs), _VP]),
    "ttx_debug_beam_step_masked": (C.c_int, [_VP, C.POINTER(DebugBeamStepArgs), C.POINTER(DebugPrefix), _VP]),
    "ttx_debug_beam_step_masked_launches": (C.c_int, [_VP]),
    "ttx_debug_sbs_step": (C.c_int, [_VP, C.POINTER(DebugSbsStepArgs), _VP]),
    "ttx_debug_sbs_step_ex": (C.c_int, [_VP, C.POINTER(DebugSbsStepArgs), _I, C.c_float, C.POINTER(DebugPrefix), _I, _VP]),
    "ttx_debug_sbs_step_pool": (C.c_int, [_VP, C.POINTER(DebugSbsStepPoolArgs), _I, _I, C.c_float, C.POINTER(DebugPrefix), _VP]),
    "ttx_debug_sbs_pool": (C.c_int, [_VP, _I, C.POINTER(DebugSbsPoolArgs), C.POINTER(C.c_int64), _VP]),
    "ttx_debug_tree_cache": (C.c_int, [_VP, C.POINTER(DebugTreeCacheArgs), _VP]),
    "ttx_debug_bsp": (C.c_int, [_VP, _I, C.POINTER(DebugBspArgs), C.POINTER(C.c_int64), _VP]),
    "ttx_debug_kvcopy": (C.c_int, [_VP, _VP, _I, _VP, C.c_int64, _VP, _VP, C.c_int64, C.c_int64, _I, _I, _I, _I, _I, _VP]),
    "ttx_debug_kvcopy_split": (C.c_int, [_VP, _VP, _I, _VP, C.c_int64, _VP, _VP, C.c_int64, C.c_int64, _I, _I, _I, _I, _I, _VP, _VP,
                                         C.c_int64, _VP]),
    "ttx_debug_probe_split": (C.c_int, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, C.POINTER(C.c_int32), _VP]),
    "ttx_debug_merge_pred": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP]),
    "ttx_debug_probe_split_select": (C.c_int, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_int32), _VP]),
    "ttx_debug_merge_pred_select": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP]),
    "ttx_debug_kvcopy_select": (C.c_int, [_VP, _VP, _I, _VP, C.c_int64, _VP, _VP, C.c_int64, C.c_int64, _I, _I, _I, _I, _I, _VP, _VP,
                                          C.c_int64, _VP, _VP, _VP]),
    "ttx_debug_embed_select": (C.c_int, [_VP, _VP, _I, _VP, _I, _I, _VP, _VP, _VP, _VP, _I, _VP, _I, _I, _I, _I, _VP, _I, _VP]),
    "ttx_debug_attn_select": (C.c_int, [_VP, _VP, _I, _VP, _VP, _I, _VP, _I, C.c_float, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                        C.c_int64, _VP, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int32), _VP, _VP, _VP]),
    "ttx_pool_last_counters": (C.c_int, [_VP, C.POINTER(C.c_int64)]),
    "ttx_attn_staged_key_limit": (C.c_int, [_I, _I]),
    "ttx_debug_attn_kernels_seen": (C.c_int, [_VP]),
    "ttx_last_kernel_profile": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
}

_lib = None


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def needs_build() -> bool:
    if not LIB_PATH.exists():
        return True
    t = LIB_PATH.stat().st_mtime
    return any(src.stat().st_mtime > t for src in SOURCES)


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile the HIP library for gfx950 in-tree (cross-compiles without a GPU): one object per translation unit, in
    parallel, objects newer than their unit and every header are kept."""
    if not force and not needs_build():
        return LIB_PATH
    OBJ_DIR.mkdir(exist_ok=True)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{INCLUDE}"] + os.environ.get("TTX_HIPCC_FLAGS", "").split()
    newest_header = max(h.stat().st_mtime for h in HEADERS)
    jobs, objs = [], []
    for unit in UNITS:
        obj = OBJ_DIR / (unit.stem + ".o")
        objs.append(str(obj))
        if not force and obj.exists() and obj.stat().st_mtime > max(unit.stat().st_mtime, newest_header) \
                and not os.environ.get("TTX_HIPCC_FLAGS"):
            continue
        cmd = [hipcc_path(), *flags, "-c", str(unit), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd))
        jobs.append((cmd, subprocess.Popen(cmd)))
    for cmd, proc in jobs:
        if proc.wait() != 0:
            raise subprocess.CalledProcessError(proc.returncode, cmd)
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(LIB_PATH), *objs]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


def lib():
    """Load (building first if the sources are newer) and type every exported symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if needs_build():
        build()
    handle = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(handle, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if handle.ttx_abi_version() != 4:
        raise RuntimeError("libttx_hip.so ABI version mismatch")
    _lib = handle
    return _lib


def check(code: int) -> None:
    if code == TTX_OK:
        return
    msg = lib().ttx_last_error().decode("utf-8", "replace")
    if code == TTX_ERR_REFERENCE:
        raise ReferenceError_(msg)
    if code == TTX_ERR_MAX_STEPS:
        raise RuntimeError("beam-speculative loop exceeded max_steps (non-terminating input)")
    raise TtxError(code, msg)
