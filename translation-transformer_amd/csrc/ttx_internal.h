// Host-side types shared by the translation units of libttx_hip.so (ttx_api.hip: C ABI, runtime, loop kernels;
// ttx_gemm.hip: GEMM family; ttx_attn.hip: attention family): the model and its weight layout, the session with its
// workspaces (declared once, in TTX_SESSION_BUFS) and its two caches of captured graphs (GraphCache, keyed by GraphKey).
// Kernels are launched from the unit that defines them; the other units reach them through the launchers declared at the
// bottom.  Two host-only headers (no HIP, compiled by the host tests as well) belong to ttx_api.hip: ttx_drive.h, the core of the
// polling loops (round-robin turns over the jobs of a call, watchdog, first error), and ttx_admit.h, the admission policy of the
// two pools (pool count and size, which batches a pool takes, length buckets).
#pragma once
#include "ttx.h"
#include "ttx_common.hip.h"

#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace ttx {
struct BeamHost;
struct BeamPoolHost;
}

struct LayerW {
  // offsets (in floats) into the blob
  size_t sa_in_w, sa_in_b, sa_out_w, sa_out_b;
  size_t ca_in_w, ca_in_b, ca_out_w, ca_out_b;  // decoder only
  size_t l1_w, l1_b, l2_w, l2_b;
  size_t n1_w, n1_b, n2_w, n2_b, n3_w, n3_b;
};

struct ttx_model {
  ttx_config cfg;
  int device;
  int activation = TTX_ACT_RELU;   // FFN non-linearity (ttx_model_set_activation): fixed once a session exists
  int n_sessions = 0;              // sessions ever created on this model

  int n_cu = 256;                  // compute units of the device (grids sized to the machine: k_attn3s)
  float* blob = nullptr;
  size_t blob_floats = 0;
  std::map<std::string, std::pair<size_t, size_t>> index;  // name -> (offset, numel)
  std::vector<LayerW> enc, dec;
  size_t src_emb, tgt_emb, enc_norm_w, enc_norm_b, dec_norm_w, dec_norm_b, cls_w, cls_b, pe;
  size_t cross_kv_w, cross_kv_b;  // packed [Ld*2d, d] / [Ld*2d]: cross-attention K,V rows of every decoder layer
  const float* p(size_t off) const { return blob + off; }
};

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  uint64_t* owner_gen = nullptr;   // the owning session's alloc_generation: bumped whenever this buffer moves
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Which kernels carry a verify step's GEMMs.  Every contraction is DEFINED as the ordered sum of fixed K slices, each
// accumulated from zero in k order (ttx_gemm.hip), and both variants evaluate exactly that sum — so the choice is free
// to follow the live row count of a step (it is made per step on the host) without touching a single bit of the result.
//   GV_BIG    one workgroup walks all slices of its output tile (128x64 / 64x64 tiles by live row count)
//   GV_SMALL  short dependent chains for steps of a few hundred rows: one wave per slice (32x32 tiles) for the K = 256
//             GEMMs up to 768 columns, one workgroup per slice (split-K slabs, summed in order by k_finish_ln) for FFN2
//   GV_BIG_FFN2_SLABS  GV_BIG for every GEMM of the step except FFN2, which runs as in GV_SMALL (between small_rows and
//             ffn2_slab_rows live rows one workgroup per 256-k slice beats the 128x64 / 64x64 tiles walking all 2 048 k's)
//   GV_MID    between qkv_small_rows and small_rows: the short-chain kernels for the d-wide K = d GEMMs, the classifier and FFN2,
//             the tiles for QKV and FFN1 (a 32x32 launch over 768 columns loses to 64x64 tiles from about 800 rows on)
enum GemmVariant { GV_BIG = 0, GV_SMALL = 1, GV_BIG_FFN2_SLABS = 2, GV_MID = 3 };

// Kernel of a GEMM launch as ttx_debug_gemm reports it (include/ttx.h); GK_BODY_128x64 is or-ed in when k_gemm24 takes its
// 128x64 body for the launch's live row count.
enum GemmKernelId { GK_GEMM3 = 1, GK_GEMM_TN = 2, GK_GEMM24_4 = 3, GK_GEMM24_0 = 4, GK_GEMM2_1 = 5, GK_GEMM2_2 = 6, GK_GEMM2_4 = 7,
                    GK_GEMM2_0 = 8, GK_BODY_128x64 = 16 };

// Kernel of an attention launch as ttx_debug_attn selects and reports it (include/ttx.h).
enum AttnKernelId { AK_ATTN = 1, AK_ATTN2 = 2, AK_ATTN3 = 3, AK_ATTN3S = 4, AK_ATTN1 = 5 };

// Key of a captured launch sequence: the GraphSite that enqueues it, then every scalar the sequence depends on, in the order
// the site lists them (the device pointers it bakes in are covered by ttx_session::alloc_generation).
//   verify step (GS_STEP_*)       B, Ls, N, D, max_len, key capacity, GemmVariant, phase (slot pool: 0 the whole step in one pass,
//                                 1 probe, 2 draft pass + accept, 3 accept alone; 4, 5, 6: the same three under draft select; else 0)
//   GS_BEAM_ITER, GS_BEAM_POOL_ITER   see beam_launch_iter / bpool_launch_iter
//   GS_SBS_POOL_ITER              see sbsp_launch_iter: a site of its own, never a graph of the beam-speculative pool
//   GS_STEP_SAMPLE                the greedy step's key with k_sample in k_argmax's place (ttx_sample_generate); B counts decoder rows
//   GS_STEP_SAMPLE_SPEC           the speculative step's key with k_sample_step and k_sample_accept in k_argmax's and k_accept's place
//                                 (ttx_sample_speculative_generate); B counts decoder rows
//   GS_STEP_POOL_SAMPLE           GS_STEP_POOL's key and phases with k_sample_step and the sampling accept in k_argmax's and k_accept's
//                                 place (ttx_sample_speculative_generate_pool): never a graph of the greedy pool
//   GS_STEP_*_PREFIX              the three sampling sites of a prompted call (forced prefixes): the same keys; k_prefix_drafts leads
//                                 the speculative ones and the sampling kernels carry the session's prefix table (row length max_len)
//   GS_STEP_*_PROPOSAL            the two speculative sampling sites of a proposed call (proposal drafts): the same keys with the
//                                 context length of k_proposal_drafts appended; that kernel leads the step, the sampling kernels
//                                 carry no table
enum GraphSite { GS_STEP_SPECULATIVE = 0, GS_STEP_GREEDY = 1, GS_STEP_ROW_RULE = 2, GS_STEP_POOL = 3, GS_BEAM_ITER = 4, GS_BEAM_POOL_ITER = 5,
                 GS_STEP_SAMPLE = 6, GS_STEP_SAMPLE_SPEC = 7, GS_STEP_POOL_SAMPLE = 8,
                 GS_STEP_SAMPLE_PREFIX = 9, GS_STEP_SAMPLE_SPEC_PREFIX = 10, GS_STEP_POOL_SAMPLE_PREFIX = 11,
                 GS_STEP_SAMPLE_SPEC_PROPOSAL = 12, GS_STEP_POOL_SAMPLE_PROPOSAL = 13, GS_SBS_POOL_ITER = 14,
                 // or-ed into the site of a sampling step that carries a per-source logit bias (k_logit_bias between the classifier
                 // and the sampling kernel, reading the session's table): the key of the unbiased step is untouched, and a biased
                 // step is never replayed for an unbiased call
                 GS_LOGIT_BIAS = 256,
                 // or-ed into the site of a sampling step under a syntax constraint (k_syntax_mask after k_logit_bias, reading the
                 // session's class table): a constrained step has keys of its own; the rule's max_len is the step's, which every key holds
                 GS_SYNTAX = 512 };
typedef std::vector<int> GraphKey;

// Captured graphs of one family of keys.  A key runs eagerly the first time it is seen (`warmed`: function attributes are set
// outside capture), is captured the second time and replayed from then on; once `map` holds more than `limit` graphs the
// session drops all it has (ttx_session::drop_graphs).
struct GraphCache {
  std::map<GraphKey, hipGraphExec_t> map;
  std::set<GraphKey> warmed;
  size_t limit;
  explicit GraphCache(size_t limit_) : limit(limit_) {}
  void clear() {
    for (auto& kv : map) (void)hipGraphExecDestroy(kv.second);
    map.clear(); warmed.clear();
  }
};

// Every workspace of a session, each name once: ttx_session expands the list to its Buf members and to the loop that registers
// them (a buffer that is not registered would never bump alloc_generation when it grows, and a captured graph would keep its old
// address).
#define TTX_SESSION_BUFS(X)                                                                                                      \
  /* activations (shared by encoder / full decoder / step) */                                                                    \
  X(x) X(x1) X(x2) X(xf) X(ao) X(q2) X(hbuf) X(slab) X(qkv) X(logits) X(ckv)                                                      \
  /* sources */                                                                                                                  \
  X(tok_src) X(src_valid) X(memory) X(memkv)                                                                                     \
  /* full decoder */                                                                                                             \
  X(tok_tgt) X(mem_pad_tmp)                                                                                                      \
  /* teacher-forced evaluation (ttx_teacher_forced_eval / ttx_token_metrics): logits / argmax / nll the caller did not ask for */ \
  X(ev_logits) X(ev_pred) X(ev_nll)                                                                                              \
  /* hypothesis scoring (ttx_score_hypotheses): decoder row -> memory row; logits / per-token values it does not hand out live */ \
  /* in ev_logits / ev_nll */                                                                                                    \
  X(sc_src_of) X(am_length)                                                                                                                   \
  /* scoring a list of batches (ttx_score_list_*): the descriptor table with the run order behind it, a chunk's packed sources and */ \
  /* hypotheses, and its score / length / finished before they are scattered to list order */                                     \
  X(sl_tab) X(sl_src) X(sl_hyp) X(sl_res)                                                                                         \
  /* ttx_hypothesis_logq / ttx_score_proposal: the per-token values the caller did not ask for */                                  \
  X(lq_tok)                                                                                                                      \
  /* loop */                                                                                                                     \
  X(drafts) X(gen) X(front) X(act_idx) X(rec) X(pred) X(state) X(kcache) X(vcache) X(src32) X(outbuf) X(haspad) X(traj)           \
  X(fin_step)                                                                                                                    \
  /* slot pool (continuous batching) */                                                                                          \
  X(rstep) X(row_of) X(src_len) X(new_slot) X(pool_io) X(memkv_new) X(valid_new) X(drafts_new)                                    \
  /* two-phase verify step of the slot pool: the probe's QKV rows [Ld][C][3d] and argmax [C], the draft pass's argmax, the */     \
  /* list of matching sequences, slot -> position in it, and {DecState probe, DecState draft pass, int executed rows} */          \
  X(qkv_probe) X(pred_probe) X(pred_draft) X(act2) X(pos2) X(state2)                                                             \
  /* draft select: per matching slot its present drafts and the first of its compacted rows; compacted row -> layout row */       \
  X(draft_mask) X(row_base) X(row_map)                                                                                           \
  /* accept in two launches: the block-wide sums between k_accept_slots and k_accept_finish (AcceptBlk) */                         \
  X(accept_blk)                                                                                                                  \
  /* snapshot of one verify step for the logits parity test (ttx_gen_params.want_logits) */                                      \
  X(snap_logits) X(snap_act) X(snap_front) X(snap_gen) X(snap_state)                                                             \
  X(leaf_score) X(leaf_tok) X(leaf_cnt) X(beam_summary)                                                                          \
  /* native beam-speculative loop */                                                                                             \
  X(bs_cand_next) X(bs_len_next) X(bs_fin_next) X(bs_logp_next) X(bs_len) X(bs_fin) X(bs_active) X(bs_logp) X(bs_per_cand)        \
  X(bs_best_n) X(bs_best_slot) X(bs_chosen) X(bs_parent) X(bs_parent_draft) X(bs_mark) X(bs_drafts_src) X(bs_cnt) X(bs_hit)       \
  /* tree (beam) decoding, beside tk[2] / tv[2] */                                                                               \
  X(t_prev_len) X(t_slot_of) X(t_src_of)                                                                                         \
  /* beam-speculative source pool (continuous batching over sources of many batches) */                                          \
  X(bp_row_of) X(bp_batch) X(bp_cand) X(bp_cand_len) X(bp_tok) X(bp_new_slot) X(bp_io) X(bp_grp) X(bp_src_acc) X(bp_enc_qkv)            \
  /* sampling loop (ttx_sample_generate): per decoder row its key, sample id, done flag and source row; the call's SampleBlock */ \
  /* speculative form: the copy drafts per source [B][N][D], before they are replicated to the decoder rows */                   \
  X(smp_key) X(smp_sample) X(smp_done) X(smp_src_of) X(smp_prm) X(smp_drafts)                                                     \
  /* forced prefixes of a prompted sampling call: the table int32 [sources][max_len] and the sources' lengths; per decoder row */ \
  /* (slot) its prefix length, its row of the table (pool; single-session loops use smp_src_of) and its source draft 0 [D] */     \
  X(pfx_tok) X(pfx_len_src) X(pfx_len) X(pfx_src) X(pfx_draft0)                                                                  \
  /* per-source logit bias of a biased call: the session's copy of the table, float [sources][V], and per pool slot its row of it */ \
  /* (single-session loops use smp_src_of, the beam loops t_src_of) */                                                            \
  X(lb_val) X(lb_src)                                                                                                            \
  /* syntax-constrained sampling: the session's copy of the call's class table, int8 [V] */                                       \
  X(syn_cls)                                                                                                                     \
  /* stochastic beam search (ttx_sbs_generate): the perturbed log-probabilities G of the candidates, read and written in turn */  \
  X(sbs_g) X(sbs_g_next)                                                                                                         \
  /* stochastic beam pool (ttx_sbs_generate_pool): the per-slot words (keys, then six int arrays), the sources' lengths and the */ \
  /* call's output pointers (SbsPoolIo) */                                                                                        \
  X(sbp_slot) X(sbp_len) X(sbp_io)
#define TTX_DECLARE_BUF(name) Buf name;
#define TTX_REGISTER_BUF(name) all.push_back(&name);

#ifndef TTX_BIG_MIN_TILES
#define TTX_BIG_MIN_TILES 400
#endif
struct ttx_session {
  ttx_model* m;
  std::vector<Buf*> all;           // every workspace below: the constructor registers them from the same list that declares them
  TTX_SESSION_BUFS(TTX_DECLARE_BUF)
  Buf tk[2], tv[2];                // tree (beam) decoding: the two cache buffers an iteration derives one from the other
  int snap_B = 0, snap_rps = 0, snap_gen_ld = 0, snap_step = 0;        // what snap_* hold
  ttx::ProbeInfo* probe_info = nullptr; // pinned + device-mapped, written by k_probe_split
  // ttx_pool_last_counters: summed over the pools of the last slot-pool call (greedy or sampling) whose first session this was
  long long pool_counters[7] = {};
  long long logit_bias_launches = 0;    // k_logit_bias launches this session enqueued or captured (ttx_debug_logit_bias_launches)
  long long syntax_launches = 0;        // k_syntax_mask launches this session enqueued or captured (ttx_debug_syntax_launches)
  long long beam_step_masked_launches = 0;   // k_beam_step_masked launches of the beam loop (ttx_debug_beam_step_masked_launches)
  ttx::BeamHost* beam_host = nullptr;   // pinned + device-mapped, written by k_bs_publish
  ttx::BeamPoolHost* bp_host = nullptr; // pinned + device-mapped, written by k_bsp_publish
  ttx::HostInfo* host_info = nullptr;   // pinned + device-mapped, written by the accept kernels
  hipStream_t own_stream = nullptr;     // the loops run on a session-owned stream (the caller's may be the null stream)
  // Captured graphs hold raw pointers into the workspaces.  EVERY growth of a buffer of this session (whichever entry
  // point caused it) bumps alloc_generation through Buf::owner_gen; the graph cache remembers the generation it was
  // captured under and is dropped as soon as the two differ (graphs_current(), called before any replay or capture).
  uint64_t alloc_generation = 0;
  uint64_t graphs_generation = 0;
  bool dead = false;               // a verify step never published its result (watchdog): the stream may still be stuck
  bool use_graphs = true;
  GraphCache step_graphs{512};     // one verify step (or one phase of a split pool step) per shape
  GraphCache iter_graphs{256};     // one iteration of the beam-speculative loop / of the beam pool per shape
  hipEvent_t ev_done = nullptr;
  void drop_graphs() { step_graphs.clear(); iter_graphs.clear(); }
  void graphs_current() { if (graphs_generation != alloc_generation) { drop_graphs(); graphs_generation = alloc_generation; } }
  ttx::DecState* host_state = nullptr;  // pinned copy target
  // function attributes (dynamic LDS limits) are per device: set once per session, outside graph capture
  bool attr_attn2[2][8] = {};      // [head dimension 32 / 64][mode]
  bool attr_select = false, attr_step = false, attr_topk = false, attr_pool_select = false, attr_sbs_step = false;
  bool attr_sbs_step_masked[5] = {};   // k_sbs_step_masked<VPL>, VPL = 1, 2, 4, 8, 16
  bool attr_step_masked = false;       // k_beam_step_masked
  bool attr_sbs_step_pool = false, attr_sbs_step_pool_masked[5] = {};   // the pool forms of the two
  bool attr_attn_probs[8] = {};    // k_attn_probs: [head dimension 32 / 64][16-byte output stores][16-byte key loads]
  // GEMM policy (all choices are between bit-identical evaluations, see GemmVariant)
  int qkv_small_rows = 800;        // a verify step with fewer live rows than this runs under GV_SMALL (TTX_QKV_SMALL_ROWS)
  int small_rows = 2000;           // ... with fewer than this under GV_MID (TTX_SMALL_ROWS)
  int ffn2_slab_rows = 5600;       // ... and with fewer than this (and at least small_rows) under GV_BIG_FFN2_SLABS (TTX_FFN2_SLAB_ROWS; 0: never)
  // k_gemm24 picks the tiling per launch from the live row count: 128x64 tiles once there are big_min_tiles of them,
  // else 64x64 (TTX_BIG_MIN_TILES)
  int big_min_tiles = TTX_BIG_MIN_TILES;
  // what the most recent launch_gemm dispatched (GemmKernelId) and the tile threshold it handed k_gemm24: ttx_debug_gemm reports
  // them so that a test can prove which kernel it reached
  int last_gemm_kernel = 0, last_gemm_big_min_tiles = 0;
  int attn_split = -1;             // -1 by launch size, 0 never, 1 always (key tiles of a head over 4 waves)
  int attn_row = -1;               // TTX_ATTN_ROW: one-row step launches on k_attn1: -1 those k_attn3s would get, 0 never, 1 every eligible one
  bool accept_spread = true;       // TTX_ACCEPT_SPREAD=0: k_accept alone at every capacity (above 256 slots: k_accept_slots + k_accept_finish)
  bool attn_fallback = false;      // TTX_ATTN_FALLBACK=1 (test hook): every attention launch on the streaming kernel k_attn
  int attn_force = 0;              // ttx_debug_attn (test hook): an AttnKernelId that replaces launch_attn's choice; 0 (always, outside that call): unset
  int attn_sel_N = 0, attn_sel_D = 0;   // > 0 around the launches of a probe (run_step, ttx_debug_attn_as): choose between k_attn2 and k_attn as a step launch in the layout (N, D) does
  int last_attn_kernel = 0;        // what the most recent launch_attn dispatched (AttnKernelId): ttx_debug_attn reports it
  unsigned attn_kernels_seen = 0;  // bit k: launch_attn has dispatched AttnKernelId k on this session (ttx_debug_attn_kernels_seen)
  // profiling of the GEMM launches (bench.py roofline): a HIP event pair around every GEMM launch
  bool profile = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  double prof_ms = 0;
  double prof_empty_pair_ms = -1;
  long long prof_launches = 0;
  bool host_timing = false;
  double host_launch_us = 0;
  long long host_captures = 0;      // TTX_HOST_TIMING: graphs captured on this session and the host time they took
  double host_capture_us = 0;
  long long host_launches = 0;
  hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr;
  ttx_session() {
    TTX_SESSION_BUFS(TTX_REGISTER_BUF)
    for (Buf* b : {&tk[0], &tk[1], &tv[0], &tv[1]}) all.push_back(b);
    for (Buf* b : all) b->owner_gen = &alloc_generation;
  }
};

namespace ttx {

// error text of the calling thread (ttx_last_error); returns `code`
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess)                                                                              \
      return ttx::fail(TTX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" + \
                                        std::to_string(__LINE__) + ")");                               \
  } while (0)

#define TTX_TRY(expr)        \
  do {                       \
    int _r = (expr);         \
    if (_r != TTX_OK) return _r; \
  } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- ttx_gemm.hip ------------------------------------------------------------------------------------------------
// Canonical slice length of a contraction over K (0: one chain; K is then not a multiple of 64).
int gemm_slice_k(int K);
// Split-K slabs of a d-wide step GEMM under `variant` (1 for everything but FFN2 under GV_SMALL).
int gemm_splits(int N, int K, bool step, int variant);
// Y = act(X W^T + b) (splits == 0; `act` is a ttx_activation) or `splits` raw slabs [splits][Mmax][ldy] (k_finish_ln sums them in slab order).
// m_ptr != null marks a verify-step launch (live row count on the device, capacity Mmax); `variant` is a GemmVariant.
int launch_gemm(ttx_session* s, hipStream_t st, const float* X, int ldx, const float* W, int ldw, const float* bias,
                float* Y, int ldy, const int* m_ptr, int Mmax, int N, int K, int act, int splits, long long slab_stride,
                int variant);
int launch_finish(ttx_session* s, hipStream_t st, const float* slabs, int n_slabs, long long slab_stride, const float* bias,
                  const float* resid, const float* g1, const float* b1, const float* g2, const float* b2,
                  const uint8_t* row_valid, float* Y, const int* m_ptr, int Mmax);
// launch_finish with the row width and epsilon given by the caller instead of the model
int launch_finish_d(hipStream_t st, const float* slabs, int n_slabs, long long slab_stride, const float* bias, const float* resid,
                    const float* g1, const float* b1, const float* g2, const float* b2, const uint8_t* row_valid, float* Y,
                    const int* m_ptr, int Mmax, int d, float eps);
// ttx_debug_gemm / ttx_debug_finish_ln (include/ttx.h): host-side validation, then one launch
int gemm_debug(ttx_session* s, const float* d_x, int ldx, const float* d_w, int ldw, const float* d_bias, float* d_y, int ldy,
               const int32_t* d_m, int m_max, int N, int K, int act, int splits, long long slab_stride, int variant, int tiling,
               int32_t* kernel_id, hipStream_t st);
int finish_debug(ttx_session* s, const float* d_slabs, int n_slabs, long long slab_stride, const float* d_bias, const float* d_resid,
                 const float* d_g1, const float* d_b1, const float* d_g2, const float* d_b2, const uint8_t* d_row_valid, float* d_y,
                 const int32_t* d_m, int m_max, int d, float eps, hipStream_t st);
int gemm_bench(ttx_session* s, int M, int N, int K, int splits, int variant, int reps, double* us_per_launch, double* max_abs_diff);

// ---- ttx_attn.hip ------------------------------------------------------------------------------------------------
// `groups` = sources / decoder rows / running-sequence slots; `q_per_group` = query rows of one group (Ls, Lt, or the
// 1 + N*D step rows of a sequence); for the step modes `D1`/`N` shape the draft tiles.
int launch_attn(int mode, ttx_session* s, hipStream_t st, const AttnArgs& a, int groups, int H, int q_per_group, int max_keys,
                int N = 1, int D1 = 1);
// ttx_debug_attn / ttx_debug_attn_hd (include/ttx.h): host-side validation, n_active into a DecState on the device, then one launch_attn with
// `kernel` (0 or an AttnKernelId) in ttx_session::attn_force; `in.d` and `in.st` are filled in here
int attn_debug(ttx_session* s, const AttnArgs& in, int H, int head_dim, int mode, int groups, int n_active, int max_keys, int kernel,
               int32_t* kernel_id, hipStream_t st);
// ttx_attn_staged_key_limit (include/ttx.h); 0 for a head dimension without kernels
int attn_staged_key_limit(int head_dim, int q_per_group);

}  // namespace ttx
