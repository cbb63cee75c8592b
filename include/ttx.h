/*
 * ttx.h — C ABI of libttx_hip.so: MI355X-native (gfx950) encoder–decoder forward and speculative
 * decoding for the Molecular Transformer hot path of Academich/translation-transformer.
 *
 * The reference has no FFI: its hot path is Python calling stock torch ops.  Each entry point below
 * names the reference function it replaces (paths relative to the reference root).  Conventions:
 *   - every pointer named d_* is a DEVICE pointer owned by the caller (a torch tensor's data_ptr());
 *     the library borrows it for the duration of the call and never frees it;
 *   - token tensors are int64 row-major exactly as the reference's LongTensors; floats are fp32;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all work is
 *     enqueued on it; calls that return host-side results synchronise that stream before returning;
 *   - every function returns 0 on success or a negative ttx_status; ttx_last_error() gives the text
 *     (thread-local).  Nothing throws across the boundary;
 *   - one host thread drives one ttx_session at a time (the Lightning predict loop is sequential:
 *     src/model/lightning_model.py:209-212); distinct sessions on distinct streams may run concurrently.
 */
#ifndef TTX_H
#define TTX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTX_ABI_VERSION 4

typedef enum ttx_status {
  TTX_OK = 0,
  TTX_ERR_INVALID = -1,      /* bad argument / shape                                             */
  TTX_ERR_HIP = -2,          /* a HIP runtime call failed                                        */
  TTX_ERR_NO_DEVICE = -3,    /* no gfx950 device visible: the library has NO CPU fallback         */
  TTX_ERR_REFERENCE = -4,    /* input on which the reference itself raises (see ttx_last_error)  */
  TTX_ERR_NOMEM = -5,
  TTX_ERR_ROW_REPLAY = -6,   /* ttx_greedy_speculative_generate_rows only: decode the batches as given instead */
  TTX_ERR_MAX_STEPS = -7     /* beam-speculative: the ttx_beam_params.max_steps guard tripped (non-terminating input) */
} ttx_status;

/* Model hyper-parameters: the init_args of VanillaTransformer (src/model/modules.py:11-38). */
typedef struct ttx_config {
  int32_t vocab_size;           /* tgt (= src when shared) vocabulary                          */
  int32_t src_vocab_size;
  int32_t embedding_dim;        /* d: multiple of 64, <= 1024                                  */
  int32_t num_heads;            /* divides d; d / num_heads (head dimension) must be 32 or 64  */
  int32_t feedforward_dim;      /* multiple of 64                                              */
  int32_t num_encoder_layers;
  int32_t num_decoder_layers;
  int32_t pad_token;            /* src == tgt pad id (0 in the reference: tokenizer_base.py:27) */
  int32_t max_positions;        /* rows of the sinusoid table minus one (embeddings.py:31: 5000) */
  float   layer_norm_eps;       /* modules.py:52: 1e-5                                         */
} ttx_config;

/* The feed-forward non-linearity of a model (the reference's `activation` init_arg: "relu" or "gelu").  TTX_ACT_GELU is the exact
 * GELU, 0.5 x (1 + erf(x / sqrt 2)) — torch's approximate="none" — not the tanh form.  TTX_ACT_NONE is only meaningful for
 * ttx_debug_gemm_act. */
typedef enum ttx_activation { TTX_ACT_NONE = 0, TTX_ACT_RELU = 1, TTX_ACT_GELU = 2 } ttx_activation;

typedef struct ttx_model ttx_model;      /* weights resident in HBM                          */
typedef struct ttx_session ttx_session;  /* workspaces, KV caches, captured graphs, one stream at a time */

/* One named fp32 host tensor of the reference state dict ("model." prefix stripped). */
typedef struct ttx_tensor {
  const char*  name;
  const float* data;      /* HOST pointer, row-major */
  int64_t      numel;
} ttx_tensor;

/* Library / device ----------------------------------------------------------------------------- */
int         ttx_abi_version(void);
const char* ttx_last_error(void);
/* Number of visible gfx950 devices (0 when there is none; never raises). */
int         ttx_device_count(void);

/* Weights in: replaces VanillaTransformer.__init__ + load_state_dict (modules.py:11-84; checkpoint key
 * layout of lightning_model.py / tests/test_batching.py:48-49).  Tensors are looked up by name; a
 * missing or mis-sized tensor is TTX_ERR_INVALID.  The sinusoid table (embeddings.py:38-45, not in the
 * state dict) is rebuilt on the host with the same fp32 formula. */
int  ttx_model_create(const ttx_config* cfg, const ttx_tensor* tensors, int n_tensors, int device,
                      ttx_model** out);
void ttx_model_destroy(ttx_model* m);
/* Packed weight blob (all weights, one contiguous device allocation) for the RCCL broadcast of
 * rank 0 creates the model from host tensors, every other rank creates it with
 * ttx_model_create_empty and receives the blob with one ncclBroadcast on [ptr, ptr+bytes). */
int  ttx_model_create_empty(const ttx_config* cfg, int device, ttx_model** out);
int  ttx_model_blob(ttx_model* m, void** d_ptr, int64_t* bytes);

/* The state dict does not carry the activation, so a model is ReLU until told otherwise.  ttx_model_set_activation accepts
 * TTX_ACT_RELU or TTX_ACT_GELU (anything else: TTX_ERR_INVALID) and is legal only while no session of the model has ever been
 * created: captured graphs and step argument blocks bake the FFN1 epilogue in.  Once ttx_session_create has succeeded on the
 * model it returns TTX_ERR_INVALID and leaves the model as it is.  ttx_model_activation returns the current value. */
int  ttx_model_set_activation(ttx_model* m, int activation);
int  ttx_model_activation(const ttx_model* m);

int  ttx_session_create(ttx_model* m, ttx_session** out);
void ttx_session_destroy(ttx_session* s);

/* Model protocol ---------------------------------------------------------- */

/* VanillaTransformer.encode_src (modules.py:110-116).  d_src: int64 [B,Ls]; PAD keys masked
 * (src == pad_token); d_memory: fp32 [B,Ls,d] out, rows at PAD positions are written as zeros. */
int ttx_encode_src(ttx_session* s, const int64_t* d_src, int B, int Ls, float* d_memory, void* stream);

/* VanillaTransformer.decode_tgt (modules.py:118-138): full-prefix decoder forward + classifier.
 * d_tgt int64 [R,Lt]; d_memory fp32 [Rm,Ls,d]; d_mem_pad uint8 [Rm,Ls] (1 = PAD key);
 * d_mem_row int32 [R] maps decoder row -> memory row (NULL: identity, Rm == R, i.e. the reference's
 * inflated memory); d_logits fp32 [R,Lt,V] out. */
int ttx_decode_tgt(ttx_session* s, const int64_t* d_tgt, int R, int Lt, const float* d_memory,
                   const uint8_t* d_mem_pad, const int32_t* d_mem_row, int Rm, int Ls, float* d_logits,
                   void* stream);

/* VanillaTransformer.forward (modules.py:86-108; step 0 of standard beam search). d_logits [B,Lt,V]. */
int ttx_forward(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_tgt, int Lt,
                float* d_logits, void* stream);

/* Teacher-forced evaluation: VanillaEncoderDecoderTransformerLightning.validation_step / test_step
 * (src/model/lightning_model.py:174-207) with the metrics of src/utils/metrics.py, quirks included:
 *   loss      nn.CrossEntropyLoss(reduction="mean") over ALL B*(Lt-1) positions (PAD targets count: no ignore_index);
 *   token_acc mean of argmax == target over all positions;
 *   seq_acc   calc_sequence_acc: per row, the positions p with target[(p+1) mod T] == eos in ascending order are paired with
 *             the EOS positions q in ascending order; a pair is a hit when cumsum(argmax == target)[p] == q; hits / pairs
 *             over the batch, NaN when no target holds an EOS.
 * Targets are read off d_tgt int64 [B,Lt] at column 1 (tgt[:, 1:]); the argmax keeps the first maximum (torch.argmax).
 * d_pred int64 [B,Lt-1] and d_nll fp32 [B,Lt-1] (per-position cross-entropy) are optional outputs (NULL: session scratch);
 * d_out3 fp32 [3] = {loss, token_acc, seq_acc}, written on the device (nothing is synchronised).  Vocabulary <= 1024,
 * B*(Lt-1) < 2^24.  Target ids outside [0, V) are the caller's to reject (the kernels read them as id 0).  Two calls on the
 * same inputs give bit-identical results.
 * ttx_token_metrics: the metric stage alone over caller-provided logits fp32 [B,Lt-1,V].
 * ttx_teacher_forced_eval: ttx_forward(src, tgt[:, :-1]) followed by the metric stage; d_logits [B,Lt-1,V] or NULL (the logits
 * then stay in session scratch). */
int ttx_token_metrics(ttx_session* s, const float* d_logits, const int64_t* d_tgt, int B, int Lt, int V, int eos, int64_t* d_pred,
                      float* d_nll, float* d_out3, void* stream);
int ttx_teacher_forced_eval(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_tgt, int Lt, int eos,
                            float* d_logits, int64_t* d_pred, float* d_nll, float* d_out3, void* stream);

/* Log-likelihood scores of hypotheses, one scale for every generator.  For a hypothesis row h[0..W-1] (column 0 holds the BOS and
 * is never scored) and logits = decode_tgt(h[:W-1], memory(src)), the model's own teacher-forced forward on the hypothesis:
 *   n         the column of the first EOS at a column >= 1 (finished = 1); else the last column >= 1 holding a non-PAD token
 *             (finished = 0); else 0 (an all-PAD row);
 *   tok_logp  [t-1] = log_softmax(logits[t-1])[h[t]] for t = 1..n and exactly 0 for t > n; a PAD before the EOS is a target like
 *             any other;
 *   score     the sum of tok_logp[0..n-1] in position order, accumulated in double and rounded once; length = n.  A row with
 *             n = 0 has score 0 and finished = 0.
 * Nothing is synchronised and every output is written on the device; every argument is checked before any launch (W >= 2,
 * vocabulary <= 1024, W - 1 and Ls within the positional table, rows * (W-1) < 2^24).  Token ids outside [0, V) are the caller's
 * to reject (the kernels read them as id 0).  Two calls on the same inputs give bit-identical results.  d_tok_logp and d_finished
 * are optional outputs (NULL: not handed out).
 * ttx_hypothesis_logprobs: the scoring stage alone over caller-provided logits fp32 [R,W-1,V]; d_hyp int64 [R,W].
 * ttx_score_hypotheses: the encoder once per source, the full-prefix decoder over the B*N rows (row r reads memory row r / N) and
 * the stage above.  d_hyp int64 [B*N] rows with row stride ld_hyp >= W, so the first W columns of a wider tensor are scored in
 * place; d_logits [B*N,W-1,V] or NULL (session scratch): what ttx_decode_tgt returns for the same rows, bit for bit. */
int ttx_hypothesis_logprobs(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad, int eos,
                            float* d_tok_logp, float* d_score, int32_t* d_length, uint8_t* d_finished, void* stream);
int ttx_score_hypotheses(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W,
                         int eos, float* d_logits, float* d_tok_logp, float* d_score, int32_t* d_length, uint8_t* d_finished,
                         void* stream);

/* Folding hypotheses: the N rows of every source reduced to their distinct hypotheses, counted and ranked, on the device.
 * Input.  d_hyp: B*N int64 rows with row stride ld_hyp >= W; source b owns rows b*N .. b*N + N - 1.  d_score: optional fp32
 *   [B,N]; a NaN score is read as -inf, so the outputs are always a permutation (rejecting NaN is the caller's job: the library
 *   reads no device value back).
 * Identity (scoring.unique_samples' rule, column 0 included).  e_j is the column of the first `eos` of row j in [0, W);
 *   c_j = e_j + 1, or W when the row holds no `eos` (such a row is UNFINISHED).  Rows i and j of one source are the same
 *   hypothesis iff c_i == c_j and their tokens agree on [0, c).  Tokens are compared as full 64-bit values.  What follows the
 *   first `eos` is never read.
 * Representative.  first[j] is the smallest i <= j equal to j; row j is a representative iff first[j] == j; its count is the
 *   number of j' with first[j'] == j; its score is ITS OWN score, whatever scores its repeats carry.
 * Order of the representatives: a precedes b
 *   TTX_FOLD_FIRST   iff a < b;
 *   TTX_FOLD_SCORE   (needs scores) iff s_a > s_b, or s_a == s_b under IEEE equality (-0.0 equals 0.0) and a < b: the order of
 *                    scoring.unique_samples;
 *   TTX_FOLD_COUNT   the larger count first, then the SCORE rule when scores are given, then a < b;
 *   flag TTX_FOLD_UNFINISHED_LAST: every finished representative precedes every unfinished one, and the order above holds
 *                    inside each class.
 * Outputs, each optional (NULL: not handed out), each written in full for every source, on the device; nothing is synchronised.
 * U is the number of representatives of the source.
 *   d_first     int32 [B,N]  by sample: first[j]
 *   d_rank_of   int32 [B,N]  by sample: the rank of the hypothesis that sample j belongs to
 *   d_n_unique  int32 [B]    U
 *   d_perm      int32 [B,N]  rank r -> sample index of the representative for r < U, -1 beyond
 *   d_count     int32 [B,N]  by rank, 0 beyond U
 *   d_out_score fp32  [B,N]  by rank: the representative's score bits (a NaN input reads -inf), -inf beyond U; all -inf when no
 *                            scores were given
 *   d_out       int64 [B,N,W] packed, by rank: the representative's row as it stands, all W columns; rows beyond U all `pad`
 *   d_logmass   fp32  [B]    (needs scores) m = the largest representative score, acc = sum_r exp((double)s_r - m) in rank order
 *                            in double, logmass = (float)(m + log(acc)); -inf when m is -inf.  With score = log p this is the
 *                            log of the probability mass the distinct hypotheses cover.
 * TTX_ERR_INVALID with nothing launched: B < 1, N < 1, N > 1024, W < 1, ld_hyp < W, a null d_hyp, an unknown order or flag bit,
 * the SCORE order or d_logmass without scores, no output requested.
 * Determinism.  A source's outputs depend on its own N rows and scores alone: bit-identical from call to call, at any B, any
 * ld_hyp and any padded W at or beyond the longest compared column (widening W changes an unfinished row's c: the invariance
 * holds for rows that hold an EOS, and for unfinished rows padded with `pad` on both sides of the comparison, which is what the
 * generators emit).  No float is added by an atomic and nothing crosses a source.
 * TTX_FOLD_DEBUG_NO_FILTER: the kernel's 64-bit filter word (which only spares token comparisons that cannot succeed) is taken as
 * 0, so every pair of rows of equal c is confirmed on its tokens; the outputs are the same.  For tests.
 * The session is optional (the kernel needs no workspace): with one the call runs on the session's device, without one on the
 * current device; `stream` is used as given (NULL: the null stream), as the scoring pair does. */
typedef enum ttx_fold_order { TTX_FOLD_FIRST = 0, TTX_FOLD_SCORE = 1, TTX_FOLD_COUNT = 2 } ttx_fold_order;
enum { TTX_FOLD_UNFINISHED_LAST = 1, TTX_FOLD_DEBUG_NO_FILTER = 2 };
int ttx_fold_hypotheses(ttx_session* s_or_null, const int64_t* d_hyp, int B, int N, int W, int ld_hyp, int pad, int eos,
                        const float* d_score_or_null, int order, int flags, int32_t* d_first, int32_t* d_rank_of,
                        int32_t* d_n_unique, int32_t* d_perm, int32_t* d_count, float* d_out_score, int64_t* d_out,
                        float* d_logmass, void* stream);

/* Per-position alternatives of hypotheses: what else the model considered where it emitted a token.  Hypothesis rows, logits, n
 * and the limits as for the scoring pair above; T = W - 1; x = logits[r,p,:]; position p of row r is live iff p < n, and for a live
 * position, t = h[p+1] and 1 <= k <= min(32, V):
 *   top_id       [p,j], j = 0..k-1: the ids of the k largest logits, largest first; equal logits: the lower id first (-0.0 equals
 *                0.0, a -inf logit is an ordinary value that sorts last).  int32 [R,T,k].
 *   top_logp     [p,j] = log_softmax(x)[top_id[p,j]], evaluated as -(log1pf(rs) + (m - x[id])) with the (m, rs) of the scoring
 *                stage, so that top_logp[p,0] == -log1pf(rs).  fp32 [R,T,k].
 *   chosen_logp  [p] = that value for t: tok_logp[p] of the scoring pair on the same logits, bit for bit (for V % 4 == 0 on a
 *                16-byte aligned d_logits, which is what the decoder writes).  fp32 [R,T].
 *   rank         [p] = the number of ids v with x[v] > x[t], or x[v] == x[t] and v < t: 0 when the emitted token was the first
 *                maximum, and top_id[p, rank[p]] == t whenever rank[p] < k.  int32 [R,T].
 *   entropy      [p] = -sum_v q_v log q_v in nats, q = softmax(x), fp32 in one fixed order; a -inf logit contributes exactly 0.
 *                fp32 [R,T].
 *   length       [r] = n.  int32 [R].
 * Positions that are not live hold top_id = -1, top_logp = 0, chosen_logp = 0, rank = -1, entropy = 0 in every element; all
 * outputs are written in full by the kernels.  Every output is optional (NULL: not handed out); at least one of the five
 * per-position outputs is required.  A row whose maximum logit is not finite is outside the contract and still gives ids and
 * ranks in [0, V).  Nothing is synchronised.  TTX_ERR_INVALID with nothing launched: the limits of the scoring pair, k < 1,
 * k > 32, k > V, no output requested, ld_hyp < W, Ls above the positional table.  A position's outputs depend only on its own
 * logits row and hypothesis: bit-identical from call to call, across batching and padded widths, and for a d_logits base that is
 * or is not 16-byte aligned.
 * ttx_hypothesis_alternatives: the stage alone over caller-provided logits fp32 [R,W-1,V]; d_hyp int64 [R,W].
 * ttx_score_alternatives: exactly the pass of ttx_score_hypotheses (d_hyp rows of stride ld_hyp >= W, d_logits [B*N,W-1,V] or
 * NULL for session scratch), then the stage. */
int ttx_hypothesis_alternatives(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad, int eos,
                                int k, int32_t* d_top_id, float* d_top_logp, float* d_chosen_logp, int32_t* d_rank,
                                float* d_entropy, int32_t* d_length, void* stream);
int ttx_score_alternatives(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W,
                           int eos, int k, float* d_logits, int32_t* d_top_id, float* d_top_logp, float* d_chosen_logp,
                           int32_t* d_rank, float* d_entropy, int32_t* d_length, void* stream);

/* Cross-attention maps of hypotheses: which source position each output token attended to.  d_src int64 [B,Ls] and d_hyp int64
 * [B*N] rows of stride ld_hyp >= W as for ttx_score_hypotheses; T = W - 1; decoder row r = b*N + k reads hyp[b,k,:T] and attends
 * to memory row b.
 *   length    [r] = n of the scoring rule on the tokens alone: the column of the first EOS at a column >= 1, else the last column
 *             >= 1 holding a non-PAD token, else 0.  Query position t (0-based, the one that predicts hyp[t+1]) is live iff
 *             t + 1 <= n: the convention of tok_logp[t-1].
 *   heads     P[r,h,t,j] = softmax_j(scale * q[r,t,h,:] . k[b,j,h,:]) over the keys j with src[b,j] != PAD, scale =
 *             1/sqrt(head_dim); q is the cross-attention Q projection of decoder layer `layer` (of the stream behind the
 *             self-attention LayerNorm), k the K half of that layer's projection of the encoder memory.  fp32 [B*N,H,T,Ls].
 *   mean      M[r,t,j] = (P[r,0,t,j] + P[r,1,t,j] + ... in ascending h, fp32) / (float)H: what nn.MultiheadAttention returns
 *             with average_attn_weights=True.  fp32 [B*N,T,Ls].
 *   align     A[r,t] = the smallest j with M[r,t,j] == max_j M[r,t,:] (the first maximum), -1 where t is not live.  int32 [B*N,T].
 * PAD keys are exactly 0.0, positions that are not live are exactly 0.0 in every element, and a source row that is all PAD gives
 * zeros, never NaN.  layer is in [0, num_decoder_layers), or -1 for the last.  d_heads, d_mean, d_align and d_length are optional
 * outputs (NULL: not computed / not handed out), at least one of the first three is required; all of them are written in full by
 * the kernels, so no caller sees uninitialised memory.  The pass ends at the tapped layer's cross attention: no logits are formed
 * and the vocabulary limit of scoring does not apply.  Nothing is synchronised.  TTX_ERR_INVALID with nothing launched: no output
 * requested, layer out of range, Ls above ttx_attn_probs_key_limit(head_dim) or the positional table, W < 2, W - 1 above the
 * positional table, rows * (W-1) >= 2^24.  A map depends only on its own (source, hypothesis): it is bit-identical from call to
 * call and across B, N and the padded widths, within the key range scoring documents (ttx_attn_staged_key_limit). */
int ttx_attention_maps(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W, int eos,
                       int layer, float* d_heads, float* d_mean, int32_t* d_align, int32_t* d_length, void* stream);

/* Host query, no device needed: the largest Ls k_attn_probs takes at head dimension head_dim (1024 at 32 and 64; 0 for a head
 * dimension without kernels). */
int ttx_attn_probs_key_limit(int head_dim);

/* Draft maker: make_drafts (src/utils/drafting.py:5-67) on the device.  d_src int64 [B,L];
 * d_drafts int64 [B,n_drafts,D] out with D = clamp(draft_len, min_draft_len, max_draft_len). */
int ttx_make_drafts(ttx_session* s, const int64_t* d_src, int B, int L, int draft_len, int n_drafts,
                    int min_draft_len, int max_draft_len, int eos_token, int pad_token, int replace_token,
                    int64_t* d_drafts, void* stream);

/* Generators -------------------------------------------------------------- */

typedef struct ttx_gen_params {
  int32_t max_len;
  int32_t draft_len;       /* greedy-speculative: D (clamped to [1,max_len] as speculative_decoding.py:64-73) */
  int32_t n_drafts;        /* N */
  int32_t pad_token, bos_token, eos_token, replace_token;
  int32_t want_logits;     /* parity tests: k > 0 records verify step k (1-based) for ttx_debug_step_snapshot */
} ttx_gen_params;

typedef struct ttx_gen_stats {
  int64_t model_calls;         /* decoder invocations == verify steps (generator.model_calls_num)      */
  int64_t accepted_tokens;     /* draft tokens accepted over all rows and steps                        */
  int64_t produced_tokens;     /* tokens written (accepted + one bonus token per row per step)         */
  int64_t verified_positions;  /* sum over steps of Bc*N*(D+1): rows of the step's GEMMs               */
  int64_t kv_prefix_positions; /* sum over steps and running rows of the cached prefix length          */
  int64_t src_positions;       /* sum over steps of Bc*Ls (cross-attention keys read)                  */
  double  encode_ms, decode_ms;/* device time (HIP events on `stream`) of the two phases               */
  int64_t src_tokens_padded;   /* encoder positions computed: rows x padded length, summed over encoder passes         */
  int64_t status;              /* this batch's own status (TTX_OK, TTX_ERR_REFERENCE, ...): the *_many calls return the
                                  first failure but decode every batch                                  */
} ttx_gen_stats;

/* TranslationInferenceGreedySpeculative.generate (src/decoding/speculative_decoding.py:39-174) with a
 * KV cache: encoder once, cross-attention K/V projected once per source, D+1 new positions per draft per
 * step.  d_src int64 [B,Ls]; d_out int64 [B,1,max_len] (PAD-filled; rows that never reach EOS stay
 * all-PAD exactly as the reference leaves them).  Returns TTX_ERR_REFERENCE where the reference raises
 * (a row finishing at a width beyond max_len, :158). */
int ttx_greedy_speculative_generate(ttx_session* s, const int64_t* d_src, int B, int Ls,
                                    const ttx_gen_params* p, int64_t* d_out, ttx_gen_stats* stats,
                                    void* stream);

/* TranslationInferenceGreedy.generate (src/decoding/standard_decoding.py:30-55) with a KV cache.
 * d_out int64 [B,1,max_len]. */
int ttx_greedy_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_gen_params* p,
                        int64_t* d_out, ttx_gen_stats* stats, void* stream);

/* The forms of a sampling call.  Every option of the sampling, stochastic beam search and log q calls (forced prefix, proposal, logit
 * bias, syntax table, filter) arrived with an entry point of its own, and entry points are added, never changed.  Per family the
 * last one is the GENERAL form and takes everything the others take: ttx_sample_generate_syntax,
 * ttx_sample_speculative_generate_syntax, ttx_sample_speculative_generate_pool_syntax (one ttx_sample_opts, one ttx_syntax),
 * ttx_sbs_generate_bias, ttx_beam_generate_constrained, ttx_hypothesis_logq_syntax, ttx_score_proposal_syntax.  Every other form of
 * a family IS its general form with the fields it does not name zeroed (a null opts, a null d_bias, a null syntax or d_cls, a null
 * filter, null lengths): the same checks, the same launches, the same bits.  A new binding needs the general forms alone. */

/* Seeded ancestral sampling: temperature, top-k and top-p (nucleus) on the device. */
typedef struct ttx_sample_params {
  int32_t max_len, num_samples;          /* n >= 1 samples per source */
  float   temperature;                   /* >= 0; 0 = greedy */
  int32_t top_k;                         /* 0 = off, else 1..32 */
  float   top_p;                         /* (0, 1]; 1 = off.  top_p < 1 with top_k = 0 runs with top_k = 32 */
  int32_t pad_token, bos_token, eos_token;
  uint64_t seed;
} ttx_sample_params;

/* The plain greedy loop of ttx_greedy_generate (KV cache, one captured graph per step shape) over R = B * n decoder rows, with
 * k_sample choosing each row's token where k_argmax would.  The encoder and the cross K/V projection run once per source; row
 * r = b * n + j attends source b and is keyed (d_row_keys[b], j); d_row_keys NULL: keys 0..B-1.  d_out int64 [B, n, max_len]: BOS,
 * the sampled tokens up to and including the row's first EOS or PAD, PAD after it.  The loop ends when every row has ended or the
 * width is exhausted; stats->model_calls counts the steps.
 *
 * The rule, for a live row with logits x[0..V-1], at position pos (1 for the first token after BOS):
 *   1  A row that has ended emits PAD; its logits are not read.
 *   2  temperature == 0: the token is k_argmax's (first maximum, see ttx_debug_argmax), bit for bit.  Otherwise y_v = x_v * inv_T
 *      with inv_T = 1.0f / temperature formed on the host, one rounded fp32 product per logit.  A -inf logit is never emitted.
 *   3  Kept set.  top_k == 0 and top_p == 1: all V tokens, in ascending id.  Otherwise mask_with_num_logits_according_nucleus
 *      (see ttx_nucleus_mask) on y with nucleus = top_p and max_num_of_unmasked_positions = top_k: tokens in rank order, best first,
 *      equal values the lower id first; rank i is kept while i < top_k and the softmax mass ranked above it is < top_p; rank 0 always.
 *   4  u = (x0 >> 8) * 2^-24, an fp32 in [0, 1), x0 = word 0 of Philox4x32-10 with key (seed_lo, seed_hi) and counter
 *      (key_lo, key_hi, sample, pos); multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, round
 *      c' = (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)).
 *   5  e_v = expf(y_v - max y), S their sum over the kept set: the first kept token (ascending id without a filter, rank order with
 *      one) whose inclusive prefix sum exceeds u * S; the last kept token with e_v > 0 if rounding leaves none.  The order of the
 *      fp32 sums is fixed by V and the filter alone (csrc/ttx_sample.hip.h), so a row's token depends on its own logits, key,
 *      sample id and position only: not on B, n, the row's place in the launch, or what shares its batch.
 *   6  EOS and PAD both end a row.
 * Limits: vocab_size <= 1024; at most 32 kept tokens when a filter is on.  TTX_ERR_INVALID with nothing launched: vocab_size >
 * 1024, num_samples < 1, temperature < 0 or not finite, top_k outside {0, 1..32}, top_p outside (0, 1] or not finite, and
 * everything ttx_greedy_generate refuses.  Per-token log-probabilities are not produced: ttx_score_hypotheses on the samples gives
 * them on the scale of every other generator (log p under the model), ttx_score_proposal under the distribution sampled from
 * (log q, below). */
int ttx_sample_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sample_params* p,
                        int64_t* d_out, ttx_gen_stats* stats, void* stream);

/* Log-probability of hypotheses under the SAMPLING distribution q (temperature, top-k, top-p), where ttx_score_hypotheses gives it
 * under the model p.  A distribution is (temperature, top_k, top_p) with ttx_sample_params' limits and defaults: temperature >= 0
 * and finite (0 = greedy), top_k 0 or 1..32, top_p in (0, 1]; top_p < 1 with top_k = 0 runs with top_k = 32. */
typedef struct ttx_dist { float temperature; int32_t top_k; float top_p; } ttx_dist;

/* The quantity.  Hypothesis rows, logits, n (= length) and finished are those of ttx_score_hypotheses; T = W - 1; for a row h and a
 * position p = t - 1 < n, x is the fp32 logits row of position p and tok_logq[p] is the log of the probability that steps 2-5 of
 * ttx_sample_generate's rule emit h[t] from x, ignoring the rounding of the inverse CDF (step 5 compares fp32 prefix sums with
 * u * S; this is the ratio e_t / S those sums approximate):
 *   temperature == 0   0.0f if h[t] is k_argmax's token (the first maximum of x), else -inf.
 *   otherwise          y_v = __fmul_rn(x_v, inv_T): the sampler's product, inv_T = 1.0f / temperature formed on the host.
 *   no filter          tok_logq = -(log1pf(rs) + (m - y_t)), where m is the row maximum of y and rs the sum of expf(y_v - m) over
 *                      every v but the first maximum: the arithmetic and summation order of the scoring stage (tok_logp) on y.
 *   filter on          the kept set is the sampler's on the bits (the same device function selects it): ranks best first, equal
 *                      values the lower id first, rank i kept while i < top_k and the softmax mass ranked above it is < top_p,
 *                      rank 0 always.  e_r = expf(y_r - m) for the kept ranks r = 0..n_kept-1, S the last element of their
 *                      inclusive prefix sums in rank order (Hillis-Steele over the 64 lanes, offsets 1, 2, .., 32: the very S the
 *                      sampler multiplies u by).  For a kept h[t]: tok_logq = (y_t - m) - logf(S); for any other: -inf.
 *   forced positions   p < forced_len[r] (d_forced_len int32 [R], NULL = all 0; clamped to [0, n] by the kernel): exactly 0.0f and
 *                      inside the support, the logits are not read.  This is what the prompted samplers and the prompted
 *                      stochastic beam search do at a prefix position: the prefix token, no draw, no cost.
 *   p >= n             exactly 0.0f.
 * Per row:  logq = the sum of tok_logq[0..n-1] in position order, accumulated in double, rounded once; -inf as soon as one term is.
 *           first_outside (int32) = the first p < n with tok_logq[p] == -inf (the token cannot be emitted there), else -1.
 * Per position, optional (NULL: not computed), int32 [R,T]:
 *   rank    the number of v with y_v > y_t, or y_v == y_t and v < t: the rule of ttx_score_alternatives on y (on x at temperature 0).
 *   n_kept  the size of the kept set: V without a filter, 1 at temperature 0.  Under a filter a token is kept iff rank < n_kept,
 *           and a token with rank == n_kept sits just outside the nucleus.
 *   Forced positions and positions p >= n hold rank = -1 and n_kept = 0.
 * With temperature 1, no filter and no forced_len, tok_logq / logq are tok_logp / score of the scoring pair (ttx_score_proposal
 * runs that very kernel; ttx_hypothesis_logq gives its bits for V % 4 == 0 on a 16-byte aligned d_logits wherever the scoring
 * stage gives a number).  A -inf logit is an ordinary value with probability 0.  A finite logit so far below the maximum that
 * expf(y_t - m) underflows to 0 (about 103 or more below it in y) is never emitted by the sampler, which requires e_t > 0; the
 * formulas above still give it its finite, very negative value rather than -inf.
 * CAVEAT.  These are the TEACHER-FORCED logits.  A row that a sampler drew from its decode-time logits can get -inf here when one
 * of its tokens sat on the boundary of the nucleus: the decode loop and the teacher-forced pass run different attention kernels
 * and agree to rounding only, so the last kept rank can differ between them.  rank and n_kept show that case:
 * first_outside = p with rank[p] == n_kept[p] is a boundary token, not a row the sampler could not have drawn.
 * A row that ended on a SAMPLED PAD is not finished under the length rule above: that last draw lies at position n, is not scored,
 * and is not part of logq (a search that accumulated its own log q, such as ttx_sbs_generate's logp, includes it).
 * Nothing is synchronised, nothing is atomic, two calls give the same bits, and a position's outputs depend on its own logits row
 * and the hypothesis alone (not on R, the batch or a d_logits base that is or is not 16-byte aligned).  d_logq and d_length are
 * required, every other output is optional.  TTX_ERR_INVALID with nothing launched: the limits of the scoring pair, a NULL or
 * out-of-range distribution (temperature < 0 or not finite, 1 / temperature not a positive finite fp32, top_k outside {0, 1..32},
 * top_p outside (0, 1]).  Negative forced_len entries live on the device and cannot be refused without a synchronisation: they are
 * clamped to 0.
 * ttx_hypothesis_logq: the stage alone over caller-provided logits fp32 [R,W-1,V]; d_hyp int64 [R,W].
 * ttx_score_proposal: exactly the pass of ttx_score_hypotheses (d_hyp rows of stride ld_hyp >= W, d_logits [B*N,W-1,V] or NULL for
 * session scratch), then the stage; d_score (and with it d_tok_logp) optionally receive ttx_score_hypotheses' outputs from the same
 * decoder pass, so that p and q of a row come from one pass. */
int ttx_hypothesis_logq(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad, int eos,
                        const ttx_dist* dist, const int32_t* d_forced_len, float* d_tok_logq, float* d_logq,
                        int32_t* d_first_outside, int32_t* d_rank, int32_t* d_n_kept, int32_t* d_length, uint8_t* d_finished,
                        void* stream);
int ttx_score_proposal(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W, int eos,
                       const ttx_dist* dist, const int32_t* d_forced_len, float* d_logits, float* d_tok_logp, float* d_score,
                       float* d_tok_logq, float* d_logq, int32_t* d_first_outside, int32_t* d_rank, int32_t* d_n_kept,
                       int32_t* d_length, uint8_t* d_finished, void* stream);

/* Speculative seeded sampling: ttx_sample_generate's samples from the greedy-speculative loop. */
typedef struct ttx_sample_spec_params {
  ttx_sample_params sample;              /* as for ttx_sample_generate */
  int32_t draft_len, n_drafts;           /* copy drafts per source: n_drafts >= 1 windows of 1 <= draft_len <= max_len source tokens */
  int32_t replace_token;                 /* takes the place of EOS and PAD inside a draft; differs from both */
  int32_t reserved;                      /* 0 */
} ttx_sample_spec_params;

/* The loop of ttx_greedy_speculative_generate (copy drafts of the source, 1 + n_drafts * draft_len positions per row and decoder
 * pass, KV cache, one captured graph per step shape) over R = B * n decoder rows, with the keyed draw of ttx_sample_generate where
 * the argmax stands.  Rows, keys and the encoder are ttx_sample_generate's; the n rows of a source share its drafts (made once per
 * source and replicated to the rows).
 *
 * The rule.  The sampler is counter-based: the token at position pos of row (key, sample) is a function of that position's logits
 * and of u(seed, key, sample, pos) alone (steps 2-5 above).  A verify step therefore knows, for every step row, the token the plain
 * sampler would emit there: step row 0 of a decoder row at front f predicts position f + 1, the row of token j (0-based) of a draft
 * predicts position f + 2 + j.  A draft token is accepted iff it equals that token; the longest accepted prefix over the drafts is
 * taken (the first draft wins ties) and the draw after it is written as the bonus token.  Every committed token is thus the plain
 * sampler's token for the prefix before it: the distribution is exact, and so is the seeding contract (same source, same key,
 * same samples in any batch, at any n).  The logits of a position come out of a pass over more rows than in ttx_sample_generate, so
 * their last bits may differ; a row can differ from ttx_sample_generate's only where u falls within that rounding of a CDF boundary.
 * A row ends with a written EOS or PAD, or when its front reaches max_len - 1; tokens beyond column max_len - 1 are dropped.
 * d_out int64 [B, n, max_len] as ttx_sample_generate writes it.  stats: model_calls = the steps of the longest row,
 * accepted_tokens draft tokens accepted, produced_tokens = accepted + one per row and step, src_tokens_padded = B * Ls.
 * TTX_ERR_INVALID with nothing launched: everything ttx_sample_generate refuses; n_drafts < 1, draft_len outside [1, max_len],
 * pad, eos and replace tokens not pairwise different, max_len + draft_len + 2 beyond the positional table. */
int ttx_sample_speculative_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                    const ttx_sample_spec_params* p, int64_t* d_out, ttx_gen_stats* stats, void* stream);

/* ttx_sample_speculative_generate over a whole list of sources on the slot pool of ttx_greedy_speculative_generate_pool
 * (continuous batching, length-bucketed admissions, the two-phase verify step, draft select, the accept step in two launches
 * above 256 slots), with the keyed draw where the argmax stands.  d_src int64 [S_total][Ls_all] holds ALL sources right-padded in
 * the order they are to be admitted, h_len (HOST, int32 [S_total]) their lengths, d_row_keys int64 [S_total] their keys in the
 * order of d_src (NULL: keys 0 .. S_total - 1).  d_out int64 [S_total][num_samples][max_len] in the order of d_src: row (s, j)
 * holds what ttx_sample_speculative_generate writes for source s with key d_row_keys[s] and sample j (BOS, the tokens up to and
 * including the first EOS or PAD, then PAD); the acceptance rule, the ending rule (EOS, PAD, front at max_len - 1) and the
 * dropped columns are that call's.  The token at a position is a function of that position's logits and of (seed, key, sample,
 * pos) alone, so a row does not depend on its slot, on when it was admitted, on the capacity or on what shares the pool.
 *
 * Work-list units are sources: the n = num_samples decoder rows of a source are admitted together into n slots (capacity counts
 * decoder rows).  The encoder, the cross K/V projection and the copy drafts run once per source of an admission sub-chunk; the
 * fill replicates them into the source's n slots.  A slot carries its key, its sample id (i % n) and its row of d_out.  There are
 * no per-row traces and no TTX_ERR_ROW_REPLAY (nothing is replayed), and no int16 limit on max_len.
 *
 * stats (zero it first) receives sums over the pools: model_calls = verify steps the device executed, accepted_tokens,
 * produced_tokens, verified_positions (the rows of matching slots under a split step), kv_prefix_positions, src_positions,
 * src_tokens_padded (sources x width per admission sub-chunk), decode_ms.  ttx_pool_last_counters reports this call's pool counters.
 * The greedy pool's switches apply and are read at pool start: TTX_TWO_PHASE, TTX_TWO_PHASE_MIN_ROWS, TTX_DRAFT_SELECT,
 * TTX_ADMIT_ROWS, TTX_ACCEPT_SPREAD, TTX_TWO_PHASE_STATS.  TTX_ACCEPT_SPREAD too is read at pool start by this call (unset: on;
 * the value a session saw when it was created, which the greedy pool goes by, plays no part here).
 * TTX_ERR_INVALID with nothing launched: everything ttx_sample_speculative_generate refuses; null pointers; capacity outside
 * [num_samples, 4096]; an h_len entry above Ls_all; a slot width beyond the positional table.  S_total == 0 returns TTX_OK. */
int ttx_sample_speculative_generate_pool(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total, int Ls_all,
                                         const int32_t* h_len, const int64_t* d_row_keys, int capacity,
                                         const ttx_sample_spec_params* p, int64_t* d_out, ttx_gen_stats* stats, void* stream);

/* Forced target prefixes (prompted decoding) for the three sampling calls above.  Each *_prefix call takes the arguments of its
 * unprompted call plus d_prefix (DEVICE, int64 [sources][ld_prefix], without BOS), ld_prefix and h_prefix_len (HOST, int32
 * [sources], like h_len): source b carries a prefix of plen = h_prefix_len[b] tokens, 0 <= plen <= max_len - 1, shared by its
 * num_samples rows.  `sources` is B (S_total for the pool).  The unprompted calls are the same code with a null prefix, and a call
 * whose lengths are all 0 (or whose h_prefix_len is NULL) IS the unprompted call: the same launches, the same graphs, the same bits.
 *
 * The position rule, for a row of source b at position pos (1 = the first token after BOS), beside the sampling rule above:
 *   pos <= plen: the token is prefix[b][pos - 1].  The logits are not read and no uniform is consumed.  An id outside [0, V) is
 *                emitted as 0, like the sampler's own guard.
 *   otherwise:   steps 2-5 of the sampling rule, unchanged: the counter of the draw is still (key, sample, pos).
 * A forced EOS or PAD ends the row exactly as an emitted one does; tokens beyond column max_len - 1 are dropped; a row that has
 * ended emits PAD.  A row therefore depends on its source, its prefix, its key and its sample id, and on nothing else: not on the
 * batch, on ld_prefix, on num_samples, on the pool's capacity or on its switches.
 *
 * Speculative calls.  The acceptance rule is NOT changed: a draft token is accepted iff it equals the token of its position, which
 * now comes from the position rule.  What changes is the drafts: before every verify step k_prefix_drafts rewrites draft 0 of every
 * active row, for j = 0 .. draft_len - 1: column c = front + 1 + j receives prefix[c - 1] if c <= plen (EOS and PAD as
 * replace_token, as in every draft), else token j of the row's own source-copy draft 0.  So a prefix of P tokens enters the KV cache
 * in ceil(P / (draft_len + 1)) verify steps; once front >= plen draft 0 is the source draft again; drafts still hold neither EOS
 * nor PAD, so a forced EOS arrives as the bonus token and is the last one written; drafts 1 .. n_drafts - 1 stay the source
 * windows.  ttx_sample_generate_prefix pays one decoder step per forced token (no one-pass prefill).
 *
 * Limits: prefixes are per source, not per sample; the plain greedy, greedy-speculative and beam generators take none.
 * TTX_ERR_INVALID with nothing launched: a length outside [0, max_len - 1] or above ld_prefix, a negative ld_prefix, a null
 * d_prefix together with a non-zero length, and everything the unprompted call refuses. */
int ttx_sample_generate_prefix(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sample_params* p,
                               const int64_t* d_prefix, int ld_prefix, const int32_t* h_prefix_len, int64_t* d_out,
                               ttx_gen_stats* stats, void* stream);
int ttx_sample_speculative_generate_prefix(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                           const ttx_sample_spec_params* p, const int64_t* d_prefix, int ld_prefix,
                                           const int32_t* h_prefix_len, int64_t* d_out, ttx_gen_stats* stats, void* stream);
int ttx_sample_speculative_generate_pool_prefix(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total, int Ls_all,
                                                const int32_t* h_len, const int64_t* d_row_keys, int capacity,
                                                const ttx_sample_spec_params* p, const int64_t* d_prefix, int ld_prefix,
                                                const int32_t* h_prefix_len, int64_t* d_out, ttx_gen_stats* stats, void* stream);

/* Proposal drafts for the two speculative sampling calls: drafts the caller brings (a cheap model's output, an earlier prediction,
 * the row's own greedy answer), OFFERED and never forced.  Each *_proposal call takes the arguments of its *_prefix call plus
 * d_proposal (DEVICE, int64 [sources][ld_proposal], without BOS, may end in EOS), ld_proposal and h_proposal_len (HOST, int32
 * [sources]): source b carries a proposal of len = h_proposal_len[b] tokens, 0 <= len <= max_len - 1, shared by its num_samples
 * rows.  k_sample_step and k_sample_accept are the unproposed call's and see no table: a draft token is accepted iff it equals the
 * token of its position, so a proposal forces no token, whatever it holds: the rows are the plain sampler's under the contract of
 * ttx_sample_speculative_generate, and only step counts change.  (That contract's one caveat holds between a proposed and an
 * unproposed call as it holds between either and the plain sampler: the drafts decide in which row of which pass a position's logits
 * are formed, and a uniform within fp32 rounding of a CDF boundary can then fall on either side.)  A call whose
 * proposal lengths are all 0 (or whose h_proposal_len is NULL) IS the *_prefix call with the same remaining arguments, launch for
 * launch: no new graph site, no upload.  A call is either prompted or proposed: non-empty prefixes together with non-empty
 * proposals are refused (TTX_ERR_INVALID, nothing launched), as is everything prefix lengths are refused for.
 *
 * The rule.  Before every verify step k_proposal_drafts rewrites draft 0 of every active row.  For a row with tokens g[0 .. f]
 * (g[0] = BOS, f the slot's front) and proposal q[0 .. len - 1] (q[i] is proposed for column i + 1; q[-1] := BOS):
 *   for each shift d in [-32, 31] (one lane of a wave per shift, d = lane - 32)
 *     c(d) = the number of a in {0 .. CTX - 1} with  f - a >= 0,  -1 <= f-1-a+d < len  and  q[f-1-a+d] == g[f-a];
 *     d is eligible iff c(d) >= 1 and 0 <= f + d < len;
 *   the eligible d with the largest c is chosen; ties go to the smaller |d|, then to d >= 0.  (A proposal equal to the row so far
 *   always selects d = 0.)
 *   Draft 0 token j (column f + 1 + j), j = 0 .. draft_len - 1, is q[f + d + j] while that index is < len, and token j of the row's
 *   own source draft 0 past the end of the proposal, as k_prefix_drafts does behind a prefix.  EOS and PAD are written as
 *   replace_token, so drafts still hold neither and EOS arrives as the bonus token.
 *   If no d is eligible, or len = 0, draft 0 is the source draft 0.  Drafts 1 .. n_drafts - 1 are never touched.
 * The rule is stateless and idempotent: it reads the row, the proposal and the source draft kept at set-up, and nothing it wrote.
 * CTX = 2; the window of 64 shifts is the wave width.  Neither forces a token.  (TTX_PROPOSAL_CTX = 2, 4 or 8, read per call,
 * overrides CTX for measurements; any other value is refused.)  With a proposal equal to the row's final tokens, L emitted tokens
 * (EOS included) take ceil(L / (draft_len + 1)) verify steps. */
int ttx_sample_speculative_generate_proposal(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                             const ttx_sample_spec_params* p, const int64_t* d_prefix, int ld_prefix,
                                             const int32_t* h_prefix_len, const int64_t* d_proposal, int ld_proposal,
                                             const int32_t* h_proposal_len, int64_t* d_out, ttx_gen_stats* stats, void* stream);
int ttx_sample_speculative_generate_pool_proposal(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total, int Ls_all,
                                                  const int32_t* h_len, const int64_t* d_row_keys, int capacity,
                                                  const ttx_sample_spec_params* p, const int64_t* d_prefix, int ld_prefix,
                                                  const int32_t* h_prefix_len, const int64_t* d_proposal, int ld_proposal,
                                                  const int32_t* h_proposal_len, int64_t* d_out, ttx_gen_stats* stats, void* stream);

/* Per-source logit bias and token allow-lists for the sampling calls and stochastic beam search: WHICH tokens a source may produce.
 * d_bias is DEVICE, fp32 [sources][ld_bias], ld_bias >= V, one row per source (`sources` is B; S_total for the pool, in the order of
 * d_src).  NULL is the unbiased call, launch for launch: no new kernel, no new buffer, the same graph keys.
 *
 * The rule.  For every decoder row of source b and every position whose logits a rule reads,
 *     x'_v = x_v + bias[b][v]        ONE rounded fp32 add (never contracted),
 * and the rule (ttx_sample_generate's steps 2-6, the stochastic beam step, log q) then runs on x'.  An entry that is exactly zero
 * (+0.0 or -0.0) skips the add: the logit keeps its bits, so a -0.0 logit keeps its sign and an all-zero bias returns the unbiased
 * call's tokens on the bits.  -inf forbids a token: every consumer defines a -inf logit as "never emitted".  An allow-list is a bias
 * of 0 / -inf.  The bias comes before temperature and filter: the kept set and its renormalisation are the sampler's, on the biased
 * row.  A forced prefix position emits its prefix token whatever the bias says (it reads no logits).  Drafts (copies, prefixes,
 * proposals) need no rule: a draft token is accepted iff it equals the keyed draw, so a token the biased sampler cannot emit is never
 * accepted.
 * Values must be finite or -inf.  NaN and +inf are outside the contract; they live on the device and this library does not read them
 * back (the Python layer's check_logit_bias refuses them).  A row whose bias leaves no finite logit is outside the contract exactly as
 * an all -inf row is: the result is some id in [0, V), never an out-of-range write.
 * Seeding contract, one item longer: a row depends on its source, key, sample id, prefix and ITS SOURCE'S BIAS ROW alone; it is
 * bit-identical in any batch, at any batch size, ld_bias or padded width, per batch or pooled (under the speculative calls' one
 * caveat), and from run to run.
 * Mechanism.  ONE launch of k_logit_bias (csrc/ttx_logit_bias.hip.h) per decoder pass, in place on the pass's logits, between the
 * classifier and the consumer.  The values are copied into a session buffer at call start, so a captured step never holds the
 * caller's pointer; a biased step has graph keys of its own.  A pool slot gets its source's row index at admission.
 * The *_ex calls take every option of their family in one struct (a NULL struct, or zeroed fields, is the plain call); the prefix and
 * proposal fields are the arguments of the *_prefix / *_proposal calls, under their rules.  ttx_sample_generate_ex refuses a proposal.
 * ttx_sbs_generate_bias is ttx_sbs_generate_ex plus the bias.  The greedy, greedy-speculative, beam and beam-speculative calls and
 * ttx_sbs_generate_pool take no bias (temperature 0 on the sampling calls, the pooled one included, is constrained greedy decoding).
 * TTX_ERR_INVALID with nothing launched: ld_bias < V with a non-null d_bias, and everything the call refuses without a bias. */
typedef struct ttx_sample_opts {
  const int64_t* d_prefix; int32_t ld_prefix; const int32_t* h_prefix_len;          /* forced prefixes, or NULL / 0 / NULL */
  const int64_t* d_proposal; int32_t ld_proposal; const int32_t* h_proposal_len;    /* proposal drafts, or NULL / 0 / NULL */
  const float* d_bias; int32_t ld_bias;                                             /* logit bias, or NULL / 0 */
} ttx_sample_opts;
int ttx_sample_generate_ex(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sample_params* p,
                           const ttx_sample_opts* opts, int64_t* d_out, ttx_gen_stats* stats, void* stream);
int ttx_sample_speculative_generate_ex(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                       const ttx_sample_spec_params* p, const ttx_sample_opts* opts, int64_t* d_out,
                                       ttx_gen_stats* stats, void* stream);
int ttx_sample_speculative_generate_pool_ex(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total, int Ls_all,
                                            const int32_t* h_len, const int64_t* d_row_keys, int capacity,
                                            const ttx_sample_spec_params* p, const ttx_sample_opts* opts, int64_t* d_out,
                                            ttx_gen_stats* stats, void* stream);
/* log q under the bias: ttx_hypothesis_logq / ttx_score_proposal with k_logit_bias applied to the teacher-forced logits before the
 * log q stage (hypothesis row r belongs to source r / N), so that logq is the log-probability under the distribution the biased sampler
 * draws from: first_outside names the first forbidden token and logq = -inf means "cannot be emitted".  ttx_score_proposal_bias runs
 * the scoring stage (d_score, d_tok_logp) on the RAW logits first, in the same pass, so p stays the model's; a caller's d_logits then
 * receives the biased logits.  ttx_hypothesis_logq_bias leaves the caller's logits alone (it biases a copy).  A NULL d_bias is the
 * call without one. */
int ttx_hypothesis_logq_bias(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad, int eos,
                             const ttx_dist* dist, const int32_t* d_forced_len, const float* d_bias, int ld_bias, int N,
                             float* d_tok_logq, float* d_logq, int32_t* d_first_outside, int32_t* d_rank, int32_t* d_n_kept,
                             int32_t* d_length, uint8_t* d_finished, void* stream);
int ttx_score_proposal_bias(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W, int eos,
                            const ttx_dist* dist, const int32_t* d_forced_len, const float* d_bias, int ld_bias, float* d_logits,
                            float* d_tok_logp, float* d_score, float* d_tok_logq, float* d_logq, int32_t* d_first_outside,
                            int32_t* d_rank, int32_t* d_n_kept, int32_t* d_length, uint8_t* d_finished, void* stream);
/* ONE launch of k_logit_bias on DEVICE arrays of the caller (tests/test_gpu_logit_bias_kernel.py), in place on d_logits fp32 [M][V];
 * rows at or beyond *d_m (int32 on the device, NULL: M) keep their bits.  Plain mapping (d_act_idx NULL): the bias row of logits row r
 * is d_src[r], or r / rows_per_src with a NULL d_src.  Step layout (d_act_idx set, k_sample_step's): lrow = d_row_map ? d_row_map[row]
 * : row, b = d_act_idx[lrow / (1 + N * D)], bias row d_src[b].  Every index is the caller's to keep in range. */
int ttx_debug_logit_bias(ttx_session* s, float* d_logits, int V, int M, const int32_t* d_m, const float* d_bias, int ld_bias,
                         const int32_t* d_src, int rows_per_src, const int32_t* d_act_idx, const int32_t* d_row_map, int N, int D,
                         void* stream);
/* The number of k_logit_bias launches the session has enqueued since it was created, eagerly or into a captured step (a replayed
 * graph adds none; ttx_debug_logit_bias is not counted).  A session that only ever served unbiased calls reports 0. */
int ttx_debug_logit_bias_launches(ttx_session* s);

/* Syntax-constrained sampling: balanced branches and ring closures.  The sampling calls can be held to rows that can still end
 * balanced: every OPEN token closed, every ring label used an even number of times, EOS inside max_len.  d_cls is DEVICE, int8 [V],
 * the SYNTAX TABLE, one class per vocabulary id:
 *     -1      FORBID   never emitted under the constraint (PAD, BOS, "?")
 *      0      neutral  (and every value not listed here)
 *      1      OPEN     "("
 *      2      CLOSE    ")"
 *      3 + l  ring label l, 0 <= l < 64   ("1", "2", "%10")
 * EOS is the call's eos token whatever its class.  A NULL struct or a NULL d_cls is the call without the constraint, launch for
 * launch: no new kernel, no new buffer, the same graph keys.
 *
 * The rule.  For a row prefix P (the tokens after BOS, as stored; an id outside [0, V) and a FORBID token count as neutral)
 *     depth(P) = #OPEN - #CLOSE,   R(P) = the 64-bit XOR of 1 << l over its ring tokens,   need = max(depth, 0) + popcount(R),
 * and for the position pos being predicted (column of the output row, BOS at 0) left = (max_len - 1) - pos columns follow it.
 * Token v keeps its logit bit for bit if it is allowed; otherwise the logit becomes -inf:
 *     EOS                                    depth == 0 and R == 0
 *     FORBID                                 never
 *     neutral                                need + 1 <= left
 *     OPEN                                   need + 2 <= left
 *     CLOSE                                  depth > 0
 *     ring l, bit l set in R   (closes)      always
 *     ring l, bit l clear in R (opens)       need + 2 <= left
 * Consequences.  The allowed set is never empty (need == 0 allows EOS; need > 0 allows a closer).  From a prefix with need <= left
 * every row ends in EOS at or before the last column with depth == 0, R == 0 and no FORBID token: every allowed token keeps
 * need <= left at the next position (a neutral costs one column of a budget that had one to spare, an opener two of two, a closer
 * pays for itself), and at need == left only closers and, at need == 0, EOS remain, so need falls to 0 no later than left does.  An
 * unprompted call starts there (need 0) whenever max_len >= 2.
 * This is a NECESSARY condition for a parseable SMILES string, not validity: valence, aromaticity, "()", "C11" and ring bonds across
 * "." are outside it.
 * A forced prefix position ignores the mask, as it ignores the bias, yet its tokens count in the state.  A prefix that already has
 * need > left is accepted: the rule then allows closers only and the row may end unfinished.  A logit bias is applied first, the mask
 * second; -inf stays -inf, so the allowed set is the intersection (which, unlike the mask's own, may be empty: outside the contract as
 * an all -inf row is).  Drafts need no rule: a draft token is accepted iff it equals the keyed draw, and the draw of a draft position
 * comes from the row masked for the prefix that includes the earlier draft tokens.  Temperature 0 is greedy decoding over the allowed
 * set.  Seeding contract, one item longer: a row depends on its source, key, sample id, prefix, bias row, the table and max_len alone.
 * Mechanism.  ONE launch of k_syntax_mask (csrc/ttx_syntax.hip.h) per decoder pass, in place on the pass's logits, after k_logit_bias
 * and before the consumer.  The kernel never reads the logits; the state is a pure function of the row, recomputed from the committed
 * tokens and the drafts, so accept, retire, admission, probe, draft select and graph replay carry nothing for it.  The table is copied
 * into a session buffer at call start; a constrained step has graph keys of its own.
 * max_len: 0 or the call's max_len for the generate calls (anything else: TTX_ERR_INVALID, nothing launched); for the scoring calls
 * the max_len the rows were generated under (0: W; else at least 2). */
typedef struct ttx_syntax {
  const int8_t* d_cls;
  int32_t max_len;
} ttx_syntax;
/* The *_ex calls plus the constraint. */
int ttx_sample_generate_syntax(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sample_params* p,
                               const ttx_sample_opts* opts, const ttx_syntax* syntax, int64_t* d_out, ttx_gen_stats* stats, void* stream);
int ttx_sample_speculative_generate_syntax(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys,
                                           const ttx_sample_spec_params* p, const ttx_sample_opts* opts, const ttx_syntax* syntax,
                                           int64_t* d_out, ttx_gen_stats* stats, void* stream);
int ttx_sample_speculative_generate_pool_syntax(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total, int Ls_all,
                                                const int32_t* h_len, const int64_t* d_row_keys, int capacity,
                                                const ttx_sample_spec_params* p, const ttx_sample_opts* opts, const ttx_syntax* syntax,
                                                int64_t* d_out, ttx_gen_stats* stats, void* stream);
/* log q under the constraint: ttx_hypothesis_logq_bias / ttx_score_proposal_bias with k_syntax_mask applied to the teacher-forced
 * logits after the bias and before the log q stage (logits row r * (W - 1) + t takes the prefix hyp[r][1 .. t]): first_outside names the
 * first token the constrained sampler could not have emitted.  A hypothesis with an unmatched CLOSE is outside the support at that
 * token; its depth is negative from there on, a state no constrained row reaches, in which the rule can leave a later position
 * (left <= 0) no token at all: d_tok_logq is NaN there and d_logq of such a row is not a number to rely on beyond "not finite"
 * (d_first_outside names the CLOSE; the Python layer reports -inf for every row that has a first_outside).  As with the bias, ttx_score_proposal_syntax scores p on the RAW logits
 * first and a caller's d_logits then receives the masked logits; ttx_hypothesis_logq_syntax masks a copy.  d_bias may be NULL. */
int ttx_hypothesis_logq_syntax(ttx_session* s, const float* d_logits, const int64_t* d_hyp, int R, int W, int V, int pad, int eos,
                               const ttx_dist* dist, const int32_t* d_forced_len, const float* d_bias, int ld_bias, int N,
                               const ttx_syntax* syntax, float* d_tok_logq, float* d_logq, int32_t* d_first_outside, int32_t* d_rank,
                               int32_t* d_n_kept, int32_t* d_length, uint8_t* d_finished, void* stream);
int ttx_score_proposal_syntax(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_hyp, int ld_hyp, int N, int W, int eos,
                              const ttx_dist* dist, const int32_t* d_forced_len, const float* d_bias, int ld_bias, const ttx_syntax* syntax,
                              float* d_logits, float* d_tok_logp, float* d_score, float* d_tok_logq, float* d_logq,
                              int32_t* d_first_outside, int32_t* d_rank, int32_t* d_n_kept, int32_t* d_length, uint8_t* d_finished,
                              void* stream);
/* ONE launch of k_syntax_mask on DEVICE arrays of the caller (tests/test_gpu_syntax_kernel.py), in place on d_logits fp32 [M][V]; rows
 * at or beyond *d_m (int32 on the device, NULL: M) keep their bits.  mode 0, k_sample's rows: d_tok int32 [M][ld_tok], the prefix of
 * row r is d_tok[r][1 .. d_front[0]], pos = d_front[0] + 1.  mode 1, k_sample_step's layout: d_tok int32 [B][ld_tok], d_front [B],
 * lrow = d_row_map ? d_row_map[row] : row, b = d_act_idx[lrow / (1 + N * D)], rs = lrow % (1 + N * D); rs == 0: the prefix
 * d_tok[b][1 .. f], pos = f + 1; rs = 1 + n * D + j: tokens 0 .. j of draft n of d_drafts int32 [B][N][D] appended, pos = f + 2 + j.
 * mode 2, teacher-forced: d_tok int64 [M / T][ld_tok], row r * T + t takes d_tok[r][1 .. t], pos = t + 1.  Every index is the
 * caller's to keep in range. */
int ttx_debug_syntax_mask(ttx_session* s, int mode, float* d_logits, int V, int M, const int32_t* d_m, const int8_t* d_cls, int max_len,
                          int eos, const void* d_tok, int ld_tok, const int32_t* d_front, const int32_t* d_act_idx,
                          const int32_t* d_row_map, const int32_t* d_drafts, int N, int D, int T, void* stream);
/* The number of k_syntax_mask launches the session has enqueued since it was created, eagerly or into a captured step (a replayed
 * graph adds none; ttx_debug_syntax_mask is not counted).  A session that only ever served unconstrained calls reports 0. */
int ttx_debug_syntax_launches(ttx_session* s);

/* Beam-speculative bookkeeping kernels.
 * ttx_nucleus_mask: mask_with_num_logits_according_nucleus (src/decoding/speculative_decoding.py:871-904): per row of
 *   d_logits [rows,V] keep the best logit and further ones, best first, while the softmax mass ranked above is
 *   < nucleus, never more than n_best (<= 32); everything else becomes `fill`.  d_out [rows,V].  V <= 1024.
 * ttx_accepted_lengths: the nucleus mask (0.9975-style) fused with calculate_n_accepted_in_drafts (:847-869):
 *   d_logits [R,D+1,V], d_drafts int64 [R,D] -> d_n_ok int32 [R] = leading draft tokens inside their position's kept set.
 * ttx_ragged_topk: topk_in_each_group (:177-238): d_score [sum of group lengths], d_offsets int32 [G+1] exclusive prefix
 *   sums, every group >= k entries; d_top fp32 [G,k] and d_idx int64 [G,k] (flat indices) best first; equal scores: lower
 *   index first (torch leaves ties unspecified). */
int ttx_nucleus_mask(ttx_session* s, const float* d_logits, int rows, int V, float nucleus, int n_best, float fill,
                     float* d_out, void* stream);
int ttx_accepted_lengths(ttx_session* s, const float* d_logits, const int64_t* d_drafts, int R, int D, int V, float nucleus,
                         int n_best, int32_t* d_n_ok, void* stream);
int ttx_ragged_topk(ttx_session* s, const float* d_score, const int32_t* d_offsets, int G, int max_group, int k,
                    float* d_top, int64_t* d_idx, void* stream);
/* TranslationInferenceBeamSearchSpeculative.generate (src/decoding/speculative_decoding.py:241-869) — the whole loop on the
 * device: generate_trying_all_the_drafts (:428-598) or generate_with_smart_drafts (:600-845), `sample` (:294-400),
 * calculate_n_accepted_in_drafts (:847-869), mask_with_num_logits_according_nucleus (:871-904) and topk_in_each_group
 * (:177-238), on a per-candidate KV cache (encoder and cross K/V once per source).  Ties between drafts with the same
 * accepted length are resolved as torch's CPU topk(1) resolves them (csrc/ttx_select.h), so the candidates are those of the
 * reference run on the CPU.  draft_len is clamped to [5, 200] as the reference's constructor does (:278-284).
 *   d_src int64 [B, Ls];  d_out int64 [B, n_best, max_len] (row stride max_len): the reference's result tensor
 *   [B, n_best, W] occupies the first W = stats->out_width columns of every row (W <= max_len), hypotheses best first.
 * Errors: TTX_ERR_REFERENCE where the reference asserts/raises (fewer candidate leaves than n_best for a source, :195;
 * no drafts, drafting.py:39-43; max_len < 3); TTX_ERR_MAX_STEPS when the guard below trips.
 * Limits of the native loop (the reference has none; TTX_ERR_INVALID names the one exceeded): n_best <= 32, n_drafts <= 64,
 * vocabulary <= 1024, n_best * (draft_len + 1) <= 1023 and 2 * n_best^2 * (draft_len + 1) * 4 bytes <= 150 KB of LDS. */
typedef struct ttx_beam_params {
  int32_t max_len;
  int32_t n_best;            /* <= 32                                                                  */
  int32_t draft_len;
  int32_t n_drafts;          /* <= 64: drafts per candidate (all drafts) / most drafts tried per candidate (smart) */
  int32_t smart_drafts_mode;
  int32_t pad_token, bos_token, eos_token, replace_token;
  int32_t max_steps;         /* 0: none (reference behaviour: its loop does not end when a candidate keeps emitting PAD
                                before any EOS); > 0: fail once more than this many iterations would be needed */
} ttx_beam_params;

typedef struct ttx_beam_stats {
  int64_t model_calls;             /* iterations == decoder invocations (generator.model_calls_num)         */
  int64_t input_lines;             /* (candidate, draft) rows built over all iterations (model_input_lines_num) */
  int64_t running_rows;            /* of those, rows of unfinished candidates (the reference's b_sz)        */
  int64_t accepted_tokens;         /* generator.accepted_tokens_num                                         */
  int64_t produced_non_pad_tokens; /* generator.produced_non_pad_tokens                                     */
  int64_t verified_positions;      /* decoder positions the KV-cached algorithm needs (running candidates + draft tokens) */
  int64_t executed_positions;      /* rows of the step GEMMs actually computed (unused smart-mode draft slots included) */
  int64_t kv_prefix_positions;     /* cached prefix positions attended                                      */
  int64_t running_candidates;      /* sum over iterations of unfinished candidates                          */
  int64_t src_tokens_padded;       /* encoder positions computed: B x Ls                                    */
  double  encode_ms, decode_ms;    /* device time (HIP events) of encoder + cross K/V + drafts / of the loop */
  int32_t out_width;               /* W: columns of the result tensor                                       */
  int32_t status;                  /* this batch's own status (the *_many call returns the first failure)   */
} ttx_beam_stats;

int ttx_beam_speculative_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_beam_params* p,
                                  int64_t* d_out, ttx_beam_stats* stats, void* stream);
/* Several batches in flight (batch i on sessions[i % n_sessions], each on its own stream; one host thread drives all of
 * them): per-batch outputs and stats are those of n_batches calls of ttx_beam_speculative_generate. */
int ttx_beam_speculative_generate_many(ttx_session** sessions, int n_sessions, int n_batches, const int64_t* const* d_src,
                                       const int* B, const int* Ls, const ttx_beam_params* p, int64_t* const* d_out,
                                       ttx_beam_stats* stats, void* stream);

/* The same generator with continuous batching over many given batches (SURVEY.md §8(f) #1 for the beam path).  In the
 * reference's loop the sources of a batch meet only in batch-wide scalars: the draft length min(max_len - longest row - 1,
 * draft_len) (:476 / :671), the stop rule (every row holds EOS, :586 / :826, or no room left, :464 / :652), the tensor width
 * and, in smart mode, the width of the -1-padded table the best draft is picked from (the batch's longest draft group,
 * :779-784 -> :225); a source all of whose n_best rows hold EOS is a fixed point of the iteration.  A session here owns a pool
 * of `capacity` source slots: given batches are admitted whole (their sources run in lock-step), ONE verify step per iteration
 * serves every live candidate of every batch in the pool, the batch-wide scalars are kept per batch on the device exactly as
 * the reference computes them, a source that finished frees its slots at once, and the pool is refilled from the work list.
 * Per source it returns
 *   d_out        int64 [R_total][n_best][max_len]  hypotheses best first, PAD beyond
 *   d_trace_len  int16 [R_total][trace_cap]        longest hypothesis after each of the source's iterations (-1 past the last)
 *   d_summary    int32 [R_total][8]                iterations of its batch when it retired, status (1 every row holds EOS,
 *                                                  3 its batch ran out of room: rows as they stood, 2 fewer leaves than
 *                                                  n_best: the reference asserts for the batch, 4 max_steps), input lines,
 *                                                  running rows, accepted-token sum, accepted count, longest hypothesis,
 *                                                  decoded candidates summed over the iterations
 * from which translation-transformer_amd/scheduling.py:replay_beam_batch derives each given batch's result width, model calls
 * and counters.  d_src int64 [R_total][Ls_all]: all sources right-padded, batch after batch in admission order; HOST arrays:
 * h_len int32 [R_total] a source's length (position after its last non-PAD token), h_batch_of int32 [R_total] its batch
 * (0, 0, .., 1, 1, ...: non-decreasing, every batch non-empty and at most `capacity` sources), h_given_ls int32 [n_batches] the
 * padded width each batch was given in (smart mode builds its window library over that width, :603-615).  `stats` receives the
 * sums of what the device executed (model_calls = iterations of all pools). */
int ttx_beam_speculative_generate_pool(ttx_session** sessions, int n_sessions, const int64_t* d_src, int R_total, int Ls_all,
                                       const int32_t* h_len, const int32_t* h_batch_of, int n_batches, const int32_t* h_given_ls,
                                       int capacity, const ttx_beam_params* p, int64_t* d_out, int16_t* d_trace_len,
                                       int32_t* d_summary, int trace_cap, ttx_beam_stats* stats, void* stream);

/* TranslationInferenceBeamSearch.generate (src/decoding/standard_decoding.py:89-174) — the whole loop on the device with a
 * per-hypothesis KV cache: the <BOS> step (:102), then up to max_len - 2 iterations of {decoder on the unfinished hypotheses,
 * artificial "35 on PAD" logits for the finished ones (:133-135), log(softmax) + running score, topk(beam) over beam x V per
 * source (:151-153), row assembly (:154-161)}, ending early once every hypothesis holds EOS (:166).
 *   d_src int64 [B, Ls];  d_out int64 [B, beam_size, max_len] (row stride max_len): the reference's result [B, beam, W]
 *   occupies the first W = stats->out_width columns, hypotheses best first. */
typedef struct ttx_beam_search_params {
  int32_t max_len, beam_size;
  int32_t pad_token, bos_token, eos_token;
} ttx_beam_search_params;
typedef struct ttx_beam_search_stats {
  int64_t model_calls;     /* generator.model_calls_num                                              */
  int64_t running_rows;    /* generator.b_sz: decoder rows over all calls (unfinished hypotheses)    */
  int32_t out_width;
  int32_t pad_;
} ttx_beam_search_stats;
int ttx_beam_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_beam_search_params* p, int64_t* d_out,
                      ttx_beam_search_stats* stats, void* stream);

/* Constrained beam search: ttx_beam_generate under a per-source logit bias ("Per-source logit bias" above), a syntax constraint
 * ("Syntax-constrained sampling" above) and forced target prefixes, each optional.  The loop is ttx_beam_generate's: per level one
 * decoder pass over the unfinished candidates, then k_logit_bias and k_syntax_mask in place on the pass's logits (the row of a
 * candidate takes its source's bias row; the mask's prefix is the candidate's row, its position the row's width, its max_len and EOS
 * the call's), then k_beam_step_masked (csrc/ttx_beam_mask.hip.h) where ttx_beam_generate launches k_beam_step.
 *
 * The rule of a step.  Per candidate: score (fp32, cumulative log-probability) and `finished`.  Source b has candidates
 * k = 0 .. beam-1 in the order of the previous selection (beam is 1 at the first step, K afterwards), rows of `width` tokens.
 *   Live, unforced parent.  total[k][v] = score[k] + logf(expf(x_v - m) / z) with m = max_v x_v and z = sum_v expf(x_v - m), in
 *     k_beam_step's expressions and order: on rows of finite logits every output equals ttx_beam_generate's bit for bit (as long
 *     as that call selects no continuation of a finished hypothesis, see the next item).  A -inf
 *     logit (a forbidden or masked token) contributes expf(-inf) = 0 to z and gives a -inf child, so the scores are
 *     log-probabilities under the constrained, renormalised distribution.  A row with no finite logit gives -inf for every child,
 *     never NaN.
 *   Finished parent.  One child, PAD, with the total ttx_beam_generate gives it: score + logf(expf(35 - 35) / z) over the
 *     reference's artificial row, 35 on PAD and 0 elsewhere (standard_decoding.py:133-135), on the bits.  The other V - 1
 *     children, which that row puts 35 below the PAD child, are -inf here: ttx_beam_generate can only select one of them when a
 *     source has fewer than K children within 35 of its best finished hypothesis, which a constraint makes the ordinary case (an
 *     allow-list of two tokens), and they would fill the free ranks with rows that go on after their EOS instead of dead rows.
 *     A finished parent with score -inf is a DEAD parent: all its children are -inf.
 *   Forced position (width <= h_prefix_len[b]: the token at column `width` lies inside the source's prefix).  A live parent has one
 *     child, tok = d_prefix[b][width - 1] (an id outside [0, V) read as 0), with total = score[k] exactly; every other child is
 *     -inf.  The logits are not read, so bias and mask do not apply, and a forced token costs no log-probability.  Finished and
 *     dead parents behave as above.
 *   Selection.  The K largest totals over the beam * V children, largest first; equal values break towards the lower flat index
 *     k * V + v.  -inf children are taken only when fewer than K finite ones exist, then by ascending flat index, none twice.
 *   A selected -inf child is a DEAD ROW: the parent's tokens followed by PAD (the forbidden token is never written), score -inf,
 *     finished; it counts with the hypotheses holding EOS in the stop rule and costs no decoder row.  Its parent index is the
 *     real parent's.  A dead row only ever has -inf children, so it gives way to any finite child of a later level.
 *   Everything else (a new row is finished when its parent was or its token is EOS; the stop rule; out_width; the counters) is
 *     ttx_beam_generate's.
 * Consequences.  With d_bias, syntax and the prefixes all absent the call IS ttx_beam_generate, launch for launch (k_beam_step, no
 * k_logit_bias, no k_syntax_mask), plus the copy of the scores.  A bias of zeros, a table of neutral classes whose max_len no row
 * reaches, and an allow-list of every token each return ttx_beam_generate's rows on the bits.  The K rows of a source are pairwise
 * distinct; fewer than K may exist under a narrow allow-list or a short max_len, and the missing ranks are dead rows, last.  Every
 * finite row of a prompted call is BOS, the prefix, a completion.  Under a syntax table every finite row that ends, ends balanced.
 *   d_bias fp32 [B][ld_bias] or NULL; syntax as for ttx_sample_generate_syntax (NULL or d_cls NULL: none; max_len 0 or the call's);
 *   d_prefix int64 [B, ld_prefix] without BOS and h_prefix_len HOST int32 [B] (NULL: no prefixes), as for ttx_sbs_generate_ex;
 *   d_out as for ttx_beam_generate; d_score fp32 [B, K] or NULL: the rows' scores, -inf for a dead row.
 * TTX_ERR_INVALID with nothing launched: ld_bias below the vocabulary, a syntax max_len that is neither 0 nor the call's, a prefix
 * length outside [0, max_len - 1] or above ld_prefix, a non-zero length with d_prefix NULL; and everything ttx_beam_generate
 * refuses.  Cost: DESIGN.md §29. */
int ttx_beam_generate_constrained(ttx_session* s, const int64_t* d_src, int B, int Ls, const ttx_beam_search_params* p,
                                  const float* d_bias, int ld_bias, const ttx_syntax* syntax, const int64_t* d_prefix, int ld_prefix,
                                  const int32_t* h_prefix_len, int64_t* d_out, float* d_score, ttx_beam_search_stats* stats,
                                  void* stream);

/* Stochastic beam search (Kool, van Hoof & Welling, "Stochastic Beams and Where to Find Them", ICML 2019): K hypotheses per source
 * that are an exact sample WITHOUT replacement from the model's sequence distribution at the given temperature.  The loop is
 * ttx_beam_generate's (per-hypothesis KV cache, one decoder pass per level over the unfinished candidates) with k_sbs_step
 * (csrc/ttx_sbs.hip.h) where that loop launches k_beam_step.
 *
 * The rule.  Per candidate: phi (fp32 log-probability), G (fp32 perturbed log-probability) and `finished`.  Start: one <BOS>
 * candidate per source with phi = 0, G = 0.  Step at position pos (1 = first token after BOS), source with key `key`, candidates
 * k = 0 .. beam-1 in the order of the previous selection; beam is 1 at the first step and K afterwards:
 *   1  y_v = x_v * inv_T with inv_T = 1.0f / temperature formed on the host, one rounded fp32 product per logit.
 *   2  m = max_v y_v, z = sum_v expf(y_v - m) in an order fixed by V alone (csrc/ttx_sbs.hip.h), lp_v = (y_v - m) - logf(z),
 *      phi'_{k,v} = phi_k + lp_v.
 *   3  u_{k,v} = ((w >> 9) + 0.5f) * 2^-23, an fp32 strictly inside (0, 1), exact; w = word v & 3 of Philox4x32-10 with key
 *      (seed_lo, seed_hi) and counter (key_lo, key_hi, 0x80000000 | (k << 8) | (v >> 2), pos); constants and round function as
 *      for ttx_sample_generate.  Bit 31 of counter word 2 keeps these draws apart from the sampler's, whose word 2 is a sample id.
 *   4  g_{k,v} = phi'_{k,v} - logf(-logf(u_{k,v})), Z_k = max_v g_{k,v}.
 *   5  G'_{k,v} = G_k exactly where g_{k,v} == Z_k; elsewhere t = G_k - g + log1pf(-expf(g - Z_k)) and
 *      G' = G_k - fmaxf(t, 0) - log1pf(expf(-fabsf(t))).  A -inf logit gives G' = -inf.
 *   6  A finished candidate has one child, token PAD at flat index k * V + pad, with phi and G unchanged; its logits are not read.
 *   7  The new candidates are the K largest G' over the beam * V children, largest first; equal values break towards the lower
 *      flat index k * V + v.  New candidate r takes the parent's row plus the token, phi', G', and finished = parent finished or
 *      token in {EOS, PAD}.  G' = -inf is selected only when fewer than K finite children exist; such a candidate is finished and
 *      its logp and gumbel are -inf.
 *   8  The loop ends when all B * K candidates are finished, or after max_len - 1 steps.
 * Consequences: rank 0 of every source carries gumbel == 0.0f exactly; G' never exceeds its parent's G; the K hypotheses of a
 * source are pairwise distinct; noise is keyed by parent rank and ranks nest, so the call with K returns the first K rows of the
 * call with K' > K; the output depends on the source, its key, the seed, the temperature and K only (not on B or the padded width).
 *
 *   d_out int64 [B, K, max_len]: BOS, the tokens up to and including the row's first EOS or PAD, PAD after it; rows in sampling
 *   order (gumbel descending).  d_logp, d_gumbel fp32 [B, K].  d_row_keys int64 [B] or NULL (keys 0 .. B-1).
 *   trace (optional): device arrays [max_len - 1, B, K] of the parent rank, token, phi' and G' of every new candidate of every
 *   level; stats->model_calls says how many levels are valid.  stats->out_width is the number of columns the loop filled.
 * Cost, measured on one MI355X (4+4 model, 32 sources, max_len 200): 1.8 % (K = 5) and 2.2 % (K = 10) more per
 * decoder step than ttx_beam_generate with the same K, and 8.8 % / 11.0 % more per call, since the sampled rows run longer.
 * The top-k / top-p filter and forced prefixes are ttx_sbs_generate_ex below; many batches on a pool of source slots are
 * ttx_sbs_generate_pool.  TTX_ERR_INVALID with nothing launched: max_len <= 1,
 * beam_size outside [1, min(32, vocab_size)], vocab_size > 1024, beam_size * vocab_size * 4 > 150 KB, a temperature that is not
 * finite or not > 0, a trace with a NULL array, and everything else ttx_beam_generate refuses. */
typedef struct ttx_sbs_params {
  int32_t max_len, beam_size;            /* beam_size = K */
  float   temperature;                   /* finite, > 0 */
  int32_t pad_token, bos_token, eos_token;
  uint64_t seed;
} ttx_sbs_params;
typedef struct ttx_sbs_trace {
  int32_t* d_parent; int32_t* d_token;   /* [max_len - 1, B, K] */
  float* d_phi; float* d_g;
} ttx_sbs_trace;
int ttx_sbs_generate(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sbs_params* p,
                     int64_t* d_out, float* d_logp, float* d_gumbel, const ttx_sbs_trace* trace_or_null,
                     ttx_beam_search_stats* stats, void* stream);

/* Stochastic beam search under a top-k / top-p filter and / or forced target prefixes: ttx_sbs_generate with a per-parent token
 * mask in front of its rule (k_sbs_step_masked, csrc/ttx_sbs.hip.h).  A masked token behaves exactly like a -inf logit, which
 * steps 5 and 7 above already define.  Per unfinished parent k of source b at position pos, before step 2:
 *   Forced position (1 <= pos <= h_prefix_len[b]).  tok = d_prefix[b][pos - 1], an id outside [0, V) read as 0 (as the prompted
 *     samplers read theirs).  The child tok has phi' = phi_k and G' = G_k exactly; every other child of the parent is -inf.  The
 *     logits are not read and no Philox block is formed.  A forced token thus costs no log-probability: logp is the
 *     log-probability of the completion given source and prefix, and the rows are a sample without replacement from that
 *     conditional distribution.  A forced EOS or PAD finishes the row as any EOS or PAD does.
 *   Free position, filter on (top_k != 0 or top_p < 1; top_p < 1 with top_k = 0 runs with top_k = 32).  The kept set is the
 *     sampler's on the bits (ttx_sample_generate, step 4: ranks of y best first, equal values the lower id first, rank i kept while
 *     the softmax mass ranked above it is < top_p and i < top_k, rank 0 always; at most 32 tokens).  A token outside it has
 *     y_v = -inf.  Steps 2-5 run unchanged on that row, m, z and Z in the order fixed by V alone, masked ids contributing
 *     expf(-inf) = 0: lp is renormalised over the kept set, so the search samples without replacement from the sequence
 *     distribution the filtered ttx_sample_generate draws from.  Philox counters stay keyed by the token id v, not by the rank in
 *     the kept set: a kept token's uniform is the one the unfiltered call forms for it.  A kept set of one token is a mask of one
 *     token, as a forced position is: that child has phi' = phi_k and G' = G_k exactly.
 *   Steps 6-8 are unchanged.  Masked children are -inf children: selected only when fewer than K finite ones exist, by ascending
 *     flat index, finished, with logp = gumbel = -inf.
 * Consequences (exact): a kept set of every token (V <= 32, top_k = 32, top_p = 1) gives ttx_sbs_generate's outputs bit for bit;
 * top_k = 1 gives the greedy row at rank 0 with logp == gumbel == 0.0f and ranks >= 1 at -inf, finished; with f NULL (or top_k = 0,
 * top_p = 1) and no non-empty prefix the call IS ttx_sbs_generate, launch for launch; every finite row of a prompted call is BOS,
 * the prefix, a completion; gumbel of rank 0 is 0.0f; rows are pairwise distinct; K returns the first K rows of K' > K; the output
 * depends on the source, its prefix, its key, the seed, the temperature, the filter and K only.
 *   f_or_null: the filter; d_prefix int64 [B, ld_prefix] without BOS and h_prefix_len HOST int32 [B] (NULL: no prefixes), as for
 *   ttx_sample_generate_prefix.  Everything else as for ttx_sbs_generate.
 * TTX_ERR_INVALID with nothing launched: top_k outside [0, 32], top_p outside (0, 1], a prefix length outside [0, max_len - 1] or
 * above ld_prefix, a non-zero length with d_prefix NULL, and everything ttx_sbs_generate refuses.
 * Cost: DESIGN.md §23. */
typedef struct ttx_sbs_filter {
  int32_t top_k;                         /* 0: off, else 1..32 */
  float   top_p;                         /* (0, 1]; 1: off */
} ttx_sbs_filter;
int ttx_sbs_generate_ex(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sbs_params* p,
                        const ttx_sbs_filter* f_or_null, const int64_t* d_prefix, int ld_prefix, const int32_t* h_prefix_len,
                        int64_t* d_out, float* d_logp, float* d_gumbel, const ttx_sbs_trace* trace_or_null,
                        ttx_beam_search_stats* stats, void* stream);
/* ttx_sbs_generate_ex under a per-source logit bias ("Per-source logit bias" above; d_bias fp32 [B][ld_bias] on the device, NULL: the
 * call without one).  k_logit_bias rewrites every level's logits before the step kernel reads them (the row of a running candidate
 * takes the bias row of the candidate's source), so phi, logp and the K rows are those of the biased, then filtered, distribution: a
 * sample without replacement from what the biased sampler draws from.  Fewer than K rows may exist under a narrow allow-list; the
 * missing ranks come back as under a filter. */
int ttx_sbs_generate_bias(ttx_session* s, const int64_t* d_src, int B, int Ls, const int64_t* d_row_keys, const ttx_sbs_params* p,
                          const ttx_sbs_filter* f_or_null, const int64_t* d_prefix, int ld_prefix, const int32_t* h_prefix_len,
                          const float* d_bias, int ld_bias, int64_t* d_out, float* d_logp, float* d_gumbel,
                          const ttx_sbs_trace* trace_or_null, ttx_beam_search_stats* stats, void* stream);

/* Stochastic beam search over a whole list of sources on a pool of source slots (continuous batching; kernels and slot state:
 * csrc/ttx_sbs_pool.hip.h).  Each of up to n_sessions pools owns C <= capacity source slots of K candidates; a
 * source is admitted into a free slot (one <BOS> candidate with phi = G = 0), steps at its OWN level with its own key and prefix,
 * and retires - its K rows, logp and gumbel written to its row of the outputs, the slot free in the same iteration - as soon as
 * all K candidates are finished or its level has reached max_len - 1.  One decoder pass per iteration serves every unfinished
 * candidate of every source in the pool.
 *
 * Exactness contract.  Row s of d_out, d_logp and d_gumbel holds, bit for bit, what ttx_sbs_generate_ex writes for that source
 * with that key and prefix under the same p and f: tokens, logp and gumbel.  It does not depend on capacity, on the number of
 * pools in flight, on the order of the list or on what shares the pool.  The contract rests on the rule being per source (a source
 * whose K candidates are finished is a fixed point of the step), on the GEMM family's single summation order and on the
 * attention kernels' padding invariance.  Range: the pool fixes the key capacity of its self-attention at max_len while the
 * per-batch loop grows it with the width in buckets of 64, so beyond the staged key limit (ttx_attn_staged_key_limit: 384
 * positions, 320 at head dimension 64) the two may run different attention kernels, which agree to rounding only.  The contract
 * holds while max_len + 1 (the prefix keys and the step's own row) does not exceed that limit.
 *
 *   d_src int64 [S_total, Ls_all], sources in admission order (sort them longest first: an admission is encoded at the width of
 *   its longest source); h_len HOST int32 [S_total], the position after each source's last non-PAD token; d_row_keys int64
 *   [S_total] or NULL (keys 0 .. S_total - 1); capacity: sources per pool; f_or_null, d_prefix [S_total, ld_prefix],
 *   h_prefix_len as for ttx_sbs_generate_ex; d_out int64 [S_total, K, max_len], d_logp, d_gumbel fp32 [S_total, K].  There is no
 *   trace.  stats: sums over the pools.  S_total == 0 returns TTX_OK with nothing launched.
 * TTX_ERR_INVALID with nothing launched: a NULL pointer (d_row_keys, f, d_prefix and h_prefix_len may be NULL), capacity outside
 * [1, 1024], an h_len entry above Ls_all or below 2, and everything ttx_sbs_generate_ex refuses.  TTX_ERR_HIP "failed to
 * terminate" once a pool's iterations exceed max_len * (S_total + 1). */
typedef struct ttx_sbs_pool_stats {
  int64_t model_calls;             /* iterations executed (decoder passes), summed over the pools             */
  int64_t running_rows;            /* unfinished candidates summed over the iterations                        */
  int64_t src_tokens_padded;       /* encoder positions computed                                              */
  int64_t live_slots;              /* occupied source slots summed over the iterations                        */
  double  decode_ms;               /* device time (HIP events) from a pool's start to its last retirement, summed */
  int32_t status;
  int32_t pad_;
  int32_t* d_src_running_rows;     /* IN, the block's one input: NULL, or a device int32 [S_total] that receives, per source, the
                                      candidates decoded for it summed over its levels (the entries sum to running_rows)   */
} ttx_sbs_pool_stats;
int ttx_sbs_generate_pool(ttx_session** sessions, int n_sessions, const int64_t* d_src, int S_total, int Ls_all,
                          const int32_t* h_len, const int64_t* d_row_keys, int capacity /* sources per pool */,
                          const ttx_sbs_params* p, const ttx_sbs_filter* f_or_null,
                          const int64_t* d_prefix, int ld_prefix, const int32_t* h_prefix_len,
                          int64_t* d_out /* [S_total][K][max_len] */, float* d_logp, float* d_gumbel /* [S_total][K] */,
                          ttx_sbs_pool_stats* stats, void* stream);

/* Several batches in flight on one GPU (the scheduling SURVEY.md §8(f) #1 names; the reference's predict loop
 * is strictly one batch at a time, src/model/lightning_model.py:209-212).  Batch i is decoded on
 * sessions[i % n_sessions]; each session runs on its own internal stream that first waits for `stream`
 * (the stream the inputs were produced on); the call returns when every output is complete.  Per-batch
 * outputs and stats are identical to n_batches calls of ttx_greedy_speculative_generate. */
int ttx_greedy_speculative_generate_many(ttx_session** sessions, int n_sessions, int n_batches,
                                         const int64_t* const* d_src, const int* B, const int* Ls,
                                         const ttx_gen_params* p, int64_t* const* d_out, ttx_gen_stats* stats,
                                         void* stream);

/* Row-scheduled decoding (second half: batches regrouped by length).  The reference's loop
 * couples the rows of a batch only through the shared width of `generated_tokens` (speculative_decoding.py:93,
 * :97-102, :145, :158): the loop ends once max(front) + draft_len + 2 >= max_len, and a row finishing at a width
 * beyond max_len raises.  Tokens, drafts and accepted lengths of a row do not depend on its neighbours.  This
 * entry point therefore decodes every row under the rule it would see ALONE in a batch (continue while
 * front + draft_len + 2 < max_len) and returns, besides d_out[i] (int64 [B_i][max_len]; rows that never produced
 * EOS stay PAD), each row's front after every verify step: d_traj[i] int16 [B_i][max_len + 1] (column 0 = 0, -1
 * past the row's last step) and d_fin_step[i] int32 [B_i] (the step that produced EOS, 0 = none).  From these a
 * caller that regrouped rows (e.g. sorted by source length) replays the reference's width rule over the ORIGINAL
 * batches and obtains exactly their outputs, errors and model-call counts; translation-transformer_amd/decoding.py
 * `generate_many(..., reorder=True)` does that.  Returns TTX_ERR_ROW_REPLAY when a row emitted PAD inside its
 * sequence (reference quirk: the outcome then depends on the neighbours; decode those batches as given). */
int ttx_greedy_speculative_generate_rows(ttx_session** sessions, int n_sessions, int n_batches,
                                         const int64_t* const* d_src, const int* B, const int* Ls,
                                         const ttx_gen_params* p, int64_t* const* d_out, int16_t* const* d_traj,
                                         int32_t* const* d_fin_step, ttx_gen_stats* stats, void* stream);

/* The same contract as ttx_greedy_speculative_generate_rows with continuous batching: rows are not cut into fixed
 * groups; every session keeps a pool of up to `capacity` slots and admits the next rows of the work list (encoder,
 * cross K/V, drafts, slot state) whenever at least a quarter of its slots are free, so the verify step keeps
 * close to capacity * (1 + n_drafts * draft_len) rows until the list is exhausted.  d_src int64 [R_total][Ls_all] holds
 * ALL rows right-padded, in the order they are to be admitted (sorted by length pads least: a chunk of rows is encoded at the
 * width of its longest row); h_len (HOST, int32 [R_total]) their lengths (position after the last non-PAD token).  d_out int64 [R_total][max_len], d_traj int16 [R_total][max_len + 1], d_fin_step int32
 * [R_total] as in ttx_greedy_speculative_generate_rows, in the order of d_src.  `stats` (zero it first) receives the
 * sums over all sessions; stats->model_calls counts the verify steps the device executed.  Returns
 * TTX_ERR_ROW_REPLAY like the rows call. */
int ttx_greedy_speculative_generate_pool(ttx_session** sessions, int n_sessions, const int64_t* d_src, int R_total, int Ls_all,
                                         const int32_t* h_len, int capacity, const ttx_gen_params* p, int64_t* d_out,
                                         int16_t* d_traj, int32_t* d_fin_step, ttx_gen_stats* stats, void* stream);

/* Host-side string work either side of the hot path (no GPU) ------------------------------------
 * ChemSMILESTokenizer (src/data_handling/tokenizer_smiles.py:8-39), the pad_sequence collate
 * (src/data_handling/seq2seq_wrappers.py:121-127) and GenericTokenizer.decode (tokenizer_base.py:80-91).
 * ttx_tokenizer_create takes the vocabulary as parallel arrays (token string, id), i.e. the reference's vocab.json
 * (decoder_dict); service ids are the reference's fixed PAD=0, BOS=1, EOS=2, UNK=3.
 * encode: number of ids the line needs (BOS/EOS included), writing min(that, cap) of them;
 * encode_batch: int64 [B, cap_cols] padded with PAD, returns the padded width (or -needed if cap_cols is too small);
 * decode: skips service tokens, stops at the first EOS, returns the string length, writes a NUL-terminated string. */
typedef struct ttx_tokenizer ttx_tokenizer;
int  ttx_tokenizer_create(const char* const* tokens, const int32_t* ids, int n, ttx_tokenizer** out);
void ttx_tokenizer_destroy(ttx_tokenizer* t);
int  ttx_tokenizer_encode(const ttx_tokenizer* t, const char* line, int32_t* out, int cap);
int  ttx_tokenizer_encode_batch(const ttx_tokenizer* t, const char* const* lines, int B, int64_t* out, int cap_cols);
int  ttx_tokenizer_decode(const ttx_tokenizer* t, const int64_t* ids, int n, char* out, int cap);

/* Parity instrumentation for the KV-cached verify step: the step selected by ttx_gen_params.want_logits (1-based step
 * number) of the most recent generate call on `s` — its pre-argmax logits and the loop state they were computed from.
 * HOST destinations: h_logits [n_active*rps, V], h_act int32 [n_active] (running rows in slot order), h_front int32 [B],
 * h_gen int32 [B, gen_ld]; info[0..5] = n_active, rps (= 1 + N*D rows per sequence), B, gen_ld, V, step.  Any of the
 * four array pointers may be null (e.g. a first call to learn the sizes). */
int ttx_debug_step_snapshot(ttx_session* s, int32_t* info, float* h_logits, int32_t* h_act, int32_t* h_front,
                            int32_t* h_gen);

/* Timing of the dominant kernel for bench.py's roofline: summed HIP-event time (events recorded on the launch stream around
 * every GEMM launch) and launch count of the generate calls on this session since the previous read (reading resets the sums);
 * `empty_pair_ms` is what the bracketing adds to a launch's figure, calibrated on the same stream with pairs around a kernel of
 * known duration (pair time minus the realtime ticks the kernel saw go by; median of 32).  Only collected when the session was
 * created with TTX_PROFILE_GEMM=1 in the environment (that session launches eagerly, without graphs).  The *_pool and *_many
 * entry points run the sessions of a call ONE AFTER ANOTHER when sessions[0] is a profiling session (each pool decodes the share of
 * the work list it takes when all start together), so that an event pair times its own launch and not the other sessions' kernels;
 * every session of the call must then be a profiling one (NativeTransformer built under TTX_PROFILE_GEMM=1 sees to that). */
int ttx_last_kernel_profile(ttx_session* s, double* gemm_ms, int64_t* gemm_launches, double* empty_pair_ms);

/* Development aid (tools/bench_gemm.py): times one GEMM shape (K = 64, 128 or a multiple of 256) in isolation on random
 * operands.  variant 2 / 46 = 64x64, 128x64 tiles; 24 = the production kernel's own choice from the row count;
 * 3 = one wave per canonical slice (32x32 tiles, K = 256); 8 = one workgroup per slice with `splits` raw slabs (FFN2).  Returns
 * microseconds per launch over `reps` back-to-back launches and the largest absolute difference to the 64x64 tiling's result
 * — 0.0 for every variant: all of them evaluate the same ordered sum of K slices (csrc/ttx_gemm.hip). */
int ttx_debug_gemm_bench(ttx_session* s, int M, int N, int K, int splits, int variant, int reps, double* us_per_launch,
                         double* max_abs_diff);

/* Test entry points (tests/test_gpu_gemm_kernels.py): ONE launch of the GEMM family / the LayerNorm finisher on DEVICE operands
 * of the caller.  Y = act(X W^T + bias) with X [m_max, ldx], W [N, ldw], Y [m_max, ldy] (splits == 0), or `splits` raw slabs
 * Y[s] = X[:, s K/splits ...] W[:, ...]^T at d_y + s * slab_stride (no bias, no activation).  d_m: live row count on the
 * device (a verify-step launch; rows >= *d_m are neither read into a result nor written) or NULL (all m_max rows).
 * variant: 0 big tiles, 1 short chains, 2 big tiles with FFN2 slabs, 3 mid; tiling: 0 the production choice between the
 * 64x64 and the 128x64 body, 1 64x64 only, 2 128x64 whenever the kernel has both.  kernel_id (optional) receives what was
 * dispatched: 1 k_gemm3, 2 k_gemm_tn, 3 k_gemm24<4>, 4 k_gemm24<0>, 5..8 k_gemm2<1|2|4|0>, plus 16 when k_gemm24 takes the
 * 128x64 body for this row count.  Nothing is launched and TTX_ERR_INVALID is returned for arguments a kernel cannot take:
 * null pointers, K not a multiple of 32, ldx / ldw not multiples of 4, X / W / bias (and Y when ldy % 4 == 0) not 16-byte
 * aligned, slabs that are not whole canonical slices (K / splits of 64, 128 or a multiple of 256; a multiple of 32 for K
 * without slices), a live row count outside [0, m_max]. */
int ttx_debug_gemm(ttx_session* s, const float* d_x, int ldx, const float* d_w, int ldw, const float* d_bias, float* d_y, int ldy,
                   const int32_t* d_m, int m_max, int N, int K, int relu, int splits, int64_t slab_stride, int variant, int tiling,
                   int32_t* kernel_id, void* stream);
/* ttx_debug_gemm with a ttx_activation (0 none, 1 ReLU, 2 exact GELU) in place of `relu`; any other value, or an activation on raw
 * slabs (splits > 0), is TTX_ERR_INVALID and nothing is launched.  ttx_debug_gemm forwards here with relu ? 1 : 0.  The kernel ids
 * are the same: GELU is another instantiation of the kernel the shape dispatches to (tests/test_gpu_gemm_gelu.py). */
int ttx_debug_gemm_act(ttx_session* s, const float* d_x, int ldx, const float* d_w, int ldw, const float* d_bias, float* d_y, int ldy,
                       const int32_t* d_m, int m_max, int N, int K, int activation, int splits, int64_t slab_stride, int variant,
                       int tiling, int32_t* kernel_id, void* stream);

/* y = LN2?( LN( (resid + bias) + (slab[0] + slab[1] + ...) ) ) over rows of width d in {64, 128, 256, 512, 1024}; rows with
 * row_valid == 0 become 0, rows >= *d_m are left alone.  d_g2 / d_b2 / d_row_valid / d_m may be NULL.  Float operands must be
 * 16-byte aligned and slab_stride a multiple of 4 covering m_max * d; otherwise TTX_ERR_INVALID, nothing launched. */
int ttx_debug_finish_ln(ttx_session* s, const float* d_slabs, int n_slabs, int64_t slab_stride, const float* d_bias,
                        const float* d_resid, const float* d_g1, const float* d_b1, const float* d_g2, const float* d_b2,
                        const uint8_t* d_row_valid, float* d_y, const int32_t* d_m, int m_max, int d, float eps, void* stream);

/* Test entry point (tests/test_gpu_attn_kernels.py): ONE launch of the attention family on DEVICE operands of the caller.  The
 * arguments are those of the kernels' argument block (csrc/ttx_common.hip.h: AttnArgs): per head, out = softmax(scale q k^T + mask) v
 * with d = 32 H, query rows at d_q + row * ldq, key / value rows at d_k / d_v + row * ldkv, output rows d wide.  mode: 0 encoder
 * (keys masked where tok == pad), 1 full-prefix decoder self-attention (the same, causal), 2 full-prefix cross-attention (memory
 * row mem_row[g] or g, key_pad 1 = PAD), 3 verify-step self-attention (slot g < n_active is sequence act_idx[g] with front
 * front[b], token row tok + b * gen_ld, cache row cache_slot[b] or b of kcache / vcache [.., cache_seq_stride] with rows d wide,
 * and the 1 + N*D step rows g * (1 + N*D) ..), 4 verify-step cross-attention (source row src_of[b] or b, its first src_len[b] or
 * Lk keys, key_pad 1 = real token).  groups: decoder rows / sources / slots; n_active (step modes) is put into a DecState on the
 * device, ordered on `stream`, before the launch; max_keys is what production passes to the launcher: the cache capacity (every
 * front <= max_keys; the caller's promise, like the indices in the device arrays) or the key count Ls.  kernel: 0 the production
 * choice, 1 k_attn, 2 k_attn2, 3 k_attn3, 4 k_attn3s, 5 k_attn1; kernel_id (optional) receives what was dispatched (1..5).  Nothing is
 * launched and TTX_ERR_INVALID is returned for arguments a kernel cannot take: a null pointer the mode requires, H <= 0, ldq /
 * ldkv that are not multiples of 4 or below d, float operands that are not 16-byte aligned, n_active outside [0, groups], max_keys
 * below L / Lk, and a forced kernel that cannot serve the request (never rerouted): k_attn3 / k_attn3s outside the step modes or
 * with H % 4 != 0, k_attn3 whose parked partials exceed 64 KB of LDS, k_attn2 beyond 384 staged keys or its LDS limit, k_attn
 * beyond its LDS limit, k_attn1 outside the step modes, with H % 4 != 0, at head dimension 64 or with N * D > 0 (it serves step
 * launches of one row per slot).  This entry point launches at head dimension 32; ttx_debug_attn_hd below takes the head dimension. */
int ttx_debug_attn(ttx_session* s, const float* d_q, int ldq, const float* d_k, const float* d_v, int ldkv, float* d_out, int H,
                   float scale, int L, int Lk, const int32_t* d_tok, int pad, const uint8_t* d_key_pad, const int32_t* d_mem_row,
                   const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_src_of, const int32_t* d_src_len,
                   const float* d_kcache, const float* d_vcache, int64_t cache_seq_stride, const int32_t* d_cache_slot, int gen_ld,
                   int N, int D, int mode, int groups, int n_active, int max_keys, int kernel, int32_t* kernel_id, void* stream);

/* ttx_debug_attn at head dimension head_dim (32 or 64; anything else is TTX_ERR_INVALID): d = head_dim * H, every other argument
 * as above (tests/test_gpu_attn_hd64.py).  k_attn3 / k_attn3s exist at head dimension 32 only: forced at 64 they are refused,
 * and the production choice for a step mode is then k_attn2 (k_attn beyond its capacity) whatever H is.  k_attn2 stages at most
 * ttx_attn_staged_key_limit keys. */
int ttx_debug_attn_hd(ttx_session* s, const float* d_q, int ldq, const float* d_k, const float* d_v, int ldkv, float* d_out, int H,
                      int head_dim, float scale, int L, int Lk, const int32_t* d_tok, int pad, const uint8_t* d_key_pad,
                      const int32_t* d_mem_row, const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_src_of,
                      const int32_t* d_src_len, const float* d_kcache, const float* d_vcache, int64_t cache_seq_stride,
                      const int32_t* d_cache_slot, int gen_ld, int N, int D, int mode, int groups, int n_active, int max_keys,
                      int kernel, int32_t* kernel_id, void* stream);

/* ttx_debug_attn_hd for a step-mode launch that chooses between k_attn2 and k_attn as a launch in the layout (sel_N, sel_D) on the
 * same cache does: what the probe of the two-phase verify step does with the draft pass's layout (DESIGN.md "Two-phase verify
 * step"), because the two kernels do not give the same bits.  kernel = 0 is the case it exists for.  Refused: sel_N < 1, sel_D < 0. */
int ttx_debug_attn_as(ttx_session* s, const float* d_q, int ldq, const float* d_k, const float* d_v, int ldkv, float* d_out, int H,
                      int head_dim, float scale, int L, int Lk, const int32_t* d_tok, int pad, const uint8_t* d_key_pad,
                      const int32_t* d_mem_row, const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_src_of,
                      const int32_t* d_src_len, const float* d_kcache, const float* d_vcache, int64_t cache_seq_stride,
                      const int32_t* d_cache_slot, int gen_ld, int N, int D, int mode, int groups, int n_active, int max_keys,
                      int kernel, int32_t* kernel_id, int sel_N, int sel_D, void* stream);

/* Test entry points (tests/test_gpu_loop_kernels.py): ONE launch of a loop kernel of csrc/ttx_loop_kernels.hip.h on DEVICE operands
 * of the caller, with production's grid and block rules.  All of them are integer or bit-copy work: the tests ask for exact
 * equality with tests/util_loop_checks.py.  Nothing is launched and TTX_ERR_INVALID is returned for arguments a kernel cannot
 * take; the device-side index arrays are read back and checked too (these are test calls).
 *
 * ttx_debug_argmax: k_argmax, one wave per row of d_logits [m_max, V] (any V >= 1): d_pred[row] = the first index of the row's
 * maximum (-0.0 == 0.0; an all -inf row and an all-NaN row give 0); rows that mix NaN with other values are outside the
 * contract and only give some id in [0, V).  d_m: live row count on the device
 * or NULL (all m_max rows); rows >= *d_m are not written.  Refused: null pointers, V < 1, m_max < 1, *d_m outside [0, m_max]. */
int ttx_debug_argmax(ttx_session* s, const float* d_logits, int V, int32_t* d_pred, const int32_t* d_m, int m_max, void* stream);

/* ttx_debug_sample (tests/test_gpu_sample_kernel.py): ONE launch of k_sample with production's grid on the caller's device operands,
 * the rule of ttx_sample_generate.  d_logits fp32 [m_max, V], d_key uint64 [m_max], d_sample uint32 [m_max], d_done int32 [m_max]
 * (read and written: rows with done != 0 give PAD and their logits are not read; a row that emits EOS or PAD is marked), d_front
 * int32 [1] (the position filled is d_front[0] + 1), d_pred int32 [m_max] out, d_m the live row count on the device or NULL (all
 * m_max rows); rows >= *d_m are not written.  Of `p` the temperature, top_k, top_p, pad_token, eos_token and seed are used.
 * Refused: null pointers, V < 1, V > 1024, m_max < 1, *d_m outside [0, m_max], and the parameter errors of ttx_sample_generate. */
int ttx_debug_sample(ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample, int32_t* d_done,
                     const int32_t* d_front, int32_t* d_pred, const int32_t* d_m, int m_max, const ttx_sample_params* p, void* stream);

/* ttx_debug_sample_step (tests/test_gpu_sample_step_kernel.py): ONE launch of k_sample_step with production's grid (B * (1 + N*D)
 * rows, 4 per workgroup) on the caller's device operands.  d_logits fp32 [B * (1 + N*D), V] in the step-row layout of
 * ttx_debug_embed; d_key uint64 [B] and d_sample uint32 [B] by decoder row; d_act_idx int32 [B]; d_front int32 [B].  Row
 * slot * (1 + N*D) + rs belongs to decoder row b = d_act_idx[slot]; it gets ttx_debug_sample's token for (d_key[b], d_sample[b]) at
 * position d_front[b] + 1 (rs == 0) or d_front[b] + 2 + (rs - 1) % D.  d_m: live row count on the device, or NULL (all rows; then
 * n_active == B); rows >= *d_m are not written.  Refused: null pointers, V outside [1, 1024], B, N, D < 1, n_active outside
 * [0, B], act_idx that are not distinct rows of [0, B), a negative front, *d_m outside [0, n_active * (1 + N*D)], and the parameter
 * errors of ttx_sample_generate. */
int ttx_debug_sample_step(ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample,
                          const int32_t* d_act_idx, const int32_t* d_front, int B, int N, int D, int n_active, int32_t* d_pred,
                          const int32_t* d_m, const ttx_sample_params* p, void* stream);

/* ttx_debug_embed: k_embed on the caller's embedding table d_table [V, d] and positional table d_pe [pe_rows, d]:
 * X[row] = table[tok] + pe[pos + 1] in fp32, ids outside [0, V) looked up as id 0.  step == 0 (full mode): tok = d_tok[row],
 * pos = row % L, rows [0, rows).  step != 0 (one verify step): slot g < n_active is sequence b = d_act_idx[g] with front f =
 * d_front[b] and owns the 1 + N*D rows g * (1 + N*D) ..: row 0 is d_gen[b * gen_ld + f] at position f, row 1 + n*D + (j-1) is
 * d_drafts[b, n, j-1] at position f + j; the grid covers B slots and the live row count n_active * (1 + N*D) is put into a
 * DecState on the device, ordered on `stream`; rows beyond it are not written.  Refused: null pointers the mode needs, d not in
 * {64, 128, 256, 512, 1024}, table / pe / X not 16-byte aligned, n_active outside [0, B], act_idx that are not distinct rows of
 * [0, B), a gen_ld too small for front + D + 2, a positional table with fewer than L + 1 (full) or front + D + 2 (step) rows. */
int ttx_debug_embed(ttx_session* s, const float* d_table, int V, const float* d_pe, int pe_rows, int d, float* d_x,
                    const int32_t* d_tok, int rows, int L, const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_gen,
                    int gen_ld, const int32_t* d_drafts, int B, int N, int D, int n_active, int step, void* stream);

/* Operands of ttx_debug_accept: the argument block of k_accept / k_greedy_accept (csrc/ttx_loop_kernels.hip.h: LoopArgs), every
 * array a DEVICE array of the caller.  act_idx int32 [B] (running rows in slot order), front int32 [B], gen int32 [B, gen_ld],
 * drafts int32 [B, N, D], pred int32 [n_active * (1 + N*D)] in the step-row layout above, rec int32 [B, 5] (b, best, n_acc,
 * front_old, flags per slot), out int64 [B, max_len], haspad int32 [B].  row_rule: traj int16 [B, traj_ld], fin_step int32 [B].
 * pool (implies row_rule): rstep, row_of int32 [B] and the caller-side rows pool_out int64 [pool_rows, max_len], pool_traj int16
 * [pool_rows, traj_ld], pool_fin_step int32 [pool_rows] take the place of out, traj and fin_step. */
typedef struct ttx_debug_accept_args {
  int32_t* d_act_idx; int32_t* d_front; int32_t* d_gen; const int32_t* d_drafts; const int32_t* d_pred; int32_t* d_rec;
  int64_t* d_out; int32_t* d_haspad;
  int16_t* d_traj; int32_t* d_fin_step;
  int32_t* d_rstep; int32_t* d_row_of; int64_t* d_pool_out; int16_t* d_pool_traj; int32_t* d_pool_fin_step;
  int32_t gen_ld, traj_ld, pool_rows, row_rule, pool;
  int32_t B, N, D, Ls, max_len, pad, bos, eos;
  int32_t greedy;          /* 1: k_greedy_accept (N = 1, D = 0, no row_rule; rows [0, n_active) all at the front of row 0) */
  int32_t threads;         /* k_accept's block size: 0 the production choice (256 for B <= 256; above, k_accept_slots + k_accept_finish, or 1024 under TTX_ACCEPT_SPREAD=0), or 256 / 1024 */
} ttx_debug_accept_args;

/* ttx_debug_accept: ONE launch of k_accept (greedy: k_greedy_accept).  `state` is a HOST array of 17 int64: on entry [0..7] =
 * n_active, r_rows, m_rows, stop, width, steps, error, n_copy and [8..12] = accepted, produced, verified_positions,
 * kv_prefix_positions, src_positions, put into a DecState on the device, ordered on `stream`; on return the same 13 words as the
 * kernel left them, copied back after the launch completed, and [13..16] = the words it published for the host (stop,
 * steps_done, width, n_active; -1 each when the kernel published nothing, as at n_active == 0).
 * threads: production never launches 256 threads for B > 256, so that is refused; 1024 threads are a launch the kernel is
 * written for at any B and are accepted everywhere, so both sizes can be compared wherever B <= 256.  k_greedy_accept always
 * runs with 256 threads.  Also refused: null required pointers, n_active outside [0, B], act_idx that are not distinct rows of
 * [0, B), a gen_ld below max_len or too small for front + D + 2 of a running row, row_of outside [0, pool_rows). */
int ttx_debug_accept(ttx_session* s, const ttx_debug_accept_args* a, int64_t* state, void* stream);

/* ttx_debug_sample_accept (tests/test_gpu_sample_accept_kernel.py): ONE launch of k_sample_accept, the accept step of
 * ttx_sample_speculative_generate, on ttx_debug_accept's argument block and `state`.  greedy, row_rule and pool are 0; d_pred
 * holds the draws of the step rows; d_haspad int32 [B] holds zeros and is not written.  A running row's tokens j = 0 .. n_acc of
 * the best draft's draws are written after its front; it ends (rec flags 1, copied to out[row, :max_len], dropped from act_idx)
 * when a written token in a column below max_len is EOS or PAD or when its new front is >= max_len - 1; width = max(old fronts) +
 * D + 2; the loop stops when no row runs; error stays as it was.  threads: 0 (256 for B <= 256, else 1024), 256 or 1024; the
 * kernel takes any B by rounds.  Refusals as for ttx_debug_accept. */
int ttx_debug_sample_accept(ttx_session* s, const ttx_debug_accept_args* a, int64_t* state, void* stream);

/* ttx_debug_sample_step_select (tests/test_gpu_sample_step_select_kernel.py): ONE launch of k_sample_step as a pass of the slot
 * pool runs it, on ttx_debug_sample_step's operands.  The launch covers n_rows rows stored compacted: d_logits fp32 [n_rows, V] and
 * d_pred int32 [n_rows]; row i draws for layout row d_row_map[i] (int32 [n_rows], as ttx_debug_embed_select reads it; NULL: row i
 * itself, and n_rows == n_active * (1 + N*D)): decoder row b = d_act_idx[d_row_map[i] / (1 + N*D)], position as in
 * ttx_debug_sample_step from the row inside the slot.  The probe layout N = 1, D = 0 is accepted (every row predicts d_front[b] + 1).
 * d_m: live row count on the device or NULL (n_rows).  Refused: what ttx_debug_sample_step refuses (D = 0 only with N = 1), n_rows
 * outside [1, n_active * (1 + N*D)], a row map entry outside the active slots' rows, *d_m outside [0, n_rows]. */
int ttx_debug_sample_step_select(ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample,
                                 const int32_t* d_act_idx, const int32_t* d_front, int B, int N, int D, int n_active, int32_t* d_pred,
                                 const int32_t* d_m, const ttx_sample_params* p, const int32_t* d_row_map, int n_rows, void* stream);

/* The forced prefixes of a debug launch (tests/test_gpu_prefix_kernels.py), as the kernels see them: d_tok int32 [n_sources][ld]
 * the table, d_len int32 [rows] and d_src int32 [rows] by decoder row (slot of a pool): the length of the row's prefix and its row
 * of the table.  Checked on the host: lengths in [0, ld], sources in [0, n_sources). */
typedef struct ttx_debug_prefix {
  const int32_t* d_tok; int32_t ld, n_sources;
  const int32_t* d_len; const int32_t* d_src;
} ttx_debug_prefix;

/* ttx_debug_prefix_drafts: ONE launch of k_prefix_drafts with production's grid (one wave per slot of B) on the caller's arrays.
 * For every active row b = d_act_idx[slot], slot < n_active, and j < D: d_drafts[b][0][j] = prefix token of column
 * c = d_front[b] + 1 + j when c <= d_len[b] (eos_token and pad_token as replace_token), else d_draft0[b][j].  d_drafts int32
 * [B, N, D]; d_draft0 int32 [B, D]; nothing else is written.  Synchronises the stream.  Refused: null pointers, B, N or D < 1,
 * n_active outside [0, B], repeated or out-of-range d_act_idx entries, negative fronts, and a prefix table outside its bounds.
 * ttx_debug_sample_prefix: ttx_debug_sample with the table (rows = m_max); a live row with d_front[0] + 1 <= d_len[row] emits its
 * prefix token (an id outside [0, V) as 0), sets done on EOS / PAD, and does not read its logits.
 * ttx_debug_sample_step_prefix: ttx_debug_sample_step_select (row map, probe layout, compacted rows) with the table (rows = B). */
int ttx_debug_prefix_drafts(ttx_session* s, const int32_t* d_act_idx, const int32_t* d_front, int B, int N, int D, int n_active,
                            int32_t* d_drafts, const int32_t* d_draft0, const ttx_debug_prefix* pfx, int eos_token, int pad_token,
                            int replace_token, void* stream);
int ttx_debug_sample_prefix(ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample, int32_t* d_done,
                            const int32_t* d_front, int32_t* d_pred, const int32_t* d_m, int m_max, const ttx_sample_params* p,
                            const ttx_debug_prefix* pfx, void* stream);
int ttx_debug_sample_step_prefix(ttx_session* s, const float* d_logits, int V, const uint64_t* d_key, const uint32_t* d_sample,
                                 const int32_t* d_act_idx, const int32_t* d_front, int B, int N, int D, int n_active, int32_t* d_pred,
                                 const int32_t* d_m, const ttx_sample_params* p, const int32_t* d_row_map, int n_rows,
                                 const ttx_debug_prefix* pfx, void* stream);

/* ttx_debug_proposal_drafts (tests/test_gpu_proposal_kernel.py): ONE launch of k_proposal_drafts with production's grid (one wave
 * per slot of B) on the caller's arrays, under the rule of "Proposal drafts" above with CTX = ctx.  d_gen int32 [B, gen_ld] the
 * rows' tokens (columns 0 .. d_front[b] are read); `proposal` the table as ttx_debug_prefix describes it (d_len, d_src by slot);
 * d_drafts int32 [B, N, D]; d_draft0 int32 [B, D]; only draft 0 of the active rows is written.  Synchronises the stream.  Refused:
 * null pointers, B, N, D or gen_ld < 1, n_active outside [0, B], repeated or out-of-range d_act_idx entries, an active front
 * outside [0, gen_ld), ctx other than 2, 4, 8, and a table outside its bounds. */
int ttx_debug_proposal_drafts(ttx_session* s, const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_gen, int gen_ld, int B,
                              int N, int D, int n_active, int32_t* d_drafts, const int32_t* d_draft0, const ttx_debug_prefix* proposal,
                              int ctx, int bos_token, int eos_token, int pad_token, int replace_token, void* stream);

/* ttx_debug_sample_accept_pool (tests/test_gpu_sample_accept_pool_kernel.py): the accept step of
 * ttx_sample_speculative_generate_pool on ttx_debug_accept's argument block and `state`: greedy 0, row_rule and pool 1; d_row_of
 * int32 [B] and d_pool_out int64 [pool_rows, max_len] are required, an ended row b is copied to d_pool_out[d_row_of[b]]; the traj /
 * fin_step / rstep pointers are unused.  d_exec_rows (device int32, or NULL): what verified_positions adds instead of n_active *
 * (1 + N*D).  spread 0: ONE launch of k_sample_accept (threads 0, 256 or 1024 as for ttx_debug_sample_accept); spread 1 (threads 0):
 * the pair k_sample_accept_slots, k_accept_finish at any B (production takes it above 256 slots), which leaves the session's
 * AcceptBlk zero (ttx_debug_accept_block).  Both forms leave the same state.  Refusals as for ttx_debug_accept. */
int ttx_debug_sample_accept_pool(ttx_session* s, const ttx_debug_accept_args* a, int64_t* state, const int32_t* d_exec_rows, int spread,
                                 void* stream);

/* ttx_debug_pool_fill_sample (tests/test_gpu_pool_fill_sample.py): ONE admission of the sampling pool, k_pool_admit then k_pool_fill,
 * on the caller's arrays: n_sources staged sources (first_src the first one's index in the call's list) x per_src samples into a
 * pool of B slots of which the n_active slots d_act_idx[0 .. n_active) are occupied.  New decoder row i takes the lowest free slot
 * b: front 0, haspad 0, rstep 0, row_of = first_src * per_src + i, src_len = Ls_new, key = d_row_keys[first_src + i / per_src]
 * (NULL: that index), sample = i % per_src; gen row BOS then PAD; drafts [N * D], validity bytes (zero from Ls_new to Ls_cap) and
 * cross K/V [Ls_new, kv_row] of staged source i / per_src; caller row d_out[row_of] = BOS then PAD.  Per-slot arrays int32 [B]
 * (d_key uint64 [B], d_sample uint32 [B]), d_gen int32 [B, gen_ld], d_drafts int32 [B, N * D], d_src_valid uint8 [B, Ls_cap], d_memkv
 * fp32 [B, Ls_cap, kv_row]; staged d_drafts_new int32 [n_sources, N * D], d_valid_new uint8 [n_sources, Ls_new], d_memkv_new fp32
 * [n_sources, Ls_new, kv_row]; d_out int64 [out_rows, max_len].  result (HOST int32 [4]): n_active, m_rows and error of the state
 * after the admission, and the n_active word published for the host.  More rows than free slots: error 4, and nothing is filled.
 * Refused: null arrays (d_row_keys may be NULL), non-positive sizes, B or rows above 4096, Ls_new > Ls_cap, kv_row not a multiple
 * of 4 or K/V arrays not 16-byte aligned, admitted rows beyond out_rows, act_idx that are not distinct slots of [0, B). */
typedef struct ttx_debug_pool_fill_args {
  int32_t* d_act_idx; int32_t* d_front; int32_t* d_haspad; int32_t* d_rstep; int32_t* d_row_of; int32_t* d_src_len;
  uint64_t* d_key; uint32_t* d_sample; const int64_t* d_row_keys;
  int32_t* d_gen; int32_t* d_drafts; const int32_t* d_drafts_new; uint8_t* d_src_valid; const uint8_t* d_valid_new;
  float* d_memkv; const float* d_memkv_new; int64_t* d_out;
  int32_t B, N, D, n_active, n_sources, per_src, first_src, Ls_new, Ls_cap, gen_ld, kv_row, max_len, out_rows, bos, pad;
} ttx_debug_pool_fill_args;
int ttx_debug_pool_fill_sample(ttx_session* s, const ttx_debug_pool_fill_args* a, int32_t* result, void* stream);

/* ttx_debug_accept_block: the first n_words int32 words of the session's AcceptBlk (csrc/ttx_loop_kernels.hip.h: the sums that
 * k_accept_slots hands k_accept_finish; 264 words), copied to the HOST array `words` after `stream` has drained.  Every word is 0
 * between accept steps.  Refused before the session has run the pair once. */
int ttx_debug_accept_block(ttx_session* s, int32_t* words, int n_words, void* stream);

/* ---- The beam family of csrc/ttx_loop_kernels.hip.h, ONE launch each on DEVICE arrays of the caller (tests/test_gpu_beam_loop_kernels.py;
 * the rules are restated in tests/util_beam_checks.py).  Every struct below is the kernel's own argument block: pointers first,
 * then int32 scalars, named as the kernel names them.  Grid, block, dynamic LDS, the logits-per-lane dispatch and the raise of the
 * LDS limit are the production launch functions of csrc/ttx_api.hip.  Arrays are sized by max_cand (the grid) where the kernel
 * indexes them by candidate.  Each entry waits for its launch.  Refused (TTX_ERR_INVALID, nothing launched): a null required
 * pointer, a non-positive size, and whatever lies beyond the limits the generators enforce: n_best (K) <= 32, n_drafts (N) <= 64,
 * V <= 1024, K * (dl + 1) <= 1023 segments, dynamic LDS <= 150 KiB. */
typedef struct ttx_debug_bs_prep_args {
  const int64_t* d_cand_next; const int32_t* d_len_next; const uint8_t* d_fin_next; const float* d_logp_next;   /* [max_cand, ld], [max_cand] x 3 */
  const int32_t* d_drafts_all;          /* all drafts: [B, N, D0] */
  const int32_t* d_lib;                 /* smart: [B, n_lib, lib_ld] */
  int32_t* d_gen; int32_t* d_front; int32_t* d_len; uint8_t* d_active; uint8_t* d_finished; float* d_logp; int32_t* d_per_cand;
  int32_t* d_drafts32;                  /* [max_cand, N, dl] */
  int32_t ld, max_cand, n_cand, beam, dl, N, pad, smart, n_lib, lib_ld, D0;
} ttx_debug_bs_prep_args;
/* ttx_debug_bs_prep: k_bs_prep on max_cand workgroups.  Also refused: n_cand > max_cand, all drafts with dl > D0, smart with
 * dl + 1 > lib_ld or n_lib < 1. */
int ttx_debug_bs_prep(ttx_session* s, const ttx_debug_bs_prep_args* a, void* stream);

typedef struct ttx_debug_bs_list_args {
  const uint8_t* d_active; const int32_t* d_per_cand; const int32_t* d_len;     /* [n_cand] */
  int32_t* d_act_idx; int32_t* d_slot_of; int32_t* d_prev_len;                  /* [n_cand] */
  int32_t* d_summary;                                                           /* [5] */
  int32_t n_cand, N, dl;
} ttx_debug_bs_list_args;
/* ttx_debug_bs_list: k_bs_list.  `words` is a HOST array of 21 int64: on entry [0..7] = the BeamCounters image (model_calls,
 * input_lines, running_rows, verified_positions, executed_positions, kv_prefix_positions, running_cands, max_group), put on the
 * device, ordered on `stream`; on return the same 8 words as the kernel left them and [8..20] = the DecState it wrote (the 13
 * words of ttx_debug_accept). */
int ttx_debug_bs_list(ttx_session* s, const ttx_debug_bs_list_args* a, int64_t* words, void* stream);

typedef struct ttx_debug_bs_hits_args {
  const float* d_logits;                /* [n_active * (1 + N*dl), V] */
  const uint8_t* d_finished; const int32_t* d_slot_of; const int32_t* d_per_cand; const int32_t* d_drafts32;
  uint8_t* d_hit;                       /* [max_cand, N * dl] */
  const int32_t* d_dl_of;               /* pool: [max_cand]; NULL: the per-batch path */
  int32_t V, max_cand, n_cand, N, dl, K;
  int32_t vpl;                          /* logits per lane: 0 the production choice by V, or 4 / 8 / 16 (refused unless 64 * vpl >= V) */
} ttx_debug_bs_hits_args;
/* ttx_debug_bs_hits: k_bs_hits with the generators' nucleus 0.9975. */
int ttx_debug_bs_hits(ttx_session* s, const ttx_debug_bs_hits_args* a, void* stream);

typedef struct ttx_debug_bs_leaves_args {
  const float* d_logits; const uint8_t* d_finished; const int32_t* d_slot_of; const int32_t* d_per_cand; const int32_t* d_drafts32;
  const float* d_logp; const uint8_t* d_hit;
  int32_t* d_best_n; int32_t* d_best_slot; int64_t* d_chosen;                   /* [max_cand], [max_cand], [max_cand, dl] */
  float* d_leaf_score; int32_t* d_leaf_tok; int32_t* d_leaf_cnt;                /* [max_cand, dl+1, K] x 2, [max_cand, dl+1] */
  const uint8_t* d_live; const int32_t* d_dl_of; const int32_t* d_grp_of; const int32_t* d_cand_batch;   /* pool; all NULL: per batch */
  int32_t V, max_cand, n_cand, N, dl, K, bos, pad, smart;
  int32_t max_group;                    /* per-batch smart mode: BeamCounters.max_group as k_bs_list left it */
  int32_t vpl;
} ttx_debug_bs_leaves_args;
/* ttx_debug_bs_leaves: k_bs_leaves.  Also refused: grp_of without cand_batch or the reverse. */
int ttx_debug_bs_leaves(ttx_session* s, const ttx_debug_bs_leaves_args* a, void* stream);

typedef struct ttx_debug_beam_select_args {
  const float* d_leaf_score; const int32_t* d_leaf_tok; const int32_t* d_leaf_cnt;
  const int32_t* d_cand; const int32_t* d_len; const int64_t* d_chosen; const int32_t* d_chosen_slot; const uint8_t* d_finished;
  int64_t* d_new_cand; float* d_new_logp; int32_t* d_parent; int32_t* d_parent_draft; int32_t* d_mark;   /* [B*K, ld_out], [B*K] .. */
  int32_t* d_summary;                   /* [5], read and written */
  int32_t* d_new_len; uint8_t* d_new_finished;                                  /* [B*K], both or neither */
  int32_t width, ld_in, ld_out, B, beam, dl, K, pad, eos;
} ttx_debug_beam_select_args;
/* ttx_debug_beam_select: k_beam_select<int> on B workgroups.  Also refused: width above ld_in or ld_out. */
int ttx_debug_beam_select(ttx_session* s, const ttx_debug_beam_select_args* a, void* stream);

typedef struct ttx_debug_beam_step_args {
  const float* d_logits; const int32_t* d_slot_of; const uint8_t* d_finished; const float* d_score; const int32_t* d_gen;
  int64_t* d_new_cand; float* d_new_score; int32_t* d_parent; int32_t* d_new_len; uint8_t* d_new_finished; int32_t* d_parent_draft;
  int32_t* d_summary;                   /* [0] += new candidates holding EOS */
  int32_t V, ld, width, B, beam, K, pad, eos;
} ttx_debug_beam_step_args;
/* ttx_debug_beam_step: k_beam_step on B workgroups.  Also refused: K > beam * V, width >= ld. */
int ttx_debug_beam_step(ttx_session* s, const ttx_debug_beam_step_args* a, void* stream);
/* ttx_debug_beam_step_masked: ONE launch of k_beam_step_masked on the same operands (tests/test_gpu_beam_mask_kernel.py).  pfx NULL
 * or the table by source (d_len, d_src int32 [B]): source b is forced at column a->width when a->width <= d_len[b].  Refused: what
 * ttx_debug_beam_step refuses, a table outside its bounds, a width inside a prefix but beyond pfx->ld. */
int ttx_debug_beam_step_masked(ttx_session* s, const ttx_debug_beam_step_args* a, const ttx_debug_prefix* pfx, void* stream);
/* The number of k_beam_step_masked launches the session's beam loop has enqueued since it was created (ttx_debug_beam_step_masked
 * is not counted).  A session that only ever served unconstrained calls reports 0. */
int ttx_debug_beam_step_masked_launches(ttx_session* s);

typedef struct ttx_debug_sbs_step_args {
  const float* d_logits; const int32_t* d_slot_of; const uint8_t* d_finished; const float* d_phi; const float* d_g; const int32_t* d_gen;
  const int64_t* d_key;                 /* [B] or NULL: keys 0 .. B-1 */
  int64_t* d_new_cand; float* d_new_phi; float* d_new_g; int32_t* d_parent; int32_t* d_new_len; uint8_t* d_new_finished;
  int32_t* d_parent_draft;
  int32_t* d_summary;                   /* [0] += new candidates that are finished */
  int32_t* d_tr_parent; int32_t* d_tr_token; float* d_tr_phi; float* d_tr_g;    /* [B, K] trace records, all four or none */
  uint64_t seed;
  int32_t V, ld, width, B, beam, K, pad, eos, pos;
  float inv_T;
} ttx_debug_sbs_step_args;
/* ttx_debug_sbs_step: k_sbs_step on B workgroups, operands as for ttx_debug_beam_step with phi, G, the keys, the position, the
 * seed and inv_T added.  Also refused: beam or K above 32, K > beam * V, width >= ld, pos < 1, inv_T not finite or not > 0. */
int ttx_debug_sbs_step(ttx_session* s, const ttx_debug_sbs_step_args* a, void* stream);
/* ttx_debug_sbs_step_ex: ONE launch of k_sbs_step_masked on the same operands (whatever top_k / top_p / pfx say: the production
 * loop launches it only under a filter or a prefix).  top_k, top_p as ttx_sbs_filter (top_p < 1 with top_k = 0 runs with 32);
 * pfx NULL or the table by source (d_len, d_src int32 [B]): source b is forced at a->pos when a->pos <= d_len[b].  waves: 0 the
 * production choice (4 up to beam 4, 8 up to beam 8, else 16), or 4, 8, 16: the outputs do not depend on it.  Also refused: top_k
 * outside [0, 32], top_p outside (0, 1], another wave count, a table outside its bounds, pos inside a prefix but beyond pfx->ld. */
int ttx_debug_sbs_step_ex(ttx_session* s, const ttx_debug_sbs_step_args* a, int top_k, float top_p, const ttx_debug_prefix* pfx,
                          int waves, void* stream);

typedef struct ttx_debug_tree_cache_args {
  const int32_t* d_len; const int32_t* d_parent; const int32_t* d_parent_draft; const int32_t* d_prev_len; const uint8_t* d_active;
  const float* d_k_old; const float* d_v_old; float* d_k_new; float* d_v_new;
  const float* d_qkv_prev; const int32_t* d_prev_slot_of;
  const int32_t* d_slot_parent; const int32_t* d_slot_self;                     /* both NULL: two buffers, cache row = candidate */
  int64_t cache_layer_stride, cache_seq_stride, qkv_layer_stride;               /* floats */
  int32_t max_cand, layers, prev_N, prev_D, d;
} ttx_debug_tree_cache_args;
/* ttx_debug_tree_cache: k_tree_cache on (max_cand, layers) workgroups.  Also refused: d not a multiple of 4, strides that are not
 * multiples of 4 floats, buffers that are not 16-byte aligned, one slot map without the other, slot maps with k_old != k_new. */
int ttx_debug_tree_cache(ttx_session* s, const ttx_debug_tree_cache_args* a, void* stream);

/* ---- The kernels of the stochastic beam pool (csrc/ttx_sbs_pool.hip.h), ONE launch per call on DEVICE arrays of the caller
 * (tests/test_gpu_sbs_pool_kernel.py; the rules are restated in tests/util_sbs_pool_checks.py).
 * ttx_debug_sbs_step_pool: k_sbs_step_pool (masked == 0) or k_sbs_step_pool_masked on C workgroups.  Candidate arrays are [C*K]
 * (candidate c = slot * K + k; d_gen int32 [C*K, ld], d_new_cand int64 [C*K, ld]), slot arrays int32 [C] (d_key int64 [C]):
 * d_row_of (-1: a free slot, whose workgroup writes nothing), d_level (pos = width), d_nlive (parents: 1 or K), d_nfin (output:
 * finished ones among the slot's K new candidates).  top_k, top_p, pfx as for ttx_debug_sbs_step_ex with the table by SLOT.
 * Refused: a null array, C outside [1, 1024], K outside [1, min(32, V)], V above 1024, K * V * 4 above 150 KB, a live slot's
 * level outside [1, ld) or parent count outside [1, K], a filter or table with masked == 0, top_k / top_p outside their ranges. */
typedef struct ttx_debug_sbs_step_pool_args {
  const float* d_logits; const int32_t* d_slot_of; const uint8_t* d_finished; const float* d_phi; const float* d_g; const int32_t* d_gen;
  const int32_t* d_row_of; const int32_t* d_level; const int32_t* d_nlive; const int64_t* d_key;
  int64_t* d_new_cand; float* d_new_phi; float* d_new_g; int32_t* d_parent; int32_t* d_new_len; uint8_t* d_new_finished;
  int32_t* d_parent_draft; int32_t* d_nfin;
  uint64_t seed;
  int32_t V, ld, C, K, pad, eos;
  float inv_T;
} ttx_debug_sbs_step_pool_args;
int ttx_debug_sbs_step_pool(ttx_session* s, const ttx_debug_sbs_step_pool_args* a, int masked, int top_k, float top_p,
                            const ttx_debug_prefix* pfx, void* stream);
/* ttx_debug_sbs_pool: the bookkeeping kernels.  op: 0 init (also needs d_src_of int32 [C*K]; zeroes d_g_in and d_g_out), 1 admit
 * (d_new_slot int32 [C]), 2 fill (d_new_slot, staged d_valid_new uint8 [R, Ls_new] and d_memkv_new fp32 [R, Ls_new, kv_row]; the
 * pool's d_src_valid uint8 [C, Ls_cap] and d_memkv fp32 [C, Ls_cap, kv_row]), 3 retire, 4 publish.  d_g_in: G as the next step
 * reads it (fill writes it); d_g_out: G as the last step wrote it (retire reads it).  d_len_all int32 [S], d_row_keys int64 [S] or
 * NULL, d_pfx_len_src int32 [S] or NULL; d_out int64 [S, K, max_len], d_out_logp / d_out_gumbel fp32 [S, K]; d_run_acc int32 [C]
 * and d_src_running int32 [S] or NULL (the per-source count of decoded candidates, written at retirement); d_dev_summary int32
 * [4].  `words`: as for ttx_debug_bsp.  Refused: a null required pointer, C outside [1, 1024], K outside [1, 32], max_len < 2,
 * ld < max_len, R outside [1, C], Ls_new outside [1, Ls_cap], kv_row not a positive multiple of 4, unaligned memkv operands. */
typedef struct ttx_debug_sbs_pool_args {
  int32_t* d_row_of; int32_t* d_level; int32_t* d_nlive; int32_t* d_nfin; int64_t* d_key; int32_t* d_pfx_len; int32_t* d_pfx_src;
  int32_t* d_run_acc;
  int64_t* d_cand_next; int32_t* d_len_next; uint8_t* d_fin_next; float* d_phi_next; int32_t* d_parent; int32_t* d_parent_draft;
  int32_t* d_cand_src_len; float* d_g_in; float* d_g_out;
  const int32_t* d_len_all; const int64_t* d_row_keys; const int32_t* d_pfx_len_src;
  int64_t* d_out; float* d_out_logp; float* d_out_gumbel; int32_t* d_src_running; int32_t* d_dev_summary;
  int32_t* d_src_of; int32_t* d_new_slot; const uint8_t* d_valid_new; uint8_t* d_src_valid; float* d_memkv; const float* d_memkv_new;
  int32_t C, K, max_len, ld, Ls_cap, pad, bos;
  int32_t R, first_row, kv_row, Ls_new;
} ttx_debug_sbs_pool_args;
int ttx_debug_sbs_pool(ttx_session* s, int op, const ttx_debug_sbs_pool_args* a, int64_t* words, void* stream);

/* ---- The bookkeeping kernels of the beam-speculative batch pool (csrc/ttx_loop_kernels.hip.h: k_bsp_init .. k_bsp_publish), ONE
 * launch per call on DEVICE arrays of the caller (tests/test_gpu_bsp_kernels.py; the rules are restated in tests/util_bsp_checks.py).
 * The struct is the kernels' argument block: every array of BeamPoolArgs, the caller-side arrays of BeamPoolIo (d_out int64
 * [rows, K, max_len], d_trace_len int16 [rows, T_cap], d_summary int32 [rows, 8], d_len_all / d_batch_all int32 [rows],
 * d_given_all int32 [batches]), the extra operands of k_bsp_init / k_bsp_admit (d_src_of, d_cand_src_len int32 [C*K]; d_new_slot
 * int32 [C]) and of k_bsp_fill (staged d_tok_new int32 [R, Ls_new], d_valid_new uint8 [R, Ls_new], d_drafts_new int32 [R, N*D0] or
 * NULL as in smart mode, d_memkv_new fp32 [R, Ls_new, kv_row]; the pool's d_src_valid uint8 [C, Ls_cap], d_memkv fp32 [C, Ls_cap,
 * kv_row]), then the int32 scalars, named as the kernels name them.  Source- and batch-slot arrays are int32 [C] (d_src_acc [C, 8]),
 * candidate arrays [C*K] (d_cand_next int64 [C*K, ld], d_gen int32 [C*K, ld], d_drafts32 int32 [C*K, N, D0], d_chosen int64 [C*K, D0],
 * d_leaf_score / d_leaf_tok [C*K, D0+1, K], d_leaf_cnt [C*K, D0+1]), d_tok int32 [C, Ls_cap], d_drafts_all int32 [C, N, D0],
 * d_dev_summary int32 [4].  The entry builds the BeamPoolIo block and uses the session's pinned BeamPoolHost.
 * op: 0 init, 1 admit, 2 fill, 3 prep, 4 select, 5 batches, 6 retire, 7 publish; grid, block, dynamic LDS and the raise of
 * k_bsp_select's LDS limit are the pool's own launch functions (csrc/ttx_api.hip: launch_bsp_*).  Each call waits for its launch.
 * `words` is a HOST array of 12 int64: on entry [0..7] = the BeamCounters image (as for ttx_debug_bs_list) and [8..11] = the
 * BeamPoolHost image (steps_done, n_live, n_running, error), both put where the kernel reads them, ordered on `stream`; on return
 * the same 12 words as the kernel left them.
 * Refused (TTX_ERR_INVALID, nothing launched): a null required pointer (every array of BeamPoolArgs and BeamPoolIo for every op,
 * d_drafts_all in all-drafts mode only; d_src_of and d_cand_src_len for init; d_new_slot and d_cand_src_len for admit; d_new_slot
 * and the fill operands but d_drafts_new for fill), a non-positive size (D0, max_steps and first_row may be 0), an unknown op,
 * C > 1024, K > 32, N > 64, K * (D0 + 1) > 1023 segments, k_bsp_select's LDS image 2 * K * (D0 + 1) * K * 4 above 150 KiB,
 * ld < max_len + D0 + 2, and for admit / fill R > C; for fill Ls_new > Ls_cap, kv_row not a multiple of 4, d_memkv or d_memkv_new
 * not 16-byte aligned. */
typedef struct ttx_debug_bsp_args {
  int32_t* d_row_of; int32_t* d_slot_batch; int32_t* d_src_acc; int32_t* d_src_state; int32_t* d_tok; int32_t* d_drafts_all;
  int32_t* d_bat_id; int32_t* d_bat_iter; int32_t* d_bat_dl; int32_t* d_bat_grp; int32_t* d_bat_live; int32_t* d_bat_nfin;
  int32_t* d_bat_longest_fin; int32_t* d_bat_longest_cur; int32_t* d_bat_state; int32_t* d_bat_given;
  int64_t* d_cand_next; int32_t* d_len_next; uint8_t* d_fin_next; float* d_logp_next; int32_t* d_parent; int32_t* d_parent_draft;
  int32_t* d_gen; int32_t* d_front; int32_t* d_len; uint8_t* d_active; uint8_t* d_finished; uint8_t* d_live; float* d_logp;
  int32_t* d_per_cand; int32_t* d_drafts32; int32_t* d_cand_dl; int32_t* d_cand_batch; int32_t* d_cache_slot; int32_t* d_cache_slot_parent;
  const int32_t* d_chosen_slot; const int64_t* d_chosen; const float* d_leaf_score; const int32_t* d_leaf_tok; const int32_t* d_leaf_cnt;
  int32_t* d_dev_summary;
  int64_t* d_out; int16_t* d_trace_len; int32_t* d_summary; const int32_t* d_len_all; const int32_t* d_batch_all; const int32_t* d_given_all;
  int32_t* d_src_of; int32_t* d_cand_src_len; int32_t* d_new_slot;
  const int32_t* d_tok_new; const uint8_t* d_valid_new; uint8_t* d_src_valid; const int32_t* d_drafts_new; float* d_memkv;
  const float* d_memkv_new;
  int32_t C, K, N, D0, Ls_cap, max_len, ld, smart, lib_ld, pad, bos, eos, repl, max_steps;
  int32_t T_cap, R, first_row, kv_row, Ls_new;
} ttx_debug_bsp_args;
int ttx_debug_bsp(ttx_session* s, int op, const ttx_debug_bsp_args* a, int64_t* words, void* stream);

/* ttx_debug_kvcopy: ONE launch of k_kvcopy on a grid of (B, Ld) workgroups: for slot < n_copy with record (b, best, n_acc,
 * front_old, .) of d_rec int32 [B, 5] and j = 0 .. n_acc, the K and V thirds of step row (j == 0 ? 0 : 1 + best*D + (j-1)) of the
 * slot, in d_qkv [Ld][B * (1 + N*D)][3d] with qkv_layer_stride floats between layers, are copied bit for bit to position
 * front_old + j of cache row b (d_kcache / d_vcache + l * cache_layer_stride + b * cache_seq_stride, positions d wide).  Nothing
 * else is written.  n_copy is put into a DecState on the device, ordered on `stream`.  Refused: null pointers, d not in {64, 128,
 * 256, 512, 1024}, n_copy outside [0, B], operands that are not 16-byte aligned, strides that are not multiples of 4 or do not
 * cover their rows, a record with b, best or n_acc out of range or front_old + n_acc + 1 positions beyond the cache row. */
int ttx_debug_kvcopy(ttx_session* s, const int32_t* d_rec, int n_copy, const float* d_qkv, int64_t qkv_layer_stride, float* d_kcache,
                     float* d_vcache, int64_t cache_layer_stride, int64_t cache_seq_stride, int N, int D, int d, int B, int Ld,
                     void* stream);

/* ttx_debug_kvcopy_split: ttx_debug_kvcopy with the indirection of the two-phase verify step (DESIGN.md "Two-phase verify step").
 * d_pos2 int32 [n_copy]: a slot with pos2 >= 0 takes its step rows from position pos2 of d_qkv instead of its own; a slot with
 * pos2 == -1 takes the K and V thirds of its single row of d_qkv_probe [Ld][B][3d] (probe_layer_stride floats between layers) and
 * commits that row alone, at front_old.  With d_pos2 and d_qkv_probe both NULL it is ttx_debug_kvcopy.  Also refused: one of the
 * two without the other, a probe buffer that is not 16-byte aligned or whose stride does not cover B rows, pos2 outside [-1, B),
 * a record with n_acc != 0 at pos2 == -1. */
int ttx_debug_kvcopy_split(ttx_session* s, const int32_t* d_rec, int n_copy, const float* d_qkv, int64_t qkv_layer_stride,
                           float* d_kcache, float* d_vcache, int64_t cache_layer_stride, int64_t cache_seq_stride, int N, int D, int d,
                           int B, int Ld, const int32_t* d_pos2, const float* d_qkv_probe, int64_t probe_layer_stride, void* stream);

/* ttx_debug_probe_split: ONE launch of k_probe_split (one workgroup: 256 threads for B <= 256, 1024 above).  Slot g < n_active is
 * sequence b = d_act_idx[g]; it matches when d_pred_probe[g] equals d_drafts[b, n, 0] for some n (drafts int32 [B, N, D]).  The
 * matching sequences are written to d_act2 in the order of d_act_idx (entries past the match count are not written) and
 * d_pos2[g] = the slot's position in d_act2, or -1.  `result` is a HOST array of 7 int32: on entry [4] = probes counted so far;
 * on return [0..2] = n_active, r_rows, m_rows of the draft pass's DecState (matches, matches * N, matches * (1 + N*D)), [3] = the
 * executed rows n_active + matches * (1 + N*D), [4] = the probe count, [5..6] = the words published for the host (matches,
 * probes_done).  Refused: null pointers, B, N or D < 1, n_active outside [0, B], act_idx that are not distinct rows of [0, B). */
int ttx_debug_probe_split(ttx_session* s, const int32_t* d_act_idx, const int32_t* d_pred_probe, const int32_t* d_drafts, int B, int N,
                          int D, int n_active, int32_t* d_act2, int32_t* d_pos2, int32_t* result, void* stream);

/* ttx_debug_merge_pred: ONE launch of k_merge_pred: d_pred [n_active * (1 + N*D)] in k_accept's layout; a slot with pos2 >= 0
 * takes the 1 + N*D predictions at position pos2 of d_pred2, any other slot d_pred_probe[g] in row 0 and -1 in its draft rows.
 * Rows past n_active * (1 + N*D) are not written.  Refused: null pointers, B, N or D < 1, n_active outside [0, B], pos2 outside
 * [-1, B). */
int ttx_debug_merge_pred(ttx_session* s, const int32_t* d_pos2, const int32_t* d_pred_probe, const int32_t* d_pred2, int32_t* d_pred,
                         int B, int N, int D, int n_active, void* stream);

/* Draft select (DESIGN.md "Two-phase verify step"): the draft pass of a split pool step runs, for every matching slot, row 0 and the D
 * rows of each draft whose first token is the probe's prediction, stored compacted.  Per position p of the draft pass:
 * draft_mask[p] (bit n: draft n is present, never 0) and row_base[p], the exclusive prefix sum of 1 + D * popcount(mask): the
 * slot's row 0 lies at row_base[p], row 1 + n*D + (j-1) of a present draft at row_base[p] + 1 + rank(n)*D + (j-1) with rank(n) =
 * popcount(mask & ((1 << n) - 1)).  The test entry points below (tests/test_gpu_draft_select.py) are those above with these
 * operands; each reads them back and refuses (TTX_ERR_INVALID, nothing launched) a mask that is 0 or has bits at or beyond N, a
 * row_base that is not that prefix sum, N > 32 or D < 1, one of the operands without the others, besides what its counterpart
 * refuses.  With the draft-select operands all NULL each is its counterpart.
 *
 * ttx_debug_probe_split_select: ttx_debug_probe_split that also writes d_draft_mask, d_row_base [matches] and d_row_map [compacted
 * rows]: compacted row -> layout row p * (1 + N*D) + rs.  result has 8 words: [2] = m_rows is the compacted total and [7] the row
 * count published for the host; [3] stays n_active + matches * (1 + N*D).  Entries past the counts are not written. */
int ttx_debug_probe_split_select(ttx_session* s, const int32_t* d_act_idx, const int32_t* d_pred_probe, const int32_t* d_drafts, int B,
                                 int N, int D, int n_active, int32_t* d_act2, int32_t* d_pos2, int32_t* d_draft_mask, int32_t* d_row_base,
                                 int32_t* d_row_map, int32_t* result, void* stream);
/* ttx_debug_merge_pred_select: d_pred2 is compacted; an absent draft's rows of a matching slot read -1. */
int ttx_debug_merge_pred_select(ttx_session* s, const int32_t* d_pos2, const int32_t* d_pred_probe, const int32_t* d_pred2,
                                int32_t* d_pred, int B, int N, int D, int n_active, const int32_t* d_row_base,
                                const int32_t* d_draft_mask, void* stream);
/* ttx_debug_kvcopy_select: ttx_debug_kvcopy_split on a compacted d_qkv (its layer stride still covers B * (1 + N*D) rows).  Also
 * refused: a record with n_acc > 0 whose best draft is absent from its slot's mask. */
int ttx_debug_kvcopy_select(ttx_session* s, const int32_t* d_rec, int n_copy, const float* d_qkv, int64_t qkv_layer_stride,
                            float* d_kcache, float* d_vcache, int64_t cache_layer_stride, int64_t cache_seq_stride, int N, int D, int d,
                            int B, int Ld, const int32_t* d_pos2, const float* d_qkv_probe, int64_t probe_layer_stride,
                            const int32_t* d_row_base, const int32_t* d_draft_mask, void* stream);
/* ttx_debug_embed_select: the step mode of ttx_debug_embed writing m_rows rows, row i holding the token and position of layout row
 * d_row_map[i].  Refused: m_rows outside [0, n_active * (1 + N*D)], a map entry outside the live slots' layout rows. */
int ttx_debug_embed_select(ttx_session* s, const float* d_table, int V, const float* d_pe, int pe_rows, int d, float* d_x,
                           const int32_t* d_act_idx, const int32_t* d_front, const int32_t* d_gen, int gen_ld, const int32_t* d_drafts,
                           int B, int N, int D, int n_active, const int32_t* d_row_map, int m_rows, void* stream);
/* ttx_debug_attn_select: a step-mode launch (mode 3 or 4) of ttx_debug_attn at head dimension 32 on compacted q / k / v / out rows;
 * kernel is 0, 3 (k_attn3) or 4 (k_attn3s).  Stored rows equal, bit for bit, the same rows of the full-layout launch. */
int ttx_debug_attn_select(ttx_session* s, const float* d_q, int ldq, const float* d_k, const float* d_v, int ldkv, float* d_out, int H,
                          float scale, int Lk, const int32_t* d_tok, int pad, const uint8_t* d_key_pad, const int32_t* d_act_idx,
                          const int32_t* d_front, const int32_t* d_src_of, const int32_t* d_src_len, const float* d_kcache,
                          const float* d_vcache, int64_t cache_seq_stride, const int32_t* d_cache_slot, int gen_ld, int N, int D, int mode,
                          int groups, int n_active, int max_keys, int kernel, int32_t* kernel_id, const int32_t* d_row_base,
                          const int32_t* d_draft_mask, void* stream);

/* Counters of the last ttx_greedy_speculative_generate_pool call whose FIRST session was `s`, summed over its pools, into a HOST
 * array of 7 int64: [0] steps, [1] split steps, [2] slot-steps probed, [3] slots matched, [4] drafts run by the draft passes (under
 * draft select the matching ones, else N per matching slot), [5] rows sent through the decoder by all steps (probes and one-pass
 * steps included), [6] 1 when the call ran under draft select, 0 when its draft passes ran every draft (TTX_DRAFT_SELECT=0, or a
 * model whose step attention runs on k_attn2 / k_attn).  ttx_gen_stats.verified_positions keeps counting the positions of matching
 * slots whether their rows ran or not. */
int ttx_pool_last_counters(ttx_session* s, int64_t* counters);

/* Host query, no device needed: the number of keys one k_attn2 workgroup can stage at head dimension head_dim when a group has
 * q_per_group query rows (up to 32 rows share one query image, more take the 64-row one): 384 at head dimension 32, 320 at 64;
 * 0 for a head dimension without kernels.  A launch whose key count (step self-attention: cache capacity + 1 + the draft rows
 * of a 64-row tile) exceeds it runs on k_attn. */
int ttx_attn_staged_key_limit(int head_dim, int q_per_group);

/* Test query: which attention kernels this session has dispatched since it was created, as a bit mask (bit k: kernel id k of
 * ttx_debug_attn, 1 k_attn .. 5 k_attn1), counted where a launch is issued (under graphs: when a step is captured).  A negative
 * error code for a null session. */
int ttx_debug_attn_kernels_seen(ttx_session* s);

/* Test entry: ONE launch of k_attn_probs (csrc/ttx_attn_probs.hip.h) on operands of the test.  d_q fp32 [R*T, ldq] and d_k fp32
 * [Rm*Ls, ldkv] with head h at columns h*head_dim .. (H * head_dim need not be a model width; head_dim 32 or 64); d_key_pad u8
 * [Rm*Ls], non-zero = PAD; d_mem_row int32 [R] (NULL: row r reads memory row r, Rm == R; a value outside [0, Rm) reads as a
 * memory row of PAD keys); d_length int32 [R]: position t of row r is live iff t < length[r].  Outputs as ttx_attention_maps has
 * them, each optional, at least one required: d_heads [R,H,T,Ls], d_mean [R,T,Ls], d_align [R,T].  Rows go out as 16-byte stores
 * when Ls % 4 == 0 and the bases are 16-byte aligned, else 4 bytes at a time, with the same bits.  Keys appended as PAD change no
 * bit of the other columns.  TTX_ERR_INVALID with nothing launched for Ls above ttx_attn_probs_key_limit(head_dim). */
int ttx_debug_attn_probs(ttx_session* s, const float* d_q, int ldq, const float* d_k, int ldkv, const uint8_t* d_key_pad,
                         const int32_t* d_mem_row, const int32_t* d_length, int R, int Rm, int H, int head_dim, int T, int Ls,
                         float scale, float* d_heads, float* d_mean, int32_t* d_align, void* stream);

/* Length-bucketed scoring of a LIST of (src, hyp) batches (csrc/ttx_score_list.hip.h): what ttx_score_hypotheses gives for every
 * batch of the list, bit for bit while sources and hypothesis windows stay within the staged key range of the attention kernels
 * (ttx_attn_staged_key_limit), computed in chunks of sources of similar length.  Batch i is described by one ttx_score_batch (HOST
 * array h_batches): d_src int64 [B,Ls], d_hyp int64 [B*N] rows of stride ld_hyp >= W (W >= 2 columns read), as ttx_score_hypotheses
 * takes them; B, Ls, N, W and ld_hyp may differ from batch to batch.  The S sources and the R hypothesis rows of the list are
 * numbered in list order (batch 0's first).  Each call uploads the table with one stream-ordered copy; the kernels read the batches
 * through it.  Neither call synchronises: the caller reads d_e / d_ls back between the two, and that is the only read-back.
 *
 * ttx_score_list_extents: d_e int32 [S], e[s] = max(2, 1 + max n over the N rows of source s) with n as under
 *   ttx_hypothesis_logprobs; d_ls int32 [S], ls[s] = max(1, 1 + the last non-PAD column of source s).  Optional: d_n int32 [R], n of
 *   every row; d_bad int32 [1], bit 0 set when a source token id lies outside [0, src_vocab_size), bit 1 when a hypothesis id lies
 *   outside [0, vocab_size), over the whole given widths.
 * ttx_score_list_run: h_order int32 [S] names every source exactly once; chunk c (ttx_score_chunk, HOST array, run in the order
 *   given) scores the sources h_order[first .. first + count), all of batches with N rows per source, in ONE teacher-forced pass over
 *   their first W hypothesis columns and first Ls source columns (shorter rows are PAD-filled): W >= e[s] and Ls >= ls[s] for every
 *   member keep every scored token and every non-PAD source token.  Outputs in list order: d_score fp32 [R], d_length int32 [R],
 *   d_finished u8 [R] or NULL, d_tok_logp fp32 or NULL: batch i at h_tok_off[i] (int64 HOST array, in floats) as [B*N, W_i - 1], a
 *   row's first min(W, W_i) - 1 values and exact zeros after them.
 * TTX_ERR_INVALID with nothing launched: a null required pointer, an empty list, ld_hyp < W, W < 2, B, N or Ls < 1 in a batch; an
 *   order or chunk table that names a source twice or leaves one out; a chunk with mixed N, W < 2, Ls < 1, 2^24 or more positions
 *   (count * N * (W - 1)) or a width beyond the positional table; a vocabulary above 1024.
 * ttx_debug_score_list (test entry): ONE launch of k_sl_extents (op 0), k_sl_pack (op 1) or k_sl_unpack (op 2) on the test's
 *   operands: h_sel int32 [n_sel] are the chunk's sources (ops 1, 2); the chunk's N, W and Ls, and the arrays, come in `a`. */
typedef struct ttx_score_batch {
  const int64_t* d_src;
  const int64_t* d_hyp;
  int32_t B, Ls, N, W, ld_hyp;
} ttx_score_batch;
typedef struct ttx_score_chunk {
  int32_t first, count;     /* the chunk's sources: h_order[first .. first + count) */
  int32_t N, W, Ls;         /* rows per source; hypothesis and source columns of the pass */
} ttx_score_chunk;
typedef struct ttx_debug_score_list_args {
  int32_t* d_e; int32_t* d_ls; int32_t* d_n; int32_t* d_bad;                                          /* op 0 */
  int64_t* d_src_c; int64_t* d_hyp_c;                                                                 /* op 1: [n_sel,Ls], [n_sel*N,W] */
  const float* d_score_c; const int32_t* d_length_c; const uint8_t* d_fin_c; const float* d_tok_c;    /* op 2, in: [n_sel*N], tok [.,W-1] */
  float* d_score; int32_t* d_length; uint8_t* d_finished; float* d_tok_logp;                          /* op 2, out: list order */
  int32_t N, W, Ls, eos;
} ttx_debug_score_list_args;
int ttx_score_list_extents(ttx_session* s, const ttx_score_batch* h_batches, int n_batches, int eos, int32_t* d_e, int32_t* d_ls,
                           int32_t* d_n, int32_t* d_bad, void* stream);
int ttx_score_list_run(ttx_session* s, const ttx_score_batch* h_batches, int n_batches, const int32_t* h_order, int n_order,
                       const ttx_score_chunk* h_chunks, int n_chunks, int eos, float* d_score, int32_t* d_length,
                       uint8_t* d_finished, float* d_tok_logp, const int64_t* h_tok_off, void* stream);
int ttx_debug_score_list(ttx_session* s, int op, const ttx_score_batch* h_batches, int n_batches, const int32_t* h_sel, int n_sel,
                         const int64_t* h_tok_off, const ttx_debug_score_list_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTX_H */
