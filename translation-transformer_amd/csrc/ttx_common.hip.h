// Types shared by the translation units of libttx_hip.so (GEMM, attention, loop kernels + C ABI): device-resident loop
// state, kernel argument blocks, wave reductions.  Hand-written HIP for gfx950 (CDNA4, wave64), fp32 throughout: the
// reference runs with `precision: null` (configs/cfg_standard_product_prediction.yaml:7) and the parity bar is token
// identity, so every dense contraction uses the f32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32 fma chain).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ttx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------------
// Device-resident loop state of one generate call (one per session).
struct DecState {
  int n_active;        // Bc: rows still decoding
  int r_rows;          // Bc * N
  int m_rows;          // Bc * N * (D+1): rows of this step's GEMMs
  int stop;            // loop finished
  int width;           // the reference's generated_tokens.size(1)
  int steps;           // decoder calls so far (model_calls_num)
  int error;           // 1: a row finished at width > max_len (the reference raises there)
  int n_copy;          // rows whose accepted K/V must be copied into the cache after this step
  long long accepted, produced, verified_positions, kv_prefix_positions, src_positions;
};

struct CopyRec { int b, best, nacc, front_old, flags; };   // flags: 1 finished this step, 2 retired without finishing

// Host-mapped (pinned) words the accept kernels publish after every step; the host polls them instead of
// synchronising the stream.
struct HostInfo { int stop; int steps_done; int width; int n_active; };

// Two-phase verify step of the slot pool (DESIGN.md "Two-phase verify step"): k_probe_split publishes how many live slots matched
// a draft's first token and how many probes have run.  A word pair of its own: HostInfo stays what the accept kernels write.
// `rows` (draft select): the compacted row count of the draft pass, written before probes_done like `matches`.
struct ProbeInfo { int matches; int probes_done; int rows; };

// ------------------------------------------------------------------------------------------------
// GEMM:  Y[m, n] = sum_k X[m, k] * W[n, k]   (torch.nn.Linear layout: both operands K-contiguous)
struct GemmArgs {
  const float* X; int ldx;
  const float* W; int ldw;
  const float* bias;         // may be null
  float* Y; int ldy;
  const int* m_ptr;          // device-resident row count (null: use M)
  int M, N, K;
  int k_per_split;           // K range handled by one blockIdx.z
  int relu;                  // epilogue: 1 clamps at zero (TTX_ACT_RELU).  GELU is not a run-time flag but a template parameter of
                             // the kernels (gemm_act below): the ReLU / no-activation code objects stay what they were without it
  int raw;                   // 1: write un-biased partial sums to slab blockIdx.z
  long long slab_stride;     // floats between slabs
  int slice_k;               // canonical slice length (see ttx_gemm.hip): the result is the ordered sum over the K range's
                             // slices of `slice_k` k's, each accumulated from zero; 0 = one chain over the whole range
  int big_min_tiles;         // k_gemm24: smallest 128x64-tile count (x slabs) at which that tiling is used instead of 64x64 (0: never)
};


// ------------------------------------------------------------------------------------------------
// Exact GELU (torch's approximate="none"): gelu(x) = 0.5 x (1 + erf(x / sqrt 2)), evaluated in ONE pinned order,
//     t = x * fl(1 / sqrt 2);   e = erff(t);   h = 0.5 * x;   y = fma(h, e, h),
// every product and the fma spelled out, so that no instantiation of a GEMM kernel can contract the expression differently from
// another: equal pre-activation bits (canonical slice order, ttx_gemm.hip) give equal GELU bits in every kernel, tiling and live
// row count.  erff is the device library's, inlined as the same instruction sequence everywhere.  The closing fma rounds
// h (1 + e) once: in the negative tail, where e -> -1, nothing is lost beyond erff's own error (DESIGN.md "GELU").
__device__ __forceinline__ float gelu_erf(float x) {
  const float t = __fmul_rn(x, 0.70710678118654752440f);
  const float e = erff(t);
  const float h = __fmul_rn(0.5f, x);
  return __fmaf_rn(h, e, h);
}

// The activation of a GEMM epilogue.  GELU = false is the epilogue the kernels always had: a clamp at `lo` (0 for ReLU, -inf for
// none), untouched by the GELU instantiations beside it.
template <bool GELU>
__device__ __forceinline__ float gemm_act(float v, float lo) {
  if constexpr (GELU) return gelu_erf(v);
  else return fmaxf(v, lo);
}

// ------------------------------------------------------------------------------------------------
// Wave reductions (64 lanes).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}


// y = LN2?( LN( (resid + bias) + (slab[0] + slab[1] + ... in slab order) ) ) — one wave per row, VPL contiguous values per lane.
struct FinishArgs {
  const float* slabs; int n_slabs; long long slab_stride;
  const float* bias;
  const float* resid;          // [M, d]
  const float* g1; const float* b1;
  const float* g2; const float* b2;   // optional second LayerNorm (final stack norm), may be null
  const uint8_t* row_valid;    // optional: rows with 0 are written as zeros
  float* Y;
  const int* m_ptr; int M; int d; float eps;
};

// ------------------------------------------------------------------------------------------------
// Head dimensions: k_attn and k_attn2 are templates over DH in {32, 64}; k_attn3 / k_attn3s are written for ATT_DH only.
constexpr int ATT_DH = 32;
enum AttnMode { ATT_ENC = 0, ATT_FULL_SELF = 1, ATT_FULL_CROSS = 2, ATT_STEP_SELF = 3, ATT_STEP_CROSS = 4 };

// Step-mode row layout (one verify step): a running sequence ("slot") owns RPS = 1 + N*D consecutive rows:
//   row 0                      the token at the row's front (position f) — identical for all N drafts, computed once
//   row 1 + n*D + (j-1)        token j (1..D) of draft n, at position f + j
__host__ __device__ inline int step_rps(int N, int D) { return 1 + N * D; }

struct AttnArgs {
  const float* q; int ldq;         // query rows (packed QKV buffer or a plain [M,d] buffer)
  const float* k; const float* v; int ldkv;   // step/encoder keys (packed QKV buffer) or cross K/V
  float* out; int d;               // [M, d]
  float scale;
  int L;                           // ENC: Ls; FULL_*: Lt (queries per row)
  int Lk;                          // FULL_CROSS / STEP_CROSS: Ls
  const int* tok; int pad;         // ENC: src tokens [B,Ls]; FULL_SELF: tgt tokens [R,Lt]; STEP_SELF: gen [B, gen_ld]
  const uint8_t* key_pad;          // FULL_CROSS: [Rm, Ls] 1 = PAD key; STEP_CROSS/ENC: src_valid (1 = real token)
  const int* mem_row;              // FULL_CROSS: decoder row -> memory row (null: identity)
  // step modes
  const DecState* st; const int* act_idx; const int* front;
  const int* src_of;               // step modes: running row -> source row of the encoder memory (null: identity)
  const int* src_len;              // STEP_CROSS: keys of each row's source (null: Lk for every row) — slot pool
  const float* kcache; const float* vcache; long long cache_seq_stride;  // floats per sequence in the cache
  const int* cache_slot;           // STEP_SELF: running row -> its sequence's slot in the cache (null: the row index itself)
  int gen_ld; int N; int D;
  // draft select (the SEL instantiations of k_attn3 / k_attn3s; both null otherwise): slot -> first row of its compacted rows in
  // q / k / v / out, and slot -> bit n set when draft n's rows are stored (see step_sel_row)
  const int* row_base; const int* draft_mask;
};

// Draft select: a slot of the draft pass stores row 0 and the D rows of every draft in `mask`, the present drafts in the order of n.
// Layout row rs (see step_rps) -> row inside the slot's compacted rows, or -1 for a row of an absent draft.
__host__ __device__ inline int step_sel_rows(unsigned mask, int D) { return 1 + D * __builtin_popcount(mask); }
__device__ __forceinline__ int step_sel_row(unsigned mask, int n, int j0, int D) {     // rs = 1 + n * D + j0
  return ((mask >> n) & 1u) ? 1 + __popc(mask & ((1u << n) - 1u)) * D + j0 : -1;
}

}  // namespace ttx
