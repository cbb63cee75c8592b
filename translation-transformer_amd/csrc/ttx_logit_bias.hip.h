// Per-source logit bias (included by ttx_api.hip only): k_logit_bias adds a source's bias row to every logits row of that source, in
// place, between the classifier and whatever consumes the logits (k_sample, k_sample_step, k_sbs_step*, k_hyp_logq).  Hand-written
// HIP for gfx950, wave64, k_sample's launch shape: ONE wave per logits row, 4 rows per workgroup, no LDS, no atomics, nothing
// crosses a wave or a row.
// The rule for a live row (include/ttx.h "Per-source logit bias" states it as the contract; tests/util_logit_bias.py restates it):
//   x'_v = x_v + bias[s, v], ONE rounded fp32 add, s the row's source;  an entry that is exactly zero (+0.0 or -0.0) skips the add,
//   so the logit keeps its bits (a -0.0 logit keeps its sign).  -inf forbids the token: every consumer defines a -inf logit as
//   "never emitted".  Rows at or beyond *m_ptr (and beyond M) are not written.
// The source of a row, the two mappings the samplers use:
//   plain   the logits row is the decoder row r:  s = tab.src ? tab.src[r] : r / rows_per_src  (the second form serves the
//           teacher-forced logits of the scoring pass, [sources * rows_per_src, V])
//   step    (k_sample_step's layout)  lrow = row_map ? row_map[row] : row,  b = act_idx[lrow / RPS],  s = tab.src[b]: the one pass,
//           the probe (N = 1, D = 0) and the compacted draft pass of the slot pool, and the running candidates of the beam loops
//           (N = 1, D = 0: row -> candidate act_idx[row] -> source tab.src[candidate], as the cross attention's src_of maps them).
// Access: a row whose logits and bias bases are both 16-byte aligned moves 16 bytes per lane and trip (V / 4 float4s, then a scalar
// tail of V % 4); any other row moves 4 bytes per lane and trip.  The choice is per row and wave-uniform and changes no bit.
#pragma once
#include "ttx_loop_kernels.hip.h"

namespace ttx {

// The bias of a call as the kernel sees it (val null: an unbiased call, no launch).  `src` goes by decoder row (slot of a pool).
struct LogitBiasTab {
  const float* val; int ld;        // [sources][ld], ld >= V
  const int* src;                  // [B] decoder row (slot) -> row of val
};

struct LogitBiasArgs {
  float* logits; int V;            // [M, V], read and written
  const int* m_ptr; int M;         // live rows on the device (null: M)
  LogitBiasTab tab;
  int rows_per_src;                // plain mapping with tab.src null: s = row / rows_per_src
  // step layout (STEP only)
  const int* act_idx;              // [n_active]
  const int* row_map;              // [rows] or null: row = layout row
  int N, D;
};

__device__ __forceinline__ float logit_bias_add(float x, float b) { return b != 0.0f ? __fadd_rn(x, b) : x; }

template <bool STEP>
__global__ __launch_bounds__(256) void k_logit_bias(const LogitBiasArgs a) {
  int rows = a.m_ptr ? *a.m_ptr : a.M;
  if (rows > a.M) rows = a.M;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                  // wave-uniform
  const int lane = threadIdx.x & 63;
  int s;
  if (STEP) {
    const int lrow = a.row_map ? a.row_map[row] : row;
    s = a.tab.src[a.act_idx[lrow / step_rps(a.N, a.D)]];
  } else {
    s = a.tab.src ? a.tab.src[row] : row / a.rows_per_src;
  }
  float* __restrict__ x = a.logits + (size_t)row * a.V;
  const float* __restrict__ b = a.tab.val + (size_t)s * a.tab.ld;
  int done = 0;                             // ids below it went 16 bytes at a time
  if ((((uintptr_t)x | (uintptr_t)b) & 15) == 0) {       // wave-uniform
    const int n4 = a.V >> 2;
    float4* __restrict__ x4 = reinterpret_cast<float4*>(x);
    const float4* __restrict__ b4 = reinterpret_cast<const float4*>(b);
    for (int i = lane; i < n4; i += 64) {
      float4 v = x4[i];
      const float4 c = b4[i];
      v.x = logit_bias_add(v.x, c.x); v.y = logit_bias_add(v.y, c.y); v.z = logit_bias_add(v.z, c.z); v.w = logit_bias_add(v.w, c.w);
      x4[i] = v;
    }
    done = n4 << 2;
  }
  for (int c = done + lane; c < a.V; c += 64) x[c] = logit_bias_add(x[c], b[c]);
}

}  // namespace ttx
