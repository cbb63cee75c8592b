// Syntax-constrained sampling (included by ttx_api.hip only): k_syntax_mask writes -inf over the tokens a row may not emit next if it
// is to end balanced (every OPEN closed, every ring label used an even number of times, EOS inside max_len), in place, between the
// classifier (and k_logit_bias) and whatever consumes the logits (k_sample, k_sample_step, k_hyp_logq).  Hand-written HIP for gfx950,
// wave64, k_logit_bias's launch shape: ONE wave per logits row, 4 rows per workgroup, no LDS, no atomics, nothing crosses a wave or a
// row.  The logits are never read: an allowed token keeps its bits whatever they are.
// The rule (include/ttx.h "Syntax-constrained sampling" states it as the contract; tests/util_syntax.py restates it).  A syntax table
// gives one int8 class per id: -1 FORBID, 1 OPEN, 2 CLOSE, 3 + l ring label l (0 <= l < 64), anything else neutral.  For a prefix P
//   depth = #OPEN - #CLOSE,  R = XOR of 1 << l over its ring tokens,  need = max(depth, 0) + popcount(R)
// (an id outside [0, V) and a FORBID token count as neutral), and for the position pos being predicted left = (max_len - 1) - pos:
//   EOS (the call's, whatever its class)   depth == 0 and R == 0
//   FORBID                                 never
//   neutral                                need + 1 <= left
//   OPEN, ring l with bit l clear in R     need + 2 <= left
//   CLOSE                                  depth > 0
//   ring l with bit l set in R             always
// The prefix and the position of a row, the three mappings:
//   plain    (k_sample's rows)  P = gen[row][1 .. front[0]], pos = front[0] + 1
//   step     (k_sample_step's layout)  lrow = row_map ? row_map[row] : row, b = act_idx[lrow / RPS], rs = lrow % RPS, f = front[b]:
//            rs == 0: P = gen[b][1 .. f], pos = f + 1;  rs = 1 + n * D + j: P = gen[b][1 .. f] then tokens 0 .. j of draft n of b (the
//            tokens k_embed<true> feeds the rows up to this one), pos = f + 2 + j
//   teacher  (hyp set; k_hyp_logq's positions)  logits [R, T, V], row = r * T + t: P = hyp[r][1 .. t], pos = t + 1
// State: lane l reads prefix tokens l, l + 64, ..; depth is a wave sum of +-1, R a wave XOR of a 64-bit word as two 32-bit shuffles per
// butterfly step.  Integers only, so any order gives the same state.
#pragma once
#include "ttx_loop_kernels.hip.h"

namespace ttx {

constexpr int SYN_FORBID = -1, SYN_OPEN = 1, SYN_CLOSE = 2, SYN_RING0 = 3, SYN_RINGS = 64;

struct SyntaxArgs {
  float* logits; int V;            // [M, V], written only
  const int* m_ptr; int M;         // live rows on the device (null: M)
  const signed char* cls;          // [V]
  int max_len, eos;
  // plain and step: the committed rows
  const int* gen; int gen_ld;      // [B, gen_ld], column 0 is BOS
  const int* front;                // plain: front[0]; step: [B]
  // step layout (STEP only)
  const int* act_idx;              // [n_active]
  const int* row_map;              // [rows] or null: row = layout row
  const int* drafts; int N, D;     // [B, N, D]
  // teacher-forced (plain with hyp set): rows of T positions
  const int64_t* hyp; int ld_hyp, T;
};

// One prefix token into a lane's share of the state.
__device__ __forceinline__ void syntax_count(const signed char* __restrict__ cls, int V, long long tok, int& depth, unsigned long long& ring) {
  if ((unsigned long long)tok >= (unsigned long long)V) return;
  const int c = cls[tok];
  if (c == SYN_OPEN) depth += 1;
  else if (c == SYN_CLOSE) depth -= 1;
  else if (c >= SYN_RING0 && c < SYN_RING0 + SYN_RINGS) ring ^= 1ull << (c - SYN_RING0);
}

template <bool STEP>
__global__ __launch_bounds__(256) void k_syntax_mask(const SyntaxArgs a) {
  int rows = a.m_ptr ? *a.m_ptr : a.M;
  if (rows > a.M) rows = a.M;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                  // wave-uniform
  const int lane = threadIdx.x & 63;
  int depth = 0, pos;
  unsigned long long ring = 0;
  if (STEP) {
    const int RPS = step_rps(a.N, a.D);
    const int lrow = a.row_map ? a.row_map[row] : row;
    const int rs = lrow % RPS;
    const int b = a.act_idx[lrow / RPS];
    const int f = a.front[b];
    const int* __restrict__ g = a.gen + (size_t)b * a.gen_ld;
    for (int i = 1 + lane; i <= f; i += 64) syntax_count(a.cls, a.V, g[i], depth, ring);
    pos = f + 1;
    if (rs != 0 && a.D > 0) {               // the probe (D == 0) has row 0 only
      const int n = (rs - 1) / a.D, j = (rs - 1) % a.D;
      const int* __restrict__ dr = a.drafts + ((size_t)b * a.N + n) * a.D;
      for (int i = lane; i <= j; i += 64) syntax_count(a.cls, a.V, dr[i], depth, ring);
      pos += 1 + j;
    }
  } else if (a.hyp) {                       // wave-uniform
    const int r = row / a.T, t = row - r * a.T;
    const int64_t* __restrict__ h = a.hyp + (size_t)r * a.ld_hyp;
    for (int i = 1 + lane; i <= t; i += 64) syntax_count(a.cls, a.V, h[i], depth, ring);
    pos = t + 1;
  } else {
    const int f = a.front[0];
    const int* __restrict__ g = a.gen + (size_t)row * a.gen_ld;
    for (int i = 1 + lane; i <= f; i += 64) syntax_count(a.cls, a.V, g[i], depth, ring);
    pos = f + 1;
  }
  unsigned lo = (unsigned)ring, hi = (unsigned)(ring >> 32);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    depth += __shfl_xor(depth, o, 64);
    lo ^= __shfl_xor(lo, o, 64);
    hi ^= __shfl_xor(hi, o, 64);
  }
  ring = ((unsigned long long)hi << 32) | lo;
  const int need = (depth > 0 ? depth : 0) + __popcll(ring);
  const int left = (a.max_len - 1) - pos;
  const bool room1 = need + 1 <= left, room2 = need + 2 <= left;
  float* __restrict__ x = a.logits + (size_t)row * a.V;
  for (int v = lane; v < a.V; v += 64) {
    const int c = a.cls[v];
    bool ok;
    if (v == a.eos) ok = depth == 0 && ring == 0;
    else if (c == SYN_FORBID) ok = false;
    else if (c == SYN_OPEN) ok = room2;
    else if (c == SYN_CLOSE) ok = depth > 0;
    else if (c >= SYN_RING0 && c < SYN_RING0 + SYN_RINGS) ok = ((ring >> (c - SYN_RING0)) & 1ull) ? true : room2;
    else ok = room1;
    if (!ok) x[v] = -INFINITY;
  }
}

}  // namespace ttx
