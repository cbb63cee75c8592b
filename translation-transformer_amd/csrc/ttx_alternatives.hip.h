// Per-position alternatives of hypotheses (included by ttx_api.hip only): what else the model considered where it emitted a
// token.  A side stage over the logits of the teacher-forced pass that ttx_score_hypotheses runs, after k_hyp_length.  Hand-written
// HIP for gfx950, wave64.  For a hypothesis row h[0..W-1], the logits x[p, 0..V-1] of decode_tgt(h[:W-1]) (p = 0..T-1, T = W - 1)
// and n = length[r], position p is live iff p < n; for a live position and t = h[p+1]:
//   top_id[p, j]    the ids of the k largest logits, largest first; equal logits: the lower id first (-0.0 == 0.0; -inf sorts last)
//   top_logp[p, j]  -(log1pf(rs) + (m - x[top_id[p, j]])) with (m, rs) of k_hyp_score's pass: met_push per lane, xor butterfly, lane 0
//                   (alt_push: a -inf logit met while the lane's maximum is still -inf leaves the lane empty, where met_push
//                   would form exp(-inf + inf); every other element takes met_push itself, so wherever k_hyp_score gives a
//                   number these are its bits, and a row with -inf entries gives numbers here)
//   chosen_logp[p]  that value for t: tok_logp[p] of k_hyp_score on the bits
//   rank[p]         the number of ids v with x[v] > x[t], or x[v] == x[t] and v < t
//   entropy[p]      -sum_v q_v log q_v, q = softmax(x[p]); a term is e * lp with lp = -(log1pf(rs) + (m - x[v])), e = expf(lp),
//                   and exactly 0 where e == 0; a lane adds its terms in ascending column order, the lanes' sums go through the
//                   xor butterfly (32, 16, .., 1)
// Positions that are not live: top_id = -1, top_logp = 0, chosen_logp = 0, rank = -1, entropy = 0.
//   k_alternatives   ONE wave per position, 4 positions per workgroup, the grid spread over all R*T positions.  The wave holds
//                    the whole row (V <= MET_MAX_V) in 16 registers per lane as order keys; k rounds of (lane-local best of
//                    the keys not yet taken, 64-bit max butterfly over (key, ~id), the owner marks it taken); per-lane rank
//                    count + integer butterfly.  No LDS, no atomics, nothing crosses a wave.
// Column order.  QUAD (V % 4 == 0): a lane owns columns 4 * (lane + 64 i) + e, the order of k_hyp_score<true>; otherwise columns
// lane + 64 j, the order of k_hyp_score<false>.  The order follows V alone; ALIGNED only chooses 16-byte loads over 4-byte loads
// of the same columns, so a base off 16 bytes gives the bits of the aligned call, and on aligned logits (what the decoder
// writes) chosen_logp is tok_logp of k_hyp_score whatever V is.
#pragma once
#include "ttx_metrics.hip.h"

namespace ttx {

constexpr int ALT_MAX_K = 32;             // alternatives per position
constexpr int ALT_SLOTS = MET_MAX_V / 64; // registers of one lane's share of a row

struct AltArgs {
  const float* logits;                    // [R, T, V]
  const int64_t* hyp;                     // rows of stride ld_hyp, W = T + 1 columns read
  const int* length;                      // [R]
  int* top_id;                            // [R, T, k] or null
  float* top_logp;                        // [R, T, k] or null
  float* chosen_logp;                     // [R, T] or null
  int* rank;                              // [R, T] or null
  float* entropy;                         // [R, T] or null
  int ld_hyp, M, T, V, k;                 // M = R * T positions
};

// Order key of a logit: unsigned order == float order, -0.0 and +0.0 share a key, and every bit pattern (NaNs too) has a place,
// so ids stay distinct and in [0, V) on rows outside the contract.
__device__ __forceinline__ unsigned alt_key(float x) {
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// met_push, except that -inf elements ahead of the lane's first finite one are passed over (see the head of the file)
__device__ __forceinline__ void alt_push(float x, int c, float& m, int& bi, float& r) {
  if (x > -INFINITY || m > -INFINITY) met_push(x, c, m, bi, r);
}

template <bool QUAD>
__device__ __forceinline__ int alt_col(int lane, int j) {
  return QUAD ? 4 * (lane + 64 * (j >> 2)) + (j & 3) : lane + 64 * j;
}

template <bool QUAD, bool ALIGNED>
__global__ __launch_bounds__(256) void k_alternatives(const AltArgs a) {
  const int pos = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pos >= a.M) return;                 // wave-uniform
  const int lane = threadIdx.x & 63;
  const int T = a.T, V = a.V, k = a.k;
  const int r = pos / T, p = pos - r * T;
  const size_t ko = (size_t)pos * k;
  if (p >= a.length[r]) {                 // wave-uniform: not live
    if (lane < k) {
      if (a.top_id) a.top_id[ko + lane] = -1;
      if (a.top_logp) a.top_logp[ko + lane] = 0.0f;
    }
    if (lane == 0) {
      if (a.chosen_logp) a.chosen_logp[pos] = 0.0f;
      if (a.rank) a.rank[pos] = -1;
      if (a.entropy) a.entropy[pos] = 0.0f;
    }
    return;
  }
  const float* x = a.logits + (size_t)pos * V;
  float v[ALT_SLOTS];
  if constexpr (QUAD) {
#pragma unroll
    for (int i = 0; i < ALT_SLOTS / 4; ++i) {
      const int c = 4 * (lane + 64 * i);
      float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (c < V) {
        if constexpr (ALIGNED) q = *reinterpret_cast<const float4*>(x + c);
        else q = make_float4(x[c], x[c + 1], x[c + 2], x[c + 3]);
      }
      v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < ALT_SLOTS; ++j) {
      const int c = lane + 64 * j;
      v[j] = (c < V) ? x[c] : 0.0f;
    }
  }
  // (m, rs) as k_hyp_score forms them: alt_push over the lane's columns in ascending order, then the xor butterfly
  float m = -INFINITY, rs = -1.0f;
  int bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < ALT_SLOTS; ++j) {
    const int c = alt_col<QUAD>(lane, j);
    if (c < V) alt_push(v[j], c, m, bi, rs);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const float orr = __shfl_xor(rs, o, 64);
    if (om > m) {
      rs = (rs + 1.0f) * expf(m - om) + orr;
      m = om;
    } else if (om == m) {
      rs += orr + 1.0f;
    } else {
      rs += (orr + 1.0f) * expf(om - m);
    }
  }
  m = __shfl(m, 0, 64);                   // lane 0's pair is the one k_hyp_score uses
  rs = __shfl(rs, 0, 64);
  const float L = log1pf(rs);
  int t = (int)a.hyp[(size_t)r * a.ld_hyp + p + 1];
  if ((unsigned)t >= (unsigned)V) t = 0;  // memory safety only: the Python layer rejects such tokens (IndexError)
  const float xt = x[t];
  if (lane == 0 && a.chosen_logp) a.chosen_logp[pos] = -(L + (m - xt));   // m - x[t] first: exact when the target is the maximum

  if (a.entropy) {
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < ALT_SLOTS; ++j) {
      if (alt_col<QUAD>(lane, j) < V) {
        const float lp = -(L + (m - v[j]));
        const float e = expf(lp);
        acc += (e > 0.0f) ? e * lp : 0.0f;   // a -inf logit: e == 0, the term is 0 and not 0 * -inf
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) a.entropy[pos] = -acc;
  }

  unsigned key[ALT_SLOTS];
  unsigned taken = 0;                     // bit j: slot j is taken or holds no column
#pragma unroll
  for (int j = 0; j < ALT_SLOTS; ++j) {
    key[j] = alt_key(v[j]);
    if (alt_col<QUAD>(lane, j) >= V) taken |= 1u << j;
  }

  if (a.rank) {
    const unsigned kt = alt_key(xt);
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < ALT_SLOTS; ++j) {
      const int c = alt_col<QUAD>(lane, j);
      if (c < V && (key[j] > kt || (key[j] == kt && c < t))) ++cnt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) a.rank[pos] = cnt;
  }

  if (a.top_id || a.top_logp) {
    int my_id = 0;                        // lane j keeps the winner of round j
    for (int round = 0; round < k; ++round) {
      // composite (key, ~column): the larger key wins, equal keys the lower column; 0 = nothing left in this lane
      unsigned long long best = 0;
#pragma unroll
      for (int j = 0; j < ALT_SLOTS; ++j) {
        const unsigned long long cand =
            ((unsigned long long)key[j] << 32) | (unsigned)(0xffffffffu - (unsigned)alt_col<QUAD>(lane, j));
        if (!((taken >> j) & 1u) && cand > best) best = cand;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
      }
      int id = (int)(0xffffffffu - (unsigned)(best & 0xffffffffu));
      if ((unsigned)id >= (unsigned)V) id = 0;   // cannot happen for k <= V; never hand out an id outside [0, V)
#pragma unroll
      for (int j = 0; j < ALT_SLOTS; ++j)
        if (alt_col<QUAD>(lane, j) == id) taken |= 1u << j;
      if (lane == round) my_id = id;
    }
    if (lane < k) {
      if (a.top_id) a.top_id[ko + lane] = my_id;
      if (a.top_logp) a.top_logp[ko + lane] = -(L + (m - x[my_id]));   // the logit as memory holds it: the bits of chosen_logp
    }
  }
}

}  // namespace ttx
