// Log-likelihood scores of finished hypotheses (included by ttx_api.hip only): the stage after the teacher-forced forward pass on
// the hypotheses themselves.  Hand-written HIP for gfx950, wave64.  For a hypothesis row h[0..W-1] (column 0, the BOS, is never
// scored) and the logits [W-1, V] of decode_tgt(h[:W-1]):
//   n        = column of the first EOS at a column >= 1 (finished = 1); else the last column >= 1 holding a non-PAD token
//              (finished = 0); else 0
//   tok_logp = log_softmax(logits[t-1])[h[t]] for t = 1..n, exactly 0 for t > n
//   score    = sum of tok_logp[0..n-1] in position order, accumulated in double, rounded once
// ONE launch, one workgroup per hypothesis: the row scan, the scored positions and the sum depend on nothing outside the row, so
// no value crosses a workgroup, nothing is atomic, and two calls on the same inputs give the same bits.  Positions past n cost a
// zero store and no pass over their logits.
//   k_score_src_of    the row map r -> r / N for the decoder's cross attention (one memory row per source)
//   k_hyp_score       16 waves per hypothesis: wave 0 scans the tokens (ballots), the waves share the n scored positions
//                     (one pass over V each: log-sum-exp with met_push's numerics and the target logit), wave 0 adds them up
#pragma once
#include "ttx_metrics.hip.h"

namespace ttx {

constexpr int SCORE_THREADS = 1024;       // k_hyp_score: 16 waves per hypothesis row

__global__ void k_score_src_of(int* src_of, int n, int per_src) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) src_of[i] = i / per_src;
}

// logits fp32 [R, W-1, V]; hyp int64 rows of stride ld_hyp, W columns read; tok_logp fp32 [R, W-1]; score fp32 [R];
// length int32 [R]; finished u8 [R] or null.
template <bool VEC4>
__global__ __launch_bounds__(SCORE_THREADS) void k_hyp_score(const float* __restrict__ logits, const int64_t* __restrict__ hyp,
                                                             int ld_hyp, int W, int V, int pad, int eos,
                                                             float* tok_logp, float* __restrict__ score,
                                                             int* __restrict__ length, uint8_t* __restrict__ finished) {
  constexpr int NW = SCORE_THREADS / 64;
  __shared__ int s_n;
  const int r = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int T = W - 1;
  const int64_t* h = hyp + (size_t)r * ld_hyp;
  float* lp = tok_logp + (size_t)r * T;
  if (w == 0) {
    int n = 0, fin = 0;
    for (int base = 1; base < W; base += 64) {
      const int c = base + lane;
      const int64_t tv = (c < W) ? h[c] : (int64_t)pad;
      const unsigned long long emask = __ballot(c < W && tv == eos);
      if (emask) {                        // wave-uniform: the first EOS ends the hypothesis
        n = base + __ffsll((long long)emask) - 1;
        fin = 1;
        break;
      }
      const unsigned long long tmask = __ballot(c < W && tv != pad);
      if (tmask) n = base + 63 - __clzll((long long)tmask);
    }
    if (lane == 0) {
      s_n = n;
      length[r] = n;
      if (finished) finished[r] = (uint8_t)fin;
    }
  }
  __syncthreads();
  const int n = s_n;
  for (int p = n + threadIdx.x; p < T; p += SCORE_THREADS) lp[p] = 0.0f;
  // position p = t - 1 scores token h[t] under logits row p
  for (int p = w; p < n; p += NW) {
    const float* x = logits + ((size_t)r * T + p) * V;
    float m = -INFINITY, rs = -1.0f;
    int bi = 0x7fffffff;
    if constexpr (VEC4) {                 // V % 4 == 0 and a 16-byte aligned base: lane reads columns 4*(lane + 64 k) .. +3
      for (int c = lane * 4; c < V; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + c);
        met_push(v.x, c, m, bi, rs);
        met_push(v.y, c + 1, m, bi, rs);
        met_push(v.z, c + 2, m, bi, rs);
        met_push(v.w, c + 3, m, bi, rs);
      }
    } else {
      for (int c = lane; c < V; c += 64) met_push(x[c], c, m, bi, rs);
    }
    // fixed xor butterfly, as k_token_metrics has it
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
    if (lane == 0) {
      int t = (int)h[p + 1];
      if ((unsigned)t >= (unsigned)V) t = 0;   // memory safety only: the Python layer rejects such tokens (IndexError)
      lp[p] = -(log1pf(rs) + (m - x[t]));      // m - x[t] first: exact when the target is the maximum
    }
  }
  __syncthreads();                        // the block's own stores to lp are visible to wave 0
  if (w == 0) {
    double acc = 0.0;                     // every lane adds the same values in position order
    for (int base = 0; base < n; base += 64) {
      const int p = base + lane;
      const float v = (p < n) ? lp[p] : 0.0f;
      const int cnt = (n - base < 64) ? n - base : 64;
      for (int i = 0; i < cnt; ++i) acc += (double)__shfl(v, i, 64);
    }
    if (lane == 0) score[r] = (float)acc;
  }
}

}  // namespace ttx
