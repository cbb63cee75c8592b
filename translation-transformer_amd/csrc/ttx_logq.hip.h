// Log-probability of hypotheses under the sampling distribution (included by ttx_api.hip only): the stage after the teacher-forced
// pass on the hypotheses themselves, next to k_hyp_score.  Hand-written HIP for gfx950, wave64.  For a hypothesis row h[0..W-1],
// the logits x[p, 0..V-1] of decode_tgt(h[:W-1]) and a distribution (temperature, top_k, top_p), position p = t - 1 of a row
// with n scored tokens (k_hyp_score's n) evaluates the sampler's own rule (ttx_sample.hip.h, steps 2-6) at the token t = h[p+1]:
//   greedy (temperature 0)   tok_logq = 0 if t is k_argmax's token (first maximum of x), else -inf;  n_kept = 1
//   otherwise                y_v = __fmul_rn(x_v, inv_T), the sampler's product
//   filter off               tok_logq = -(log1pf(rs) + (m - y_t)), (m, rs) of k_hyp_score's pass on y (alt_push per lane in
//                            k_hyp_score's column order, its xor butterfly, lane 0's pair);  n_kept = V
//   filter on                sample_topk_to_lanes<VPL> ITSELF gives the kept set (lane i holds rank i); e_i = expf(y_i - m) for
//                            i < n_kept, S the last element of wave_scan_incl(e): the S sample_row multiplies u by;
//                            tok_logq = (y_t - m) - logf(S) for a kept t, -inf for any other
//   forced (p < forced_len)  tok_logq = 0, the logits are not read;  rank = -1, n_kept = 0
//   rank                     the number of v with y_v > y_t, or y_v == y_t and v < t (alt_key order, as k_alternatives has it; at
//                            temperature 0 on x itself)
//   p >= n                   tok_logq = 0, rank = -1, n_kept = 0
//   logq          the sum of tok_logq[0..n-1] in position order, in double, rounded once (-inf as soon as one term is)
//   first_outside the first p < n with tok_logq == -inf, else -1
// k_hyp_logq<VPL>: ONE launch, one workgroup per hypothesis, wave 0 scans the tokens (ballots, k_hyp_score's scan), the waves
// share the n positions, each position by ONE wave with the row in registers (V <= 64 * VPL), wave 0 adds up.  No LDS beyond the
// row's n, no atomics, nothing crosses a workgroup: two calls give the same bits, and a position's results depend on its own logits
// row and the hypothesis alone.  Column order of the unfiltered pass by V alone (V % 4 == 0: k_hyp_score<true>'s, else
// k_hyp_score<false>'s); a 16-byte aligned base only chooses 16-byte loads of the same columns.
#pragma once
#include "ttx_alternatives.hip.h"
#include "ttx_sample.hip.h"

namespace ttx {

constexpr int LOGQ_THREADS = 1024;        // 16 waves per hypothesis row, as k_hyp_score: 4 per SIMD, a budget of 128 VGPRs (<16> takes 76)

struct LogqArgs {
  const float* logits;                    // [R, T, V]
  const int64_t* hyp;                     // rows of stride ld_hyp, W = T + 1 columns read
  const int* forced_len;                  // [R] or null; clamped to [0, n]
  float* tok_logq;                        // [R, T], never null (session scratch when the caller wants none)
  float* logq;                            // [R] or null
  int* first_outside;                     // [R] or null
  int* rank;                              // [R, T] or null
  int* n_kept;                            // [R, T] or null
  int* length;                            // [R] or null
  uint8_t* finished;                      // [R] or null
  int ld_hyp, W, V, pad, eos;
  float inv_T, top_p;                     // inv_T = 1 when greedy
  int top_k, greedy;                      // top_k 0: filter off
};

// The number of ids v with key(y_v) > key(y_t), or equal keys and v < t, y = x * inv_T: every lane returns it.
template <int VPL>
__device__ __forceinline__ int logq_rank(const float* __restrict__ x, int V, float inv_T, int t, int lane) {
  const unsigned kt = alt_key(__fmul_rn(x[t], inv_T));
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane + 64 * i;
    if (c < V) {
      const unsigned k = alt_key(__fmul_rn(x[c], inv_T));
      if (k > kt || (k == kt && c < t)) ++cnt;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  return cnt;
}

template <int VPL>
__global__ __launch_bounds__(LOGQ_THREADS) void k_hyp_logq(const LogqArgs a) {
  constexpr int NW = LOGQ_THREADS / 64;
  __shared__ int s_n;
  const int r = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int W = a.W, V = a.V, T = W - 1;
  const int64_t* h = a.hyp + (size_t)r * a.ld_hyp;
  float* lp = a.tok_logq + (size_t)r * T;
  if (w == 0) {                           // k_hyp_score's scan
    int n = 0, fin = 0;
    for (int base = 1; base < W; base += 64) {
      const int c = base + lane;
      const int64_t tv = (c < W) ? h[c] : (int64_t)a.pad;
      const unsigned long long emask = __ballot(c < W && tv == a.eos);
      if (emask) {                        // wave-uniform: the first EOS ends the hypothesis
        n = base + __ffsll((long long)emask) - 1;
        fin = 1;
        break;
      }
      const unsigned long long tmask = __ballot(c < W && tv != a.pad);
      if (tmask) n = base + 63 - __clzll((long long)tmask);
    }
    if (lane == 0) {
      s_n = n;
      if (a.length) a.length[r] = n;
      if (a.finished) a.finished[r] = (uint8_t)fin;
    }
  }
  __syncthreads();
  const int n = s_n;
  int fl = a.forced_len ? a.forced_len[r] : 0;
  fl = fl < 0 ? 0 : (fl > n ? n : fl);
  // not live (p >= n) and forced (p < fl): no pass over the logits
  for (int p = threadIdx.x; p < T; p += LOGQ_THREADS) {
    if (p < fl || p >= n) {
      lp[p] = 0.0f;
      if (a.rank) a.rank[(size_t)r * T + p] = -1;
      if (a.n_kept) a.n_kept[(size_t)r * T + p] = 0;
    }
  }
  for (int p = fl + w; p < n; p += NW) {
    const float* x = a.logits + ((size_t)r * T + p) * V;
    int t = (int)h[p + 1];
    if ((unsigned)t >= (unsigned)V) t = 0;   // memory safety only: the Python layer rejects such tokens (IndexError)
    float q;
    int nk;
    if (a.greedy) {
      // k_argmax, statement for statement (sample_row's greedy branch)
      float best = -INFINITY;
      int bi = 0x7fffffff;
      for (int c = lane; c < V; c += 64) {
        const float v = x[c];
        if (v > best) { best = v; bi = c; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
      }
      const int tok = (bi < V) ? bi : 0;
      q = (t == tok) ? 0.0f : -INFINITY;
      nk = 1;
    } else if (a.top_k > 0) {
      int my_idx, n_kept;
      float my_val, m;
      sample_topk_to_lanes<VPL>(x, V, a.inv_T, a.top_p, a.top_k, lane, my_idx, my_val, n_kept, m);
      const float e = (lane < n_kept) ? expf(my_val - m) : 0.0f;
      const float C = wave_scan_incl(e, lane);
      const float S = __shfl(C, 63, 64);
      const unsigned long long hit = __ballot(lane < n_kept && my_idx == t);
      q = -INFINITY;
      if (hit) {                          // wave-uniform
        const float yt = __shfl(my_val, __ffsll((long long)hit) - 1, 64);
        q = (yt - m) - logf(S);
      }
      nk = n_kept;
    } else {
      // (m, rs) of k_hyp_score's pass on y: alt_push over the lane's columns in ascending order, then the xor butterfly
      float m = -INFINITY, rs = -1.0f;
      int bi = 0x7fffffff;
      if (V % 4 == 0) {                   // lane reads columns 4 * (lane + 64 k) .. + 3
        const bool al = reinterpret_cast<uintptr_t>(x) % 16 == 0;
        for (int c = lane * 4; c < V; c += 256) {
          float4 v;
          if (al) v = *reinterpret_cast<const float4*>(x + c);
          else v = make_float4(x[c], x[c + 1], x[c + 2], x[c + 3]);
          alt_push(__fmul_rn(v.x, a.inv_T), c, m, bi, rs);
          alt_push(__fmul_rn(v.y, a.inv_T), c + 1, m, bi, rs);
          alt_push(__fmul_rn(v.z, a.inv_T), c + 2, m, bi, rs);
          alt_push(__fmul_rn(v.w, a.inv_T), c + 3, m, bi, rs);
        }
      } else {
        for (int c = lane; c < V; c += 64) alt_push(__fmul_rn(x[c], a.inv_T), c, m, bi, rs);
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
      m = __shfl(m, 0, 64);               // lane 0's pair is the one k_hyp_score uses
      rs = __shfl(rs, 0, 64);
      q = -(log1pf(rs) + (m - __fmul_rn(x[t], a.inv_T)));   // m - y_t first: exact when the target is the maximum
      nk = V;
    }
    int rk = 0;
    if (a.rank) rk = logq_rank<VPL>(x, V, a.inv_T, t, lane);
    if (lane == 0) {
      lp[p] = q;
      if (a.rank) a.rank[(size_t)r * T + p] = rk;
      if (a.n_kept) a.n_kept[(size_t)r * T + p] = nk;
    }
  }
  __syncthreads();                        // the block's own stores to lp are visible to wave 0
  if (w == 0 && (a.logq || a.first_outside)) {
    double acc = 0.0;                     // every lane adds the same values in position order
    int first = -1;
    for (int base = 0; base < n; base += 64) {
      const int p = base + lane;
      const float v = (p < n) ? lp[p] : 0.0f;
      const unsigned long long out = __ballot(p < n && v == -INFINITY);
      if (out && first < 0) first = base + __ffsll((long long)out) - 1;
      const int cnt = (n - base < 64) ? n - base : 64;
      for (int i = 0; i < cnt; ++i) acc += (double)__shfl(v, i, 64);
    }
    if (lane == 0) {
      if (a.logq) a.logq[r] = (float)acc;
      if (a.first_outside) a.first_outside[r] = first;
    }
  }
}

// first_outside from per-token values that another kernel wrote (ttx_score_proposal under the model's own distribution, where
// k_hyp_score gives tok_logq): the first p < length[r] with tok[r, p] == -inf, else -1.  One wave per row, 4 rows per workgroup.
__global__ __launch_bounds__(256) void k_logq_first_outside(const float* __restrict__ tok, const int* __restrict__ length,
                                                            int* __restrict__ first_outside, int R, int T) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;                     // wave-uniform
  const int lane = threadIdx.x & 63;
  int n = length[r];
  n = n < 0 ? 0 : (n > T ? T : n);
  int first = -1;
  for (int base = 0; base < n; base += 64) {
    const int p = base + lane;
    const unsigned long long out = __ballot(p < n && tok[(size_t)r * T + p] == -INFINITY);
    if (out) {                            // wave-uniform
      first = base + __ffsll((long long)out) - 1;
      break;
    }
  }
  if (lane == 0) first_outside[r] = first;
}

}  // namespace ttx
