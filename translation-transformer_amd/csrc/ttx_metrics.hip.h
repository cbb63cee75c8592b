// Teacher-forced evaluation metrics of libttx_hip.so (included by ttx_api.hip only): the loss / token accuracy / sequence
// accuracy stage of VanillaEncoderDecoderTransformerLightning.validation_step and test_step (src/model/lightning_model.py:174-207,
// src/utils/metrics.py).  Hand-written HIP for gfx950, wave64.  Two launches, no atomics, no hand-off between workgroups:
//   k_token_metrics   one wave per (row, position): first-index argmax and nll = logsumexp(x) - x[target] in one pass over V
//   k_batch_metrics   one workgroup: mean nll, token accuracy and calc_sequence_acc over all B*T positions, in a fixed order
#pragma once
#include "ttx_common.hip.h"

namespace ttx {

constexpr int MET_MAX_V = 1024;           // the library's vocabulary limit (ttx_nucleus_mask, the beam loops)
constexpr int MET_BATCH_THREADS = 1024;   // k_batch_metrics: 16 waves, rows dealt out round-robin

// One lane's running (max m, first index of the max, r = sum of exp(x - m) over its elements minus the 1 of the max itself)
// after element x at index c.  Indices reach a lane in ascending order, so a strict '>' keeps the first maximum.  Keeping the
// max's own 1 out of r lets nll = log1p(r) + m - x[t] resolve the small losses of confident positions (r << 1) that a sum next
// to 1.0 would round away.  An empty lane is (m, r) = (-inf, -1).
__device__ __forceinline__ void met_push(float x, int c, float& m, int& bi, float& r) {
  if (x > m) {
    r = (r + 1.0f) * expf(m - x);         // m == -inf on the first element: 0 * 0
    m = x;
    bi = c;
  } else {
    r += expf(x - m);
  }
}

// logits fp32 [M, V] (M = B*T rows, row r = (b, p)); tgt int64 [B, Lt] read at column p + 1.
// pred int64 [M]: torch.argmax (first maximum); nll fp32 [M]: -log_softmax(x)[target] = log(sum exp(x - max)) + (max - x[target]).
template <bool VEC4>
__global__ __launch_bounds__(256) void k_token_metrics(const float* __restrict__ logits, const int64_t* __restrict__ tgt, int Lt,
                                                       int M, int V, int64_t* __restrict__ pred, float* __restrict__ nll) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const int T = Lt - 1;
  const float* x = logits + (size_t)row * V;
  float m = -INFINITY, r = -1.0f;
  int bi = 0x7fffffff;
  if constexpr (VEC4) {                   // V % 4 == 0 and a 16-byte aligned base: lane reads columns 4*(lane + 64 k) .. +3
    for (int c = lane * 4; c < V; c += 256) {
      const float4 v = *reinterpret_cast<const float4*>(x + c);
      met_push(v.x, c, m, bi, r);
      met_push(v.y, c + 1, m, bi, r);
      met_push(v.z, c + 2, m, bi, r);
      met_push(v.w, c + 3, m, bi, r);
    }
  } else {
    for (int c = lane; c < V; c += 64) met_push(x[c], c, m, bi, r);
  }
  // fixed xor butterfly; lane 0's operands and their order are the same in every call
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const float orr = __shfl_xor(r, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (om > m) {
      r = (r + 1.0f) * expf(m - om) + orr;
      m = om;
      bi = oi;
    } else if (om == m) {
      r += orr + 1.0f;                    // two empty lanes: -1 + -1 + 1 stays empty
      bi = oi < bi ? oi : bi;
    } else {
      r += (orr + 1.0f) * expf(om - m);
    }
  }
  if (lane == 0) {
    const int b = row / T, p = row - b * T;
    int t = (int)tgt[(size_t)b * Lt + 1 + p];
    if ((unsigned)t >= (unsigned)V) t = 0;     // memory safety only: the Python layer rejects such targets (IndexError)
    pred[row] = (int64_t)((bi < V) ? bi : 0);  // a row of NaNs compares false everywhere: never hand out an id outside [0, V)
    nll[row] = log1pf(r) + (m - x[t]);        // m - x[t] first: exact when the target is the maximum
  }
}

// One workgroup over all B*T positions.  Wave w takes rows w, w + 16, ...; inside a row the lanes walk 64 positions at a time,
// each lane summing its positions' nll in double in position order; the 16 wave totals are added in wave order by thread 0.
// calc_sequence_acc (metrics.py) per row, with q_1 < ... < q_k the EOS positions of the row's target:
//   selected positions are p with eos[(p + 1) mod T] (the mask's roll(-1)), taken in ascending order and paired with the EOS
//   positions in ascending order; a pair is a hit when cumsum(hit)[p] == q.  Without an EOS at position 0 the selected p pairs
//   with q = p + 1.  With one, the order shifts by one: the selected p pairs with the last EOS at or before p (and p = T - 1,
//   selected through the wrap, with q_k).
// out3 = {mean nll, token hits / (B*T), sequence hits / pairs (NaN without pairs)}.
__global__ __launch_bounds__(MET_BATCH_THREADS) void k_batch_metrics(const int64_t* __restrict__ pred, const float* __restrict__ nll,
                                                                     const int64_t* __restrict__ tgt, int B, int Lt, int eos,
                                                                     float* __restrict__ out3) {
  constexpr int NW = MET_BATCH_THREADS / 64;
  __shared__ double s_nll[NW];
  __shared__ long long s_tok[NW], s_pairs[NW], s_seq[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int T = Lt - 1;
  const unsigned long long le_mask = (lane == 63) ? ~0ull : ((2ull << lane) - 1);   // lanes 0..lane
  double acc = 0.0;
  long long tok_hits = 0, pairs = 0, seq_hits = 0;      // pairs / seq_hits: wave-uniform (from ballots)
  for (int b = w; b < B; b += NW) {
    const int64_t* tr = tgt + (size_t)b * Lt + 1;        // target_future row
    const bool eos0 = tr[0] == eos;
    int carry = 0;                                       // cumsum(hit) before this chunk
    int last_eos = -1;                                   // last EOS position before this chunk
    for (int base = 0; base < T; base += 64) {
      const int p = base + lane;
      const bool valid = p < T;
      bool hit = false, is_eos = false, next_eos = false;
      if (valid) {
        const int64_t tv = tr[p];
        const size_t r = (size_t)b * T + p;
        hit = pred[r] == tv;
        is_eos = tv == eos;
        next_eos = tr[(p + 1 == T) ? 0 : p + 1] == eos;
        acc += (double)nll[r];
        tok_hits += hit ? 1 : 0;
      }
      const unsigned long long hmask = __ballot(hit);
      const unsigned long long emask = __ballot(is_eos);
      const int csum = carry + __popcll(hmask & le_mask);                 // cumsum(hit)[p]
      const unsigned long long e_le = emask & le_mask;
      const int eos_at_or_before = e_le ? base + 63 - __clzll(e_le) : last_eos;
      const int q = eos0 ? eos_at_or_before : p + 1;
      const bool sel = valid && next_eos;
      pairs += __popcll(__ballot(sel));
      seq_hits += __popcll(__ballot(sel && csum == q));
      carry += __popcll(hmask);
      if (emask) last_eos = base + 63 - __clzll(emask);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, 64);
    tok_hits += __shfl_xor(tok_hits, o, 64);
  }
  if (lane == 0) {
    s_nll[w] = acc;
    s_tok[w] = tok_hits;
    s_pairs[w] = pairs;
    s_seq[w] = seq_hits;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tn = 0.0;
    long long tt = 0, tp = 0, ts = 0;
    for (int i = 0; i < NW; ++i) {
      tn += s_nll[i];
      tt += s_tok[i];
      tp += s_pairs[i];
      ts += s_seq[i];
    }
    const long long n = (long long)B * T;
    // torch: float sums of 0/1 values (exact) divided by the count in fp32
    out3[0] = (float)(tn / (double)n);
    out3[1] = (float)tt / (float)n;
    out3[2] = tp ? (float)ts / (float)tp : __builtin_nanf("");
  }
}

}  // namespace ttx
