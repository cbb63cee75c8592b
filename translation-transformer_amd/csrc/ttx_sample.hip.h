// Seeded ancestral sampling on the greedy step (included by ttx_api.hip only): k_sample chooses a row's next token from its
// logits where the greedy loop launches k_argmax.  Hand-written HIP for gfx950, wave64: ONE wave per logits row, 4 rows per
// workgroup, the row in registers (V <= 64 * VPL <= 1024), no LDS, no atomics, nothing crosses a wave or a row.
// The rule for a live row r (include/ttx.h states it as the contract; tests/util_sample_checks.py restates it in float64):
//   1  done[r] != 0: pred[r] = pad, the logits are not read.
//   2  greedy block (temperature 0): pred[r] is k_argmax's answer on the bits (first maximum, its NaN rule); no scaling.
//   3  y_v = x_v * inv_T, one rounded fp32 product per logit (never contracted into the subtraction that follows).
//   4  kept set.  Filter off: all V tokens, in ascending id.  Filter on: sample_topk_to_lanes below, i.e. topk_to_lanes
//      (mask_with_num_logits_according_nucleus) on y: ranks best first, equal values the lower id first, rank i kept while the
//      softmax mass ranked above it is < top_p and i < top_k, rank 0 always; lane i holds rank i.
//   5  u = (x0 >> 8) * 2^-24 with x0 = word 0 of Philox4x32-10, key (seed_lo, seed_hi), counter (key_lo, key_hi, sample, pos),
//      pos = front[0] + 1.
//   6  e_v = expf(y_v - m) over the kept set (m the row's maximum of y), C its inclusive prefix sums in the order of 4, S the
//      last of them, t = u * S: the first kept token with e_v > 0 and C_v > t; if rounding leaves none, the last kept token with
//      e_v > 0.  A -inf logit has e_v = 0 and is never emitted.
//      Order of the sums (fixed by V and the filter alone).  Filter off: lane l owns the VPL consecutive ids l * VPL .. and adds
//      them in ascending order; the lanes' totals go through a Hillis-Steele inclusive scan (offsets 1, 2, .., 32); the prefix of
//      an id is its lane's exclusive scan value plus the lane's running sum.  Filter on: the scan alone, over the ranks.
//   7  the token is eos or pad: done[r] = 1.
// Rows at or beyond *m_ptr are not written.  Rows outside the contract (NaN, +inf, all -inf) give some id in [0, V).
// k_sample_step is steps 2-6 (sample_row, shared with k_sample) on the rows of a speculative verify step: see its comment below.
// Forced prefixes (PrefixTab, include/ttx.h "Forced target prefixes"): a live row whose position is inside its source's prefix emits
// the prefix token (an id outside [0, V) as 0) and skips steps 2-6; the logits are not read and no uniform is formed.  k_prefix_drafts
// rewrites draft 0 of every active row of a prompted speculative loop before each step.
#pragma once
#include "ttx_loop_kernels.hip.h"

namespace ttx {

constexpr int SAMPLE_MAX_V = 64 * NUC_VPL;   // 1 024
constexpr int SAMPLE_MAX_KEEP = NUC_MAX_KEEP;

// The call's parameters, device-resident so that a captured step holds none of them (written by k_sample_params).
struct SampleBlock {
  unsigned long long seed;
  float inv_T;                     // 1 / temperature, formed on the host; unused when greedy
  float top_p;
  int top_k;                       // 0: filter off (then top_p is 1); else 1..32
  int greedy;                      // temperature == 0
  int pad, eos;
};

// The forced prefixes of a prompted call as the kernels see them (tok null: an unprompted call, nothing below is read).  `len` and
// `src` go by decoder row (slot of a pool): the length of the row's prefix and the row of `tok` that holds it.
struct PrefixTab {
  const int* tok; int ld;          // [sources][ld]
  const int* len;                  // [B]
  const int* src;                  // [B]
};

// The forced token of decoder row b at position pos (1 <= pos <= len[b] <= ld), as every lane of the row's wave reads it.
__device__ __forceinline__ int prefix_token(const PrefixTab& t, int b, int pos, int V) {
  const int tok = t.tok[(size_t)t.src[b] * t.ld + pos - 1];
  return (unsigned)tok < (unsigned)V ? tok : 0;
}

struct SampleArgs {
  const float* logits; int V;      // [M, V]
  int* pred;                       // [M]
  const int* m_ptr; int M;         // live rows on the device (null: M)
  const unsigned long long* key;   // [M]
  const unsigned* sample;          // [M]
  int* done;                       // [M], read and written
  const int* front;                // front[0] + 1 is the position being filled
  const SampleBlock* prm;
  PrefixTab pfx;                   // by row
};

__global__ void k_sample_params(SampleBlock* out, SampleBlock v) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *out = v;
}

// Row r = b * n + j of a sampling loop: source b, sample j, key (row_keys[b] or b, j), not done.
__global__ void k_sample_init(unsigned long long* key, unsigned* sample, int* done, int* src_of, const int64_t* row_keys, int R, int n) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int b = r / n;
  key[r] = row_keys ? (unsigned long long)row_keys[b] : (unsigned long long)b;
  sample[r] = (unsigned)(r - b * n);
  done[r] = 0;
  src_of[r] = b;
}

// Word 0 of Philox4x32-10 (Salmon et al., SC'11): integer arithmetic only.
__device__ __forceinline__ unsigned philox4x32_10_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

__device__ __forceinline__ float sample_uniform(unsigned long long seed, unsigned long long key, unsigned sample, unsigned pos) {
  const unsigned x0 = philox4x32_10_word0((unsigned)key, (unsigned)(key >> 32), sample, pos, (unsigned)seed, (unsigned)(seed >> 32));
  return (float)(x0 >> 8) * 5.9604644775390625e-08f;     // 24 bits * 2^-24: exact, in [0, 1)
}

// Hillis-Steele inclusive scan over the 64 lanes, offsets 1, 2, .., 32.
__device__ __forceinline__ float wave_scan_incl(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

// topk_to_lanes on y = x * inv_T: the same selection and the same arithmetic on the scaled row (lane r holds rank r).
template <int VPL>
__device__ __forceinline__ void sample_topk_to_lanes(const float* __restrict__ p, int V, float inv_T, float nucleus, int n_best, int lane,
                                                     int& my_idx, float& my_val, int& n_kept, float& m_out) {
  float v[VPL];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < V ? __fmul_rn(p[c], inv_T) : -INFINITY;
    m = fmaxf(m, v[i]);
  }
  m = wave_max(m);
  float z = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) z += (lane + 64 * i < V) ? expf(v[i] - m) : 0.f;
  z = wave_sum(z);
  m_out = m;
  n_kept = 0;
  my_idx = -1; my_val = -INFINITY;
  float above = 0.f;                        // softmax mass of the ranks already taken
  for (int rank = 0; rank < n_best && rank < V; ++rank) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      if (v[i] > best || (v[i] == best && lane + 64 * i < bi && v[i] != -INFINITY)) { best = v[i]; bi = lane + 64 * i; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (bi == 0x7fffffff) break;            // nothing finite left
    if (rank != 0 && !(above < nucleus)) break;   // the mass above only grows: no later rank can be kept
    if (lane == rank) { my_idx = bi; my_val = best; }
    ++n_kept;
    above += expf(best - m) / z;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      if (lane + 64 * i == bi) v[i] = -INFINITY;
  }
}

// Steps 2-6 of the rule for one logits row `p` of V <= 64 * VPL values, by one wave: the token of row (key, sample) at position `pos`.
// Shared by k_sample and k_sample_step, so that both emit the same token from the same bits.  Every lane returns the token.
template <int VPL>
__device__ __forceinline__ int sample_row(const float* __restrict__ p, int V, const SampleBlock& prm, unsigned long long key,
                                          unsigned sample, unsigned pos, int lane) {
  int tok;
  if (prm.greedy) {
    // k_argmax, statement for statement
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < V; c += 64) {
      const float v = p[c];
      if (v > best) { best = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    tok = (bi < V) ? bi : 0;
  } else {
    const float u = sample_uniform(prm.seed, key, sample, pos);
    if (prm.top_k > 0) {
      int my_idx, n_kept;
      float my_val, m;
      sample_topk_to_lanes<VPL>(p, V, prm.inv_T, prm.top_p, prm.top_k, lane, my_idx, my_val, n_kept, m);
      const float e = (lane < n_kept) ? expf(my_val - m) : 0.0f;
      const float C = wave_scan_incl(e, lane);
      const float t = __fmul_rn(u, __shfl(C, 63, 64));
      const unsigned long long live = __ballot(e > 0.0f);
      const unsigned long long hit = __ballot(e > 0.0f && C > t);
      const int src = hit ? __ffsll((long long)hit) - 1 : (live ? 63 - __clzll((long long)live) : 0);
      tok = __shfl(my_idx, src, 64);
    } else {
      // lane l owns ids l * VPL .. l * VPL + VPL - 1
      float e[VPL];
      float m = -INFINITY;
      const int c0 = lane * VPL;
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        e[j] = (c0 + j < V) ? __fmul_rn(p[c0 + j], prm.inv_T) : -INFINITY;
        m = fmaxf(m, e[j]);
      }
      m = wave_max(m);
      float tot = 0.0f;
      int last = -1;                        // the lane's last id with e > 0
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        e[j] = (c0 + j < V) ? expf(e[j] - m) : 0.0f;
        tot += e[j];
        if (e[j] > 0.0f) last = c0 + j;
      }
      const float C = wave_scan_incl(tot, lane);
      const float t = __fmul_rn(u, __shfl(C, 63, 64));
      const unsigned long long live = __ballot(last >= 0);
      const unsigned long long hit = __ballot(last >= 0 && C > t);
      const int src = hit ? __ffsll((long long)hit) - 1 : (live ? 63 - __clzll((long long)live) : 0);
      // inside the chosen lane: the first id whose prefix exceeds t, else the lane's last id with e > 0
      const float before = __shfl_up(C, 1, 64);
      float run = lane ? before : 0.0f;     // the scan value of the lanes before this one
      int pick = -1;
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        run += e[j];
        if (pick < 0 && e[j] > 0.0f && run > t) pick = c0 + j;
      }
      if (pick < 0) pick = last;
      tok = __shfl(pick, src, 64);
    }
    if ((unsigned)tok >= (unsigned)V) tok = 0;   // rows outside the contract only: never an id outside [0, V)
  }
  return tok;
}

template <int VPL>
__global__ __launch_bounds__(256) void k_sample(const SampleArgs a) {
  const int rows = a.m_ptr ? *a.m_ptr : a.M;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                  // wave-uniform
  const int lane = threadIdx.x & 63;
  const SampleBlock prm = *a.prm;
  if (a.done[row]) {                        // wave-uniform
    if (lane == 0) a.pred[row] = prm.pad;
    return;
  }
  const int pos = a.front[0] + 1;
  int tok;
  if (a.pfx.tok && pos <= a.pfx.len[row]) tok = prefix_token(a.pfx, row, pos, a.V);     // wave-uniform
  else tok = sample_row<VPL>(a.logits + (size_t)row * a.V, a.V, prm, a.key[row], a.sample[row], (unsigned)pos, lane);
  if (lane == 0) {
    a.pred[row] = tok;
    if (tok == prm.eos || tok == prm.pad) a.done[row] = 1;
  }
}

// The sampler on the rows of a speculative verify step (ttx_sample_speculative_generate), in the step-row layout of k_embed<true>:
// row = slot * RPS + rs belongs to decoder row b = act_idx[slot] at front f = front[b]; rs == 0 predicts position f + 1, row
// rs = 1 + n * D + j (token j of draft n, at position f + 1 + j) predicts position f + 2 + j.  The token is sample_row's for
// (key[b], sample[b], that position): what k_sample emits there from the same logits.  key and sample are indexed by decoder row,
// not by slot (the active list compacts).  k_argmax's launch shape and live-row rule; no done flags (rows retire through the
// active list); rows at or beyond *m_ptr are not written.
// Slot pool: `act_idx` is the list of the pass (the probe's: every live slot; the draft pass's: the matching slots), `pred` the
// pass's own buffer, and under draft select `row_map` gives the layout row of every compacted row as k_embed<true> reads it: the
// logits and pred are indexed by the compacted row, the position comes from the layout row.  The probe layout is N = 1, D = 0.
struct SampleStepArgs {
  const float* logits; int V;      // [M, V]
  int* pred;                       // [M]
  const int* m_ptr; int M;         // live rows on the device (null: M)
  const unsigned long long* key;   // [B]
  const unsigned* sample;          // [B]
  const int* act_idx;              // [n_active]
  const int* front;                // [B]
  int N, D;
  const SampleBlock* prm;
  const int* row_map;              // [rows] or null: row = layout row
  PrefixTab pfx;                   // by decoder row, like key and sample
};

template <int VPL>
__global__ __launch_bounds__(256) void k_sample_step(const SampleStepArgs a) {
  const int rows = a.m_ptr ? *a.m_ptr : a.M;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                  // wave-uniform
  const int lane = threadIdx.x & 63;
  const SampleBlock prm = *a.prm;
  const int RPS = step_rps(a.N, a.D);
  const int lrow = a.row_map ? a.row_map[row] : row;
  const int rs = lrow % RPS;
  const int b = a.act_idx[lrow / RPS];
  int pos = a.front[b] + 1;
  if (rs != 0 && a.D > 0) pos += 1 + (rs - 1) % a.D;       // the probe (D == 0) has row 0 only
  int tok;
  if (a.pfx.tok && pos <= a.pfx.len[b]) tok = prefix_token(a.pfx, b, pos, a.V);        // wave-uniform
  else tok = sample_row<VPL>(a.logits + (size_t)row * a.V, a.V, prm, a.key[b], a.sample[b], (unsigned)pos, lane);
  if (lane == 0) a.pred[row] = tok;
}

// Copy drafts of the sampling loop: the n decoder rows of a source share its drafts.  in [B, nd] -> out [B * n, nd].
__global__ void k_sample_rep_drafts(const int* in, int* out, int R, int n, int nd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < R * nd) out[i] = in[(size_t)(i / nd / n) * nd + i % nd];
}

// ------------------------------------------------------------------------------------------------
// Forced prefixes in the speculative sampling loops.  The acceptance rule is untouched: a draft token is accepted iff it is the token
// of its position, and inside the prefix that token is the prefix's (k_sample_step above).  So the prefix is offered as draft 0:
// before every verify step, column c = front + 1 + j of draft 0 of every active row receives prefix[c - 1] while c <= len (EOS and
// PAD as `repl`, as k_make_drafts writes them, so that drafts still hold neither and a forced EOS arrives as the bonus token), and
// token j of the row's own source draft 0 beyond it.  Stateless and idempotent: the D ints of every active row are rewritten from
// `draft0`, which nothing writes after the row was set up, so once front >= len draft 0 is the source draft again.  Drafts 1 .. N-1
// are not touched.  One wave per slot, grid for the capacity; per slot one round of independent loads (front, len, src by the
// row) and then D independent ones.
struct PrefixDraftsArgs {
  const DecState* st;              // n_active live slots
  const int* act_idx;              // [n_active]
  const int* front;                // [B]
  int* drafts; int N, D;           // [B, N, D], draft 0 of the active rows rewritten
  const int* draft0;               // [B, D] the rows' source draft 0
  PrefixTab pfx;
  int eos, pad, repl;
};

__global__ __launch_bounds__(256) void k_prefix_drafts(const PrefixDraftsArgs a) {
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= a.st->n_active) return;       // wave-uniform
  const int lane = threadIdx.x & 63;
  const int b = a.act_idx[slot];
  const int f = a.front[b], len = a.pfx.len[b], src = a.pfx.src[b];
  const int* pre = a.pfx.tok + (size_t)src * a.pfx.ld;
  const int* own = a.draft0 + (size_t)b * a.D;
  int* out = a.drafts + (size_t)b * a.N * a.D;
  for (int j = lane; j < a.D; j += 64) {
    const int c = f + 1 + j;
    int t;
    if (c <= len) {
      t = pre[c - 1];
      if (t == a.eos || t == a.pad) t = a.repl;
    } else {
      t = own[j];
    }
    out[j] = t;
  }
}

// The session's prefix table of a prompted call: int64 [S][ld_in] -> int32 [S][ld], columns at or beyond a source's length (and
// beyond ld_in) as `pad`.  Lengths are bounded by min(ld, ld_in) (checked on the host).
__global__ void k_prefix_load(const int64_t* in, int ld_in, const int* len, int* out, int S, int ld, int pad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * ld) return;
  const int s = i / ld, c = i - s * ld;
  int t = pad;
  if (c < len[s] && c < ld_in) {
    const int64_t v = in[(size_t)s * ld_in + c];
    t = (v >= 0 && v <= 0x7fffffff) ? (int)v : -1;       // an id no int32 holds stays outside every vocabulary
  }
  out[i] = t;
}

// Prefix length of every decoder row of a single-session loop: its source's.
__global__ void k_prefix_rows(const int* len_src, const int* src_of, int* len_row, int R) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < R) len_row[r] = len_src[src_of[r]];
}

}  // namespace ttx
