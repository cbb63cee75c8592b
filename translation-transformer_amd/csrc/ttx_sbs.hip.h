// Stochastic beam search (Kool, van Hoof & Welling, ICML 2019) on the standard beam loop (included by ttx_api.hip only): k_sbs_step
// stands where the beam loop launches k_beam_step.  Hand-written HIP for gfx950, wave64: one workgroup of four waves per source,
// one wave per parent row at a time, the conditional maxima G' of the beam * V children in an LDS image, then K selection rounds.
// The rule (include/ttx.h states it as the contract under ttx_sbs_generate; tests/util_sbs_checks.py restates it in float64), for
// parent k of a source with key `key` at position pos:
//   1  y_v = x_v * inv_T, one rounded fp32 product per logit.
//   2  m = max y, z = sum expf(y_v - m), lp_v = (y_v - m) - logf(z), phi'_v = phi_k + lp_v.
//      Order of z (fixed by V alone): lane l owns the ids 4l .. 4l+3 of every block of 256 ids and adds its ids in ascending
//      order; the 64 lane totals go through the xor butterfly (offsets 32, 16, .., 1).  m and Z use the same walk with fmaxf.
//   3  u_v = ((w >> 9) + 0.5f) * 2^-23, w = word v & 3 of Philox4x32-10 with key (seed_lo, seed_hi) and counter
//      (key_lo, key_hi, 0x80000000 | k << 8 | v >> 2, pos): one Philox block per four consecutive ids, all four words used.
//   4  g_v = phi'_v - logf(-logf(u_v)), Z = max g.
//   5  G'_v = G_k where g_v == Z; elsewhere t = (G_k - g_v) + log1pf(-expf(g_v - Z)), G'_v = G_k - fmaxf(t, 0) - log1pf(expf(-fabsf(t))).
//   6  a finished parent has the single child PAD with phi and G unchanged; its logits are not read.
//   7  the K largest G' of the source's beam * V children, largest first, equal values the lower flat index k * V + v first.
// LDS: the image [beam * V] fp32 (dynamic, at most 150 KB), beside it per parent m, logf(z) and Z (3 x 32 fp32) from which phi' of
// the K winners is recomputed with the very operations of step 2, and the four waves' partial winners of a selection round.  In the
// image a child that does not exist (a finished parent's non-PAD ids) or that was already selected is NaN: it loses every comparison.
//
// k_sbs_step_masked (ttx_sbs_generate_ex: a top-k / top-p filter and forced prefixes) puts a per-parent token mask in front of the
// same rule; k_sbs_step itself is launched whenever a call has neither.  Per unfinished parent at position pos:
//   forced (1 <= pos <= the source's prefix length): the child `tok` = the prefix token (an id outside [0, V) as 0) has phi' = phi_k
//      and G' = G_k on the bits, every other child is -inf; the logits are not read and no Philox block is formed.
//   free, filter on: the kept set is sample_topk_to_lanes on y (the sampler's, on the bits: at most 32 tokens, rank r in lane r);
//      every other token has y_v = -inf, and steps 2-5 run on that row: m, z and Z by the walk above, masked ids adding
//      expf(-inf) = 0, so lp is renormalised over the kept set.  Philox counters stay keyed by the token id.  A kept set of ONE
//      token is a mask of one token, as a forced position is, and is written the same way (y - m = 0, z = 1, lp = 0, g == Z).
// On a kept id the walk uses k_sbs_step's own expressions, statement for statement, so that the compiler treats both alike (it
// fuses the product y = x * inv_T into the subtraction y - m in both): under a mask of every token the outputs are k_sbs_step's bits.
// The ranks reach the walk's ownership (lane l: ids 4l .. 4l+3 of every 256-block) by one shuffle of my_idx per kept rank into a
// per-lane bit mask (bit 4 * block + i: at most 16 bits); nothing goes through LDS inside the unsynchronised walk.  The filter's
// up to 32 dependent selection rounds per parent row are the cost, so the kernel runs 4, 8 or 16 waves per source (by the beam):
// a wave still owns whole parent rows, and the K selection rounds take their partial winners from as many waves; no sum or maximum
// changes its order with the wave count.
//
// Both kernels have a pool form in csrc/ttx_sbs_pool.hip.h (k_sbs_step_pool, k_sbs_step_pool_masked): the same statements with pos,
// width, the parent count and the key read per slot.  A change to the rule here is made there as well;
// tests/test_gpu_sbs_pool_kernel.py holds the two to the same bits.
#pragma once
#include "ttx_sample.hip.h"

namespace ttx {

constexpr int SBS_MAX_BEAM = NUC_MAX_KEEP;   // 32: rank k sits in bits 8..12 of counter word 2
constexpr int SBS_MAX_V = 64 * NUC_VPL;      // 1 024: v >> 2 sits in bits 0..7

struct SbsStepArgs {
  const float* logits; int V;                   // the step's logits, one row per running candidate (compact order)
  const int* slot_of; const uint8_t* finished; const float* phi; const float* g;   // [n_cand]
  const int* gen; int ld; int width;            // current rows [n_cand, ld], `width` tokens each
  int B, beam, K, pad, eos;
  const int64_t* row_keys;                      // [B] or null: keys 0 .. B-1
  unsigned long long seed; int pos; float inv_T;
  int64_t* new_cand; float* new_phi; float* new_g; int* parent; int* new_len; uint8_t* new_finished; int* parent_draft;
  int* summary;                                 // [0] += new candidates that are finished
  int* tr_parent; int* tr_token; float* tr_phi; float* tr_g;   // this level's trace [B, K] (all null: no trace)
  // k_sbs_step_masked only (k_sbs_step reads none of them)
  int top_k; float top_p;                       // top_k 0: filter off (then top_p is 1); else 1..32
  PrefixTab pfx;                                // by source (tok null: no forced prefixes)
};

// All four words of Philox4x32-10 (the constants and the round of philox4x32_10_word0).
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&w)[4]) {
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// 23 bits + a half, times 2^-23: exact, strictly inside (0, 1).
__device__ __forceinline__ float sbs_uniform(unsigned w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// lp_v of step 2 from the row's logit: the one expression both the image and the winners' phi' are formed with.
__device__ __forceinline__ float sbs_logprob(float x, float inv_T, float m, float logz) { return (__fmul_rn(x, inv_T) - m) - logz; }

__global__ __launch_bounds__(256) void k_sbs_step(SbsStepArgs a) {
  extern __shared__ float img[];                // [beam * V]
  __shared__ float s_m[SBS_MAX_BEAM], s_logz[SBS_MAX_BEAM];
  __shared__ float s_best[4];
  __shared__ int s_bi[4];
  __shared__ int s_sel;
  const int b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long key = a.row_keys ? (unsigned long long)a.row_keys[b] : (unsigned long long)b;
  const float qnan = __int_as_float(0x7fc00000);
  for (int k = wave; k < a.beam; k += 4) {
    const int c = b * a.beam + k;
    float* im = img + (size_t)k * a.V;
    const float Gk = a.g[c];
    if (a.finished[c]) {
      for (int v = lane; v < a.V; v += 64) im[v] = (v == a.pad) ? Gk : qnan;
      continue;
    }
    const float* row = a.logits + (size_t)a.slot_of[c] * a.V;
    float m = -INFINITY;
    for (int v0 = 4 * lane; v0 < a.V; v0 += 256)
      for (int i = 0; i < 4 && v0 + i < a.V; ++i) m = fmaxf(m, __fmul_rn(row[v0 + i], a.inv_T));
    m = wave_max(m);
    float z = 0.f;
    for (int v0 = 4 * lane; v0 < a.V; v0 += 256)
      for (int i = 0; i < 4 && v0 + i < a.V; ++i) z += expf(__fmul_rn(row[v0 + i], a.inv_T) - m);
    z = wave_sum(z);
    const float logz = logf(z);
    const float phik = a.phi[c];
    float Z = -INFINITY;
    for (int v0 = 4 * lane; v0 < a.V; v0 += 256) {
      unsigned w[4];
      philox4x32_10((unsigned)key, (unsigned)(key >> 32), 0x80000000u | ((unsigned)k << 8) | (unsigned)(v0 >> 2), (unsigned)a.pos,
                    (unsigned)a.seed, (unsigned)(a.seed >> 32), w);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (v0 + i < a.V) {
          const float phic = phik + sbs_logprob(row[v0 + i], a.inv_T, m, logz);
          const float gv = phic - logf(-logf(sbs_uniform(w[i])));
          im[v0 + i] = gv;
          Z = fmaxf(Z, gv);
        }
      }
    }
    Z = wave_max(Z);
    for (int v0 = 4 * lane; v0 < a.V; v0 += 256)      // every lane converts the ids it wrote itself
      for (int i = 0; i < 4 && v0 + i < a.V; ++i) {
        const float gv = im[v0 + i];
        float Gc = Gk;
        if (!(gv == Z)) {
          const float t = (Gk - gv) + log1pf(-expf(gv - Z));
          Gc = Gk - fmaxf(t, 0.f) - log1pf(expf(-fabsf(t)));
        }
        im[v0 + i] = Gc;
      }
    if (lane == 0) { s_m[k] = m; s_logz[k] = logz; }
  }
  __syncthreads();
  const int n = a.beam * a.V;
  for (int r = 0; r < a.K; ++r) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256) {
      const float v = img[i];
      if (v > best || (v == best && i < bi)) { best = v; bi = i; }   // -inf children stay selectable; NaN loses
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { s_best[wave] = best; s_bi[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      int sel = s_bi[0];
      float bv = s_best[0];
      for (int w = 1; w < 4; ++w)
        if (s_best[w] > bv || (s_best[w] == bv && s_bi[w] < sel)) { sel = s_bi[w]; bv = s_best[w]; }
      if (sel == 0x7fffffff) sel = 0;           // no child left (outside the contract): keep the indexing in range
      s_sel = sel;
    }
    __syncthreads();
    const int sel = s_sel;
    const int k = sel / a.V, tok = sel % a.V;
    const int c = b * a.beam + k, out = b * a.K + r;
    const int* root = a.gen + (size_t)c * a.ld;
    int64_t* dst = a.new_cand + (size_t)out * a.ld;
    for (int col = threadIdx.x; col < a.ld; col += 256) dst[col] = col < a.width ? (int64_t)root[col] : (col == a.width ? (int64_t)tok : (int64_t)a.pad);
    if (threadIdx.x == 0) {
      const bool pfin = a.finished[c] != 0;
      const float Gc = img[sel];
      const float phic = pfin ? a.phi[c] : a.phi[c] + sbs_logprob(a.logits[(size_t)a.slot_of[c] * a.V + tok], a.inv_T, s_m[k], s_logz[k]);
      a.new_phi[out] = phic;
      a.new_g[out] = Gc;
      a.parent[out] = c;
      a.parent_draft[out] = 0;
      a.new_len[out] = a.width + 1;
      const bool fin = pfin || tok == a.eos || tok == a.pad || Gc == -INFINITY;
      a.new_finished[out] = fin ? 1 : 0;
      if (fin) atomicAdd(&a.summary[0], 1);
      if (a.tr_parent) {
        a.tr_parent[out] = k; a.tr_token[out] = tok; a.tr_phi[out] = phic; a.tr_g[out] = Gc;
      }
      img[sel] = qnan;
    }
    __syncthreads();
  }
}

// Row b of a prefix table by source: source b's own row.
__global__ void k_sbs_prefix_src(int* src, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) src[b] = b;
}

constexpr int SBS_MASKED_MAX_WAVES = 16;

// k_sbs_step behind a per-parent token mask (see the head of this file).  blockDim.x = 64 * waves, waves in {4, 8, 16}.
template <int VPL>
__global__ __launch_bounds__(64 * SBS_MASKED_MAX_WAVES) void k_sbs_step_masked(SbsStepArgs a) {
  extern __shared__ float img[];                // [beam * V]
  __shared__ float s_m[SBS_MAX_BEAM], s_logz[SBS_MAX_BEAM];
  __shared__ int s_forced[SBS_MAX_BEAM];        // the forced token of a parent at a forced position, else -1
  __shared__ float s_best[SBS_MASKED_MAX_WAVES];
  __shared__ int s_bi[SBS_MASKED_MAX_WAVES];
  __shared__ int s_sel;
  const int b = blockIdx.x;
  const int nthr = blockDim.x, nw = nthr >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long key = a.row_keys ? (unsigned long long)a.row_keys[b] : (unsigned long long)b;
  const float qnan = __int_as_float(0x7fc00000);
  const bool forced = a.pfx.tok && a.pos <= a.pfx.len[b];                       // workgroup-uniform
  const int ftok = forced ? prefix_token(a.pfx, b, a.pos, a.V) : -1;
  for (int k = wave; k < a.beam; k += nw) {
    const int c = b * a.beam + k;
    float* im = img + (size_t)k * a.V;
    const float Gk = a.g[c];
    if (a.finished[c]) {
      for (int v = lane; v < a.V; v += 64) im[v] = (v == a.pad) ? Gk : qnan;
      if (lane == 0) s_forced[k] = -1;
      continue;
    }
    if (forced) {
      for (int v = lane; v < a.V; v += 64) im[v] = (v == ftok) ? Gk : -INFINITY;
      if (lane == 0) s_forced[k] = ftok;
      continue;
    }
    const float* row = a.logits + (size_t)a.slot_of[c] * a.V;
    // the kept set as the walk owns it: bit 4 * j + i of `keep` is id 256 * j + 4 * lane + i
    unsigned keep = 0xffffu;
    if (a.top_k > 0) {
      int my_idx, n_kept;
      float my_val, m_top;
      sample_topk_to_lanes<VPL>(row, a.V, a.inv_T, a.top_p, a.top_k, lane, my_idx, my_val, n_kept, m_top);
      if (n_kept <= 1) {                        // wave-uniform.  A mask of one token, as a forced position is: y - m = 0, z = 1, lp = 0
        const int only = __shfl(my_idx, 0, 64);  // and g == Z, so phi' = phi_k and G' = G_k on the bits, with no walk and no noise
        for (int v = lane; v < a.V; v += 64) im[v] = (v == only) ? Gk : -INFINITY;      // (no finite logit at all: every child -inf)
        if (lane == 0) s_forced[k] = only;
        continue;
      }
      keep = 0u;
      for (int r = 0; r < n_kept; ++r) {
        const int id = __shfl(my_idx, r, 64);
        if (((id & 255) >> 2) == lane) keep |= 1u << (((id >> 8) << 2) | (id & 3));
      }
    }
    float m = -INFINITY;
    for (int v0 = 4 * lane, j = 0; v0 < a.V; v0 += 256, ++j)
      for (int i = 0; i < 4 && v0 + i < a.V; ++i)
        m = fmaxf(m, (keep >> (4 * j + i) & 1u) ? __fmul_rn(row[v0 + i], a.inv_T) : -INFINITY);
    m = wave_max(m);
    float z = 0.f;
    for (int v0 = 4 * lane, j = 0; v0 < a.V; v0 += 256, ++j)
      for (int i = 0; i < 4 && v0 + i < a.V; ++i)
        z += (keep >> (4 * j + i) & 1u) ? expf(__fmul_rn(row[v0 + i], a.inv_T) - m) : 0.f;   // k_sbs_step's own expression on a kept id
    z = wave_sum(z);
    const float logz = logf(z);
    const float phik = a.phi[c];
    float Z = -INFINITY;
    for (int v0 = 4 * lane, j = 0; v0 < a.V; v0 += 256, ++j) {
      const unsigned kb = (keep >> (4 * j)) & 15u;
      if (kb == 0u) {                           // no kept id among the four: -inf children, and no Philox block is needed
        for (int i = 0; i < 4 && v0 + i < a.V; ++i) im[v0 + i] = -INFINITY;
        continue;
      }
      unsigned w[4];
      philox4x32_10((unsigned)key, (unsigned)(key >> 32), 0x80000000u | ((unsigned)k << 8) | (unsigned)(v0 >> 2), (unsigned)a.pos,
                    (unsigned)a.seed, (unsigned)(a.seed >> 32), w);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (v0 + i < a.V) {
          float gv = -INFINITY;
          if (kb >> i & 1u) {
            const float phic = phik + sbs_logprob(row[v0 + i], a.inv_T, m, logz);
            gv = phic - logf(-logf(sbs_uniform(w[i])));
          }
          im[v0 + i] = gv;
          Z = fmaxf(Z, gv);
        }
      }
    }
    Z = wave_max(Z);
    for (int v0 = 4 * lane; v0 < a.V; v0 += 256)      // every lane converts the ids it wrote itself
      for (int i = 0; i < 4 && v0 + i < a.V; ++i) {
        const float gv = im[v0 + i];
        float Gc = Gk;
        if (!(gv == Z)) {
          const float t = (Gk - gv) + log1pf(-expf(gv - Z));
          Gc = Gk - fmaxf(t, 0.f) - log1pf(expf(-fabsf(t)));
        }
        im[v0 + i] = Gc;
      }
    if (lane == 0) { s_m[k] = m; s_logz[k] = logz; s_forced[k] = -1; }
  }
  __syncthreads();
  const int n = a.beam * a.V;
  for (int r = 0; r < a.K; ++r) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += nthr) {
      const float v = img[i];
      if (v > best || (v == best && i < bi)) { best = v; bi = i; }   // -inf children stay selectable; NaN loses
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { s_best[wave] = best; s_bi[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      int sel = s_bi[0];
      float bv = s_best[0];
      for (int w = 1; w < nw; ++w)
        if (s_best[w] > bv || (s_best[w] == bv && s_bi[w] < sel)) { sel = s_bi[w]; bv = s_best[w]; }
      if (sel == 0x7fffffff) sel = 0;           // no child left (outside the contract): keep the indexing in range
      s_sel = sel;
    }
    __syncthreads();
    const int sel = s_sel;
    const int k = sel / a.V, tok = sel % a.V;
    const int c = b * a.beam + k, out = b * a.K + r;
    const int* root = a.gen + (size_t)c * a.ld;
    int64_t* dst = a.new_cand + (size_t)out * a.ld;
    for (int col = threadIdx.x; col < a.ld; col += nthr) dst[col] = col < a.width ? (int64_t)root[col] : (col == a.width ? (int64_t)tok : (int64_t)a.pad);
    if (threadIdx.x == 0) {
      const bool pfin = a.finished[c] != 0;
      const float Gc = img[sel];
      float phic;
      if (pfin) phic = a.phi[c];
      else if (s_forced[k] >= 0) phic = (tok == s_forced[k]) ? a.phi[c] : -INFINITY;
      else if (Gc == -INFINITY) phic = -INFINITY;       // a masked child (or a -inf logit): its logit says nothing about lp
      else phic = a.phi[c] + sbs_logprob(a.logits[(size_t)a.slot_of[c] * a.V + tok], a.inv_T, s_m[k], s_logz[k]);
      a.new_phi[out] = phic;
      a.new_g[out] = Gc;
      a.parent[out] = c;
      a.parent_draft[out] = 0;
      a.new_len[out] = a.width + 1;
      const bool fin = pfin || tok == a.eos || tok == a.pad || Gc == -INFINITY;
      a.new_finished[out] = fin ? 1 : 0;
      if (fin) atomicAdd(&a.summary[0], 1);
      if (a.tr_parent) {
        a.tr_parent[out] = k; a.tr_token[out] = tok; a.tr_phi[out] = phic; a.tr_g[out] = Gc;
      }
      img[sel] = qnan;
    }
    __syncthreads();
  }
}

}  // namespace ttx
