// Folding sampled hypotheses (included by ttx_api.hip only): the N rows of every source reduced to their distinct hypotheses,
// counted and ranked, on the device.  Hand-written HIP for gfx950, wave64.  The rule is the contract of ttx_fold_hypotheses in
// include/ttx.h; in short, for row j of a source: c_j = (column of the first EOS in [0, W)) + 1, or W without an EOS (the row is
// unfinished); rows i and j are one hypothesis iff c_i == c_j and their 64-bit tokens agree on [0, c); first[j] is the smallest
// such i <= j; the rows with first[j] == j are the representatives, counted and ordered by the comparator of fold_precedes.
// ONE launch of k_fold_hyps, one workgroup of four waves per source: nothing crosses a source, no float is ever added by an
// atomic, and the only atomics are integer counts in LDS, whose result does not depend on the order.  Two calls on the same
// inputs give the same bits, at any B.
//   phase 1  one wave per row (rows strided by 4): c_j by a ballot over the EOS hits, and a 64-bit filter word: the integer sum
//            over the compared columns of a position-keyed mix of the token, so the lanes can add in any order
//   phase 2  one wave per row j: lane l tests candidate i = base + l < j on (c, filter), 64 at a time; the set bits of the ballot
//            are confirmed in ascending i by a lane-strided comparison of the tokens themselves (the source's rows were just read
//            and sit in L2).  Equality NEVER rests on the filter word: it only spares comparisons that cannot succeed
//   phase 3  integer counts per representative (LDS atomics), the representatives compacted in index order by wave 0, and the
//            rank of each = the number of representatives that precede it: O(U^2) comparisons per source out of LDS
//   phase 4  scatter by rank, gather the rows into `out` (16-byte accesses where the rows allow it), logmass in rank order
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ttx.h"

namespace ttx {

constexpr int FOLD_THREADS = 256;         // k_fold_hyps: four waves per source
constexpr int FOLD_MAX_N = 1024;          // rows per source: the LDS arrays below are sized by it (36 KB in all)

struct FoldArgs {
  const int64_t* hyp;                     // B*N rows of stride ld_hyp, W columns read
  const float* score_in;                  // [B, N] or null
  int32_t* first;                         // [B, N] by sample, or null
  int32_t* rank_of;                       // [B, N] by sample, or null
  int32_t* n_unique;                      // [B], or null
  int32_t* perm;                          // [B, N] by rank, or null
  int32_t* count;                         // [B, N] by rank, or null
  float* score;                           // [B, N] by rank, or null
  int64_t* out;                           // [B, N, W] packed, by rank, or null
  float* logmass;                         // [B], or null (needs score_in)
  int N, W, ld_hyp, pad, eos, order, flags;
};

// splitmix64's finaliser over the token keyed by its column: equal rows give equal sums whatever the order of the additions
__device__ __forceinline__ uint64_t fold_mix(int64_t tok, int col) {
  uint64_t x = (uint64_t)tok + (uint64_t)(col + 1) * 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// does representative a precede representative b (a != b)?  cf = (c << 1) | finished; scores hold no NaN (read as -inf)
__device__ __forceinline__ bool fold_precedes(int a, int b, const int* cf, const int* cnt, const float* sc, int order, bool unf_last,
                                              bool has_scores) {
  if (unf_last) {
    const int fa = cf[a] & 1, fb = cf[b] & 1;
    if (fa != fb) return fa != 0;
  }
  if (order == TTX_FOLD_COUNT) {
    const int ca = cnt[a], cb = cnt[b];
    if (ca != cb) return ca > cb;
  }
  if (order == TTX_FOLD_SCORE || (order == TTX_FOLD_COUNT && has_scores)) {
    const float sa = sc[a], sb = sc[b];
    if (sa > sb) return true;
    if (sa < sb) return false;            // neither: equal under IEEE (-0.0 == 0.0, -inf == -inf)
  }
  return a < b;
}

template <bool VEC2>
__global__ __launch_bounds__(FOLD_THREADS) void k_fold_hyps(const FoldArgs a) {
  constexpr int NW = FOLD_THREADS / 64;
  __shared__ int s_cf[FOLD_MAX_N];        // (c_j << 1) | finished
  __shared__ uint64_t s_filter[FOLD_MAX_N];   // the filter word; after phase 2 the exp terms of logmass (double) by rank
  __shared__ int s_first[FOLD_MAX_N];
  __shared__ int s_count[FOLD_MAX_N];     // by sample index: the count of a representative
  __shared__ float s_score[FOLD_MAX_N];   // by sample index, NaN read as -inf (all -inf without scores)
  __shared__ int s_rep[FOLD_MAX_N];       // the representatives in index order, U of them
  __shared__ int s_rank[FOLD_MAX_N];      // by sample index: the rank of a representative
  __shared__ int s_perm[FOLD_MAX_N];      // rank -> sample index
  __shared__ int s_U;
  const int N = a.N, W = a.W;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t* rows = a.hyp + (size_t)b * N * a.ld_hyp;
  const bool has_scores = a.score_in != nullptr;
  const bool no_filter = (a.flags & TTX_FOLD_DEBUG_NO_FILTER) != 0;
  const bool unf_last = (a.flags & TTX_FOLD_UNFINISHED_LAST) != 0;
  const int64_t eos = (int64_t)a.eos;

  // ---- phase 1: c_j, finished, the filter word; the scores ----
  for (int j = tid; j < N; j += FOLD_THREADS) {
    float s = -INFINITY;
    if (has_scores) {
      s = a.score_in[(size_t)b * N + j];
      if (s != s) s = -INFINITY;
    }
    s_score[j] = s;
    s_count[j] = 0;
  }
  for (int j = w; j < N; j += NW) {
    const int64_t* h = rows + (size_t)j * a.ld_hyp;
    uint64_t f = 0;
    int c = W, fin = 0;
    for (int base = 0; base < W; base += 64) {
      const int col = base + lane;
      const int64_t tv = (col < W) ? h[col] : 0;
      const unsigned long long emask = __ballot(col < W && tv == eos);
      int lim = W;                        // compared columns of this chunk: col < lim
      if (emask) {                        // wave-uniform: what follows the first EOS is never read
        c = base + __ffsll((long long)emask);
        fin = 1;
        lim = c;
      }
      if (col < lim) f += fold_mix(tv, col);
      if (emask) break;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) f += __shfl_xor(f, o, 64);      // integer sum: any order
    if (lane == 0) {
      s_cf[j] = (c << 1) | fin;
      s_filter[j] = no_filter ? 0ull : f;
    }
  }
  __syncthreads();

  // ---- phase 2: first[j] ----
  for (int j = w; j < N; j += NW) {
    const int cfj = s_cf[j];
    const uint64_t fj = s_filter[j];
    const int c = cfj >> 1;
    const int64_t* hj = rows + (size_t)j * a.ld_hyp;
    int first = j;
    for (int base = 0; base < j && first == j; base += 64) {
      const int i = base + lane;
      unsigned long long mask = __ballot(i < j && s_cf[i] == cfj && s_filter[i] == fj);
      while (mask) {                      // wave-uniform: candidates in ascending i, each confirmed on its tokens
        const int i0 = base + __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const int64_t* hi = rows + (size_t)i0 * a.ld_hyp;
        bool same = true;
        for (int cb = 0; cb < c; cb += 64) {
          const int col = cb + lane;
          const bool differ = col < c && hi[col] != hj[col];
          if (__ballot(differ)) {
            same = false;
            break;
          }
        }
        if (same) {
          first = i0;
          break;
        }
      }
    }
    if (lane == 0) {
      s_first[j] = first;
      atomicAdd(&s_count[first], 1);      // phase 3's counts: integers in LDS, the order does not matter
    }
  }
  __syncthreads();

  // ---- phase 3: the representatives in index order, then their ranks ----
  if (w == 0) {
    int U = 0;
    for (int base = 0; base < N; base += 64) {
      const int j = base + lane;
      const bool rep = j < N && s_first[j] == j;
      const unsigned long long m = __ballot(rep);
      if (rep) s_rep[U + __popcll(m & ((1ull << lane) - 1ull))] = j;
      U += __popcll(m);
    }
    if (lane == 0) s_U = U;
  }
  __syncthreads();
  const int U = s_U;
  for (int t = tid; t < U; t += FOLD_THREADS) {
    const int me = s_rep[t];
    int r = 0;
    for (int u = 0; u < U; ++u) {
      const int other = s_rep[u];         // one address per wave: an LDS broadcast
      if (other != me && fold_precedes(other, me, s_cf, s_count, s_score, a.order, unf_last, has_scores)) ++r;
    }
    s_rank[me] = r;
    s_perm[r] = me;
  }
  __syncthreads();

  // ---- phase 4: the outputs, every element of every one written ----
  const size_t o = (size_t)b * N;
  if (tid == 0 && a.n_unique) a.n_unique[b] = U;
  for (int j = tid; j < N; j += FOLD_THREADS) {
    if (a.first) a.first[o + j] = s_first[j];
    if (a.rank_of) a.rank_of[o + j] = s_rank[s_first[j]];
    const int src = j < U ? s_perm[j] : -1;                            // j as a rank from here on
    if (a.perm) a.perm[o + j] = src;
    if (a.count) a.count[o + j] = src >= 0 ? s_count[src] : 0;
    if (a.score) a.score[o + j] = (src >= 0 && has_scores) ? s_score[src] : -INFINITY;
  }
  if (a.out) {
    for (int r = w; r < N; r += NW) {
      int64_t* dst = a.out + (o + r) * (size_t)W;
      if (r < U) {
        const int64_t* src = rows + (size_t)s_perm[r] * a.ld_hyp;
        if constexpr (VEC2) {             // W and ld_hyp even, both bases 16-byte aligned: every row starts on 16 bytes
          for (int col = lane * 2; col < W; col += 128)
            *reinterpret_cast<longlong2*>(dst + col) = *reinterpret_cast<const longlong2*>(src + col);
        } else {
          for (int col = lane; col < W; col += 64) dst[col] = src[col];
        }
      } else {
        if constexpr (VEC2) {
          const longlong2 p2 = make_longlong2((long long)a.pad, (long long)a.pad);
          for (int col = lane * 2; col < W; col += 128) *reinterpret_cast<longlong2*>(dst + col) = p2;
        } else {
          for (int col = lane; col < W; col += 64) dst[col] = (int64_t)a.pad;
        }
      }
    }
  }
  if (a.logmass) {
    // m = the largest representative score; the terms exp(s_r - m) by all threads, their sum by thread 0 in rank order
    float m = -INFINITY;
    for (int u = 0; u < U; ++u) m = fmaxf(m, s_score[s_rep[u]]);      // every thread the same value (LDS broadcasts)
    double* term = reinterpret_cast<double*>(s_filter);               // the filter words are dead since phase 2
    for (int r = tid; r < U; r += FOLD_THREADS) term[r] = exp((double)s_score[s_perm[r]] - (double)m);
    __syncthreads();
    if (tid == 0) {
      float lm = -INFINITY;
      if (m != -INFINITY) {
        double acc = 0.0;
        for (int r = 0; r < U; ++r) acc += term[r];
        lm = (float)((double)m + log(acc));
      }
      a.logmass[b] = lm;
    }
  }
}

}  // namespace ttx
