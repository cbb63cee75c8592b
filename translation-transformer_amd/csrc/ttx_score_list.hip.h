// Length-bucketed scoring of a LIST of (src, hyp) batches (included by ttx_api.hip only): the three kernels around the teacher-forced
// pass of ttx_score_hypotheses.  Hand-written HIP for gfx950, wave64.  The batches of a list are read through a descriptor table on
// the device (SlBatch, one entry per batch, uploaded once per call), so the host issues no per-batch work.
//   k_sl_extents  one wave per row of the list.  A hypothesis row: n by k_hyp_score's rule (the column of the first EOS at a column
//                 >= 1, else the last column >= 1 holding a non-PAD token, else 0) and atomicMax(e[s], max(2, 1 + n)) into its
//                 source's entry (e is zeroed before the launch; a maximum of integers does not depend on the order).  A source
//                 row: ls[s] = max(1, 1 + its last non-PAD column).  Both kinds of row also check every token id they own, over the
//                 whole given width, against the vocabulary (bad[0] |= 1 for a source id, 2 for a hypothesis id): the call's one
//                 read-back then carries what torch.nn.Embedding would have raised on.
//   k_sl_pack     one wave per row of a chunk: the first min(own width, chunk width) columns of the selected source / hypothesis row,
//                 PAD up to the chunk width.  16-byte copies when both row starts are 16-byte aligned, 8-byte ones otherwise.
//   k_sl_unpack   one wave per hypothesis row of a chunk: score, length, finished and (optionally) the per-token values back to list
//                 order; a tok_logp row takes its first min(W_c, W_i) - 1 values and exact zeros up to W_i - 1.
// No kernel here touches a logit: the values are k_hyp_score's, on the packed rows.
#pragma once
#include "ttx_common.hip.h"

namespace ttx {

// One batch of the list as the kernels see it: the caller's ttx_score_batch and the batch's place in list order.
struct SlBatch {
  const int64_t* src;                     // [B, Ls]
  const int64_t* hyp;                     // [B*N] rows of stride ld_hyp, W columns read
  int B, Ls, N, W, ld_hyp;
  int src0;                               // sources of the batches before this one
  int row0;                               // hypothesis rows of the batches before this one
  int pad_;
  long long tok0;                         // this batch's offset into the ragged tok_logp output, in floats
};

// the batch that holds source s / hypothesis row r of the list: the last entry whose first source / row is <= the index
__device__ inline int sl_batch_of_src(const SlBatch* __restrict__ tab, int nb, int s) {
  int lo = 0, hi = nb - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].src0 <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ inline int sl_batch_of_row(const SlBatch* __restrict__ tab, int nb, int r) {
  int lo = 0, hi = nb - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].row0 <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// e int32 [S] (zeroed by the caller), ls int32 [S], n_out int32 [R] or null, bad int32 [1] (zeroed by the caller) or null.
// Rows 0 .. R-1 are the list's hypothesis rows, R .. R+S-1 its sources.  4 rows per workgroup.
__global__ __launch_bounds__(256) void k_sl_extents(const SlBatch* __restrict__ tab, int nb, int S, int R, int Vs, int Vt, int pad, int eos,
                                                    int* e, int* __restrict__ ls, int* __restrict__ n_out, int* bad) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= R + S) return;                 // wave-uniform
  if (g < R) {
    const int i = sl_batch_of_row(tab, nb, g);
    const SlBatch t = tab[i];
    const int lr = g - t.row0;
    const int64_t* h = t.hyp + (size_t)lr * t.ld_hyp;
    int n = 0;
    bool done = false, oob = false;
    for (int base = 0; base < t.W; base += 64) {
      const int c = base + lane;
      const bool in = c < t.W;
      const int64_t tv = in ? h[c] : (int64_t)pad;
      oob |= in && (tv < 0 || tv >= Vt);
      if (!done) {                        // wave-uniform
        const unsigned long long emask = __ballot(in && c >= 1 && tv == eos);
        if (emask) {                      // the first EOS ends the hypothesis
          n = base + __ffsll((long long)emask) - 1;
          done = true;
        } else {
          const unsigned long long tmask = __ballot(in && c >= 1 && tv != pad);
          if (tmask) n = base + 63 - __clzll((long long)tmask);
        }
      }
    }
    const bool any_oob = __ballot(oob) != 0ull;
    if (lane == 0) {
      if (n_out) n_out[g] = n;
      atomicMax(&e[t.src0 + lr / t.N], n + 1 > 2 ? n + 1 : 2);
      if (bad && any_oob) atomicOr(bad, 2);
    }
  } else {
    const int s = g - R;
    const int i = sl_batch_of_src(tab, nb, s);
    const SlBatch t = tab[i];
    const int64_t* x = t.src + (size_t)(s - t.src0) * t.Ls;
    int last = -1;
    bool oob = false;
    for (int base = 0; base < t.Ls; base += 64) {
      const int c = base + lane;
      const bool in = c < t.Ls;
      const int64_t tv = in ? x[c] : (int64_t)pad;
      oob |= in && (tv < 0 || tv >= Vs);
      const unsigned long long tmask = __ballot(in && tv != pad);
      if (tmask) last = base + 63 - __clzll((long long)tmask);
    }
    const bool any_oob = __ballot(oob) != 0ull;
    if (lane == 0) {
      ls[s] = last + 1 > 1 ? last + 1 : 1;
      if (bad && any_oob) atomicOr(bad, 1);
    }
  }
}

// ncopy columns of `from`, then PAD up to `width`, by one wave.  Pairs of columns move as 16 bytes when both rows start on 16 bytes.
__device__ inline void sl_copy_row(const int64_t* from, int ncopy, int64_t* dst, int width, int64_t pad, int lane) {
  const bool vec = ((reinterpret_cast<uintptr_t>(from) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;   // wave-uniform
  int done = 0;
  if (vec) {
    const int pairs = ncopy >> 1;
    for (int p = lane; p < pairs; p += 64) reinterpret_cast<longlong2*>(dst)[p] = reinterpret_cast<const longlong2*>(from)[p];
    done = pairs * 2;
  }
  for (int c = done + lane; c < ncopy; c += 64) dst[c] = from[c];
  for (int c = ncopy + lane; c < width; c += 64) dst[c] = pad;
}

// sel int32 [Bc]: the chunk's sources (indices in list order), every one of a batch with N rows per source.
// src_c int64 [Bc, Lsc]; hyp_c int64 [Bc*N, Wc].  Rows 0 .. Bc-1 are the sources, Bc .. Bc + Bc*N - 1 the hypotheses.
__global__ __launch_bounds__(256) void k_sl_pack(const SlBatch* __restrict__ tab, int nb, const int* __restrict__ sel, int Bc, int N, int Wc,
                                                 int Lsc, int pad, int64_t* __restrict__ src_c, int64_t* __restrict__ hyp_c) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= Bc + Bc * N) return;           // wave-uniform
  const int rr = g - Bc;                  // hypothesis row of the chunk when >= 0
  const int j = g < Bc ? g : rr / N;
  const int s = sel[j];
  const SlBatch t = tab[sl_batch_of_src(tab, nb, s)];
  const int b = s - t.src0;
  if (g < Bc) {
    sl_copy_row(t.src + (size_t)b * t.Ls, t.Ls < Lsc ? t.Ls : Lsc, src_c + (size_t)j * Lsc, Lsc, (int64_t)pad, lane);
  } else {
    const int k = rr - j * N;
    sl_copy_row(t.hyp + ((size_t)b * N + k) * t.ld_hyp, t.W < Wc ? t.W : Wc, hyp_c + (size_t)rr * Wc, Wc, (int64_t)pad, lane);
  }
}

// The chunk's results (score_c fp32, length_c int32, fin_c u8 [Bc*N]; tok_c fp32 [Bc*N, Wc-1]) to list order: score / length /
// finished [R], tok (or null) ragged, batch i at tok0[i] with rows of W_i - 1 floats.
__global__ __launch_bounds__(256) void k_sl_unpack(const SlBatch* __restrict__ tab, int nb, const int* __restrict__ sel, int Bc, int N, int Wc,
                                                   const float* __restrict__ score_c, const int* __restrict__ length_c,
                                                   const uint8_t* __restrict__ fin_c, const float* __restrict__ tok_c,
                                                   float* __restrict__ score, int* __restrict__ length, uint8_t* __restrict__ finished,
                                                   float* __restrict__ tok) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= Bc * N) return;                // wave-uniform
  const int j = g / N, k = g - j * N;
  const int s = sel[j];
  const SlBatch t = tab[sl_batch_of_src(tab, nb, s)];
  const size_t lr = (size_t)(s - t.src0) * N + k;
  if (lane == 0) {
    score[t.row0 + lr] = score_c[g];
    length[t.row0 + lr] = length_c[g];
    if (finished) finished[t.row0 + lr] = fin_c[g];
  }
  if (tok) {
    const int Ti = t.W - 1;
    const int ncopy = (t.W < Wc ? t.W : Wc) - 1;
    const float* from = tok_c + (size_t)g * (Wc - 1);
    float* dst = tok + t.tok0 + lr * Ti;
    for (int c = lane; c < ncopy; c += 64) dst[c] = from[c];
    for (int c = ncopy + lane; c < Ti; c += 64) dst[c] = 0.0f;
  }
}

}  // namespace ttx
