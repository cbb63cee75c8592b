// Cross-attention maps of hypotheses (included by ttx_api.hip only): the normalised attention probabilities that the attention
// kernels form and drop.  Hand-written HIP for gfx950, wave64, VALU (DESIGN §14 says why not MFMA).
//   P[r,h,t,j] = softmax_j(scale * q[r,t,h,:] . k[b,j,h,:]) over the keys j of memory row b = mem_row[r] with key_pad[b,j] == 0
//   M[r,t,j]   = (P[r,0,t,j] + P[r,1,t,j] + ... in ascending h, fp32) / (float)H
//   A[r,t]     = the smallest j with M[r,t,j] == max_j M[r,t,:]
// Query position t of row r is live iff t < length[r].  PAD keys and positions that are not live are exactly 0.0 (A = -1); a live
// position whose keys are all PAD is all zeros (A = 0).
//   k_hyp_length   length[r] from the tokens: the row scan of k_hyp_score, one wave per row
//   k_attn_probs   one workgroup per (row, tile of AP_TQ query positions), heads in ascending order.  Per head: the waves share
//                  the 64-key slots; a lane holds ONE key row in registers (read once per workgroup) and takes its dot product with
//                  the AP_TQ staged queries; then one wave per query row runs the softmax with lane = j % 64, slot = j / 64: the
//                  order of every sum is a function of the key index alone, so key columns appended as PAD add only + 0.0f terms
//                  and change no bit; p = e * (1 / sum) then touches each element alone.  Head sums stay in LDS, each element
//                  owned by one lane: no atomics, no second pass.
#pragma once
#include "ttx_common.hip.h"

namespace ttx {

constexpr int AP_THREADS = 256;           // 4 waves
constexpr int AP_TQ = 16;                 // query positions per workgroup
constexpr int AP_MAX_KEYS = 1024;         // 2 * AP_TQ * 1024 * 4 B of scores and head sums + the queries: 132 KiB of 160 KiB LDS

__host__ __device__ inline int ap_padded_keys(int Ls) { return (Ls + 63) & ~63; }
// dynamic LDS of one workgroup: scores [AP_TQ, LsP], head sums [AP_TQ, LsP] (when the mean or the alignment is wanted), the query
// tile [AP_TQ, DH], the key mask [LsP] (u8)
inline size_t ap_lds_bytes(int Ls, int head_dim, bool want_mean) {
  const size_t LsP = (size_t)ap_padded_keys(Ls);
  return ((want_mean ? 2 : 1) * AP_TQ * LsP + (size_t)AP_TQ * head_dim) * sizeof(float) + LsP;
}

// hyp int64 rows of stride ld_hyp, W columns read; length int32 [R]: the column of the first EOS at a column >= 1, else the last
// column >= 1 holding a non-PAD token, else 0.  One wave per row, 4 rows per workgroup.
__global__ __launch_bounds__(256) void k_hyp_length(const int64_t* __restrict__ hyp, int ld_hyp, int R, int W, int pad, int eos,
                                                    int* __restrict__ length) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;                     // wave-uniform
  const int64_t* h = hyp + (size_t)r * ld_hyp;
  int n = 0;
  for (int base = 1; base < W; base += 64) {
    const int c = base + lane;
    const int64_t tv = (c < W) ? h[c] : (int64_t)pad;
    const unsigned long long emask = __ballot(c < W && tv == eos);
    if (emask) {                          // wave-uniform: the first EOS ends the hypothesis
      n = base + __ffsll((long long)emask) - 1;
      break;
    }
    const unsigned long long tmask = __ballot(c < W && tv != pad);
    if (tmask) n = base + 63 - __clzll((long long)tmask);
  }
  if (lane == 0) length[r] = n;
}

struct AttnProbsArgs {
  const float* q;                         // [R*T, ldq], head h at columns h*DH ..
  const float* k;                         // [Rm*Ls, ldkv], head h at columns h*DH ..
  const uint8_t* key_pad;                 // [Rm*Ls], non-zero = PAD key
  const int* mem_row;                     // [R] or null (memory row r)
  const int* length;                      // [R]
  float* heads;                           // [R, H, T, Ls] or null
  float* mean;                            // [R, T, Ls] or null
  int* align;                             // [R, T] or null
  int ldq, ldkv, R, Rm, H, T, Ls;
  float scale;
};

// one output row of Ls floats from LDS (src) or zeros (src null), by one wave; VEC: 16-byte stores (Ls % 4 == 0, aligned base)
template <bool VEC>
__device__ inline void ap_store_row(float* __restrict__ dst, const float* src, int Ls, int lane) {
  if constexpr (VEC) {
    for (int j = lane * 4; j < Ls; j += 256) {
      const float4 v = src ? *reinterpret_cast<const float4*>(src + j) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      *reinterpret_cast<float4*>(dst + j) = v;
    }
  } else {
    for (int j = lane; j < Ls; j += 64) dst[j] = src ? src[j] : 0.0f;
  }
}

// one finished row by one wave: p = e * inv for the exponentials e in LDS; p is added to the head sums (msum; first: it starts
// them) and stored to dst (null: not wanted).  Every element is a function of its own e alone, so the two forms give the same bits.
template <bool VEC>
__device__ inline void ap_emit_row(float* __restrict__ dst, const float* e, float* msum, bool first, float inv, int Ls, int lane) {
  if constexpr (VEC) {
    for (int j = lane * 4; j < Ls; j += 256) {
      float4 v = *reinterpret_cast<const float4*>(e + j);
      v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
      if (msum) {
        float4 m = v;
        if (!first) {
          m = *reinterpret_cast<const float4*>(msum + j);
          m.x += v.x; m.y += v.y; m.z += v.z; m.w += v.w;
        }
        *reinterpret_cast<float4*>(msum + j) = m;
      }
      if (dst) *reinterpret_cast<float4*>(dst + j) = v;
    }
  } else {
    for (int j = lane; j < Ls; j += 64) {
      const float v = e[j] * inv;
      if (msum) msum[j] = first ? v : msum[j] + v;
      if (dst) dst[j] = v;
    }
  }
}

// VEC_OUT: heads / mean rows go out as float4 (the launch checks Ls % 4 == 0 and 16-byte aligned bases); VEC_K: key rows are read
// as float4 (ldkv % 4 == 0 and a 16-byte aligned base).
template <int DH, bool VEC_OUT, bool VEC_K>
__global__ __launch_bounds__(AP_THREADS) void k_attn_probs(const AttnProbsArgs a) {
  extern __shared__ __align__(16) unsigned char ap_smem[];
  constexpr int NW = AP_THREADS / 64;
  const int T = a.T, Ls = a.Ls, H = a.H;
  const int LsP = ap_padded_keys(Ls);
  const int nslot = LsP >> 6;
  const bool want_mean = a.mean != nullptr || a.align != nullptr;
  float* sc = reinterpret_cast<float*>(ap_smem);                    // [AP_TQ, LsP]
  float* macc = sc + (size_t)AP_TQ * LsP;                           // [AP_TQ, LsP] when want_mean
  float* qs = macc + (want_mean ? (size_t)AP_TQ * LsP : 0);         // [AP_TQ, DH]
  uint8_t* padm = reinterpret_cast<uint8_t*>(qs + AP_TQ * DH);      // [LsP]

  const int ntile = (T + AP_TQ - 1) / AP_TQ;
  const int r = blockIdx.x / ntile;
  const int t0 = (blockIdx.x - r * ntile) * AP_TQ;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (r >= a.R) return;
  int n = a.length[r];
  n = n < 0 ? 0 : (n > T ? T : n);
  const int b = a.mem_row ? a.mem_row[r] : r;
  const bool b_ok = (unsigned)b < (unsigned)a.Rm;                   // a row map outside the memory: every key counts as PAD
  const int tq = (T - t0 < AP_TQ) ? T - t0 : AP_TQ;                 // rows of this tile inside T
  const int nlive = (n - t0 < 0) ? 0 : (n - t0 < tq ? n - t0 : tq); // the live ones come first

  // rows that are not live: zeros and -1, by the kernel itself
  for (int qi = nlive + w; qi < tq; qi += NW) {
    const size_t t = (size_t)t0 + qi;
    if (a.heads)
      for (int h = 0; h < H; ++h) ap_store_row<VEC_OUT>(a.heads + (((size_t)r * H + h) * T + t) * Ls, nullptr, Ls, lane);
    if (a.mean) ap_store_row<VEC_OUT>(a.mean + ((size_t)r * T + t) * Ls, nullptr, Ls, lane);
    if (a.align && lane == 0) a.align[(size_t)r * T + t] = -1;
  }
  if (nlive == 0) return;                                           // workgroup-uniform

  for (int j = threadIdx.x; j < LsP; j += AP_THREADS)
    padm[j] = (j < Ls && b_ok) ? (a.key_pad[(size_t)b * Ls + j] != 0) : 1;

  for (int h = 0; h < H; ++h) {
    // the query tile of head h; rows that are not live read as zeros and are never used
    for (int i = threadIdx.x; i < AP_TQ * DH; i += AP_THREADS) {
      const int qi = i / DH, c = i - qi * DH;
      qs[i] = (qi < nlive) ? a.q[((size_t)r * T + t0 + qi) * a.ldq + h * DH + c] : 0.0f;
    }
    __syncthreads();                      // qs and padm written; the previous head's rows of sc are stored

    // scores: wave w takes key slots w, w + NW, ..; lane = key within the slot, its key row in registers
    for (int slot = w; slot < nslot; slot += NW) {
      const int j = slot * 64 + lane;
      float kr[DH];
      if (j < Ls && b_ok) {
        const float* kp = a.k + ((size_t)b * Ls + j) * a.ldkv + h * DH;
        if constexpr (VEC_K) {
#pragma unroll
          for (int c = 0; c < DH; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(kp + c);
            kr[c] = v.x; kr[c + 1] = v.y; kr[c + 2] = v.z; kr[c + 3] = v.w;
          }
        } else {
#pragma unroll
          for (int c = 0; c < DH; ++c) kr[c] = kp[c];
        }
      } else {
#pragma unroll
        for (int c = 0; c < DH; ++c) kr[c] = 0.0f;
      }
      for (int qi = 0; qi < nlive; ++qi) {
        const float4* qv = reinterpret_cast<const float4*>(qs + qi * DH);   // the same address in every lane: a broadcast
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
        for (int c = 0; c < DH; c += 4) {
          const float4 v = qv[c >> 2];
          a0 = fmaf(v.x, kr[c], a0);
          a1 = fmaf(v.y, kr[c + 1], a1);
          a2 = fmaf(v.z, kr[c + 2], a2);
          a3 = fmaf(v.w, kr[c + 3], a3);
        }
        sc[(size_t)qi * LsP + j] = (a0 + a1) + (a2 + a3);
      }
    }
    __syncthreads();

    // softmax: one wave per live query row; lane owns keys lane, lane + 64, ..
    float inv[AP_TQ / NW];                // 1 / sum of the rows this wave owns (row w + NW * i)
#pragma unroll
    for (int i = 0; i < AP_TQ / NW; ++i) {
      const int qi = w + NW * i;
      inv[i] = 0.0f;
      if (qi >= nlive) continue;          // wave-uniform
      float* srow = sc + (size_t)qi * LsP;
      float m = -INFINITY;
      for (int s = 0; s < nslot; ++s) {
        const int j = s * 64 + lane;
        const float x = srow[j] * a.scale;   // rounded once; the exponent below reads it back
        srow[j] = x;
        if (!padm[j]) m = fmaxf(m, x);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      float sum = 0.0f;
      for (int s = 0; s < nslot; ++s) {   // slots in ascending order, then a fixed butterfly: a function of j alone
        const int j = s * 64 + lane;
        const float e = padm[j] ? 0.0f : expf(srow[j] - m);
        srow[j] = e;
        sum += e;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
      inv[i] = sum > 0.0f ? 1.0f / sum : 0.0f;            // all keys PAD: every e is 0 and so is every p
    }
    __syncthreads();                      // the rows are complete in LDS for the lanes that emit them
    // p = e / sum as e * (1 / sum), added to the head sums and stored, 4 keys per lane where the rows are 16-byte aligned.  A row
    // of head sums is only ever touched by the wave that owns the row, each element by the same lane for every head.
#pragma unroll
    for (int i = 0; i < AP_TQ / NW; ++i) {
      const int qi = w + NW * i;
      if (qi >= nlive) continue;
      ap_emit_row<VEC_OUT>(a.heads ? a.heads + (((size_t)r * H + h) * T + t0 + qi) * Ls : nullptr, sc + (size_t)qi * LsP,
                           want_mean ? macc + (size_t)qi * LsP : nullptr, h == 0, inv[i], Ls, lane);
    }
  }

  if (!want_mean) return;
  __syncthreads();                        // the head sums are complete in LDS
  // head mean and its first maximum
  for (int qi = w; qi < nlive; qi += NW) {
    float* mrow = macc + (size_t)qi * LsP;
    float best = -1.0f;                   // every mean is >= 0
    int bj = 0x7fffffff;
    for (int s = 0; s < nslot; ++s) {
      const int j = s * 64 + lane;
      if (j < Ls) {
        const float v = mrow[j] / (float)H;
        mrow[j] = v;
        if (v > best) { best = v; bj = j; }
      }
    }
    if (a.align) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ov > best || (ov == best && oj < bj)) { best = ov; bj = oj; }
      }
      if (lane == 0) a.align[(size_t)r * T + t0 + qi] = bj;
    }
  }
  if (a.mean) {
    __syncthreads();
    for (int qi = w; qi < nlive; qi += NW)
      ap_store_row<VEC_OUT>(a.mean + ((size_t)r * T + t0 + qi) * Ls, macc + (size_t)qi * LsP, Ls, lane);
  }
}

}  // namespace ttx
