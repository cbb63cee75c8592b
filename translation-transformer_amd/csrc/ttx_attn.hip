// Attention translation unit of libttx_hip.so: k_attn3 (the verify step: one wave per (sequence,
// head, 32 step rows), registers only), k_attn2 (encoder and full-prefix decoder: K staged in LDS, MFMA), k_attn (streaming
// fallback for key counts beyond k_attn2's LDS images), and their launcher.
#include "ttx_internal.h"

#include <algorithm>

namespace ttx {

// ------------------------------------------------------------------------------------------------
// Attention.  One wave per (row, head, tile of <= MAXQ queries).  Keys come in two segments:
//   A: `nA` keys every query may see (KV cache prefix / encoder memory), individually maskable;
//   B: `nB` keys with the causal rule  key j visible to query i  <=>  j <= qpos0 + i.
// Scores live in LDS as S[key][MAXQ+1]; softmax by wavefront shuffles; P·V with lane = head dim.
constexpr int ATT_MAXQ = 16;
constexpr int ATT_SQ = ATT_MAXQ + 1;

__host__ __device__ inline size_t attn_lds_bytes(int max_keys, int dh) {
  return sizeof(float) * ((size_t)ATT_MAXQ * dh + (size_t)max_keys * ATT_SQ + ATT_MAXQ);
}

// keyptr(key, kp, vp): K/V row pointers of key; vis(i, key): may query i (0..nq) see key?
template <int DH, class KeyPtr, class Vis>
__device__ __forceinline__ void attn_core(const float* __restrict__ q, int ldq, int nq, int nk, KeyPtr keyptr, Vis vis,
                                          float* __restrict__ out, int ldo, float scale, float* lds) {
  const int lane = threadIdx.x & 63;
  float* Qs = lds;                               // [MAXQ][DH]
  float* S = lds + ATT_MAXQ * DH;                // [nk][SQ]
  float* inv = S + (size_t)nk * ATT_SQ;          // [MAXQ]

  for (int e = lane * 4; e < nq * DH; e += 256) {
    const int i = e / DH, c = e % DH;
    *reinterpret_cast<float4*>(&Qs[i * DH + c]) = *reinterpret_cast<const float4*>(q + (size_t)i * ldq + c);
  }
  __syncthreads();

  // phase 1: scores, lane <-> key
  for (int c0 = 0; c0 < nk; c0 += 64) {
    const int key = c0 + lane;
    if (key < nk) {
      const float* kp;
      const float* vp;
      keyptr(key, kp, vp);
      float4 kr[DH / 4];
#pragma unroll
      for (int c = 0; c < DH / 4; ++c) kr[c] = *reinterpret_cast<const float4*>(kp + 4 * c);
      for (int i = 0; i < nq; ++i) {
        const float4* qv = reinterpret_cast<const float4*>(&Qs[i * DH]);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) {
          const float4 qq = qv[c];
          dot = fmaf(kr[c].x, qq.x, dot); dot = fmaf(kr[c].y, qq.y, dot);
          dot = fmaf(kr[c].z, qq.z, dot); dot = fmaf(kr[c].w, qq.w, dot);
        }
        S[(size_t)key * ATT_SQ + i] = vis(i, key) ? dot * scale : -INFINITY;
      }
    }
  }
  __syncthreads();

  // phase 2: softmax over keys, one query at a time
  for (int i = 0; i < nq; ++i) {
    float m = -INFINITY;
    for (int key = lane; key < nk; key += 64) m = fmaxf(m, S[(size_t)key * ATT_SQ + i]);
    m = wave_max(m);
    float sum = 0.f;
    for (int key = lane; key < nk; key += 64) {
      const float sv = S[(size_t)key * ATT_SQ + i];
      const float p = (sv == -INFINITY) ? 0.f : expf(sv - m);
      S[(size_t)key * ATT_SQ + i] = p;
      sum += p;
    }
    sum = wave_sum(sum);
    if (lane == 0) inv[i] = sum > 0.f ? 1.0f / sum : 0.f;
  }
  __syncthreads();

  // phase 3: out[i][d] = sum_key P[i][key] V[key][d]; DH = 32: lane = d + 32 * (key parity), the two parities meet in one
  // exchange; DH = 64: lane = d, every lane walks all keys in order
  constexpr int KPAR = 64 / DH;
  const int d = lane & (DH - 1), half = lane / DH;
  float acc[ATT_MAXQ];
#pragma unroll
  for (int i = 0; i < ATT_MAXQ; ++i) acc[i] = 0.f;
#pragma unroll 4
  for (int key = half; key < nk; key += KPAR) {
    const float* kp;
    const float* vp;
    keyptr(key, kp, vp);
    const float v = vp[d];
    const float* pr = &S[(size_t)key * ATT_SQ];
#pragma unroll
    for (int i = 0; i < ATT_MAXQ; ++i)
      if (i < nq) acc[i] = fmaf(pr[i], v, acc[i]);
  }
  if constexpr (KPAR == 2) {
#pragma unroll
    for (int i = 0; i < ATT_MAXQ; ++i) acc[i] += __shfl_xor(acc[i], 32, 64);
  }
  if (half == 0) {
#pragma unroll
    for (int i = 0; i < ATT_MAXQ; ++i)
      if (i < nq) out[(size_t)i * ldo + d] = acc[i] * inv[i];
  }
}




// Streaming fallback for key counts beyond the LDS images of k_attn2: one wave per (group, head, <=16 queries).
template <int MODE, int DH>
__global__ __launch_bounds__(64) void k_attn(AttnArgs a) {
  static_assert(DH == 32 || DH == 64, "k_attn is written for head dimensions 32 and 64");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int hd = blockIdx.y * DH;
  const int q0 = blockIdx.z * ATT_MAXQ;
  const int g = blockIdx.x;

  if constexpr (MODE == ATT_ENC || MODE == ATT_FULL_SELF || MODE == ATT_FULL_CROSS) {
    const int nq = min(ATT_MAXQ, a.L - q0);
    if (nq <= 0) return;
    const size_t row0 = (size_t)g * a.L;
    if constexpr (MODE == ATT_FULL_CROSS) {
      const int mr = a.mem_row ? a.mem_row[g] : g;
      const size_t mrow0 = (size_t)mr * a.Lk;
      const uint8_t* kpad = a.key_pad + mrow0;
      const float* kb = a.k + mrow0 * a.ldkv + hd;
      const float* vb = a.v + mrow0 * a.ldkv + hd;
      const int ld = a.ldkv;
      attn_core<DH>(a.q + (row0 + q0) * a.ldq + hd, a.ldq, nq, a.Lk,
                [=](int key, const float*& kp, const float*& vp) { kp = kb + (size_t)key * ld; vp = vb + (size_t)key * ld; },
                [=](int, int key) { return kpad[key] == 0; },
                a.out + (row0 + q0) * a.d + hd, a.d, a.scale, lds);
    } else {
      const int* tk = a.tok + row0;
      const int pad = a.pad;
      const float* kb = a.k + row0 * a.ldkv + hd;
      const float* vb = a.v + row0 * a.ldkv + hd;
      const int ld = a.ldkv;
      const bool causal = (MODE == ATT_FULL_SELF);
      attn_core<DH>(a.q + (row0 + q0) * a.ldq + hd, a.ldq, nq, causal ? min(a.L, q0 + nq) : a.L,
                [=](int key, const float*& kp, const float*& vp) { kp = kb + (size_t)key * ld; vp = vb + (size_t)key * ld; },
                [=](int i, int key) { return tk[key] != pad && (!causal || key <= q0 + i); },
                a.out + (row0 + q0) * a.d + hd, a.d, a.scale, lds);
    }
  } else {
    if (g >= a.st->n_active) return;
    const int RPS = step_rps(a.N, a.D), D = a.D;
    const int nq = min(ATT_MAXQ, RPS - q0);
    if (nq <= 0) return;
    const int b = a.act_idx[g];
    const size_t srow0 = (size_t)g * RPS;              // first step row of this slot
    if constexpr (MODE == ATT_STEP_SELF) {
      const int f = a.front[b];
      const int* tk = a.tok + (size_t)b * a.gen_ld;
      const int pad = a.pad;
      const size_t cb = a.cache_slot ? a.cache_slot[b] : b;      // the sequence's slot in the cache (batch pool: candidate -> slot map)
      const float* kc = a.kcache + cb * a.cache_seq_stride + hd;
      const float* vc = a.vcache + cb * a.cache_seq_stride + hd;
      const float* kb = a.k + srow0 * a.ldkv + hd;
      const float* vb = a.v + srow0 * a.ldkv + hd;
      const int ld = a.ldkv, dd = a.d;
      const bool front_ok = tk[f] != pad;
      // keys: cached prefix [0,f), then every step row of the slot (row 0 = position f, draft rows after it)
      attn_core<DH>(a.q + (srow0 + q0) * a.ldq + hd, a.ldq, nq, f + RPS,
                [=](int key, const float*& kp, const float*& vp) {
                  if (key < f) { kp = kc + (size_t)key * dd; vp = vc + (size_t)key * dd; }
                  else { kp = kb + (size_t)(key - f) * ld; vp = vb + (size_t)(key - f) * ld; }
                },
                [=](int i, int key) {
                  if (key < f) return tk[key] != pad;
                  const int kr = key - f, qr = q0 + i;
                  if (kr == 0) return front_ok;               // position f is visible to every step row
                  if (qr == 0) return false;
                  const int kn = (kr - 1) / D, qn = (qr - 1) / D;
                  return kn == qn && kr <= qr;                // same draft, not later
                },
                a.out + (srow0 + q0) * a.d + hd, a.d, a.scale, lds);
    } else {
      const size_t mrow0 = (size_t)(a.src_of ? a.src_of[b] : b) * a.Lk;
      const uint8_t* kv = a.key_pad + mrow0;
      const float* kb = a.k + mrow0 * a.ldkv + hd;
      const float* vb = a.v + mrow0 * a.ldkv + hd;
      const int ld = a.ldkv;
      // slot pool: only the slot's own source positions hold data (the rest of its row is stale or uninitialised,
      // and a masked key's V still enters 0 * V)
      attn_core<DH>(a.q + (srow0 + q0) * a.ldq + hd, a.ldq, nq, a.src_len ? a.src_len[b] : a.Lk,
                [=](int key, const float*& kp, const float*& vp) { kp = kb + (size_t)key * ld; vp = vb + (size_t)key * ld; },
                [=](int, int key) { return kv[key] != 0; },
                a.out + (srow0 + q0) * a.d + hd, a.d, a.scale, lds);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Attention v2 (the fast path; k_attn above stays as the long-sequence fallback).
// One 256-thread workgroup per (group, head, tile of <= 32 queries) where a group is one source /
// decoder row / running sequence, so the N drafts of a sequence share one pass over the cached prefix
// and over the encoder memory.  K and V of every visible key are staged in LDS by coalesced 128-B row
// loads issued back to back (one latency, not one per key chunk); S = Q·Kᵀ and O = P·V run on the fp32
// MFMA (32x32x2), key tiles / key ranges split over the 4 waves; softmax by wavefront shuffles.
constexpr int A2_MT = 32;                  // rows of one MFMA tile
constexpr int A2_QT = 64;                  // queries per workgroup (two MFMA row tiles share the staged K/V)
// per head dimension dh (32 or 64):
__host__ __device__ constexpr int a2_ldq(int dh) { return dh + 4; }                 // LDS row stride of Q and K rows (conflict-free ds_read_b128)
__host__ __device__ constexpr int a2_op(int dh) { return 4 * A2_MT * (dh + 1); }    // floats of the four waves' partial output tiles (aliased onto the score image)
// V rows held in registers: 8 keys per step per wave.  dh = 32: 12 steps of one value -> up to 384 keys.  dh = 64: a step holds
// two values per key (dims r and r + 32); 10 steps = 80 registers -> up to 320 keys, the most whose LDS images (a 64-query
// launch: 147 584 B; 352 keys would need 160 000 B) stay under the 150 KB limit of the launcher.
__host__ __device__ constexpr int a2_vsteps(int dh) { return dh == 32 ? 12 : 10; }

__host__ __device__ inline int a2_nkp(int nk) { return (nk + 31) & ~31; }
__host__ __device__ inline int a2_qcap(int q_per_group) { return q_per_group <= A2_MT ? A2_MT : A2_QT; }
__host__ __device__ inline size_t a2_score_floats(int nkp, int dh) {
  const size_t sf = (size_t)A2_MT * (nkp + 4);
  return sf > (size_t)a2_op(dh) ? sf : (size_t)a2_op(dh);
}
__host__ __device__ inline size_t attn2_lds_bytes(int max_keys, int qcap, int dh) {
  const size_t nkp = a2_nkp(max_keys);
  return sizeof(float) * ((size_t)qcap * a2_ldq(dh) + nkp * a2_ldq(dh) + a2_score_floats((int)nkp, dh) + A2_MT) +
         sizeof(int) * (nkp + A2_QT);
}
__host__ __device__ inline bool attn2_fits(int max_keys, int dh) { return a2_nkp(max_keys) <= 32 * a2_vsteps(dh); }

// Visibility is decided from one int per key and one per query, computed once while staging:
//   key flag A2_MASKED   masked (PAD key / padding row)
//   key flag A2_ALL      visible to every query (cached prefix, encoder memory)
//   otherwise a2_flag(group, position): visible to queries of the same group at position >= key position.
// Groups are spaced 2^17 apart and positions are < 2^16, so "same group and kpos <= qpos" is the single unsigned
// comparison (qf - kf) < 2^16.
constexpr int A2_ALL = 0x7fffffff;
constexpr int A2_MASKED = 0x7ffffffe;
__host__ __device__ inline int a2_flag(int group, int pos) { return (group << 17) | pos; }
__device__ __forceinline__ bool a2_visible(int qf, int kf) {
  return kf == A2_ALL || (unsigned)(qf - kf) < 65536u;
}

// keyptr(key, kp, vp): branch-free K/V row pointers of key (0 <= key < nk); keyflag(key), qflag(qi): see above.
template <int DH, class KeyPtr, class KeyFlag, class QFlag>
__device__ __forceinline__ void attn2_core(const float* __restrict__ q, int ldq, int nq, int nk, KeyPtr keyptr, KeyFlag keyflag,
                                           QFlag qflag, float* __restrict__ out, int ldo, float scale, float* lds, int qcap) {
  constexpr int A2_LDQ = a2_ldq(DH), A2_VSTEPS = a2_vsteps(DH);
  constexpr int A2_OS = DH + 1;                      // row stride of a partial output tile
  constexpr int A2_NV = DH / 32;                     // values per key and lane in O = P·V: dims r, r + 32, ...
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int r = lane & 31, h = lane >> 5;
  const int nkp = a2_nkp(nk);
  const int lds_s = nkp + 4;
  float* Qs = lds;                                   // [qcap][DH+4]
  float* Ks = Qs + qcap * A2_LDQ;                    // [nkp][DH+4]
  float* S = Ks + (size_t)nkp * A2_LDQ;              // [32][nkp+4]   scores of the current row tile
  float* Op = S;                                     // [4 waves][32][DH+1] partial outputs reuse the score image
  float* inv = S + a2_score_floats(nkp, DH);         // [32]
  int* kfl = reinterpret_cast<int*>(inv + A2_MT);    // [nkp]
  int* qfl = kfl + nkp;                              // [64]

  // ---- stage Q, K, V: a row is DH floats = DH/4 lanes x float4, so the 256 threads take A2_RP = 32 (DH = 32) or 16
  // (DH = 64) rows per pass.  Loads are unconditional (indices are clamped; rows past nq / nk are masked through the
  // flags) and all of them are requested before the first LDS write.
  constexpr int A2_LPR = DH / 4, A2_RP = 256 / A2_LPR;
  constexpr int A2_QP = A2_MT / A2_RP;               // passes over one 32-query row tile
  const int lr = (unsigned)t / A2_LPR, lc = ((unsigned)t % A2_LPR) * 4;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4 qv0[A2_QP], qv1[A2_QP];
#pragma unroll
  for (int p = 0; p < A2_QP; ++p) {
    qv0[p] = *reinterpret_cast<const f32x4*>(q + (size_t)min(lr + p * A2_RP, nq - 1) * ldq + lc);
    qv1[p] = qv0[p];
  }
  if (qcap > A2_MT) {
#pragma unroll
    for (int p = 0; p < A2_QP; ++p)
      qv1[p] = *reinterpret_cast<const f32x4*>(q + (size_t)min(lr + p * A2_RP + 32, nq - 1) * ldq + lc);
  }
  constexpr int A2_U = 8;                            // passes of A2_RP keys in flight
  // V never touches LDS: in O = P·V lane (dh, h) needs V[key][dh] for its wave's keys only, so each wave keeps its
  // nkp/4 value rows in registers (requested here, consumed after the softmax).  Wave w owns the 8-key groups
  // w, w+4, w+8, ...: a fixed interleave, so the order in which a row's keys are summed does not depend on how far
  // the batch's padding extends (masked keys add exact zeros) — results are the same in any batch.
  const int kq = nkp / 4;
  float vr[A2_NV][A2_VSTEPS][4];
  for (int k0 = 0; k0 < nkp; k0 += A2_RP * A2_U) {
    f32x4 kv[A2_U];
#pragma unroll
    for (int u = 0; u < A2_U; ++u) {
      const float* kp;
      const float* vp;
      keyptr(min(k0 + u * A2_RP + lr, nk - 1), kp, vp);
      kv[u] = *reinterpret_cast<const f32x4*>(kp + lc);
    }
    if (k0 == 0) {
#pragma unroll
      for (int si = 0; si < A2_VSTEPS; ++si) {
        if (si * 8 < kq) {
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const float* kp;
            const float* vp;
            keyptr(min((wave + 4 * si) * 8 + 4 * h + jj, nk - 1), kp, vp);
#pragma unroll
            for (int n = 0; n < A2_NV; ++n) vr[n][si][jj] = vp[r + 32 * n];
          }
        }
      }
      // the visibility flags' token loads ride behind the K/V requests
      for (int key = t; key < nkp; key += 256) kfl[key] = (key < nk) ? keyflag(key) : A2_MASKED;
      if (t < A2_QT) qfl[t] = qflag(t);
    }
    // every K request is in flight before the first value is consumed: the empty asm reads all eight registers,
    // so the scheduler cannot sink a load down to its LDS write
    asm volatile("" : "+v"(kv[0]), "+v"(kv[1]), "+v"(kv[2]), "+v"(kv[3]), "+v"(kv[4]), "+v"(kv[5]), "+v"(kv[6]), "+v"(kv[7]));
#pragma unroll
    for (int u = 0; u < A2_U; ++u) {
      const int key = k0 + u * A2_RP + lr;
      if (k0 + u * A2_RP < nkp) *reinterpret_cast<f32x4*>(&Ks[(size_t)key * A2_LDQ + lc]) = kv[u];
    }
  }
#pragma unroll
  for (int p = 0; p < A2_QP; ++p) *reinterpret_cast<f32x4*>(&Qs[(lr + p * A2_RP) * A2_LDQ + lc]) = qv0[p];
  if (qcap > A2_MT) {
#pragma unroll
    for (int p = 0; p < A2_QP; ++p) *reinterpret_cast<f32x4*>(&Qs[(lr + p * A2_RP + 32) * A2_LDQ + lc]) = qv1[p];
  }
  __syncthreads();

  const int n_mt = (nq + A2_MT - 1) / A2_MT;         // 1 or 2 row tiles

  // The two row tiles (queries 0-31, 32-63) run one after the other through the same score buffer: K and V
  // stay staged, the S image is reused.
  const int n_kt = nkp / 32;
  for (int mt = 0; mt < n_mt; ++mt) {
    const int q0 = mt * A2_MT;
    // ---- S = scale * Q Kᵀ with masking; key tiles are dealt to the 4 waves
    for (int kt = wave; kt < n_kt; kt += 4) {
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      const float* ap = &Qs[(q0 + r) * A2_LDQ + 4 * h];
      const float* bp = &Ks[(size_t)(kt * 32 + r) * A2_LDQ + 4 * h];
#pragma unroll
      for (int kk = 0; kk < DH; kk += 8) {
        const float4 av = *reinterpret_cast<const float4*>(ap + kk);
        const float4 bv = *reinterpret_cast<const float4*>(bp + kk);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
      }
      const int key = kt * 32 + r;
      const int kf = kfl[key];
      const int* qf = qfl + q0 + 4 * h;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int dq = (v & 3) + 8 * (v >> 2);        // rows past nq carry a query flag that sees nothing but A2_ALL
        S[(size_t)(dq + 4 * h) * lds_s + key] = a2_visible(qf[dq], kf) ? acc[v] * scale : -INFINITY;
      }
    }
    __syncthreads();

    // ---- softmax: every wave owns 8 query rows, 8 lanes per row (each lane nkp/8 keys, 3-step shuffles).
    // Rows past nq hold finite or -inf scores of no consequence: their outputs are never stored.
    {
      const int ql = wave * 8 + (lane >> 3), l8 = lane & 7;
      float* row = S + (size_t)ql * lds_s;
      float m = -INFINITY;
      for (int key = l8; key < nkp; key += 8) m = fmaxf(m, row[key]);
      m = fmaxf(m, __shfl_xor(m, 4, 8));
      m = fmaxf(m, __shfl_xor(m, 2, 8));
      m = fmaxf(m, __shfl_xor(m, 1, 8));
      const float mm = (m == -INFINITY) ? 0.f : m;   // fully masked row: every p becomes exp(-inf) = 0
      float sum = 0.f;
      for (int key = l8; key < nkp; key += 8) {
        const float p = __expf(row[key] - mm);
        row[key] = p;
        sum += p;
      }
      sum += __shfl_xor(sum, 4, 8);
      sum += __shfl_xor(sum, 2, 8);
      sum += __shfl_xor(sum, 1, 8);
      if (l8 == 0) inv[ql] = sum > 0.f ? 1.0f / sum : 0.f;
    }
    __syncthreads();

    // ---- O = P V: wave w takes keys [w*nkp/4, (w+1)*nkp/4) with its V rows from registers; partial sums meet in LDS
    // (DH = 64: one accumulator per 32 output dims, both fed by the same P values)
    {
      f32x16 acc[A2_NV];
#pragma unroll
      for (int n = 0; n < A2_NV; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
      const float* prow = S + (size_t)r * lds_s + 4 * h + wave * 8;
#pragma unroll
      for (int si = 0; si < A2_VSTEPS; ++si) {
        if (si * 8 < kq) {
          const float4 pv = *reinterpret_cast<const float4*>(prow + si * 32);
#pragma unroll
          for (int n = 0; n < A2_NV; ++n) {
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(pv.x, vr[n][si][0], acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(pv.y, vr[n][si][1], acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(pv.z, vr[n][si][2], acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(pv.w, vr[n][si][3], acc[n], 0, 0, 0);
          }
        }
      }
      __syncthreads();                                // every wave has read its P columns: the image becomes Op
      float* part = Op + (size_t)wave * (A2_MT * A2_OS);
#pragma unroll
      for (int n = 0; n < A2_NV; ++n)
#pragma unroll
        for (int v = 0; v < 16; ++v) part[((v & 3) + 8 * (v >> 2) + 4 * h) * A2_OS + r + 32 * n] = acc[n][v];
    }
    __syncthreads();
    for (int e = t; e < A2_MT * DH; e += 256) {
      const int ql = (unsigned)e / DH, c = (unsigned)e % DH;
      const float o = Op[ql * A2_OS + c] + Op[A2_MT * A2_OS + ql * A2_OS + c] + Op[2 * A2_MT * A2_OS + ql * A2_OS + c] +
                      Op[3 * A2_MT * A2_OS + ql * A2_OS + c];
      if (q0 + ql < nq) out[(size_t)(q0 + ql) * ldo + c] = o * inv[ql];
    }
    if (mt + 1 < n_mt) __syncthreads();               // S, inv and Op are rewritten by the next row tile
  }
}

// amdgpu_waves_per_eu(1, 2): the LDS images allow at most two workgroups per CU, so let the compiler keep the
// staging loads in registers (with the default occupancy target it spills them to scratch to stay under 64 VGPRs)
// DH = 64 asks for exactly two: left at (1, 2) the compiler takes 232 VGPRs + 64 AGPRs and one workgroup per CU; held to 256
// registers it needs 231 - 236 VGPRs, no AGPRs and no scratch
template <int MODE, int DH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DH == 32 ? 1 : 2, 2))) void k_attn2(AttnArgs a) {
  static_assert(DH == 32 || DH == 64, "k_attn2 is written for head dimensions 32 and 64");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int hd = blockIdx.y * DH;
  const int tile = blockIdx.z;
  auto q_any = [](int) { return 0; };

  if constexpr (MODE == ATT_ENC || MODE == ATT_FULL_CROSS) {
    const int g = blockIdx.x;
    const int q0 = tile * A2_QT;
    const int nq = min(A2_QT, a.L - q0);
    if (nq <= 0) return;
    const size_t row0 = (size_t)g * a.L;
    if constexpr (MODE == ATT_ENC) {
      const int* tk = a.tok + row0;
      const int pad = a.pad;
      const float* kb = a.k + row0 * a.ldkv + hd;
      const float* vb = a.v + row0 * a.ldkv + hd;
      const int ld = a.ldkv;
      attn2_core<DH>(a.q + (row0 + q0) * a.ldq + hd, a.ldq, nq, a.L,
                 [=](int key, const float*& kp, const float*& vp) { kp = kb + (size_t)key * ld; vp = vb + (size_t)key * ld; },
                 [=](int key) { return tk[key] != pad ? A2_ALL : A2_MASKED; }, q_any,
                 a.out + (row0 + q0) * a.d + hd, a.d, a.scale, lds, a2_qcap(a.L));
    } else {
      const int mr = a.mem_row ? a.mem_row[g] : g;
      const size_t mrow0 = (size_t)mr * a.Lk;
      const uint8_t* kpad = a.key_pad + mrow0;
      const float* kb = a.k + mrow0 * a.ldkv + hd;
      const float* vb = a.v + mrow0 * a.ldkv + hd;
      const int ld = a.ldkv;
      attn2_core<DH>(a.q + (row0 + q0) * a.ldq + hd, a.ldq, nq, a.Lk,
                 [=](int key, const float*& kp, const float*& vp) { kp = kb + (size_t)key * ld; vp = vb + (size_t)key * ld; },
                 [=](int key) { return kpad[key] == 0 ? A2_ALL : A2_MASKED; }, q_any,
                 a.out + (row0 + q0) * a.d + hd, a.d, a.scale, lds, a2_qcap(a.L));
    }
  } else if constexpr (MODE == ATT_FULL_SELF) {
    const int g = blockIdx.x;
    const int q0 = tile * A2_QT;
    const int nq = min(A2_QT, a.L - q0);
    if (nq <= 0) return;
    const size_t row0 = (size_t)g * a.L;
    const int* tk = a.tok + row0;
    const int pad = a.pad;
    const float* kb = a.k + row0 * a.ldkv + hd;
    const float* vb = a.v + row0 * a.ldkv + hd;
    const int ld = a.ldkv;
    attn2_core<DH>(a.q + (row0 + q0) * a.ldq + hd, a.ldq, nq, min(a.L, q0 + nq),
               [=](int key, const float*& kp, const float*& vp) { kp = kb + (size_t)key * ld; vp = vb + (size_t)key * ld; },
               [=](int key) { return tk[key] != pad ? a2_flag(0, key) : A2_MASKED; },
               [=](int qi) { return a2_flag(0, q0 + qi); },
               a.out + (row0 + q0) * a.d + hd, a.d, a.scale, lds, a2_qcap(a.L));
  } else {
    // step modes: group = running sequence (slot); a workgroup takes 64 of the slot's RPS step rows
    const int slot = blockIdx.x;
    if (slot >= a.st->n_active) return;
    const int D = a.D, RPS = step_rps(a.N, a.D);
    const int r0 = tile * A2_QT;                       // first step row of this tile
    const int nq = min(A2_QT, RPS - r0);
    if (nq <= 0) return;
    const int b = a.act_idx[slot];
    const size_t srow0 = (size_t)slot * RPS;
    if constexpr (MODE == ATT_STEP_SELF) {
      const int f = a.front[b];
      const int* tk = a.tok + (size_t)b * a.gen_ld;
      const int pad = a.pad;
      const size_t cb = a.cache_slot ? a.cache_slot[b] : b;      // the sequence's slot in the cache (batch pool: candidate -> slot map)
      const float* kc = a.kcache + cb * a.cache_seq_stride + hd;
      const float* vc = a.vcache + cb * a.cache_seq_stride + hd;
      const float* kb = a.k + srow0 * a.ldkv + hd;
      const float* vb = a.v + srow0 * a.ldkv + hd;
      const int ld = a.ldkv, dd = a.d;
      // keys: cached prefix [0,f) | step row 0 (position f) | the rows of every draft that has a query in this tile
      const int rlast = r0 + nq - 1;
      const int n_lo = (r0 == 0) ? 0 : (r0 - 1) / D;
      const int n_hi = (rlast == 0) ? -1 : (rlast - 1) / D;
      const int kr0 = 1 + n_lo * D;                    // first draft row staged
      const int n_draft_keys = (n_hi >= n_lo && D > 0) ? (n_hi - n_lo + 1) * D : 0;
      attn2_core<DH>(a.q + (srow0 + r0) * a.ldq + hd, a.ldq, nq, f + 1 + n_draft_keys,
                 [=](int key, const float*& kp, const float*& vp) {
                   const bool cached = key < f;
                   const int srow = (key == f) ? 0 : kr0 + (key - f - 1);
                   const size_t off = cached ? (size_t)key * dd : (size_t)srow * ld;
                   kp = (cached ? kc : kb) + off;
                   vp = (cached ? vc : vb) + off;
                 },
                 [=](int key) {
                   if (key <= f) return tk[key] != pad ? A2_ALL : A2_MASKED;   // prefix and the front token
                   const int kr = kr0 + (key - f - 1);
                   const int kn = (kr - 1) / D;
                   return a2_flag(kn - n_lo, kr - 1 - kn * D);
                 },
                 [=](int qi) {
                   const int qr = r0 + qi;
                   if (qr == 0 || D == 0) return a2_flag(0x3fff, 0);           // sees prefix + front token only
                   const int qn = (qr - 1) / D;
                   return a2_flag(qn - n_lo, qr - 1 - qn * D);
                 },
                 a.out + (srow0 + r0) * a.d + hd, a.d, a.scale, lds, a2_qcap(RPS));
    } else {
      const size_t mrow0 = (size_t)(a.src_of ? a.src_of[b] : b) * a.Lk;
      const uint8_t* kv = a.key_pad + mrow0;
      const float* kb = a.k + mrow0 * a.ldkv + hd;
      const float* vb = a.v + mrow0 * a.ldkv + hd;
      const int ld = a.ldkv;
      attn2_core<DH>(a.q + (srow0 + r0) * a.ldq + hd, a.ldq, nq, a.src_len ? a.src_len[b] : a.Lk,   // see k_attn: slot pool
                 [=](int key, const float*& kp, const float*& vp) { kp = kb + (size_t)key * ld; vp = vb + (size_t)key * ld; },
                 [=](int key) { return kv[key] != 0 ? A2_ALL : A2_MASKED; }, q_any,
                 a.out + (srow0 + r0) * a.d + hd, a.d, a.scale, lds, a2_qcap(RPS));
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Attention v3 for the verify step: ONE WAVE per (running sequence, head, 32 step rows), no barrier in the main loop.
//
// Everything stays in the layout the fp32 MFMA produces.  Scores are computed TRANSPOSED, S^T = K Q^T (A operand =
// 32 keys of the tile, B operand = the 32 queries), so a lane (r, h) ends up with 16 scores of ONE query r (keys
// (v&3) + 8(v>>2) + 4h of the tile): the online-softmax statistics of a query live in its own two lanes (one
// exchange with lane^32), and the probabilities are already the B operand of the second product
// O^T = V^T P^T in exactly the key pairing (own register t of the h = 0 lane with own register t of the h = 1 lane)
// the MFMA contracts; its A operand V^T is 16 coalesced 128-B row reads per tile.  O^T again keeps one query per
// lane, so rescaling by exp(m_old - m_new) and the final 1/l are per-lane scalars.  Keys are visited in tiles of
// 32 in a fixed order: a row's arithmetic does not depend on the batch it sits in.
//
// Arithmetic (the same whichever wave computes a tile): every 32-key tile i yields a partial (m_i, l_i, O_i) with its
// own maximum; the partials are folded IN TILE ORDER into (M, L, O) by  M' = max(M, m_i),  L' = L e^(M-M') + l_i e^(m_i-M'),
// O' likewise.  Two kernels evaluate it:
//   k_attn3s  many sequences (row groups, slot pools): one wave per unit (sequence, head, 32 step rows), folding as it goes,
//             the units of a launch STREAMED through a grid of the machine's size (see the kernel);
//   k_attn3   few sequences (a 32-row batch): the four waves of a workgroup take tiles w, w+4, ... of ONE unit, park the
//             partials in LDS and then fold them in tile order (wave w finishing dims 8w + 4h .. +3): bit-identical results,
//             four times the parallelism.  The host picks by launch size.
constexpr int A3_QT = 32;            // step rows per wave
#ifndef TTX_A3S_WGS_PER_CU
#define TTX_A3S_WGS_PER_CU 2         // grid of k_attn3s: workgroups per CU (two waves per SIMD are resident)
#endif
#ifndef TTX_A3_SPLIT_BELOW
#define TTX_A3_SPLIT_BELOW 1024      // launches with fewer units (slots x heads x 32-row tiles) share a unit's key tiles over four waves
#endif

// A3Tile = what one 32-key tile needs from memory, per lane.
struct A3Tile {
  float4 k0, k1, k2, k3;     // A operand of S^T: key key0 + r, dims 8g + 4h .. +3
  float v[16];               // A operand of O^T: V[key(t, h)][r], key(t, h) = key0 + (t&3) + 8(t>>2) + 4h
  int own;                   // validity word of key key0 + r (token / source-valid byte)
};

__device__ __forceinline__ void a3_fold(float& M, float& L, float mi, float li, float& a, float& b) {
  const float Mn = fmaxf(M, mi);
  a = (M == -INFINITY) ? 0.f : __expf(M - Mn);
  b = (mi == -INFINITY) ? 0.f : __expf(mi - Mn);
  L = __fmaf_rn(L, a, __fmul_rn(li, b));
  M = Mn;
}
constexpr int A3_PART = 16 * 64 + 64;          // floats of one parked tile partial: O_i [16][64], m_i [32], l_i [32]

// The scalars of one unit.  Keys of STEP_SELF: cached prefix [0, f) | step row 0 (position f) | the rows of every draft that has
// a query in this unit's 32 rows.  Keys below `lin_limit` sit at klin / vlin + key * lin_ld (the cache, or the encoder memory): a
// tile made of such keys takes its addresses from one base.  `n_plain` = number of leading keys that every query sees whenever
// they are real tokens (cached prefix and front token, or all encoder positions): tiles made of such keys skip the per-key
// visibility flags altogether.
struct A3Unit {
  const float* q; float* out;
  const float* klin; const float* vlin;
  const float* kb; const float* vb;            // STEP_SELF: this step's K / V rows of the sequence (packed QKV buffer)
  const int* tk;                               // STEP_SELF: the sequence's token row
  const uint8_t* kvalid;                       // STEP_CROSS: source-valid bytes
  int nq, nk, n_plain, lin_limit, ntiles;
  int f, kr0, n_lo, r0;
  unsigned mask;                               // SEL: the slot's present drafts
};

__device__ __forceinline__ int a3_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// x / D for 0 <= x < 2^32 / D without a division per lane: magic = floor(2^32 / D) + 1 (D >= 2)
__device__ __forceinline__ unsigned a3_magic(int D) { return D >= 2 ? (unsigned)(0x100000000ull / (unsigned)D) + 1u : 0u; }
__device__ __forceinline__ int a3_div(int x, int D, unsigned magic) { return D >= 2 ? (int)__umulhi((unsigned)x, magic) : x; }

// SEL (draft select): the slot's rows are stored compacted from row_base[slot] on: row 0, then the D rows of every
// draft in draft_mask[slot].  Queries and keys KEEP their layout positions (r0 + r, f + rs), so every sum runs in the order it has
// without SEL; only the memory row a position maps to changes (step_sel_row), a row of an absent draft aliasing the slot's row 0:
// a valid address with finite data, visible to that draft's own queries alone, and those are never stored.
template <int MODE, bool SEL>
__device__ __forceinline__ A3Unit a3_unit(const AttnArgs& a, int slot, int head, int qt, int RPS, unsigned magic) {
  A3Unit c;
  const int hd = head * ATT_DH;
  const int r0 = qt * A3_QT;
  const int b = a3_uniform(a.act_idx[slot]);
  size_t srow0 = (size_t)slot * RPS;
  c.r0 = r0;
  c.nq = min(A3_QT, RPS - r0);
  c.mask = 0u;
  if constexpr (SEL) {
    srow0 = (size_t)a3_uniform(a.row_base[slot]);
    c.mask = (unsigned)a3_uniform(a.draft_mask[slot]);
    c.q = a.q + srow0 * a.ldq + hd;                  // the slot's row 0: a3_sel_row gives the row from there
    c.out = a.out + srow0 * a.d + hd;
  } else {
    c.q = a.q + (srow0 + r0) * a.ldq + hd;
    c.out = a.out + (srow0 + r0) * a.d + hd;
  }
  if constexpr (MODE == ATT_STEP_SELF) {
    const int D = a.D;
    const int f = a3_uniform(a.front[b]);
    const int rlast = r0 + c.nq - 1;
    const int n_lo = (r0 == 0) ? 0 : a3_div(r0 - 1, D, magic);
    const int n_hi = (rlast == 0) ? -1 : a3_div(rlast - 1, D, magic);
    const int n_draft_keys = (n_hi >= n_lo && D > 0) ? (n_hi - n_lo + 1) * D : 0;
    c.f = f;
    c.n_lo = n_lo;
    c.kr0 = 1 + n_lo * D;
    c.tk = a.tok + (size_t)b * a.gen_ld;
    const size_t cb = a.cache_slot ? (size_t)a3_uniform(a.cache_slot[b]) : (size_t)b;
    c.klin = a.kcache + cb * a.cache_seq_stride + hd;
    c.vlin = a.vcache + cb * a.cache_seq_stride + hd;
    c.kb = a.k + srow0 * a.ldkv + hd;
    c.vb = a.v + srow0 * a.ldkv + hd;
    c.kvalid = nullptr;
    c.nk = f + 1 + n_draft_keys;
    c.n_plain = f + 1;
    c.lin_limit = f;
  } else {
    const size_t mrow0 = (size_t)(a.src_of ? a3_uniform(a.src_of[b]) : b) * a.Lk;
    const int nkeys = a.src_len ? a3_uniform(a.src_len[b]) : a.Lk;      // see k_attn: slot pool
    c.kvalid = a.key_pad + mrow0;
    c.klin = a.k + mrow0 * a.ldkv + hd;
    c.vlin = a.v + mrow0 * a.ldkv + hd;
    c.kb = c.klin;
    c.vb = c.vlin;
    c.tk = nullptr;
    c.f = 0; c.kr0 = 0; c.n_lo = 0;
    c.nk = nkeys;
    c.n_plain = (nkeys + 31) & ~31;
    c.lin_limit = nkeys;
  }
  if constexpr (SEL) {
    // a unit none of whose rows is stored (row 0 is not among them and all its drafts are absent) folds one key and leaves
    // (the first and last draft of the unit are worked out here again, for both modes, and not shared with STEP_SELF's lines above:
    // hoisting them changes the register allocation of the existing k_attn3s<STEP_SELF> instantiation, which is to stay as it was)
    if (r0 > 0) {
      const int n_lo = a3_div(r0 - 1, a.D, magic), n_hi = a3_div(r0 + c.nq - 2, a.D, magic);
      const unsigned span = ((2u << n_hi) - 1u) & ~((1u << n_lo) - 1u);
      if (!(c.mask & span)) c.nk = 1;
    }
  }
  c.ntiles = (c.nk + 31) >> 5;
  return c;
}

// SEL: layout row `rs` of the unit's slot -> row inside the slot's compacted rows; -1: a row of an absent draft
__device__ __forceinline__ int a3_sel_row(const AttnArgs& a, const A3Unit& c, int rs, unsigned magic) {
  if (rs == 0) return 0;
  const int n = a3_div(rs - 1, a.D, magic);
  return step_sel_row(c.mask, n, rs - 1 - n * a.D, a.D);
}

// K / V row of key `key` (0 <= key < nk) as an offset in floats from the unit's bases: 32-bit arithmetic (a sequence's cache, its
// step rows and a source's memory rows each span far less than 2^31 floats)
template <int MODE, bool SEL>
__device__ __forceinline__ void a3_keyrow(const AttnArgs& a, const A3Unit& c, int key, unsigned magic, const float*& kp, const float*& vp) {
  if constexpr (MODE == ATT_STEP_SELF) {
    const bool cached = key < c.f;
    int srow = (key == c.f) ? 0 : c.kr0 + (key - c.f - 1);
    if constexpr (SEL) srow = max(a3_sel_row(a, c, max(srow, 0), magic), 0);
    const int off = cached ? key * a.d : srow * a.ldkv;
    kp = (cached ? c.klin : c.kb) + off;
    vp = (cached ? c.vlin : c.vb) + off;
  } else {
    const int off = key * a.ldkv;
    kp = c.klin + off;
    vp = c.vlin + off;
  }
}
template <int MODE>
__device__ __forceinline__ int a3_keyown(const AttnArgs& a, const A3Unit& c, int key) {
  if constexpr (MODE == ATT_STEP_SELF) return c.tk[min(key, c.f)] != a.pad ? 1 : 0;      // prefix / front token is a real token
  else return (int)c.kvalid[key];
}
// visibility flag of key `key` (a2_visible's convention); `real` = the key's validity word; keys past nk are masked
template <int MODE>
__device__ __forceinline__ int a3_keyflag(const AttnArgs& a, const A3Unit& c, int key, bool real, unsigned magic) {
  if (key >= c.nk) return A2_MASKED;
  if constexpr (MODE == ATT_STEP_SELF) {
    const int D = a.D;
    const int kr = c.kr0 + max(key - c.f - 1, 0);
    const int kn = a3_div(kr - 1, max(D, 1), magic);
    const int draft_flag = a2_flag(kn - c.n_lo, kr - 1 - kn * D);
    return key <= c.f ? (real ? A2_ALL : A2_MASKED) : draft_flag;
  } else {
    return real ? A2_ALL : A2_MASKED;
  }
}
template <int MODE>
__device__ __forceinline__ int a3_qflag(const AttnArgs& a, const A3Unit& c, int qi, unsigned magic) {
  if constexpr (MODE == ATT_STEP_SELF) {
    const int D = a.D;
    const int qr = c.r0 + qi;
    if (qr == 0 || D == 0) return a2_flag(0x3fff, 0);           // sees prefix + front token only
    const int qn = a3_div(qr - 1, D, magic);
    return a2_flag(qn - c.n_lo, qr - 1 - qn * D);
  } else {
    return 0;
  }
}

struct A3Query {
  float qx[16];              // B operand of S^T: query r, dims 8g + 4h .. +3, already times the scale
  int qf;                    // (rows past nq repeat the last query; they are never stored)
  int orow;                  // SEL: row the lane's query is stored at, from the slot's row 0 on; -1: not stored
};

template <int MODE, bool SEL>
__device__ __forceinline__ A3Query a3_load_query(const AttnArgs& a, const A3Unit& c, int r, int h, unsigned magic) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  A3Query qq;
  const float* qp;
  if constexpr (SEL) {
    const int m = a3_sel_row(a, c, c.r0 + min(r, c.nq - 1), magic);
    qq.orow = r < c.nq ? m : -1;
    qp = c.q + (size_t)max(m, 0) * a.ldq + 4 * h;
  } else {
    qq.orow = 0;
    qp = c.q + (size_t)min(r, c.nq - 1) * a.ldq + 4 * h;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 v = *reinterpret_cast<const f32x4*>(qp + 8 * g);
    v *= a.scale;
    qq.qx[4 * g] = v.x; qq.qx[4 * g + 1] = v.y; qq.qx[4 * g + 2] = v.z; qq.qx[4 * g + 3] = v.w;
  }
  qq.qf = a3_qflag<MODE>(a, c, min(r, c.nq - 1), magic);
  return qq;
}

// every load of a tile is unconditional (key indices clamped to nk - 1; such keys are masked): a conditional load
// costs a branch and a full vmcnt(0) round trip each
template <int MODE, bool SEL>
__device__ __forceinline__ A3Tile a3_load_tile(const AttnArgs& a, const A3Unit& c, int key0, int r, int h, unsigned magic) {
  A3Tile tl;
  const int lin_ld = (MODE == ATT_STEP_SELF) ? a.d : a.ldkv;
  if (key0 + 32 <= c.lin_limit) {                   // uniform: all 32 keys exist and are laid out linearly
    const float* kp = c.klin + (key0 + r) * lin_ld + 4 * h;
    tl.k0 = *reinterpret_cast<const float4*>(kp);
    tl.k1 = *reinterpret_cast<const float4*>(kp + 8);
    tl.k2 = *reinterpret_cast<const float4*>(kp + 16);
    tl.k3 = *reinterpret_cast<const float4*>(kp + 24);
    tl.own = a3_keyown<MODE>(a, c, key0 + r);
    const float* vp = c.vlin + (key0 + 4 * h) * lin_ld + r;
#pragma unroll
    for (int t = 0; t < 16; ++t) tl.v[t] = vp[((t & 3) + 8 * (t >> 2)) * lin_ld];
    return tl;
  }
  const float *kp, *vp;
  const int kown = min(key0 + r, c.nk - 1);
  a3_keyrow<MODE, SEL>(a, c, kown, magic, kp, vp);
  tl.k0 = *reinterpret_cast<const float4*>(kp + 4 * h);
  tl.k1 = *reinterpret_cast<const float4*>(kp + 4 * h + 8);
  tl.k2 = *reinterpret_cast<const float4*>(kp + 4 * h + 16);
  tl.k3 = *reinterpret_cast<const float4*>(kp + 4 * h + 24);
  tl.own = a3_keyown<MODE>(a, c, kown);
  if constexpr (SEL && MODE == ATT_STEP_SELF) {
    // the row of key key0 + r is mapped ONCE, by the lane that loads its K, and handed to the lanes that load its V (as the
    // visibility flags are in a3_tile_partial): an offset from the cache base (>= 0) or, complemented, from the step rows
    const int code = kown < c.f ? (int)(vp - c.vlin) : ~(int)(vp - c.vb);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int j0 = (t & 3) + 8 * (t >> 2);
      const int c0 = __builtin_amdgcn_readlane(code, j0), c1 = __builtin_amdgcn_readlane(code, j0 + 4);
      const int cc = h ? c1 : c0;
      tl.v[t] = (cc >= 0 ? c.vlin + cc : c.vb + ~cc)[r];
    }
    return tl;
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const float *kq, *vq;
    a3_keyrow<MODE, SEL>(a, c, min(key0 + (t & 3) + 8 * (t >> 2) + 4 * h, c.nk - 1), magic, kq, vq);
    tl.v[t] = vq[r];
  }
  return tl;
}

// One tile's partial (m_i = mx, l_i = rs, O_i = oi) from its loaded operands.
template <int MODE>
__device__ __forceinline__ void a3_tile_partial(const AttnArgs& a, const A3Unit& c, const A3Tile& cur, const A3Query& q, int key0,
                                                int r, int h, unsigned magic, float& mx, float& rs, f32x16& oi) {
  f32x16 sacc;
#pragma unroll
  for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k0.x, q.qx[0], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k0.y, q.qx[1], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k0.z, q.qx[2], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k0.w, q.qx[3], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k1.x, q.qx[4], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k1.y, q.qx[5], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k1.z, q.qx[6], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k1.w, q.qx[7], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k2.x, q.qx[8], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k2.y, q.qx[9], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k2.z, q.qx[10], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k2.w, q.qx[11], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k3.x, q.qx[12], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k3.y, q.qx[13], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k3.z, q.qx[14], sacc, 0, 0, 0);
  sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.k3.w, q.qx[15], sacc, 0, 0, 0);
  mx = -INFINITY;
  if (key0 + 32 <= c.n_plain) {                       // uniform: a tile of plain keys (most tiles)
    // validity of the tile's 32 keys as a bit mask (lanes 0..31 hold keys key0 .. key0+31), keys past nk cleared
    unsigned valid = (unsigned)__ballot(cur.own != 0);
    if (c.nk - key0 < 32) valid &= (1u << (c.nk - key0)) - 1u;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int j = (t & 3) + 8 * (t >> 2) + 4 * h;
      sacc[t] = ((valid >> j) & 1u) ? sacc[t] : -INFINITY;
      mx = fmaxf(mx, sacc[t]);
    }
  } else {
    // the flag of key key0 + r is worked out ONCE, by the lane that loaded the key (one magic-number division per lane and
    // tile), and handed to the lanes that hold its scores: key (t&3) + 8(t>>2) + 4h sits in lane (t&3) + 8(t>>2) (+ 4)
    const int kflag = a3_keyflag<MODE>(a, c, key0 + r, cur.own != 0, magic);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int j0 = (t & 3) + 8 * (t >> 2);
      const int kf0 = __builtin_amdgcn_readlane(kflag, j0), kf1 = __builtin_amdgcn_readlane(kflag, j0 + 4);
      const bool vis = a2_visible(q.qf, h ? kf1 : kf0);
      sacc[t] = vis ? sacc[t] : -INFINITY;
      mx = fmaxf(mx, sacc[t]);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32));                               // m_i
  const float base = (mx == -INFINITY) ? 0.f : mx;                  // nothing visible in this tile: every exp below is 0
  rs = 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    sacc[t] = __expf(sacc[t] - base);
    rs += sacc[t];
  }
  rs += __shfl_xor(rs, 32);                                          // l_i
#pragma unroll
  for (int i = 0; i < 16; ++i) oi[i] = 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t) oi = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.v[t], sacc[t], oi, 0, 0, 0);
}

// Few sequences: one workgroup per unit, its key tiles shared out over the four waves.
template <int MODE, bool SEL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_attn3(AttnArgs a) {
  static_assert(MODE == ATT_STEP_SELF || MODE == ATT_STEP_CROSS, "k_attn3 serves the verify step");
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) float a3_lds[];      // one A3_PART per key tile
  const int slot = blockIdx.x;
  if (slot >= a.st->n_active) return;
  const int RPS = step_rps(a.N, a.D);
  if ((int)blockIdx.z * A3_QT >= RPS) return;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
  const unsigned magic = a3_magic(a.D);
  const A3Unit c = a3_unit<MODE, SEL>(a, slot, blockIdx.y, blockIdx.z, RPS, magic);
  const A3Query q = a3_load_query<MODE, SEL>(a, c, r, h, magic);
  A3Tile cur = a3_load_tile<MODE, SEL>(a, c, min(wave, c.ntiles - 1) * 32, r, h, magic);
  for (int it = wave; it < c.ntiles; it += 4) {
    // the next tile's loads go out before this tile's arithmetic (the empty asm keeps them above it); the copy at the
    // bottom of the loop is where they are waited for
    A3Tile nxt = a3_load_tile<MODE, SEL>(a, c, min(it + 4, c.ntiles - 1) * 32, r, h, magic);
    asm volatile("" ::: "memory");
    float mx, rs;
    f32x16 oi;
    a3_tile_partial<MODE>(a, c, cur, q, it * 32, r, h, magic, mx, rs, oi);
    float* part = a3_lds + (size_t)it * A3_PART;
#pragma unroll
    for (int i = 0; i < 16; ++i) part[i * 64 + lane] = oi[i];
    if (h == 0) { part[16 * 64 + r] = mx; part[16 * 64 + 32 + r] = rs; }
    cur = nxt;
  }
  __syncthreads();
  float m = -INFINITY, l = 0.f;
  float o4[4] = {0.f, 0.f, 0.f, 0.f};
  for (int it = 0; it < c.ntiles; ++it) {            // the fold, in tile order; this wave owns values 4w .. 4w+3
    const float* part = a3_lds + (size_t)it * A3_PART;
    float fa, fb;
    a3_fold(m, l, part[16 * 64 + r], part[16 * 64 + 32 + r], fa, fb);
#pragma unroll
    for (int v = 0; v < 4; ++v) o4[v] = __fmaf_rn(o4[v], fa, __fmul_rn(part[(4 * wave + v) * 64 + lane], fb));
  }
  if (SEL ? q.orow >= 0 : r < c.nq) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    f32x4 w = {o4[0] * inv, o4[1] * inv, o4[2] * inv, o4[3] * inv};
    *reinterpret_cast<f32x4*>(c.out + (size_t)(SEL ? q.orow : r) * a.d + 4 * h + 8 * wave) = w;
  }
}

// Many sequences: the units of the launch as a STREAM.  A pool launch reads ~8 KB of K/V per tile and head, and a wave that
// handled one unit and exited would spend its first tile's memory latency (and the dependent scalar loads in front of it:
// slot -> sequence -> front / source) idle, in phase with every other wave that started with it.  Here the grid has the
// machine's size (two waves per SIMD) and every wave walks units u = wave, wave + W, ...: while the last tile of a unit is in the
// matrix pipe, the first tile and the queries of the NEXT unit are already in flight, and that unit's scalars were fetched one
// unit earlier.
template <int MODE, bool SEL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_attn3s(AttnArgs a, int H, int qtiles) {
  static_assert(MODE == ATT_STEP_SELF || MODE == ATT_STEP_CROSS, "k_attn3s serves the verify step");
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int RPS = step_rps(a.N, a.D);
  const unsigned magic = a3_magic(a.D);
  const int W = (int)gridDim.x * 4;
  const int n_units = a.st->n_active * H * qtiles;
  int u = a3_uniform((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (u >= n_units) return;
  // unit u = ((slot * qtiles) + q tile) * H + head
  auto unit = [&](int uu) {
    const int head = uu % H, t = uu / H;
    return a3_unit<MODE, SEL>(a, t / qtiles, head, t % qtiles, RPS, magic);
  };
  A3Unit cu = unit(u);
  A3Query cq = a3_load_query<MODE, SEL>(a, cu, r, h, magic);
  A3Tile cur = a3_load_tile<MODE, SEL>(a, cu, 0, r, h, magic);
  int un = u + W;
  A3Unit nu = unit(min(un, n_units - 1));               // the next unit's scalars, one unit ahead
  float m = -INFINITY, l = 0.f;
  f32x16 o;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
  int it = 0;
  for (;;) {
    const bool last = it + 1 >= cu.ntiles;
    const bool more = un < n_units;
    // what the matrix pipe needs next goes out before this tile's arithmetic: the unit's next tile, or the first tile and the
    // queries of the next unit
    A3Tile nxt = cur;
    A3Query nq = cq;
    if (!last) {
      nxt = a3_load_tile<MODE, SEL>(a, cu, it * 32 + 32, r, h, magic);
    } else if (more) {
      nxt = a3_load_tile<MODE, SEL>(a, nu, 0, r, h, magic);
      nq = a3_load_query<MODE, SEL>(a, nu, r, h, magic);
    }
    asm volatile("" ::: "memory");
    float mx, rs, fa, fb;
    f32x16 oi;
    a3_tile_partial<MODE>(a, cu, cur, cq, it * 32, r, h, magic, mx, rs, oi);
    a3_fold(m, l, mx, rs, fa, fb);
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = __fmaf_rn(o[i], fa, __fmul_rn(oi[i], fb));
    cur = nxt;
    if (!last) {
      ++it;
      continue;
    }
    // o[v] = O[query r][dim (v&3) + 8(v>>2) + 4h]: four float4 per lane
    if (SEL ? cq.orow >= 0 : r < cu.nq) {
      const float inv = l > 0.f ? 1.0f / l : 0.f;
      float* op = cu.out + (size_t)(SEL ? cq.orow : r) * a.d + 4 * h;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        f32x4 w = {o[4 * v] * inv, o[4 * v + 1] * inv, o[4 * v + 2] * inv, o[4 * v + 3] * inv};
        *reinterpret_cast<f32x4*>(op + 8 * v) = w;
      }
    }
    if (!more) break;
    cu = nu;
    cq = nq;
    un += W;
    nu = unit(min(un, n_units - 1));
    it = 0;
    m = -INFINITY;
    l = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
  }
}

// One step row per sequence (q_per_group == 1: the probe of a two-phase verify step, any (1, 0) step launch).  k_attn3s would give
// such a unit a 32-column MFMA tile with 31 copies of the one query; here the same fmaf chains run on the VALU, in the order the
// MFMAs of a3_tile_partial contract them (dims 8g + c + 4h, keys (t&3) + 8(t>>2) + 4h), so the bits are those of k_attn3 /
// k_attn3s.  A wave takes two heads of one slot, one per 32-lane half.  Scores: lane = key, its 128-B K row in registers, the
// scaled query of the half's head in 32 registers.  Output: lane = dim, the tile's 32 probabilities handed over through LDS (every
// lane of a half reads the same addresses: a broadcast), V rows read 256 B at a time across the wave.  No unit is walked: one
// wave, one (slot, head pair); the launch leaves latency hiding to the waves resident beside it.
template <int MODE>
__global__ __launch_bounds__(64) void k_attn1(AttnArgs a) {
  static_assert(MODE == ATT_STEP_SELF || MODE == ATT_STEP_CROSS, "k_attn1 serves the verify step");
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) float a1_p[2][64];          // the probabilities of a tile, two tiles in turn
  constexpr int A1_KROW = 36;                                            // floats between the LDS rows of two keys
  __shared__ __attribute__((aligned(16))) float a1_k[64 * A1_KROW + 32];    // the K rows of a tile: [head of the pair][key][32 dims]
  const int slot = blockIdx.x;
  if (slot >= a.st->n_active) return;
  const int lane = threadIdx.x, r = lane & 31, ho = (lane >> 5) * ATT_DH;
  const A3Unit c = a3_unit<MODE, false>(a, slot, 2 * (int)blockIdx.y, 0, 1, 0u);
  float q[32];
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(c.q + ho + 4 * g);
    q[4 * g] = __fmul_rn(v.x, a.scale); q[4 * g + 1] = __fmul_rn(v.y, a.scale);
    q[4 * g + 2] = __fmul_rn(v.z, a.scale); q[4 * g + 3] = __fmul_rn(v.w, a.scale);
  }
  // K / V row of key `key` < nk (a3_keyrow with one step row: the cached prefix, then the slot's row of this step), as a select
  auto a1_row = [&](int key, const float* lin, const float* stp) -> const float* {
    if constexpr (MODE == ATT_STEP_SELF) return key < c.f ? lin + key * a.d : stp;
    else return lin + key * a.ldkv;
  };
  // every load is unconditional, key indices clamped to nk - 1 (such keys are masked), as in a3_load_tile.  K rows are fetched
  // whole: the 256 B a key holds for the two heads go to 16 consecutive lanes (load j: keys 4j .. 4j + 3), so that every 128-B line
  // is touched by one instruction, and reach the lane that owns the key through LDS (row of (head, key): 144 B apart, the second
  // head's rows 128 B further, which keeps both the 16-byte writes and the row reads off each other's banks).
  const int kc4 = (lane & 15) * 4, ksub = lane >> 4;
  float* const kst = a1_k + (lane & 8) * (A1_KROW * 4 + 4) + (lane & 7) * 4;      // + key * A1_KROW: where this lane's pieces go
  const float* const krd = a1_k + (lane >> 5) * (A1_KROW * 32 + 32) + r * A1_KROW;
  f32x4 kg[8];
  int own;
  auto load_k = [&](int key0) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      kg[j] = *reinterpret_cast<const f32x4*>(a1_row(min(key0 + 4 * j + ksub, c.nk - 1), c.klin, c.kb) + kc4);
    own = a3_keyown<MODE>(a, c, min(key0 + r, c.nk - 1));
  };
  float m = -INFINITY, l = 0.f, o = 0.f;
  if (c.ntiles > 0) load_k(0);
  for (int it = 0; it < c.ntiles; ++it) {
    const int key0 = it * 32;
    // the tile's V rows go out before its scores are worked out, and the next tile's K rows right after them, into the registers
    // the scores have just freed (the empty asm statements keep the loads where they stand).  The tile index of that prefetch is
    // clamped, as in k_attn3: a unit's last iteration fetches its last tile's K rows again (from L1 / L2) and never uses them,
    // which keeps the loop body free of a branch around loads and of the full vmcnt(0) wait such a branch costs
    float vv[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      vv[j] = a1_row(min(key0 + j, c.nk - 1), c.vlin, c.vb)[ho + r];
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(kst + (4 * j + ksub) * A1_KROW) = kg[j];
    __syncthreads();
    f32x4 kk[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) kk[g] = *reinterpret_cast<const f32x4*>(krd + 4 * g);
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s = __fmaf_rn(kk[2 * g][e], q[8 * g + e], s);
        s = __fmaf_rn(kk[2 * g + 1][e], q[8 * g + 4 + e], s);
      }
    s = (key0 + r < c.nk && own != 0) ? s : -INFINITY;
    asm volatile("" ::: "memory");
    __syncthreads();                                                    // every row of the tile has been read
    load_k(min(it + 1, c.ntiles - 1) * 32);
    asm volatile("" ::: "memory");
    float mx = s;                                                       // m_i: over the 32 keys of the half
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float base = (mx == -INFINITY) ? 0.f : mx;                  // nothing visible in this tile: every exp below is 0
    float* pl = a1_p[it & 1];
    pl[lane] = __expf(s - base);
    __syncthreads();
    float p[32];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(pl + ho + 4 * g);
      p[4 * g] = v.x; p[4 * g + 1] = v.y; p[4 * g + 2] = v.z; p[4 * g + 3] = v.w;
    }
    float rs0 = 0.f, rs1 = 0.f, oi = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int j = (t & 3) + 8 * (t >> 2);
      rs0 = __fadd_rn(rs0, p[j]);
      rs1 = __fadd_rn(rs1, p[j + 4]);
      oi = __fmaf_rn(vv[j], p[j], oi);
      oi = __fmaf_rn(vv[j + 4], p[j + 4], oi);
    }
    float fa, fb;
    a3_fold(m, l, mx, __fadd_rn(rs0, rs1), fa, fb);                     // l_i
    o = __fmaf_rn(o, fa, __fmul_rn(oi, fb));
  }
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  c.out[ho + r] = o * inv;
}

// ------------------------------------------------------------------------------------------------
static constexpr size_t kAttn2LdsLimit = 150 * 1024;

template <int MODE, int DH>
static int launch_attn_mode(ttx_session* s, hipStream_t st, const AttnArgs& a, int groups, int H, int q_per_group, int max_keys, int N, int D1) {
  if (groups <= 0 || q_per_group <= 0) return TTX_OK;
  constexpr bool step = (MODE == ATT_STEP_SELF || MODE == ATT_STEP_CROSS);
  // step modes: q_per_group = RPS = 1 + N*D rows per running sequence.  Self-attention keys of one workgroup:
  // prefix (< max_keys) + front row + the rows of every draft with a query among its 64 rows.
  const int D = D1 - 1;
  // test hook (ttx_debug_attn): a forced kernel replaces the choice below and is refused where it cannot serve the launch;
  // unset (0), want3 and want2 are the production conditions
  const int force = s->attn_force;
  const bool want3 = force ? (force == AK_ATTN3 || force == AK_ATTN3S || force == AK_ATTN1) : !s->attn_fallback;
  const bool want2 = force ? force == AK_ATTN2 : !s->attn_fallback;
  if (force == AK_ATTN1 && !(step && H % 4 == 0 && DH == ATT_DH && q_per_group == 1))
    return fail(TTX_ERR_INVALID, "k_attn1 serves one-row step launches (N * D = 0) at head dimension 32 with a head count that is a multiple of 4");
  if ((force == AK_ATTN3 || force == AK_ATTN3S) && !(step && H % 4 == 0 && DH == ATT_DH))
    return fail(TTX_ERR_INVALID, "k_attn3 / k_attn3s serve the step modes at head dimension 32 with a head count that is a multiple of 4");
  // draft select (a.row_base / a.draft_mask): compacted step rows, which only the SEL instantiations of k_attn3 / k_attn3s read
  const bool sel = a.row_base != nullptr;
  if (sel && !(step && DH == ATT_DH && H % 4 == 0 && want3 && a.draft_mask && N <= 32 && D >= 1))
    return fail(TTX_ERR_INVALID, "draft select runs on k_attn3 / k_attn3s only: a step launch at head dimension 32, a head count that is a "
                                 "multiple of 4, 1 <= N <= 32 and D >= 1");
  if constexpr (step && DH == ATT_DH) {
    // the verify step: one wave per (sequence, head, 32 step rows), registers only — no key-count limit.  Head dimension 32
    // only: at 64 a step launch takes the route below (k_attn2, k_attn beyond its capacity) whatever H is.
    if (H % 4 == 0 && want3) {
      // few sequences (a 32-row batch): the key tiles of one (sequence, head) are shared out over the four waves of
      // a workgroup (k_attn3); many (row groups, slot pools): one wave per (sequence, head), streamed (k_attn3s).
      // Bit-identical either way.
      const int qtiles = cdiv(q_per_group, A3_QT);
      const int keys3 = (MODE == ATT_STEP_SELF) ? max_keys + 1 + N * std::max(D, 0) : max_keys;
      const size_t lds3 = sizeof(float) * (size_t)A3_PART * cdiv(keys3, 32);
      bool split = s->attn_split != 0 && (s->attn_split > 0 || (long long)groups * H * qtiles < TTX_A3_SPLIT_BELOW) && lds3 <= 64 * 1024;
      if (force == AK_ATTN3 && lds3 > 64 * 1024) return fail(TTX_ERR_INVALID, "k_attn3: the parked tile partials exceed 64 KB of LDS");
      if (force) split = (force == AK_ATTN3);
      // one row per sequence (the probe of a two-phase step): the launches k_attn3s would get run on k_attn1, bit-identical too.
      // Like `split`, decided by what a step's graph key holds (groups, layout) and the session's switches.
      const bool row = force ? force == AK_ATTN1 : (q_per_group == 1 && !sel && s->attn_row != 0 && (s->attn_row > 0 || !split));
      s->last_attn_kernel = row ? AK_ATTN1 : split ? AK_ATTN3 : AK_ATTN3S;
      if (row) {
        hipLaunchKernelGGL((k_attn1<MODE>), dim3(groups, H / 2), dim3(64), 0, st, a);
      } else if (split) {
        if (sel) hipLaunchKernelGGL((k_attn3<MODE, true>), dim3(groups, H, qtiles), dim3(256), lds3, st, a);
        else hipLaunchKernelGGL((k_attn3<MODE, false>), dim3(groups, H, qtiles), dim3(256), lds3, st, a);
      } else {
        // a grid of the machine's size (two workgroups = eight waves per CU), every wave walking its share of the units
        const long long units = (long long)groups * H * qtiles;
        const int wgs = (int)std::min<long long>((units + 3) / 4, (long long)TTX_A3S_WGS_PER_CU * s->m->n_cu);
        if (sel) hipLaunchKernelGGL((k_attn3s<MODE, true>), dim3(wgs), dim3(256), 0, st, a, H, qtiles);
        else hipLaunchKernelGGL((k_attn3s<MODE, false>), dim3(wgs), dim3(256), 0, st, a, H, qtiles);
      }
      HIP_TRY(hipGetLastError());
      return TTX_OK;
    }
  }
  const int draft_keys = (D > 0) ? (std::min(N, (A2_QT + D - 2) / D + 1)) * D : 0;
  const int keys2 = (MODE == ATT_STEP_SELF) ? max_keys + 1 + draft_keys : max_keys;
  const size_t lds2 = attn2_lds_bytes(keys2, a2_qcap(q_per_group), DH);
  if (force == AK_ATTN2 && !(lds2 <= kAttn2LdsLimit && attn2_fits(keys2, DH)))
    return fail(TTX_ERR_INVALID, "k_attn2: more keys than its register and LDS images hold");
  // k_attn2 or k_attn: the two do not give the same bits, and the probe of a two-phase verify step recomputes row 0 of a launch in
  // the layout (attn_sel_N, attn_sel_D).  It takes the kernel THAT launch takes (whose images hold the probe's fewer keys and rows).
  bool fits2 = lds2 <= kAttn2LdsLimit && attn2_fits(keys2, DH);
  if (step && s->attn_sel_N > 0) {
    const int cN = s->attn_sel_N, cD = s->attn_sel_D;
    const int c_draft = (cD > 0) ? (std::min(cN, (A2_QT + cD - 2) / cD + 1)) * cD : 0;
    const int c_keys2 = (MODE == ATT_STEP_SELF) ? max_keys + 1 + c_draft : max_keys;
    fits2 = fits2 && attn2_lds_bytes(c_keys2, a2_qcap(step_rps(cN, cD)), DH) <= kAttn2LdsLimit && attn2_fits(c_keys2, DH);
  }
  if (fits2 && want2) {
    s->last_attn_kernel = AK_ATTN2;
    const int tiles = cdiv(q_per_group, A2_QT);
    bool& attr_set = s->attr_attn2[DH == ATT_DH ? 0 : 1][MODE];
    if (lds2 > 64 * 1024 && !attr_set) {                        // per device: kept per session, set outside graph capture
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn2<MODE, DH>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)kAttn2LdsLimit));
      attr_set = true;
    }
    hipLaunchKernelGGL((k_attn2<MODE, DH>), dim3(groups, H, tiles), dim3(256), lds2, st, a);
    HIP_TRY(hipGetLastError());
    return TTX_OK;
  }
  const int keys1 = (MODE == ATT_STEP_SELF) ? max_keys + q_per_group : max_keys;
  const size_t lds = attn_lds_bytes(keys1, DH);
  if (lds > kAttn2LdsLimit) return fail(TTX_ERR_INVALID, "sequence too long for the attention kernels' LDS score buffer");
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn<MODE, DH>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  s->last_attn_kernel = AK_ATTN;
  hipLaunchKernelGGL((k_attn<MODE, DH>), dim3(groups, H, cdiv(q_per_group, ATT_MAXQ)), dim3(64), lds, st, a);
  HIP_TRY(hipGetLastError());
  return TTX_OK;
}

template <int DH>
static int launch_attn_dh(int mode, ttx_session* s, hipStream_t st, const AttnArgs& a, int groups, int H, int q_per_group, int max_keys,
                          int N, int D1) {
  switch (mode) {
    case ATT_ENC: return launch_attn_mode<ATT_ENC, DH>(s, st, a, groups, H, q_per_group, max_keys, N, D1);
    case ATT_FULL_SELF: return launch_attn_mode<ATT_FULL_SELF, DH>(s, st, a, groups, H, q_per_group, max_keys, N, D1);
    case ATT_FULL_CROSS: return launch_attn_mode<ATT_FULL_CROSS, DH>(s, st, a, groups, H, q_per_group, max_keys, N, D1);
    case ATT_STEP_SELF: return launch_attn_mode<ATT_STEP_SELF, DH>(s, st, a, groups, H, q_per_group, max_keys, N, D1);
    case ATT_STEP_CROSS: return launch_attn_mode<ATT_STEP_CROSS, DH>(s, st, a, groups, H, q_per_group, max_keys, N, D1);
  }
  return fail(TTX_ERR_INVALID, "unknown attention mode");
}

// the head dimension of a launch is a.d / H
int launch_attn(int mode, ttx_session* s, hipStream_t st, const AttnArgs& a, int groups, int H, int q_per_group, int max_keys,
                int N, int D1) {
  if (!(H > 0 && (a.d == H * 32 || a.d == H * 64))) return fail(TTX_ERR_INVALID, "attention kernels exist for head dimensions 32 and 64");
  s->last_attn_kernel = 0;
  const int rc = a.d == H * 32 ? launch_attn_dh<32>(mode, s, st, a, groups, H, q_per_group, max_keys, N, D1)
                               : launch_attn_dh<64>(mode, s, st, a, groups, H, q_per_group, max_keys, N, D1);
  if (rc == TTX_OK && s->last_attn_kernel) s->attn_kernels_seen |= 1u << s->last_attn_kernel;      // what a test reads back
  return rc;
}

// Keys k_attn2 can stage for one workgroup at head dimension `head_dim` when a group has `q_per_group` query rows: the register
// image of V and the LDS limit, whichever is reached first (ttx_attn_staged_key_limit).
int attn_staged_key_limit(int head_dim, int q_per_group) {
  if ((head_dim != 32 && head_dim != 64) || q_per_group <= 0) return 0;
  int keys = 32 * a2_vsteps(head_dim);
  while (keys > 0 && attn2_lds_bytes(keys, a2_qcap(q_per_group), head_dim) > kAttn2LdsLimit) keys -= 32;
  return keys;
}

// ------------------------------------------------------------------------------------------------
// Test entry point (ttx_debug_attn): ONE launch of launch_attn on the caller's device operands.  What the kernels take on trust
// from the production call sites and the host can see is checked here, so that a test cannot launch a kernel on arguments it
// cannot handle; the device-side index arrays and the front positions (<= max_keys, as under production's kcap) are the caller's.
static bool attn_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int attn_debug(ttx_session* s, const AttnArgs& in, int H, int head_dim, int mode, int groups, int n_active, int max_keys, int kernel,
               int32_t* kernel_id, hipStream_t st) {
  if (!s) return fail(TTX_ERR_INVALID, "null session");
  if (head_dim != 32 && head_dim != 64) return fail(TTX_ERR_INVALID, "ttx_debug_attn_hd: head_dim is 32 or 64");
  if (mode < ATT_ENC || mode > ATT_STEP_CROSS || kernel < 0 || kernel > AK_ATTN1)
    return fail(TTX_ERR_INVALID, "ttx_debug_attn: mode is 0..4, kernel 0..5");
  if (H <= 0 || groups <= 0 || max_keys <= 0) return fail(TTX_ERR_INVALID, "ttx_debug_attn: H, groups and max_keys must be positive");
  const bool step = (mode == ATT_STEP_SELF || mode == ATT_STEP_CROSS);
  const bool cross = (mode == ATT_FULL_CROSS || mode == ATT_STEP_CROSS);
  AttnArgs a = in;
  a.d = H * head_dim;
  if (!a.q || !a.k || !a.v || !a.out) return fail(TTX_ERR_INVALID, "ttx_debug_attn: q, k, v and out are required");
  if (cross ? !a.key_pad : !a.tok) return fail(TTX_ERR_INVALID, "ttx_debug_attn: self modes need tok, cross modes key_pad");
  if (step && !a.act_idx) return fail(TTX_ERR_INVALID, "ttx_debug_attn: the step modes need act_idx");
  if (mode == ATT_STEP_SELF && (!a.front || !a.kcache || !a.vcache))
    return fail(TTX_ERR_INVALID, "ttx_debug_attn: STEP_SELF needs front, kcache and vcache");
  if ((a.ldq & 3) || (a.ldkv & 3) || a.ldq < a.d || a.ldkv < a.d)
    return fail(TTX_ERR_INVALID, "ttx_debug_attn: ldq and ldkv must be multiples of 4 that cover d = head_dim * H");
  for (const void* p : {(const void*)a.q, (const void*)a.k, (const void*)a.v, (const void*)a.out, (const void*)a.kcache, (const void*)a.vcache})
    if (!attn_aligned16(p)) return fail(TTX_ERR_INVALID, "ttx_debug_attn: float operands must be 16-byte aligned");
  int q_per_group = a.L;
  if (step) {
    if (a.N < 1 || a.D < 0) return fail(TTX_ERR_INVALID, "ttx_debug_attn: step modes need N >= 1 and D >= 0");
    if (n_active < 0 || n_active > groups) return fail(TTX_ERR_INVALID, "ttx_debug_attn: n_active must lie in [0, groups]");
    if (mode == ATT_STEP_SELF && (a.gen_ld <= 0 || a.cache_seq_stride <= 0 || (a.cache_seq_stride & 3)))
      return fail(TTX_ERR_INVALID, "ttx_debug_attn: STEP_SELF needs gen_ld > 0 and a cache_seq_stride that is a positive multiple of 4");
    q_per_group = step_rps(a.N, a.D);
  } else if (a.L <= 0 || (mode != ATT_FULL_CROSS && max_keys < a.L)) {
    return fail(TTX_ERR_INVALID, "ttx_debug_attn: L must be positive and max_keys cover it");
  }
  if (cross && (a.Lk <= 0 || max_keys < a.Lk)) return fail(TTX_ERR_INVALID, "ttx_debug_attn: Lk must be positive and max_keys cover it");
  HIP_TRY(hipSetDevice(s->m->device));
  DecState* dst = nullptr;
  if (step) {
    // n_active reaches the kernels as production hands it over: in a DecState on the device, written on the launch's stream
    HIP_TRY(hipMalloc((void**)&dst, sizeof(DecState)));
    hipError_t e = hipMemsetAsync(dst, 0, sizeof(DecState), st);
    if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&dst->n_active), n_active, 1, st);
    if (e != hipSuccess) { (void)hipFree(dst); HIP_TRY(e); }
    a.st = dst;
  }
  const int keep = s->attn_force;
  s->attn_force = kernel;
  s->last_attn_kernel = 0;
  int rc = launch_attn(mode, s, st, a, groups, H, q_per_group, max_keys, step ? a.N : 1, step ? a.D + 1 : 1);
  s->attn_force = keep;
  if (dst) {
    const hipError_t e = hipStreamSynchronize(st);     // the launch reads the state: keep it until the launch is through
    (void)hipFree(dst);
    if (rc == TTX_OK) HIP_TRY(e);
  }
  if (rc == TTX_OK && kernel_id) *kernel_id = s->last_attn_kernel;
  return rc;
}

}  // namespace ttx
