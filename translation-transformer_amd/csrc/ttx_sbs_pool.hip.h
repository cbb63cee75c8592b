// Stochastic beam search on a pool of source slots (ttx_sbs_generate_pool; included by ttx_api.hip only).  Hand-written HIP for
// gfx950, wave64.
//
// Why a pool over SOURCES is exact.  The K rows of a source depend on the source, its key, its prefix, the seed, the temperature,
// the filter and K only (include/ttx.h, ttx_sbs_generate): nothing in the rule looks across sources, the noise is keyed by
// (key, parent rank, token, position), and a source all of whose K candidates are finished is a fixed point of the step (K finished
// parents, one PAD child each with phi and G unchanged, selected in the order they already stand in).  The per-batch loop keeps
// such a source until the batch's last row ends; the pool hands its rows out at once and gives the slot to the next source.
//
// The pool owns C source slots of K candidates each, candidate c = slot * K + k.  What the per-batch loop passes to k_sbs_step as
// launch scalars is per-slot state here, read on the device:
//   row_of   the source's row of the call's outputs, -1: the slot is free
//   level    pos = width = the length of the slot's candidates (1 at admission)
//   nlive    parents of the next step: 1 at the source's first level (the <BOS> candidate at k = 0), K afterwards
//   key      the source's row key
//   pfx_len, pfx_src   the source's prefix length and its row of the call's prefix table (PrefixTab by slot)
//   nfin     how many of the K candidates the last step produced are finished
//   iteration = k_bs_prep (N = 1, dl = 0) -> k_tree_cache (two buffers) -> k_bs_list -> verify step -> k_sbs_step_pool or
//               k_sbs_step_pool_masked -> k_sbsp_retire -> k_sbsp_publish           (admission: k_sbsp_admit -> k_sbsp_fill)
// Free slots and the K - 1 candidates a fresh source does not have yet are `finished` in the candidate arrays, so that the shared
// kernels neither decode nor cache them; the step kernel never reads them (it looks at nlive parents).
//
// Hazards the bookkeeping answers:
//   G ping-pongs between two buffers by the parity of the POOL's iteration, not of the source's level: admission writes G = 0 into
//     the buffer the next iteration reads, retirement reads the buffer the step of its own iteration wrote.
//   A reused slot carries nothing over: k_sbsp_fill rewrites every per-slot word, all K candidate rows and flags and the parents
//     (-1: k_tree_cache inherits nothing), and the source's keys of the cross K/V; positions beyond the source are masked by the
//     slot's source length.
//   An iteration is replayed from a graph captured by an earlier call: whatever belongs to the call (the output arrays) is read
//     through a device block (SbsPoolIo) that every call rewrites; the keys and lengths of the call are read at admission only,
//     which is never captured.
//   Retirement frees the slot in the iteration that finished it: all K finished, or the slot's own level at max_len - 1.
#pragma once
#include "ttx_sbs.hip.h"

namespace ttx {

struct SbsPoolStepArgs {
  const float* logits; int V;                   // the step's logits, one row per running candidate (compact order)
  const int* slot_of; const uint8_t* finished; const float* phi; const float* g;   // [C * K]
  const int* gen; int ld;                       // current rows [C * K, ld]
  int C, K, pad, eos;
  const int* row_of; const int* level; const int* nlive; const int64_t* key;       // [C] (see the head of this file)
  unsigned long long seed; float inv_T;
  int64_t* new_cand; float* new_phi; float* new_g; int* parent; int* new_len; uint8_t* new_finished; int* parent_draft;
  int* nfin;                                    // [C]: finished ones among the slot's K new candidates
  // k_sbs_step_pool_masked only
  int top_k; float top_p;                       // top_k 0: filter off (then top_p is 1); else 1..32
  PrefixTab pfx;                                // len and src by SLOT (tok null: no forced prefixes)
};

// k_sbs_step over the live slots of a pool: the rule, the walk and every floating-point expression are k_sbs_step's, statement
// for statement; pos, width, the parent count and the key come from the slot.  A free slot's workgroup writes nothing.
__global__ __launch_bounds__(256) void k_sbs_step_pool(SbsPoolStepArgs a) {
  extern __shared__ float img[];                // [K * V]
  __shared__ float s_m[SBS_MAX_BEAM], s_logz[SBS_MAX_BEAM];
  __shared__ float s_best[4];
  __shared__ int s_bi[4];
  __shared__ int s_sel;
  const int b = blockIdx.x;
  if (a.row_of[b] < 0) return;                  // workgroup-uniform
  const int pos = a.level[b], width = pos;
  const int beam = min(max(a.nlive[b], 1), a.K);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long key = (unsigned long long)a.key[b];
  const float qnan = __int_as_float(0x7fc00000);
  for (int k = wave; k < beam; k += 4) {
    const int c = b * a.K + k;
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
      philox4x32_10((unsigned)key, (unsigned)(key >> 32), 0x80000000u | ((unsigned)k << 8) | (unsigned)(v0 >> 2), (unsigned)pos,
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
  const int n = beam * a.V;
  int nfin = 0;                                 // thread 0's
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
    const int c = b * a.K + k, out = b * a.K + r;
    const int* root = a.gen + (size_t)c * a.ld;
    int64_t* dst = a.new_cand + (size_t)out * a.ld;
    for (int col = threadIdx.x; col < a.ld; col += 256) dst[col] = col < width ? (int64_t)root[col] : (col == width ? (int64_t)tok : (int64_t)a.pad);
    if (threadIdx.x == 0) {
      const bool pfin = a.finished[c] != 0;
      const float Gc = img[sel];
      const float phic = pfin ? a.phi[c] : a.phi[c] + sbs_logprob(a.logits[(size_t)a.slot_of[c] * a.V + tok], a.inv_T, s_m[k], s_logz[k]);
      a.new_phi[out] = phic;
      a.new_g[out] = Gc;
      a.parent[out] = c;
      a.parent_draft[out] = 0;
      a.new_len[out] = width + 1;
      const bool fin = pfin || tok == a.eos || tok == a.pad || Gc == -INFINITY;
      a.new_finished[out] = fin ? 1 : 0;
      nfin += fin ? 1 : 0;
      img[sel] = qnan;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) a.nfin[b] = nfin;
}

// k_sbs_step_masked over the live slots of a pool (see k_sbs_step_pool).  blockDim.x = 64 * waves, waves in {4, 8, 16}.
template <int VPL>
__global__ __launch_bounds__(64 * SBS_MASKED_MAX_WAVES) void k_sbs_step_pool_masked(SbsPoolStepArgs a) {
  extern __shared__ float img[];                // [K * V]
  __shared__ float s_m[SBS_MAX_BEAM], s_logz[SBS_MAX_BEAM];
  __shared__ int s_forced[SBS_MAX_BEAM];        // the forced token of a parent at a forced position, else -1
  __shared__ float s_best[SBS_MASKED_MAX_WAVES];
  __shared__ int s_bi[SBS_MASKED_MAX_WAVES];
  __shared__ int s_sel;
  const int b = blockIdx.x;
  if (a.row_of[b] < 0) return;                  // workgroup-uniform
  const int pos = a.level[b], width = pos;
  const int beam = min(max(a.nlive[b], 1), a.K);
  const int nthr = blockDim.x, nw = nthr >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long key = (unsigned long long)a.key[b];
  const float qnan = __int_as_float(0x7fc00000);
  const bool forced = a.pfx.tok && pos <= a.pfx.len[b] && pos <= a.pfx.ld;      // workgroup-uniform
  const int ftok = forced ? prefix_token(a.pfx, b, pos, a.V) : -1;
  for (int k = wave; k < beam; k += nw) {
    const int c = b * a.K + k;
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
      if (n_kept <= 1) {                        // wave-uniform.  A mask of one token, as a forced position is
        const int only = __shfl(my_idx, 0, 64);
        for (int v = lane; v < a.V; v += 64) im[v] = (v == only) ? Gk : -INFINITY;
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
      philox4x32_10((unsigned)key, (unsigned)(key >> 32), 0x80000000u | ((unsigned)k << 8) | (unsigned)(v0 >> 2), (unsigned)pos,
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
  const int n = beam * a.V;
  int nfin = 0;                                 // thread 0's
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
    const int c = b * a.K + k, out = b * a.K + r;
    const int* root = a.gen + (size_t)c * a.ld;
    int64_t* dst = a.new_cand + (size_t)out * a.ld;
    for (int col = threadIdx.x; col < a.ld; col += nthr) dst[col] = col < width ? (int64_t)root[col] : (col == width ? (int64_t)tok : (int64_t)a.pad);
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
      a.new_len[out] = width + 1;
      const bool fin = pfin || tok == a.eos || tok == a.pad || Gc == -INFINITY;
      a.new_finished[out] = fin ? 1 : 0;
      nfin += fin ? 1 : 0;
      img[sel] = qnan;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) a.nfin[b] = nfin;
}

// ------------------------------------------------------------------------------------------------
// Pool bookkeeping (modelled on k_bsp_*; the pinned block the host polls is the beam pool's BeamPoolHost).
// The caller's output arrays of one pool call, in a device block of the session: an iteration is replayed from a captured graph, which
// must not hold pointers of the call that captured it.
struct SbsPoolIo {
  int64_t* out; float* out_logp; float* out_gumbel;     // [S][K][max_len], [S][K], [S][K]
  int* src_running;                                     // [S] or null: the candidates each source had decoded, summed over its levels
};

struct SbsPoolArgs {
  int C, K, max_len, ld, Ls_cap, pad, bos;
  int* row_of; int* level; int* nlive; int* nfin; int64_t* key; int* pfx_len; int* pfx_src;        // [C]
  int* run_acc;                                 // [C]: candidates the slot's source has had decoded so far (1 at its first level)
  int64_t* cand_next; int* len_next; uint8_t* fin_next; float* phi_next; int* parent; int* parent_draft; int* cand_src_len;   // [C * K]
  float* g_in;                                  // G as the NEXT step reads it (admission writes here)
  const float* g_out;                           // G as this iteration's step wrote it (retirement reads here)
  // by source row of the call
  const int* len_all; const int64_t* row_keys; const int* pfx_len_src;      // row_keys null: the row index; pfx_len_src null: no prefixes
  const SbsPoolIo* io;
  BeamCounters* cnt; BeamPoolHost* host; int* dev_summary;                   // dev_summary [4]: live slots, running candidates, error, -
};

// Every slot free, every candidate finished and without a parent, the counters and the pinned block zero.
__global__ void k_sbsp_init(SbsPoolArgs a, float* g_a, float* g_b, int* src_of) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
  const int MC = a.C * a.K;
  for (int i = tid; i < a.C; i += nth) {
    a.row_of[i] = -1; a.level[i] = 1; a.nlive[i] = 0; a.nfin[i] = 0; a.key[i] = 0; a.pfx_len[i] = 0; a.pfx_src[i] = 0;
    a.run_acc[i] = 0;
  }
  for (size_t i = tid; i < (size_t)MC * a.ld; i += nth) a.cand_next[i] = a.pad;
  for (int i = tid; i < MC; i += nth) {
    a.len_next[i] = 1; a.fin_next[i] = 1; a.phi_next[i] = 0.f; a.parent[i] = -1; a.parent_draft[i] = 0; a.cand_src_len[i] = 1;
    g_a[i] = 0.f; g_b[i] = 0.f; src_of[i] = i / a.K;
  }
  if (tid == 0) {
    a.cnt->model_calls = 0; a.cnt->input_lines = 0; a.cnt->running_rows = 0; a.cnt->verified_positions = 0; a.cnt->executed_positions = 0;
    a.cnt->kv_prefix_positions = 0; a.cnt->running_cands = 0; a.cnt->max_group = 0; a.cnt->pad_ = 0;
    a.dev_summary[0] = 0; a.dev_summary[1] = 0; a.dev_summary[2] = 0; a.dev_summary[3] = 0;
    a.host->steps_done = 0; a.host->n_live = 0; a.host->n_running = 0; a.host->error = 0;
    __threadfence_system();
  }
}

// One thread.  The R new sources (rows first_row .. first_row + R - 1 of the call) take the lowest free slots; a source that finds
// none (the host admits only what it knows to be free) gets slot -1, which k_sbsp_fill skips, and the pool reports an error.
__global__ void k_sbsp_admit(SbsPoolArgs a, int* new_slot, int R, int first_row) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int s = 0, got = 0;
  for (; got < R; ++got) {
    while (s < a.C && a.row_of[s] >= 0) ++s;
    if (s >= a.C) break;
    new_slot[got] = s;
    a.row_of[s] = first_row + got;
    ++s;
  }
  if (got != R) {
    for (int i = got; i < R; ++i) new_slot[i] = -1;
    a.dev_summary[2] = 1; a.host->error = 1; __threadfence_system();
  }
}

struct SbsPoolFillArgs {
  SbsPoolArgs a;
  const int* new_slot; int R, first_row, Ls_new;
  uint8_t* src_valid; const uint8_t* valid_new;                       // [C][Ls_cap] <- [R][Ls_new]
  float* memkv; const float* memkv_new; int kv_row;                   // floats per source position (Ld * 2 * d)
};

// grid (R, 1 + Ls_new): block (i, 0) writes the whole state of source i's slot (one <BOS> candidate with phi = G = 0 and length 1
// at k = 0, the other K - 1 absent), block (i, 1 + key) copies the cross K/V of one source position.
__global__ __launch_bounds__(256) void k_sbsp_fill(SbsPoolFillArgs f) {
  const SbsPoolArgs& a = f.a;
  const int i = blockIdx.x, t = threadIdx.x;
  const int s = f.new_slot[i];
  if (s < 0 || s >= a.C) return;
  if (blockIdx.y == 0) {
    const int row = f.first_row + i;
    for (int e = t; e < a.K * a.ld; e += blockDim.x) a.cand_next[(size_t)s * a.K * a.ld + e] = (e == 0) ? a.bos : a.pad;
    for (int k = t; k < a.K; k += blockDim.x) {
      const int c = s * a.K + k;
      a.len_next[c] = 1; a.fin_next[c] = (k == 0) ? 0 : 1; a.phi_next[c] = 0.f; a.g_in[c] = 0.f; a.parent[c] = -1; a.parent_draft[c] = 0;
      a.cand_src_len[c] = a.len_all[row];
    }
    if (t == 0) {
      a.level[s] = 1; a.nlive[s] = 1; a.nfin[s] = 0; a.run_acc[s] = 1;
      a.key[s] = a.row_keys ? a.row_keys[row] : (int64_t)row;
      a.pfx_len[s] = a.pfx_len_src ? a.pfx_len_src[row] : 0;
      a.pfx_src[s] = row;
    }
    for (int c = t; c < a.Ls_cap; c += blockDim.x)
      f.src_valid[(size_t)s * a.Ls_cap + c] = (c < f.Ls_new) ? f.valid_new[(size_t)i * f.Ls_new + c] : (uint8_t)0;
  } else {
    const int key = blockIdx.y - 1;
    const float4* src = reinterpret_cast<const float4*>(f.memkv_new + ((size_t)i * f.Ls_new + key) * f.kv_row);
    float4* dst = reinterpret_cast<float4*>(f.memkv + ((size_t)s * a.Ls_cap + key) * f.kv_row);
    for (int c = t; c < f.kv_row / 4; c += blockDim.x) dst[c] = src[c];
  }
}

// One workgroup per slot, after the step: a slot all of whose K new candidates are finished, or whose level has reached
// max_len - 1, hands its rows (all max_len columns: PAD beyond the row), logp and gumbel to its source's row of the outputs and is
// free from this iteration on; any other live slot moves to its next level with K parents.
__global__ __launch_bounds__(256) void k_sbsp_retire(SbsPoolArgs a) {
  const int s = blockIdx.x, t = threadIdx.x;
  const int row = a.row_of[s];
  if (row < 0) return;
  const int lvl = a.level[s];
  const int nf = a.nfin[s];
  const bool goes_on = nf != a.K && lvl < a.max_len - 1;
  __syncthreads();                              // every thread has read level before thread 0 moves it
  if (goes_on) {
    if (t == 0) { a.level[s] = lvl + 1; a.nlive[s] = a.K; a.run_acc[s] += a.K - nf; }      // the next level decodes the unfinished ones
    return;
  }
  const SbsPoolIo io = *a.io;
  for (int e = t; e < a.K * a.max_len; e += blockDim.x) {
    const int k = e / a.max_len, col = e - k * a.max_len;
    io.out[((size_t)row * a.K + k) * a.max_len + col] = a.cand_next[((size_t)s * a.K + k) * a.ld + col];
  }
  for (int k = t; k < a.K; k += blockDim.x) {
    const int c = s * a.K + k;
    io.out_logp[(size_t)row * a.K + k] = a.phi_next[c];
    io.out_gumbel[(size_t)row * a.K + k] = a.g_out[c];
    a.fin_next[c] = 1; a.parent[c] = -1;
  }
  __syncthreads();                              // every thread has read row_of
  if (t == 0) {
    if (io.src_running) io.src_running[row] = a.run_acc[s];
    a.row_of[s] = -1; a.nlive[s] = 0;
  }
}

// Last kernel of an iteration (one workgroup): live slots, running candidates and the iteration count to the pinned block.
__global__ __launch_bounds__(256) void k_sbsp_publish(SbsPoolArgs a) {
  __shared__ int s_live, s_run;
  if (threadIdx.x == 0) { s_live = 0; s_run = 0; }
  __syncthreads();
  int live = 0, run = 0;
  for (int s = threadIdx.x; s < a.C; s += blockDim.x)
    if (a.row_of[s] >= 0) { live += 1; run += a.K - a.nfin[s]; }
  atomicAdd(&s_live, live); atomicAdd(&s_run, run);
  __syncthreads();
  if (threadIdx.x == 0) {
    a.dev_summary[0] = s_live; a.dev_summary[1] = s_run;
    a.host->n_live = s_live; a.host->n_running = s_run;
    __threadfence_system();
    a.host->steps_done = (int)a.cnt->model_calls;
    __threadfence_system();
  }
}

}  // namespace ttx
