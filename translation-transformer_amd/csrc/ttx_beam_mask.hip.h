// Constrained beam search (included by ttx_api.hip only): k_beam_step_masked stands where the standard beam loop launches k_beam_step
// when the call carries a logit bias, a syntax constraint or forced prefixes.  Hand-written HIP for gfx950, wave64: one workgroup of
// four waves per source, one wave per parent row at a time, the beam * V totals in an LDS image (dynamic, at most 150 KB), then K
// selection rounds, as k_beam_step.  The rule (include/ttx.h states it as the contract under ttx_beam_generate_constrained;
// tests/util_beam_mask_checks.py restates it), for parent k of source b with `width` tokens in its row:
//   live, free      total[k][v] = score[k] + logf(expf(x_v - m) / z), m = max x, z = sum expf(x_v - m): k_beam_step's expressions in
//                   k_beam_step's order (lane l owns ids l, l + 64, ..; the 64 lane values through the xor butterfly), so rows of finite
//                   logits give k_beam_step's bits.  A -inf logit (a biased or masked token) adds expf(-inf) = 0 to z and gives a -inf
//                   child: the totals are log-probabilities under the constrained, renormalised distribution.  A row with no finite
//                   logit (m == -inf) gives -inf for every child; x - m is never formed there.
//   finished        one child, PAD, with the total k_beam_step gives it (the reference's artificial row, 35 on PAD and 0 elsewhere:
//                   score + logf(expf(0) / z), the same expressions); the other V - 1 children, which that row puts 35 below, do
//                   not exist here (-inf): where a constraint leaves a source fewer than K hypotheses they would fill the free ranks
//                   with rows that go on after their EOS.  With score -inf (a dead parent) every child is -inf.
//   live, forced    (pfx.tok set and width <= pfx.len[b]: position `width` lies inside the source's prefix)  the prefix token (an id
//                   outside [0, V) as 0) has total = score[k] on the bits, every other child is -inf; the logits are not read.
//   selection       the K largest totals, largest first, equal values the lower flat index k * V + v first.  A round is k_beam_step's
//                   round, statement for statement (strictly greater within a thread's ascending walk, then the butterfly and the
//                   four waves with the index as the tie-break), which never picks a -inf child.  When it finds nothing, every
//                   finite child is taken, and the same round goes on to pick the lowest flat index whose child is -inf: -inf
//                   children come after every finite one, by ascending flat index.  A child already taken is NaN in the image and
//                   matches neither search, so none is taken twice; the image holds no other NaN (a total that is not a number,
//                   outside the contract, is stored as -inf).  K <= beam * V (checked by every caller on the host), so one of
//                   the two searches always finds a child.  Rounds with a finite child cost what k_beam_step's cost.
//   dead row        a selected -inf child: the parent's tokens followed by PAD (the token is not written), new_score = -inf,
//                   new_finished = 1 and one more in summary[0], so the loop's stop rule counts it as finished and no decoder row is
//                   spent on it; parent is the real parent (k_tree_cache indexes with it).
// No atomics but the summary add, vector stores only, nothing crosses a workgroup.
#pragma once
#include "ttx_sample.hip.h"

namespace ttx {

constexpr int BEAM_NONE = 0x7fffffff;        // "no child found" of a selection search; never used as an index

__global__ __launch_bounds__(256) void k_beam_step_masked(BeamStepArgs a, PrefixTab pfx) {
  extern __shared__ float tot[];                // [beam * V]
  __shared__ float s_best[4];
  __shared__ int s_bi[4];
  __shared__ int s_sel;
  const int b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float taken = __int_as_float(0x7fc00000);
  const bool forced = pfx.tok && a.width <= pfx.len[b];                        // workgroup-uniform
  const int ftok = forced ? prefix_token(pfx, b, a.width, a.V) : -1;
  for (int k = wave; k < a.beam; k += 4) {
    const int c = b * a.beam + k;
    const bool fin = a.finished[c] != 0;
    const float sc = a.score[c];
    float* im = tot + (size_t)k * a.V;
    if (!fin && forced) {
      const float own = sc == sc ? sc : -INFINITY;
      for (int v = lane; v < a.V; v += 64) im[v] = (v == ftok) ? own : -INFINITY;
      continue;
    }
    const float* row = fin ? nullptr : a.logits + (size_t)a.slot_of[c] * a.V;
    float m = -INFINITY;
    for (int v = lane; v < a.V; v += 64) m = fmaxf(m, fin ? (v == a.pad ? 35.0f : 0.0f) : row[v]);
    m = wave_max(m);
    if (m == -INFINITY) {                       // wave-uniform: no finite logit, so no child exists
      for (int v = lane; v < a.V; v += 64) im[v] = -INFINITY;
      continue;
    }
    float z = 0.f;
    for (int v = lane; v < a.V; v += 64) z += expf((fin ? (v == a.pad ? 35.0f : 0.0f) : row[v]) - m);
    z = wave_sum(z);
    for (int v = lane; v < a.V; v += 64) {
      const float x = fin ? (v == a.pad ? 35.0f : 0.0f) : row[v];
      const float t = sc + logf(expf(x - m) / z);
      im[v] = (t == t && !(fin && v != a.pad)) ? t : -INFINITY;
    }
  }
  __syncthreads();
  const int n = a.beam * a.V;
  for (int r = 0; r < a.K; ++r) {
    float best = -INFINITY;
    int bi = BEAM_NONE;
    for (int i = threadIdx.x; i < n; i += 256) {
      const float v = tot[i];
      if (v > best) { best = v; bi = i; }       // ascending i per thread: the first of equal values stays
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
      s_sel = sel;
    }
    __syncthreads();
    const bool dead = s_sel == BEAM_NONE;       // workgroup-uniform: no finite child is left
    if (dead) {                                 // the lowest flat index that holds -inf (r < K <= beam * V children, r of them taken)
      int lo = BEAM_NONE;
      for (int i = threadIdx.x; i < n; i += 256)
        if (tot[i] == -INFINITY) { lo = i; break; }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o, 64));
      if (lane == 0) s_bi[wave] = lo;
      __syncthreads();
      if (threadIdx.x == 0) s_sel = min(min(s_bi[0], s_bi[1]), min(s_bi[2], s_bi[3]));
      __syncthreads();
    }
    const int sel = s_sel;
    const int k = sel / a.V, tok = sel % a.V;
    const int c = b * a.beam + k, out = b * a.K + r;
    const int* root = a.gen + (size_t)c * a.ld;
    int64_t* dst = a.new_cand + (size_t)out * a.ld;
    for (int col = threadIdx.x; col < a.ld; col += 256)
      dst[col] = col < a.width ? (int64_t)root[col] : ((col == a.width && !dead) ? (int64_t)tok : (int64_t)a.pad);
    if (threadIdx.x == 0) {
      a.new_score[out] = tot[sel];
      a.parent[out] = c;
      a.parent_draft[out] = 0;
      a.new_len[out] = a.width + 1;
      const bool has_eos = dead || a.finished[c] || tok == a.eos;
      a.new_finished[out] = has_eos ? 1 : 0;
      if (has_eos) atomicAdd(&a.summary[0], 1);
      tot[sel] = taken;
    }
    __syncthreads();
  }
}

}  // namespace ttx
