// Caller-supplied proposal drafts of the speculative sampling loops (include/ttx.h "Proposal drafts"; included by ttx_api.hip only).
// A proposal is offered, never forced: k_sample_step and k_sample_accept are the unproposed call's, so whatever this kernel writes
// into draft 0 changes step counts and never a token.  Before every verify step k_proposal_drafts aligns the proposal q of every
// active row with the row's tokens g[0 .. f] and rewrites draft 0 from the aligned place:
//   shift d = lane - 32, one lane of the slot's wave per shift;
//   c(d) = #{ a in [0, ctx) : f - a >= 0, -1 <= f-1-a+d < len, q[f-1-a+d] == g[f-a] }, with q[-1] = BOS;
//   d is eligible iff c(d) >= 1 and 0 <= f + d < len; the eligible d with the largest c wins, ties to the smaller |d|, then to d >= 0;
//   draft 0 token j = q[f + d + j] while that index is < len (EOS and PAD as `repl`), else token j of the row's source draft 0;
//   no eligible d (or len == 0): draft 0 is the source draft 0.
// Stateless and idempotent: the D ints of every active row are rewritten from `draft0` and the table, which nothing writes after the
// row was set up.  Drafts 1 .. N-1 are not touched.  One wave per slot, grid for the capacity: one round of independent loads (front,
// len, src), 2 * ctx independent loads per lane, a 6-stage butterfly, then D independent loads and stores.
#pragma once
#include "ttx_sample.hip.h"

namespace ttx {

// Tokens of context compared per shift (2, 4 or 8: step counts only).  2 took the fewest steps on edited proposals: after an
// insertion or a deletion the new shift outvotes the old one once ctx / 2 tokens lie behind the edit.
constexpr int PROPOSAL_CTX = 2;

struct ProposalDraftsArgs {
  const DecState* st;              // n_active live slots
  const int* act_idx;              // [n_active]
  const int* front;                // [B]
  const int* gen; int gen_ld;      // [B, gen_ld], columns 0 .. front valid, column 0 = BOS
  int* drafts; int N, D;           // [B, N, D], draft 0 of the active rows rewritten
  const int* draft0;               // [B, D] the rows' source draft 0
  PrefixTab tab;                   // the proposals: tok [sources][ld], len and src by decoder row
  int bos, eos, pad, repl;
  int ctx;
};

__global__ __launch_bounds__(256) void k_proposal_drafts(const ProposalDraftsArgs a) {
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= a.st->n_active) return;       // wave-uniform
  const int lane = threadIdx.x & 63;
  const int b = a.act_idx[slot];
  const int f = a.front[b], len = a.tab.len[b], src = a.tab.src[b];
  const int* q = a.tab.tok + (size_t)src * a.tab.ld;
  const int* g = a.gen + (size_t)b * a.gen_ld;
  const int* own = a.draft0 + (size_t)b * a.D;
  int* out = a.drafts + (size_t)b * a.N * a.D;
  const int d = lane - 32;
  int c = 0;
  for (int x = 0; x < a.ctx; ++x) {
    const int gi = f - x, qi = f - 1 - x + d;
    if (gi >= 0 && qi >= -1 && qi < len) c += ((qi < 0 ? a.bos : q[qi]) == g[gi]) ? 1 : 0;
  }
  const bool ok = c >= 1 && f + d >= 0 && f + d < len;
  // one int orders the shifts: the count, then the tie order (0, +1, -1, +2, -2, ..), then the lane itself to recover the winner
  const int rank = 2 * (d < 0 ? -d : d) + (d < 0 ? 1 : 0);       // 0 .. 65
  int key = ok ? ((c << 16) | ((127 - rank) << 8) | lane) : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  const int base = key ? f + (key & 0xff) - 32 : len;             // wave-uniform; no eligible shift: every index is past the end
  for (int j = lane; j < a.D; j += 64) {
    const int i = base + j;
    int t;
    if (i < len) {
      t = q[i];
      if (t == a.eos || t == a.pad) t = a.repl;
    } else {
      t = own[j];
    }
    out[j] = t;
  }
}

}  // namespace ttx
