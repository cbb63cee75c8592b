// Host-only admission policy of the slot pools (the greedy / sampling slot pool, the beam-speculative batch pool and the
// stochastic-beam source pool): how many pools a call runs and how wide and deep they are, which batches of the work list a pool
// takes when it has free slots, the length buckets an admission is encoded in, and pool_step, the one rule every pool's turn goes
// by between two iterations.  No HIP in here: tests/host/admit_host.cpp compiles it with g++.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace ttx {

// Slot width of a pool: 192 positions, beyond that in steps of 64, clamped to the positional table — calls whose longest sources
// differ share workspaces and the captured step graph (a slot's keys are bounded by its own source length, so the padding
// costs memory only: 0.8 GB of cross K/V per 512-slot pool at 192).
inline int pool_slot_width(int len_max, int max_positions) {
  const int w = std::min(std::max(192, ((len_max + 63) / 64) * 64), max_positions);
  return std::max(w, std::max(2, len_max));
}

// Pools of a call and the slots of each: short lists run as several small pools (of at least min(capacity / 2, small_pool)
// rows each: 32 for the greedy pool, 8 for the beam pool), never more pools than batches, and no pool gets more slots than a
// fair share of the rows, or fewer than the largest batch (the greedy pool's batches are single rows: max_batch 1).
struct PoolShape { int n_jobs, C; };
inline PoolShape pool_shape(int n_sessions, int n_batches, int R_total, int capacity, int small_pool, int max_batch) {
  const int per_pool = std::max(1, std::min(capacity / 2, small_pool));
  const int n_jobs = std::max(1, std::min({n_sessions, n_batches, (R_total + per_pool - 1) / per_pool}));
  return {n_jobs, std::min(capacity, std::max(max_batch, (R_total + n_jobs - 1) / n_jobs))};
}

// The work list of a pool call is whole batches in order: batch b owns the rows [first[b], first[b + 1]), first has n_batches + 1
// entries (the greedy pool admits rows: unit batches, first[b] = b).
//
// Serial (profiling) pass, asked when pool `job` of n_jobs takes its first turn with the list at batch `cursor`: the pool decodes
// an equal contiguous share of the rest of the list, rounded up to whole batches.  Returns the batch its share ends at.
inline int serial_quota(const int* first, int n_batches, int cursor, int job, int n_jobs) {
  const int rest = first[n_batches] - first[cursor];
  const int target = first[cursor] + (rest + (n_jobs - job) - 1) / (n_jobs - job);
  int end = cursor;
  while (end < n_batches && first[end] < target) ++end;
  return end;
}

struct AdmitState {
  int cursor;        // next batch of the work list
  int free_slots;    // of this pool
  int n_live;        // rows decoding in this pool
  bool first_fill;   // this pool has not launched a step yet
  int job, n_jobs;   // this pool, the pools of the call
  int n_running;     // pools of the call that are still decoding (this one included)
  bool serial;       // profiling: one pool after another ...
  int quota_end;     // ... each over its serial_quota
};

// The batches pool `job` admits now (possibly none), C slots per pool:
//  - an admission goes into an empty pool, or takes at least a quarter pool and at least the next batch;
//  - whole batches, as many as fit the free slots;
//  - the last rows of the list are shared out over the pools still running, so that they drain together instead of one pool
//    swallowing the rest and finishing alone (a first batch is taken whatever the share says);
//  - the first fill of a list that fits the pools at once is an equal share for every pool not yet started (the pools before
//    this one have taken theirs), so that nothing is left waiting for a later admission.
// With unit batches this is the greedy pool's rule: the condition reduces to n_live == 0 || free_slots >= max(1, C / 4), and the
// loop stops at min(free_slots, remaining, share) rows (share >= 1, and free_slots >= 1 whenever the condition holds).
inline int plan_admission(const int* first, int n_batches, int C, const AdmitState& a) {
  const int list_end = a.serial ? a.quota_end : n_batches;
  const int min_admit = std::max(1, C / 4);
  if (a.cursor >= list_end) return 0;
  if (a.n_live != 0 && a.free_slots < std::max(min_admit, first[a.cursor + 1] - first[a.cursor])) return 0;
  const int remaining = first[list_end] - first[a.cursor];
  const auto cdiv = [](int x, int y) { return (x + y - 1) / y; };
  int share = std::max(1, cdiv(remaining, std::max(1, a.serial ? 1 : a.n_running)));
  if (!a.serial && a.first_fill && (long long)a.n_jobs * C >= first[n_batches]) share = std::max(1, cdiv(remaining, a.n_jobs - a.job));
  int take = 0, end = a.cursor;
  while (end < list_end) {
    const int sz = first[end + 1] - first[end];
    if (take + sz > a.free_slots || (take > 0 && take + sz > share)) break;
    take += sz;
    ++end;
  }
  return end - a.cursor;
}

// One turn of a running pool, decided in one place.  The pool's turn (the lambda drive_jobs calls) reads its pinned words into a
// PoolLook, asks pool_step, and acts on the answer with its own admit, launch and read-back calls: decide here, act at the call site.
//   WAIT    the iteration in flight has not published: nothing was touched and nothing but `published` was read (the spin path: the
//           caller's volatile read and one compare; of the answer only act and first_batch are set)
//   FAILED  the device set its error word: nothing was admitted
//   DRAIN   nothing is live and nothing was admitted: enqueue the read-back and go to the finishing phase
//   LAUNCH  admit batches [first_batch, first_batch + n_take) = rows [first_row, first_row + rows) if n_take > 0, then launch the
//           next iteration over n_live slots (n_running: the device's running count plus the admitted rows)
//   STUCK   as LAUNCH, but the pool has launched more than max_launches iterations: fail ("failed to terminate"), admit nothing
// pool_step settles the serial quota on the pool's first published turn, advances the list's cursor and counts the pool out of
// list.n_running when it drains.  `launched` and `phase` are the caller's to advance, after it has acted: launched when an iteration
// is enqueued, phase (1 running) when the read-back is.
struct PoolList {      // one per call, shared by its pools
  const int* first;
  int n_batches;
  int cursor;          // next batch of the work list
  int n_jobs;          // pools of the call, all started before the first turn ...
  int n_running;       // ... and those that have not drained yet (n_jobs at first)
};
inline PoolList pool_list(const int* first, int n_batches, int n_jobs) { return {first, n_batches, 0, n_jobs, n_jobs}; }
struct PoolState { int launched = 0, phase = 0, quota_end = -1; };      // one per pool; phase: 0 not started, 1 running, 2 finishing, 3 done
struct PoolLook {      // what the host just read from the pool's pinned words
  bool published;      // steps_done has reached `launched`
  bool error;          // looked at on every published turn, the first one included (the words are zeroed at the pool's start)
  int n_live, n_running;      // read only when published; before the first launch `published` and both counts are ignored (nothing
                              // in flight, counts 0)
};
struct PoolPlan {
  enum Act { WAIT, FAILED, STUCK, DRAIN, LAUNCH } act;
  int first_batch, n_take, first_row, rows, n_live, n_running;
};
// Inlined into every turn on purpose: out of line, each fruitless look of the spin loop paid for the call and for the PoolLook and
// PoolPlan going through memory.
__attribute__((always_inline)) inline PoolPlan pool_step(PoolState& p, PoolList& l, const PoolLook& look, int job, int C, bool serial, long long max_launches) {
  const bool fresh = p.launched == 0;
  PoolPlan plan{PoolPlan::WAIT, l.cursor, 0, 0, 0, 0, 0};
  if (!fresh && !look.published) return plan;
  plan.first_row = l.first[l.cursor];
  if (look.error) { plan.act = PoolPlan::FAILED; return plan; }
  const int n_live = fresh ? 0 : look.n_live;
  if (serial && p.quota_end < 0) p.quota_end = serial_quota(l.first, l.n_batches, l.cursor, job, l.n_jobs);
  plan.n_take = plan_admission(l.first, l.n_batches, C, {l.cursor, C - n_live, n_live, fresh, job, l.n_jobs, l.n_running, serial, p.quota_end});
  l.cursor += plan.n_take;
  plan.rows = l.first[l.cursor] - plan.first_row;
  plan.n_live = n_live + plan.rows;
  plan.n_running = (fresh ? 0 : look.n_running) + plan.rows;
  if (plan.n_live == 0) { plan.act = PoolPlan::DRAIN; --l.n_running; }
  else plan.act = p.launched > max_launches ? PoolPlan::STUCK : PoolPlan::LAUNCH;
  return plan;
}

// Length buckets inside an admission.  An admission is encoded at the width of its longest row, so a chunk of 1 024 length-sorted
// rows pads its short rows to the longest one: in the encoder, in the cross K/V, and, through src_len, in every cross-attention
// launch of the rows' slots.  Its rows are therefore admitted in consecutive sub-chunks, each at its own width (its longest row,
// at least 2).  A sub-chunk closes once rows x width reaches `budget` padded rows: the GEMM tiles run at their large-launch rates
// from about 16 000 rows, so a shorter launch would give back what the padding saves.  A last sub-chunk of fewer
// than budget / 2 padded rows joins the one before it; an admission below the budget stays one chunk.  budget 0: one chunk.
// `ends` receives the end (exclusive, relative to `len`) of every sub-chunk.
constexpr long long ADMIT_ROWS = 16384;
inline int chunk_width(const int32_t* len, int first, int end) {
  int w = 2;
  for (int r = first; r < end; ++r) w = std::max(w, (int)len[r]);
  return w;
}
inline void admit_chunks(const int32_t* len, int n, long long budget, std::vector<int>& ends) {
  ends.clear();
  if (budget > 0 && (long long)n * chunk_width(len, 0, n) >= budget) {
    int first = 0, w = 2;
    for (int r = 0; r < n; ++r) {
      w = std::max(w, (int)len[r]);
      if ((long long)(r + 1 - first) * w >= budget) { ends.push_back(r + 1); first = r + 1; w = 2; }
    }
    if (first < n) {
      const bool merge = !ends.empty() && (long long)(n - first) * chunk_width(len, first, n) * 2 < budget;
      if (merge) ends.back() = n; else ends.push_back(n);
    }
  } else {
    ends.push_back(n);
  }
}

}  // namespace ttx
