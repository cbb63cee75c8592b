// Host build of csrc/ttx_admit.h for tests/test_admit_host.py (g++, no GPU): the same source libttx_hip.so compiles.
#include "ttx_admit.h"
#include "ttx_drive.h"

extern "C" int ttx_host_admit_chunks(const int32_t* len, int n, long long budget, int* ends, int cap) {
  std::vector<int> v;
  ttx::admit_chunks(len, n, budget, v);
  for (int i = 0; i < (int)v.size() && i < cap; ++i) ends[i] = v[i];
  return (int)v.size();
}

extern "C" int ttx_host_chunk_width(const int32_t* len, int first, int end) { return ttx::chunk_width(len, first, end); }

extern "C" int ttx_host_pool_slot_width(int len_max, int max_positions) { return ttx::pool_slot_width(len_max, max_positions); }

extern "C" void ttx_host_pool_shape(int n_sessions, int n_batches, int R_total, int capacity, int small_pool, int max_batch, int* out2) {
  const ttx::PoolShape s = ttx::pool_shape(n_sessions, n_batches, R_total, capacity, small_pool, max_batch);
  out2[0] = s.n_jobs;
  out2[1] = s.C;
}

extern "C" int ttx_host_serial_quota(const int* first, int n_batches, int cursor, int job, int n_jobs) {
  return ttx::serial_quota(first, n_batches, cursor, job, n_jobs);
}

extern "C" int ttx_host_plan_admission(const int* first, int n_batches, int C, int cursor, int free_slots, int n_live, int first_fill,
                                       int job, int n_jobs, int n_running, int serial, int quota_end) {
  return ttx::plan_admission(first, n_batches, C, {cursor, free_slots, n_live, first_fill != 0, job, n_jobs, n_running, serial != 0, quota_end});
}

// A whole pool call on a fake device, through pool_step and under drive_jobs, with the turn the three pools have: look, decide,
// act.  The device publishes an iteration after `looks[k]` fruitless looks and retires `retire[k]` rows in it (k: the call's
// iterations in launch order; past the end of a script the value is 0, and no more rows retire than are live); the iteration
// numbered `error_at` (1-based, 0: none) publishes with the error word set.  Every pool_step answer goes to `log`, POOL_LOG_WORDS
// ints each: job, act, first_batch, n_take, first_row, rows, n_live, n_running, the list's cursor and running pools after the
// answer, the pool's quota_end and launched.  Returns the number of answers (the first `cap` are kept); *rc: 0, or -1 after
// FAILED, -2 after STUCK, -3 when drive_jobs gave up.
constexpr int POOL_LOG_WORDS = 12;
extern "C" int ttx_host_pool_call(const int* first, int n_batches, int n_jobs, int C, int serial, long long max_launches, const int* looks,
                                  int n_looks, const int* retire, int n_retire, int error_at, int* log, int cap, int* rc) {
  struct FakePool {
    ttx::PoolState pool;
    int steps_done = 0, error = 0, n_live = 0;       // the pinned words
    int wait = 0, next_live = 0, next_error = 0;     // the iteration in flight
  };
  std::vector<FakePool> jobs(n_jobs);
  for (FakePool& j : jobs) j.pool.phase = 1;
  ttx::PoolList list = ttx::pool_list(first, n_batches, n_jobs);
  int n_log = 0, n_iter = 0;
  const auto turn = [&](int i) -> int {
    FakePool& j = jobs[i];
    if (j.pool.phase != 1) { j.pool.phase = 3; return ttx::TURN_FINISHED; }
    if (j.steps_done < j.pool.launched) {            // the device: one look nearer to publishing
      if (j.wait > 0) --j.wait;
      else { j.steps_done = j.pool.launched; j.n_live = j.next_live; j.error = j.next_error; }
    }
    ttx::PoolLook look{j.steps_done >= j.pool.launched, false, -1000, -1000};      // unpublished counts must not be used
    if (look.published) look = {true, j.error != 0, j.n_live, j.n_live};
    const ttx::PoolPlan plan = ttx::pool_step(j.pool, list, look, i, C, serial != 0, max_launches);
    if (n_log < cap) {
      const int rec[POOL_LOG_WORDS] = {i, (int)plan.act, plan.first_batch, plan.n_take, plan.first_row, plan.rows, plan.n_live, plan.n_running,
                                       list.cursor, list.n_running, j.pool.quota_end, j.pool.launched};
      std::copy(rec, rec + POOL_LOG_WORDS, log + (size_t)n_log * POOL_LOG_WORDS);
    }
    ++n_log;
    switch (plan.act) {
      case ttx::PoolPlan::WAIT: return ttx::TURN_WAITING;
      case ttx::PoolPlan::FAILED: return -1;
      case ttx::PoolPlan::STUCK: return -2;
      case ttx::PoolPlan::DRAIN: j.pool.phase = 2; break;
      case ttx::PoolPlan::LAUNCH:
        j.wait = n_iter < n_looks ? looks[n_iter] : 0;
        j.next_live = plan.n_live - std::min(plan.n_live, n_iter < n_retire ? retire[n_iter] : 0);
        ++n_iter;
        j.next_error = n_iter == error_at;
        ++j.pool.launched;
        break;
    }
    return ttx::TURN_PROGRESSED;
  };
  const ttx::DriveResult r = ttx::drive_jobs(n_jobs, serial != 0, 5, turn);
  *rc = r.hung ? -3 : r.rc;
  return n_log;
}
