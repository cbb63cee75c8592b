// Host build of csrc/ttx_admit.h for tests/test_admit_host.py (g++, no GPU): the same source libttx_hip.so compiles.
#include "ttx_admit.h"

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
