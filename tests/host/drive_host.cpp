// Host build of csrc/ttx_drive.h for tests/test_drive_host.py (g++, no GPU): drive_jobs over scripted jobs.
// Job i answers its turns from script[i * ld .. + len[i]), one entry per turn, the last one for ever after.  An entry is a Turn
// (0 idle, 1 waiting, 2 progressed, 3 finished), a negative error code, or 1000 + ms: waiting for ms milliseconds from the first
// turn that met the entry, then the next entry.
#include "ttx_drive.h"

extern "C" int ttx_host_drive(int n, int serial, int watchdog_s, const int* script, const int* len, int ld, int* visits, int visits_cap,
                              long long* n_visits, int* hung, int* stalled_job, double* seconds) {
  using clock = std::chrono::steady_clock;
  std::vector<int> pos(n, 0);
  std::vector<clock::time_point> since(n);
  std::vector<char> timing(n, 0);
  long long turns = 0;
  const auto t0 = clock::now();
  const ttx::DriveResult r = ttx::drive_jobs(n, serial != 0, watchdog_s, [&](int i) -> int {
    if (turns < visits_cap) visits[turns] = i;
    ++turns;
    for (;;) {
      const int e = script[i * ld + pos[i]];
      if (e < 1000) {
        if (pos[i] + 1 < len[i]) ++pos[i];
        return e;
      }
      if (!timing[i]) { timing[i] = 1; since[i] = clock::now(); }
      if (clock::now() - since[i] < std::chrono::milliseconds(e - 1000)) return ttx::TURN_WAITING;
      timing[i] = 0;
      ++pos[i];                        // a timed wait is never the last entry
    }
  });
  *seconds = std::chrono::duration<double>(clock::now() - t0).count();
  *n_visits = turns;
  *hung = r.hung ? 1 : 0;
  *stalled_job = r.stalled_job;
  return r.rc;
}
