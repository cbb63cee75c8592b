// Host-only core of the polling loop every decoding entry point runs under (no HIP in here: tests/host/drive_host.cpp compiles it
// with g++ and drives it with fake jobs).  A call decodes on n jobs (sessions, each on its own stream; the single-session calls
// have n = 1) from one host thread: drive_jobs() visits them round-robin
// and gives each a turn; what a turn does (start a batch, enqueue the next step once the last one has published, admit rows,
// collect the result) is the caller's.  The core owns the order of the visits, the serial mode, the pause, the watchdog and the
// rule that the first error ends the call.
#pragma once
#include <chrono>
#include <cstdlib>
#include <vector>

namespace ttx {

// The polling loops give up after this long without a published step (a failed kernel never publishes): TTX_WATCHDOG_SECONDS.
inline int watchdog_seconds() {
  static const int limit_s = [] { const char* e = getenv("TTX_WATCHDOG_SECONDS"); return e && atoi(e) > 0 ? atoi(e) : 120; }();
  return limit_s;
}

inline bool watchdog_expired(std::chrono::steady_clock::time_point since, int limit_s) {
  return std::chrono::steady_clock::now() - since > std::chrono::seconds(limit_s);
}

// A polling loop's wait for the step in flight: stalled() counts one fruitless look and asks the watchdog on every 65 536th,
// advanced() restarts both when the step has published.  No HIP call while polling: only the clock.
struct Progress {
  unsigned idle_spins = 0;
  std::chrono::steady_clock::time_point last_progress = std::chrono::steady_clock::now();
  bool stalled(int limit_s) { return (++idle_spins & 0xffff) == 0 && watchdog_expired(last_progress, limit_s); }
  void advanced() { idle_spins = 0; last_progress = std::chrono::steady_clock::now(); }
};

// What turn(i) reports; a negative value is an error code (TTX_ERR_*) and ends the call.
enum Turn {
  TURN_IDLE = 0,      // nothing to do for this job right now, and nothing of it is awaited from the device's step
  TURN_WAITING = 1,   // the step in flight has not published yet: counted against the watchdog
  TURN_PROGRESSED = 2,
  TURN_FINISHED = 3,  // this job is finished for good: it gets no further turn
};

struct DriveResult {
  int rc;             // 0, or the first error a turn returned
  bool hung;          // a job waited for longer than the watchdog time: nothing of the call may be synchronised
  int stalled_job;    // that job, else -1
};

// Turns for jobs 0 .. n-1 in index order, round after round, until every job has finished; a round in which nobody progressed
// ends with a pause.  serial: only the lowest unfinished job gets turns (profiling: one pool after another).
template <class TurnFn>
inline DriveResult drive_jobs(int n, bool serial, int watchdog_s, TurnFn&& turn) {
  std::vector<Progress> progress(n);
  std::vector<char> finished(n, 0);
  int left = n;
  while (left > 0) {
    bool progressed = false;
    for (int i = 0; i < n; ++i) {
      if (finished[i]) continue;
      const int t = turn(i);
      if (t < 0) return {t, false, -1};
      if (t == TURN_WAITING) {
        if (progress[i].stalled(watchdog_s)) return {0, true, i};
      } else if (t != TURN_IDLE) {
        progress[i].advanced();
        progressed = true;
        if (t == TURN_FINISHED) { finished[i] = 1; --left; }
      }
      if (serial) break;
    }
    if (!progressed) __builtin_ia32_pause();
  }
  return {0, false, -1};
}

}  // namespace ttx
