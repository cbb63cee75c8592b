"""csrc/ttx_drive.h (the host core of the polling loops) compiled for the host and driven with scripted jobs: the order of the
visits, the serial mode, the first error, the watchdog and its reset.  This is the only place where the hang path runs: nothing on
the GPU is made to hang."""
import ctypes
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "translation-transformer_amd" / "csrc"
IDLE, WAITING, PROGRESSED, FINISHED = 0, 1, 2, 3
WATCHDOG_S = 1


def wait_ms(ms):
    return 1000 + ms


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    out = tmp_path_factory.mktemp("drive") / "libdrive.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{CSRC}", "-o", str(out), str(ROOT / "tests" / "host" / "drive_host.cpp")],
                   check=True)
    return ctypes.CDLL(str(out))


def drive(drv, scripts, serial=False, watchdog_s=WATCHDOG_S, cap=4096):
    n, ld = len(scripts), max(len(s) for s in scripts)
    flat = (ctypes.c_int * (n * ld))(*[v for s in scripts for v in list(s) + [0] * (ld - len(s))])
    lens = (ctypes.c_int * n)(*[len(s) for s in scripts])
    visits = (ctypes.c_int * cap)()
    n_visits, hung, stalled, seconds = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    rc = drv.ttx_host_drive(n, int(serial), watchdog_s, flat, lens, ld, visits, cap, ctypes.byref(n_visits), ctypes.byref(hung),
                            ctypes.byref(stalled), ctypes.byref(seconds))
    return {"rc": rc, "hung": bool(hung.value), "stalled_job": stalled.value, "seconds": seconds.value, "n_visits": n_visits.value,
            "visits": list(visits[:min(cap, n_visits.value)])}


def test_round_robin_in_index_order_and_finished_jobs_get_no_turn(drv):
    r = drive(drv, [[PROGRESSED, PROGRESSED, FINISHED], [FINISHED], [IDLE, WAITING, PROGRESSED, FINISHED]])
    assert (r["rc"], r["hung"], r["stalled_job"]) == (0, False, -1)
    assert r["visits"] == [0, 1, 2, 0, 2, 0, 2, 2]
    assert drive(drv, [[FINISHED]] * 5)["visits"] == [0, 1, 2, 3, 4]


def test_serial_mode_gives_turns_to_the_lowest_unfinished_job_only(drv):
    r = drive(drv, [[PROGRESSED, WAITING, IDLE, FINISHED], [PROGRESSED, FINISHED], [FINISHED]], serial=True)
    assert (r["rc"], r["hung"]) == (0, False)
    assert r["visits"] == [0, 0, 0, 0, 1, 1, 2]


def test_first_error_ends_the_loop_and_is_returned(drv):
    r = drive(drv, [[PROGRESSED, PROGRESSED, -7], [PROGRESSED, -2], [PROGRESSED] * 9 + [FINISHED]])
    assert (r["rc"], r["hung"], r["stalled_job"]) == (-2, False, -1)
    assert r["visits"] == [0, 1, 2, 0, 1]                     # job 1 fails in the second round: nobody gets a turn after that
    r = drive(drv, [[-4], [FINISHED]])
    assert (r["rc"], r["visits"]) == (-4, [0])


def test_a_job_that_only_waits_is_reported_hung_after_the_watchdog_time_and_not_before(drv):
    r = drive(drv, [[PROGRESSED, FINISHED], [PROGRESSED, WAITING], [IDLE]])
    assert (r["rc"], r["hung"], r["stalled_job"]) == (0, True, 1)
    assert WATCHDOG_S <= r["seconds"] < WATCHDOG_S + 1.0
    assert r["n_visits"] > 65536                              # the clock is asked on every 65 536th fruitless look only


def test_progress_resets_the_wait(drv):
    # 2 x 0.6 s of waiting around a published step is longer than the watchdog time in all, and no hang
    r = drive(drv, [[wait_ms(600), PROGRESSED, wait_ms(600), FINISHED], [FINISHED]])
    assert (r["rc"], r["hung"], r["stalled_job"]) == (0, False, -1)
    assert r["seconds"] >= 1.2
    # the same job beside one that waits 1.3 s in one piece: that one is hung, whatever the other does meanwhile
    r = drive(drv, [[wait_ms(600), PROGRESSED, wait_ms(600), FINISHED], [wait_ms(1300), FINISHED]])
    assert (r["rc"], r["hung"], r["stalled_job"]) == (0, True, 1)
