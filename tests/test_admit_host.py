"""csrc/ttx_admit.h (the admission policy of the pools) compiled for the host: admit_chunks against the rule of util_admit.py,
plan_admission inside a simulated pool loop against the properties the pools rely on and against both rules it replaced,
restated here from the two entry points it was factored out of, and pool_step, the rule of a pool's turn, over whole calls on a
fake device (tests/host/admit_host.cpp: ttx_host_pool_call) under the real polling core."""
import ctypes
import random
import subprocess
from pathlib import Path

import pytest

from util_admit import chunk_ends

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "translation-transformer_amd" / "csrc"
I32P = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def adm(tmp_path_factory):
    out = tmp_path_factory.mktemp("admit") / "libadmit.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{CSRC}", "-o", str(out), str(ROOT / "tests" / "host" / "admit_host.cpp")],
                   check=True)
    lib = ctypes.CDLL(str(out))
    lib.ttx_host_admit_chunks.argtypes = [I32P, ctypes.c_int, ctypes.c_longlong, I32P, ctypes.c_int]
    lib.ttx_host_chunk_width.argtypes = [I32P, ctypes.c_int, ctypes.c_int]
    lib.ttx_host_pool_shape.argtypes = [ctypes.c_int] * 6 + [I32P]
    lib.ttx_host_pool_shape.restype = None
    lib.ttx_host_serial_quota.argtypes = [I32P] + [ctypes.c_int] * 4
    lib.ttx_host_plan_admission.argtypes = [I32P] + [ctypes.c_int] * 11
    lib.ttx_host_pool_call.argtypes = [I32P] + [ctypes.c_int] * 4 + [ctypes.c_longlong, I32P, ctypes.c_int, I32P, ctypes.c_int, ctypes.c_int,
                                       I32P, ctypes.c_int, I32P]
    return lib


def i32(values):
    return (ctypes.c_int32 * len(values))(*values)


def cdiv(a, b):
    return -(-a // b)


def test_admit_chunks_follow_the_rule(adm):
    rng = random.Random(5)
    cases = [([28], 1), ([41] * 40, 400), ([127] * 4 + [91] * 6 + [28] * 4, 500), ([127] * 4 + [91] * 6 + [28] * 9, 500),
             ([76] * 3 + [2] * 12, 20), ([1, 1, 1], 3), ([5], 0)]
    for _ in range(3000):
        n = rng.randint(1, 80)
        lens = sorted((rng.randint(1, 130) for _ in range(n)), reverse=rng.random() < 0.8)
        cases.append((lens, rng.choice([0, 1, 2, 7, 50, 140, 400, 1000, 16384])))
    for lens, budget in cases:
        ends = (ctypes.c_int32 * len(lens))()
        k = adm.ttx_host_admit_chunks(i32(lens), len(lens), budget, ends, len(lens))
        assert list(ends[:k]) == chunk_ends(lens, budget), (lens, budget)
        assert adm.ttx_host_chunk_width(i32(lens), 0, len(lens)) == max(2, max(lens))


def test_slot_width_and_pool_shape_as_both_pools_had_them(adm):
    for len_max in list(range(0, 400, 7)) + [191, 192, 193, 256, 257, 1000]:
        for max_pos in (150, 192, 200, 256, 1024):
            want = max(min(max(192, cdiv(len_max, 64) * 64), max_pos), max(2, len_max))
            assert adm.ttx_host_pool_slot_width(len_max, max_pos) == want
    rng = random.Random(9)
    out = (ctypes.c_int32 * 2)()
    for _ in range(4000):
        n_sessions, R, capacity = rng.randint(1, 6), rng.randint(1, 3000), rng.randint(1, 1024)
        # the greedy pool: rows are unit batches
        adm.ttx_host_pool_shape(n_sessions, R, R, capacity, 32, 1, out)
        n_jobs = min(n_sessions, cdiv(R, max(1, min(capacity // 2, 32))))
        assert list(out) == [n_jobs, min(capacity, max(1, cdiv(R, n_jobs)))]
        # the beam pool
        n_batches = rng.randint(1, R)
        max_batch = rng.randint(cdiv(R, n_batches), max(cdiv(R, n_batches), min(capacity, R - n_batches + 1)))
        adm.ttx_host_pool_shape(n_sessions, n_batches, R, capacity, 8, max_batch, out)
        n_jobs = max(1, min(n_sessions, n_batches, cdiv(R, max(1, min(capacity // 2, 8)))))
        assert list(out) == [n_jobs, min(capacity, max(max_batch, cdiv(R, n_jobs)))]


# ---- the two rules plan_admission replaced, as the entry points had them inline -------------------------------------------------
def greedy_take(R_total, C, cursor, n_act, first_fill, i, n_jobs, n_running, serial, quota_end):
    min_admit = max(1, C // 4)
    free_slots = C - n_act
    list_end = quota_end if serial else R_total
    if not (cursor < list_end and (n_act == 0 or free_slots >= min_admit)):
        return 0
    remaining = list_end - cursor
    share = max(1, cdiv(remaining, max(1, 1 if serial else n_running)))
    if not serial and first_fill and n_jobs * C >= R_total:
        share = max(1, cdiv(remaining, n_jobs - i))
    return min(free_slots, remaining, share)


def beam_take(first, n_batches, C, cursor_b, n_live, first_fill, i, n_jobs, n_run_jobs, serial, quota_b):
    min_admit = max(1, C // 4)
    free_slots = C - n_live
    list_end_b = quota_b if serial else n_batches
    if not (cursor_b < list_end_b and (n_live == 0 or free_slots >= max(min_admit, first[cursor_b + 1] - first[cursor_b]))):
        return 0
    remaining = first[list_end_b] - first[cursor_b]
    share = max(1, cdiv(remaining, max(1, 1 if serial else n_run_jobs)))
    if not serial and first_fill and n_jobs * C >= first[n_batches]:
        share = max(1, cdiv(remaining, n_jobs - i))
    take, b_end = 0, cursor_b
    while b_end < list_end_b:
        sz = first[b_end + 1] - first[b_end]
        if take + sz > free_slots or (take > 0 and take + sz > share):
            break
        take += sz
        b_end += 1
    return b_end - cursor_b


def simulate(adm, rng, R_total, max_batch, n_jobs, C, serial, script=None):
    """The pools' loop around plan_admission with a device that retires a random number of slots per step.  Returns the admissions
    [(pool, first batch, batches)] after asserting the properties of every one.  `script` (a dict) receives the work list and what
    the device retired, step by step."""
    sizes = []
    while sum(sizes) < R_total:
        sizes.append(min(rng.randint(1, max_batch), R_total - sum(sizes)))
    n_batches = len(sizes)
    first = [0]
    for sz in sizes:
        first.append(first[-1] + sz)
    cfirst = i32(first)
    unit = max_batch == 1
    live, launched, phase, quota = [0] * n_jobs, [False] * n_jobs, [1] * n_jobs, [-1] * n_jobs
    quota_start = [None] * n_jobs
    cursor, admissions, turns = 0, [], 0
    while any(ph == 1 for ph in phase):
        turns += 1
        assert turns < 200000, "the pool loop does not terminate"
        only = min(i for i in range(n_jobs) if phase[i] == 1)
        for i in range(n_jobs):
            if phase[i] != 1 or (serial and i != only):
                continue
            if serial and quota[i] < 0:
                quota[i] = adm.ttx_host_serial_quota(cfirst, n_batches, cursor, i, n_jobs)
                quota_start[i] = cursor
                target = first[cursor] + cdiv(R_total - first[cursor], n_jobs - i)
                assert quota[i] == next(b for b in range(cursor, n_batches + 1) if b == n_batches or first[b] >= target)
            n_running = sum(ph == 1 for ph in phase)
            state = (cursor, C - live[i], live[i], int(not launched[i]), i, n_jobs, n_running, int(serial), quota[i])
            n = adm.ttx_host_plan_admission(cfirst, n_batches, C, *state)
            assert n == beam_take(first, n_batches, C, cursor, live[i], not launched[i], i, n_jobs, n_running, serial, quota[i]), state
            take = first[cursor + n] - first[cursor]                     # whole batches: never split
            if unit:
                assert n == take == greedy_take(R_total, C, cursor, live[i], not launched[i], i, n_jobs, n_running, serial, quota[i]), state
            if n:
                assert take <= C - live[i], "an admission beyond the free slots"
                if live[i] > 0:
                    assert C - live[i] >= max(C // 4, sizes[cursor]), "a small admission into a pool that is not empty"
                assert not serial or cursor + n <= quota[i]
                admissions.append((i, cursor, n))
                cursor += n
                live[i] += take
            if live[i] == 0:
                phase[i] = 3                                             # nothing live, nothing admitted: this pool is done
                assert cursor == (quota[i] if serial else n_batches), "a pool finished with its list not empty"
            else:
                launched[i] = True
                retired = rng.randint(0, live[i])                        # one step: some slots retire
                live[i] -= retired
                if script is not None:
                    script.setdefault("retire", []).append(retired)
    if script is not None:
        script["first"] = first
    # every batch (so every row) exactly once and in list order
    assert [a[1] for a in admissions] == sorted(a[1] for a in admissions)
    assert sum(a[2] for a in admissions) == n_batches and cursor == n_batches
    pos = 0
    for _, b0, n in admissions:
        assert b0 == pos
        pos += n
    if serial:                                                           # contiguous quotas that cover the list
        started = [i for i in range(n_jobs) if quota_start[i] is not None]
        assert started == list(range(len(started))) and quota_start[0] == 0
        for a, b in zip(started, started[1:]):
            assert quota_start[b] == quota[a]
        assert quota[started[-1]] == n_batches
        for i, b0, n in admissions:
            assert quota_start[i] <= b0 and b0 + n <= quota[i]
    return admissions


@pytest.mark.parametrize("serial", [False, True])
def test_plan_admission_in_a_simulated_pool_loop(adm, serial):
    rng = random.Random(31 if serial else 17)
    n_cases = 0
    for case in range(600):
        C = rng.choice([1, 2, 3, 4, 5, 7, 8, 16, 33, 64]) if case % 3 else rng.randint(1, 64)
        R_total = rng.randint(1, 300)
        max_batch = 1 if case % 2 == 0 else rng.randint(1, C)
        n_jobs = rng.randint(1, 4)
        admissions = simulate(adm, rng, R_total, max_batch, n_jobs, C, serial)
        assert admissions
        n_cases += 1
    assert n_cases == 600


def test_first_fill_of_a_list_that_fits_is_split_evenly(adm):
    """100 rows over 4 pools of 32 slots: 25 each at the first fill, although the first pool alone has room for 32."""
    first = i32(list(range(101)))
    cursor, takes = 0, []
    for i in range(4):
        n = adm.ttx_host_plan_admission(first, 100, 32, cursor, 32, 0, 1, i, 4, 4, 0, -1)
        takes.append(n)
        cursor += n
    assert takes == [25, 25, 25, 25]
    # a list that does not fit: the free slots, then a share of the rest for the pools still running
    assert adm.ttx_host_plan_admission(first, 100, 16, 0, 16, 0, 1, 0, 4, 4, 0, -1) == 16
    assert adm.ttx_host_plan_admission(first, 100, 16, 90, 8, 8, 0, 1, 4, 4, 0, -1) == 3      # ceil(10 / 4)
    assert adm.ttx_host_plan_admission(first, 100, 16, 90, 3, 13, 0, 1, 4, 4, 0, -1) == 0      # below a quarter pool


# ---- pool_step: whole calls on a fake device ------------------------------------------------------------------------------------
WAIT, FAILED, STUCK, DRAIN, LAUNCH = range(5)
FIELDS = ("job", "act", "first_batch", "n_take", "first_row", "rows", "n_live", "n_running", "cursor", "running_pools", "quota_end", "launched")


def pool_call(adm, sizes, n_jobs, C, serial=False, max_launches=10 ** 6, looks=(), retire=(), error_at=0, first=None):
    """-> (rc, [answer of every pool_step call, as a dict of FIELDS])"""
    if first is None:
        first = [0]
        for sz in sizes:
            first.append(first[-1] + sz)
    cap = 1 << 16
    log = (ctypes.c_int32 * (cap * len(FIELDS)))()
    rc = ctypes.c_int32(99)
    n = adm.ttx_host_pool_call(i32(first), len(first) - 1, n_jobs, C, int(serial), max_launches, i32(list(looks) or [0]), len(looks),
                               i32(list(retire) or [0]), len(retire), error_at, log, cap, ctypes.byref(rc))
    assert 0 < n <= cap
    return rc.value, [dict(zip(FIELDS, log[k * len(FIELDS):(k + 1) * len(FIELDS)])) for k in range(n)]


POOL_CASES = [([1] * 5, 1, 2), ([1] * 5, 2, 2), ([2, 1, 2], 1, 2), ([2, 1, 2], 2, 2)]      # batch sizes, pools, slots per pool


@pytest.mark.parametrize("serial", [False, True])
@pytest.mark.parametrize("sizes,n_jobs,C", POOL_CASES)
def test_pool_step_runs_a_whole_call(adm, sizes, n_jobs, C, serial):
    looks, retire = [0, 3, 1, 0, 2, 5, 0, 1], [1, 0, 2, 1, 1, 0, 2, 1, 1, 2, 1, 1]
    rc, log = pool_call(adm, sizes, n_jobs, C, serial=serial, looks=looks, retire=retire + [C] * 8)
    assert rc == 0 and not [a for a in log if a["act"] in (FAILED, STUCK)]
    first = [sum(sizes[:b]) for b in range(len(sizes) + 1)]
    # nothing is admitted or launched while unpublished: WAIT only, with the cursor and the counts untouched
    cursor, launched, waits = 0, [0] * n_jobs, 0
    for a in log:
        if a["act"] == WAIT:
            waits += 1
            assert launched[a["job"]] > 0, "a WAIT with nothing in flight"
            assert (a["cursor"], a["n_take"], a["rows"], a["n_live"], a["n_running"]) == (cursor, 0, 0, 0, 0), a
        else:
            assert a["first_batch"] == cursor and a["cursor"] == cursor + a["n_take"]
        assert a["launched"] == launched[a["job"]]
        cursor = a["cursor"]
        launched[a["job"]] += a["act"] == LAUNCH
    assert waits == sum(looks[:sum(launched)]), "the device publishes after its scripted number of looks"
    # every batch exactly once, in order and whole
    taken = [(a["first_batch"], a["n_take"], a["first_row"], a["rows"]) for a in log if a["n_take"]]
    assert all(a["act"] == LAUNCH for a in log if a["n_take"]), "an admission is followed by a launch in the same turn"
    pos = 0
    for b0, n, r0, rows in taken:
        assert b0 == pos and r0 == first[b0] and rows == first[b0 + n] - r0 and rows <= C
        pos += n
    assert pos == len(sizes) == cursor
    # DRAIN exactly once per pool, at zero live, as the pool's last answer; the running pools count down with it
    for i in range(n_jobs):
        mine = [a for a in log if a["job"] == i]
        assert [a["act"] for a in mine].count(DRAIN) == 1 and mine[-1]["act"] == DRAIN
        assert (mine[-1]["n_live"], mine[-1]["n_take"]) == (0, 0)
    assert all(a["n_live"] > 0 for a in log if a["act"] == LAUNCH)
    drains = [a["running_pools"] for a in log if a["act"] == DRAIN]
    assert drains == list(range(n_jobs - 1, -1, -1))
    # serial: one pool after another, and their quotas partition the list
    if serial:
        assert [a["job"] for a in log] == sorted(a["job"] for a in log)
        quotas = [[a for a in log if a["job"] == i][-1]["quota_end"] for i in range(n_jobs)]
        assert quotas == sorted(quotas) and quotas[-1] == len(sizes)
        for a in log:
            if a["n_take"]:
                lo = quotas[a["job"] - 1] if a["job"] else 0
                assert lo <= a["first_batch"] and a["first_batch"] + a["n_take"] <= quotas[a["job"]]
    else:
        assert all(a["quota_end"] == -1 for a in log)


def test_pool_step_error_word_fails_before_any_admission(adm):
    # two slots, one row retires per iteration: the second look would admit row 2, but iteration 1 published the error word
    rc, log = pool_call(adm, [1] * 5, 1, 2, retire=[1] * 9, looks=[2], error_at=1)
    assert rc == -1 and [a["act"] for a in log] == [LAUNCH, WAIT, WAIT, FAILED]
    assert (log[0]["n_take"], log[0]["cursor"]) == (2, 2)
    assert (log[-1]["n_take"], log[-1]["rows"], log[-1]["cursor"]) == (0, 0, 2)
    rc, log = pool_call(adm, [1] * 5, 1, 2, retire=[1] * 9)                    # the same call without it goes on admitting
    assert rc == 0 and log[1]["act"] == LAUNCH and log[1]["n_take"] == 1


@pytest.mark.parametrize("bound", [0, 1, 4])
def test_pool_step_stuck_exactly_beyond_the_bound(adm, bound):
    rc, log = pool_call(adm, [2, 1, 2], 1, 2, max_launches=bound)            # nothing ever retires
    assert rc == -2
    assert [a["act"] for a in log] == [LAUNCH] * (bound + 1) + [STUCK]         # launched 0 .. bound pass, bound + 1 is stuck
    assert [a["launched"] for a in log] == list(range(bound + 2))
    rc, log = pool_call(adm, [2, 1, 2], 1, 2, max_launches=3, retire=[2, 1, 2])     # three iterations: the bound is never met
    assert rc == 0 and [a["act"] for a in log] == [LAUNCH] * 3 + [DRAIN]


@pytest.mark.parametrize("serial", [False, True])
def test_pool_step_admits_what_the_simulated_loop_admits(adm, serial):
    """The inputs of test_plan_admission_in_a_simulated_pool_loop: pool_step under drive_jobs takes the batches that test's Python
    loop takes with plan_admission alone, pool by pool."""
    rng = random.Random(31 if serial else 17)
    for case in range(600):
        C = rng.choice([1, 2, 3, 4, 5, 7, 8, 16, 33, 64]) if case % 3 else rng.randint(1, 64)
        R_total = rng.randint(1, 300)
        max_batch = 1 if case % 2 == 0 else rng.randint(1, C)
        n_jobs = rng.randint(1, 4)
        script = {}
        admissions = simulate(adm, rng, R_total, max_batch, n_jobs, C, serial, script)
        rc, log = pool_call(adm, None, n_jobs, C, serial=serial, retire=script["retire"], first=script["first"])
        assert rc == 0
        assert [(a["job"], a["first_batch"], a["n_take"]) for a in log if a["n_take"]] == admissions, (case, C, R_total, n_jobs)
