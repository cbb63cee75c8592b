"""The schedule of the pools, pinned (tests/golden/pool_schedule.npz and pool_schedule_more.npz, written by
tests/golden/make_golden_pool_schedule.py).
On ONE session a pool's schedule is deterministic: one step is in flight and the host decides after each publish.  So which rows
share which step follows from the admission rule (csrc/ttx_admit.h), the order of the host's turns (csrc/ttx_drive.h) and the step
policy alone, and shows in the integer counters of the call, in the words of ttx_pool_last_counters and in the per-row traces.
Every check is exact equality with what the library gave when the fixture was recorded: a change to the admission rule or to the
driver that moves a single row to another step fails here, while the other GPU tests (tokens against the goldens) keep passing.

greedy pool  40 fixture rows of mixed lengths, longest first, 8 slots, TTX_ADMIT_ROWS=100 (every admission of two rows or more is
             split into length buckets): every step in one pass (TTX_TWO_PHASE=0), the default, and every step split
             (TTX_TWO_PHASE_MIN_ROWS=0, the probe path: 8 slots stay below the default threshold of the split)
beam pool    six batches of 1 to 4 sources, 4 source slots, smart_drafts_mode 0 and 1
pool_schedule_more.npz, the ten fixture sources, longest first, through 4 slots:
SBS pool       beam_size 3, max_len 30, mixed 64-bit keys: the counters of the call, the candidates decoded per source, the tokens
sampling pool  2 keyed samples per source (two sources fill the pool), (n_drafts, draft_len) = (3, 10): the counters of the call,
               the words of ttx_pool_last_counters, the tokens"""
import numpy as np
import pytest

import util_pool_schedule as U
from util_models import load_npz

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    import translation_transformer_amd as tta
    assert tta.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    m = U.make_model(tta)
    yield m
    m.close()


@pytest.fixture(scope="module")
def golden():
    return load_npz("pool_schedule.npz")


@pytest.fixture(scope="module")
def golden_more():
    return load_npz("pool_schedule_more.npz")


def check(golden, prefix, got):
    assert sorted(k for k in golden if k.startswith(prefix)) == sorted(prefix + k for k in got)
    for k, v in got.items():
        want = golden[prefix + k]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        assert np.array_equal(v, want), (k, np.argwhere(v != want)[:8].tolist(), v[v != want][:8].tolist(), want[v != want][:8].tolist())


@pytest.mark.parametrize("case", list(U.GREEDY_CASES))
def test_greedy_pool_schedule(model, golden, case):
    got = U.greedy_pool(model, case)
    assert got["stats"][0] > U.GREEDY_ROWS // U.GREEDY_CAPACITY and (got["fin_step"] > 0).all()     # many steps, every row finished
    check(golden, f"greedy__{case}__", got)


@pytest.mark.parametrize("case", list(U.BEAM_CASES))
def test_beam_pool_schedule(model, golden, case):
    check(golden, f"beam__{case}__", U.beam_pool(model, case))


def test_sbs_pool_schedule(model, golden_more):
    got = U.sbs_pool(model)
    S = got["out"].shape[0]
    assert got["stats"][0] > U.SBS_MAX_LEN and got["stats"][4] == 0          # more iterations than one fill decodes: the pool was refilled
    assert got["src_running_rows"].shape == (S,) and (got["src_running_rows"] > 0).all() and S > 2 * U.MORE_CAPACITY
    check(golden_more, "sbs__", got)


def test_sampling_pool_schedule(model, golden_more):
    got = U.sampling_pool(model)
    S = got["out"].shape[0]
    assert got["stats"][0] > S * U.SAMPLE_PER_SRC // U.MORE_CAPACITY and (got["out"][:, :, 0] == U.BOS).all()   # many steps, every row written
    check(golden_more, "sampling__", got)
