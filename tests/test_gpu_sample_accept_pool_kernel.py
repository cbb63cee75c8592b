"""The accept step of the sampling slot pool (csrc/ttx_loop_kernels.hip.h), through ttx_debug_sample_accept_pool, on operands the
test builds, against the restatement of tests/util_sample_pool.py (accept_pool_step: util_sample_spec's rule with the pool's caller
rows and executed-row count).  Both forms are checked and held to each other: ONE launch of k_sample_accept (256 and 1 024 threads)
and the pair k_sample_accept_slots + k_accept_finish, which must leave the session's AcceptBlk zero.  Every array, counter and
published word must equal the restatement, ended rows must land in pool_out[row_of[b]] with every other caller row keeping its
sentinel, and the guard margins must be intact (util_loop_checks.check_loop).

Cases: util_sample_spec's constructed cases (accepted lengths 0 .. D on each draft and ties in every order, EOS and PAD as the bonus
token and one past it, fronts on max_len - 2, max_len - 1 and beyond with an EOS in a kept and in a dropped column) at (N, D) in
(1,1), (2,2), (3,4), (5,13) = 65 elements with a draft straddling a pass of 64, (1,70) = a draft longer than a pass, (64,1) = one
element per draft; B in 1, 5, 300, 1 100 with none, some and all rows retiring, 270 of 300 among them; the executed-row count; and
7 consecutive steps on one device state.
"""
import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_sample_pool as P
import util_sample_spec as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
ND = [(1, 1), (2, 2), (3, 4), (5, 13), (1, 70), (64, 1)]


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def launch(native, dev: U.DeviceLoop, s: U.LoopState, pred: np.ndarray, threads: int = 0, spread: bool = False, exec_rows=None) -> None:
    dev.pred.set(pred)
    ex = None if exec_rows is None else torch.tensor([exec_rows], dtype=torch.int32, device=DEV)
    words = native.debug_sample_accept_pool(dev.entry_words(), B=s.B, n=s.N, d=s.D, Ls=s.Ls, max_len=s.max_len, pad=s.pad, bos=s.bos,
                                            eos=s.eos, gen_ld=s.gen_ld, pool_rows=s.pool_rows, threads=threads, spread=spread,
                                            exec_rows=ex, pred=dev.pred.v, **dev.tensors())
    dev.set_exit_words(words)
    if spread:
        assert not any(native.debug_accept_block()), "the pair left words in the AcceptBlk"


def forms(B: int) -> list:
    """(threads, spread) of every launch the entry makes at B slots."""
    return [(0, False), (1024, False), (0, True)] + ([(256, False)] if B <= 256 else [])


def check_all_forms(native, s: U.LoopState, pred: np.ndarray, what: str, exec_rows=None) -> U.LoopState:
    want = P.accept_pool_step(s, pred, exec_rows)
    dev = U.DeviceLoop(s, DEV)
    for threads, spread in forms(s.B):
        dev.load(s)
        launch(native, dev, s, pred, threads, spread, exec_rows)
        U.check_loop(dev, want, f"{what}, threads {threads}, spread {spread}")
    n = s.words["n_active"]
    fin = want.rec[:n, 4] == 1
    rows = s.act_idx[:n]
    ended = set(int(r) for r in s.row_of[rows[fin]])
    sent = U.SENTINEL[torch.int64]
    for r in range(s.pool_rows):                                        # ended rows, and nothing else, reached the caller's rows
        assert (want.pool_out[r] != sent).all() if r in ended else (want.pool_out[r] == sent).all(), f"{what}: caller row {r}"
    assert (want.haspad == 0).all() and want.words["error"] == s.words["error"]
    return want


def constructed(N: int, D: int) -> list:
    return [("lengths",) + X.lengths_case(N, D), ("ending",) + X.ending_case(N, D), ("limit",) + X.limit_case(N, D)]


@pytest.mark.parametrize("N,D", ND)
def test_constructed_cases(native, N, D):
    for name, s, pred in constructed(N, D):
        want = check_all_forms(native, P.to_pool(s, seed=N + D), pred, f"{name} N {N} D {D}")
        n = s.words["n_active"]
        if name == "lengths":
            assert set(want.rec[:n, 2]) >= {0, D}, "the case does not reach both ends of the accepted lengths"
        if name == "limit":
            assert (want.rec[:n, 4] == 1).any() and (want.rec[:n, 4] == 0).any()


@pytest.mark.parametrize("B,n_fin", [(1, 0), (1, 1), (5, 0), (5, 2), (5, 5), (300, 0), (300, 120), (300, 270), (300, 300), (1100, 400)])
def test_retiring_rows(native, B, n_fin):
    s, pred = X.retire_case(B, n_fin, seed=B + n_fin)
    want = check_all_forms(native, P.to_pool(s, seed=B), pred, f"{n_fin} of {B} retire")
    assert int((want.rec[:B, 4] == 1).sum()) == n_fin and want.words["stop"] == int(n_fin == B)


@pytest.mark.parametrize("N,D", [(5, 13), (3, 4)])
def test_wide_slots_at_many_slots(native, N, D):
    """300 slots of 65 elements: every wave of the spread form meets a draft that straddles its pass."""
    rng = np.random.default_rng(N * D)
    s = P.make_pool_state(300, N, D, 90, rng.integers(0, 60, size=300), n_active=290, seed=5)
    pred = U.plant_random(s, rng, p_fin=0.3, p_pad=0.1)
    check_all_forms(native, s, pred, f"300 slots N {N} D {D}")


def test_verified_positions_follow_the_executed_rows(native):
    s, pred = X.retire_case(40, 13, 11)
    s = P.to_pool(s)
    base = check_all_forms(native, s, pred, "exec_rows absent")
    got = check_all_forms(native, s, pred, "exec_rows 57", exec_rows=57)
    assert got.words["verified_positions"] == s.words["verified_positions"] + 57
    assert base.words["verified_positions"] == s.words["verified_positions"] + 40 * U.rps(s.N, s.D)


def test_nobody_running_publishes_nothing(native):
    s, pred = X.retire_case(5, 2, 1)
    s = P.to_pool(s)
    s.words.update(n_active=0, r_rows=0, m_rows=0)
    want = check_all_forms(native, s, pred, "n_active 0")
    assert want.words["host_steps_done"] == -1 and want.words["steps"] == s.words["steps"]


@pytest.mark.parametrize("B,N,D,spread", [(300, 2, 2, True), (300, 2, 2, False), (7, 3, 4, True)])
def test_replay_of_seven_steps(native, B, N, D, spread):
    """7 consecutive steps on ONE device state: nothing is carried wrongly from step to step, the active list keeps its order through
    the compactions, the AcceptBlk is zero between the steps."""
    rng = np.random.default_rng(B + N)
    max_len = 40
    s = P.to_pool(X.init_state(rng.integers(3, 40, size=(B, N, D)), max_len, Ls=9), seed=3)
    dev = U.DeviceLoop(s, DEV)
    for step in range(1, 8):
        assert not s.words["stop"]
        pred = U.new_pred(s)
        for slot in range(int(s.words["n_active"])):
            acc = rng.integers(0, D + 1, size=N)
            ends = rng.random() < 0.1
            U.plant(s, pred, slot, acc, rng, [(int(acc.argmax()), int(acc.max()), U.EOS if rng.random() < 0.5 else U.PAD)] if ends else [])
        dev.bufs["drafts"].set(s.drafts)
        s = P.accept_pool_step(s, pred)
        launch(native, dev, s, pred, spread=spread)
        U.check_loop(dev, s, f"B {B} spread {spread}, step {step}")
    assert s.words["steps"] == 7 and 0 < s.words["n_active"] and (s.words["n_active"] < B or B < 50)


def test_invalid_arguments_are_refused(native):
    import translation_transformer_amd as tta
    s, pred = X.retire_case(300, 120, 16)
    s = P.to_pool(s)
    dev = U.DeviceLoop(s, DEV)

    def refused(**kw):
        dev.pred.set(pred)
        a = dict(B=s.B, n=s.N, d=s.D, Ls=s.Ls, max_len=s.max_len, pad=s.pad, bos=s.bos, eos=s.eos, gen_ld=s.gen_ld, pool_rows=s.pool_rows,
                 pred=dev.pred.v, **dev.tensors())
        a.update(kw)
        with pytest.raises(tta.TtxError) as e:
            native.debug_sample_accept_pool(dev.entry_words(), **a)
        assert e.value.code == -1

    refused(threads=256)
    refused(threads=1024, spread=True)
    refused(gen_ld=s.max_len - 1)
    refused(row_of=None)
    refused(pool_out=None)
    refused(pool_rows=0)
    refused(pool_rows=3)                                                 # a row_of beyond the caller's rows
    refused(haspad=None)
    dev.load(s)
    launch(native, dev, s, pred)                                         # and nothing was launched in between
    U.check_loop(dev, P.accept_pool_step(s, pred), "after the refusals")
