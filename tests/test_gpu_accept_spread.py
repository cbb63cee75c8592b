"""k_accept in two launches (k_accept_slots on many workgroups, then k_accept_finish on one; csrc/ttx_loop_kernels.hip.h) against the
one-workgroup k_accept on the same operands, through ttx_debug_accept: ``threads = 0`` is the production route, which is the pair
above 256 slots, ``threads = 1024`` the single kernel.  All of it is integer work: every output array, the guard margins around
it and all 17 state words are compared by exact equality, against each other and against the plain restatement of
tests/util_loop_checks.py.  After every call the block of sums between the two launches (ttx_debug_accept_block) is zero again.

Paths executed on purpose: B = 257 (the first capacity of the pair), 300, 1 024 (every slot workgroup full), 1 100 (a ragged last
workgroup; two rounds of the finish kernel's compaction); n_active = 0 (nothing published, nothing summed), 1, 63 / 64 / 65 (around
one slot workgroup), B; no rule, row_rule and pool; rows that finish, rows the width rule retires, a PAD written inside a row
(haspad, errors 2 and 3), more than 256 finishers (the finished-row list overflows and the copy scans all slots)."""
import numpy as np
import pytest
import torch

import util_loop_checks as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_DRAFTS, D_LEN, MAX_LEN = 3, 10, 60


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def launch(native, dev: U.DeviceLoop, s: U.LoopState, pred: np.ndarray, threads: int) -> None:
    dev.pred.set(pred)
    words = native.debug_accept(dev.entry_words(), B=s.B, n=s.N, d=s.D, Ls=s.Ls, max_len=s.max_len, pad=s.pad, bos=s.bos, eos=s.eos,
                                gen_ld=s.gen_ld, threads=threads, row_rule=bool(s.row_rule), pool=bool(s.pool), traj_ld=s.traj_ld,
                                pool_rows=s.pool_rows, pred=dev.pred.v, **dev.tensors())
    dev.set_exit_words(words)


def pair_against_single(native, s: U.LoopState, pred: np.ndarray, what: str) -> U.LoopState:
    """Both routes from the same operands: identical arrays (margins included) and words, equal to the restatement's; block zero."""
    want = U.accept_step(s, pred)
    dev = U.DeviceLoop(s, DEV)
    launch(native, dev, s, pred, 1024)
    single = {k: b.buf.clone() for k, b in dev.bufs.items()}            # Buf.buf: the array and its guard margins
    single_words = dict(dev.words)
    U.check_loop(dev, want, f"{what}: one workgroup")
    dev.load(s)
    launch(native, dev, s, pred, 0)
    U.check_loop(dev, want, f"{what}: pair")
    for k, b in dev.bufs.items():
        assert torch.equal(b.buf, single[k]), f"{what}: {k} differs between the pair and the one-workgroup kernel"
    assert dev.words == single_words, f"{what}: state words differ"
    blk = native.debug_accept_block()
    assert not any(blk), f"{what}: the block between the launches is not zero: {[(i, v) for i, v in enumerate(blk) if v][:8]}"
    return want


def mixed_case(B: int, n_active: int, mode: str, seed: int, p_pad: float = 0.0):
    """Ragged fronts, every fifth row so far right that the width rule retires it under row_rule, EOS among the predictions of about
    a third of the slots."""
    rng = np.random.default_rng(seed)
    fronts = rng.integers(0, MAX_LEN - D_LEN - 6, size=B)
    fronts[rng.integers(0, B)] = 0
    if mode != "plain":                                                  # without the rule such a front would end the whole loop
        fronts[::5] = rng.integers(MAX_LEN - D_LEN - 2, MAX_LEN - D_LEN + 1, size=len(fronts[::5]))     # f + D + 2 >= max_len
    s = U.make_state(B, N_DRAFTS, D_LEN, MAX_LEN, fronts, n_active=n_active, seed=seed, row_rule=mode != "plain", pool=mode == "pool")
    return s, U.plant_random(s, rng, p_fin=0.35, p_pad=p_pad)


@pytest.mark.parametrize("mode", ["plain", "row_rule", "pool"])
@pytest.mark.parametrize("B", [257, 300, 1024, 1100])
def test_pair_equals_single(native, B, mode):
    for n_active in (0, 1, 63, 64, 65, B):
        s, pred = mixed_case(B, n_active, mode, seed=B * 7 + n_active)
        want = pair_against_single(native, s, pred, f"B {B} n_active {n_active} {mode}")
        if n_active == 0:
            assert want.words["host_steps_done"] == -1
            continue
        flags = want.rec[:n_active, 4]
        assert want.words["n_copy"] == n_active
        if n_active >= 63:
            assert (flags == 1).any() and (flags == 0).any(), "the case has finishers and rows that run on"
            assert (flags == 2).any() == (mode != "plain"), "rows retired by the width rule, under the rule alone"


@pytest.mark.parametrize("mode", ["plain", "pool"])
@pytest.mark.parametrize("B,n_fin", [(300, 257), (1100, 256), (1100, 300), (1100, 1100)])
def test_many_finishers(native, B, n_fin, mode):
    s, pred = U.finish_case(B, n_fin, seed=B + n_fin)
    if mode == "pool":
        t = U.make_state(B, s.N, s.D, s.max_len, s.front, seed=B + n_fin, row_rule=True, pool=True)
        t.act_idx, t.gen, t.drafts = s.act_idx, s.gen, s.drafts
        s = t
    want = pair_against_single(native, s, pred, f"{n_fin} of {B} finish, {mode}")
    assert int((want.rec[:B, 4] == 1).sum()) == n_fin and want.words["stop"] == int(n_fin == B)


@pytest.mark.parametrize("mode", ["plain", "row_rule", "pool"])
def test_pad_inside_a_row(native, mode):
    """A PAD among the written tokens of running rows: haspad, and error 3 under the rule (error 2 needs an all-PAD column)."""
    s, pred = mixed_case(300, 300, mode, seed=5, p_pad=0.2)
    want = pair_against_single(native, s, pred, f"PAD written, {mode}")
    assert want.haspad.sum() > 0 and want.words["error"] == (0 if mode == "plain" else 3)
    if mode == "plain":
        s.gen[:, 3] = U.PAD                                             # quirk 2: column 3 is PAD in every running row
        s.front[:] = np.maximum(s.front, 6)
        want = pair_against_single(native, s, pred, "PAD column")
        assert want.words["error"] == 2 and want.words["stop"] == 1


def test_consecutive_steps_on_one_state(native):
    """Steps of the pair on ONE device state until the run ends by itself: the block is zero between any two of them."""
    rng = np.random.default_rng(11)
    s = U.init_state(rng.integers(3, 40, size=(700, N_DRAFTS, D_LEN)), 150, Ls=9)
    dev = U.DeviceLoop(s, DEV)
    steps = 0
    while not s.words["stop"]:
        assert steps < 40, "the replay did not end by itself"
        pred = U.plant_random(s, rng, p_fin=0.8)
        dev.bufs["drafts"].set(s.drafts)
        s = U.accept_step(s, pred)
        launch(native, dev, s, pred, 0)
        steps += 1
        U.check_loop(dev, s, f"step {steps}")
        assert not any(native.debug_accept_block()), f"step {steps}: block not zero"
    assert steps >= 8
