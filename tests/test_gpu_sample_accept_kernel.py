"""k_sample_accept (csrc/ttx_loop_kernels.hip.h), the accept step of speculative sampling, one launch at a time through
ttx_debug_sample_accept, on operands the test builds, against the restatement of tests/util_sample_spec.py
(tests/test_sample_spec_host.py shows on the CPU that it reproduces position-by-position sampling and that the checker fails when it
should).  All of it is integer work: every array, every counter and every word published for the host must equal the restatement,
the sentinels must stand wherever the rule does not write, and the guard margins must be intact (util_loop_checks.check_loop).

Cases (util_sample_spec.accept_cases): accepted lengths 0 .. D on the first, a middle and the last draft and ties in every order; EOS
and PAD as the bonus token after every accepted length, one past it, and on a draft that was not chosen; new fronts on max_len - 2,
on max_len - 1 exactly and beyond it by 1 .. D, with an EOS in a kept and in a dropped column; some, none and all rows retiring; B = 1;
300 slots at (N, D) = (2, 2) with more finishers than the finished-row list holds; 1 100 slots (two rounds of the slot loop); several
consecutive steps on one device state; and k_kvcopy on the records the step produced.
"""
import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_sample_spec as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def launch(native, dev: U.DeviceLoop, s: U.LoopState, pred: np.ndarray, threads: int = 0) -> None:
    dev.pred.set(pred)
    words = native.debug_sample_accept(dev.entry_words(), B=s.B, n=s.N, d=s.D, Ls=s.Ls, max_len=s.max_len, pad=s.pad, bos=s.bos,
                                       eos=s.eos, gen_ld=s.gen_ld, threads=threads, pred=dev.pred.v, **dev.tensors())
    dev.set_exit_words(words)


def legal_threads(B: int) -> list:
    return [0, 1024] + ([256] if B <= 256 else [])


_CASES = {}


def case(name):
    if not _CASES:
        _CASES.update({n: (s, p) for n, s, p in X.accept_cases()})
    return _CASES[name]


@pytest.mark.parametrize("name", X.ACCEPT_CASE_NAMES)
def test_single_step(native, name):
    s, pred = case(name)
    want = X.sample_accept_step(s, pred)
    dev = U.DeviceLoop(s, DEV)
    for threads in legal_threads(s.B):
        dev.load(s)
        launch(native, dev, s, pred, threads)
        U.check_loop(dev, want, f"{name}, threads {threads}")
    n = s.words["n_active"]
    assert want.words["n_copy"] == n and want.words["error"] == s.words["error"] and (want.haspad == 0).all()
    assert want.words["stop"] == int(want.rec[:n, 4].all())


def test_nobody_running_publishes_nothing(native):
    s, pred = X.retire_case(5, 2, 1)
    s.words.update(n_active=0, r_rows=0, m_rows=0)
    want = X.sample_accept_step(s, pred)
    dev = U.DeviceLoop(s, DEV)
    launch(native, dev, s, pred)
    U.check_loop(dev, want, "n_active 0")
    assert want.words["host_steps_done"] == -1 and want.words["steps"] == s.words["steps"]


@pytest.mark.parametrize("B,N,D", [(300, 2, 2), (7, 3, 4)])
def test_replay(native, B, N, D):
    """Consecutive steps on ONE device state until the loop stops by itself: nothing is carried wrongly from step to step, the
    active list keeps its order through several compactions, and every row reaches the output."""
    rng = np.random.default_rng(B)
    max_len = 24
    s = X.init_state(rng.integers(3, 40, size=(B, N, D)), max_len, Ls=9)
    dev = U.DeviceLoop(s, DEV)
    steps = 0
    while not s.words["stop"]:
        assert steps < max_len, "the replay did not end by itself"
        pred = U.new_pred(s)
        for slot in range(int(s.words["n_active"])):
            acc = rng.integers(0, D + 1, size=N)
            ends = rng.random() < 0.15
            U.plant(s, pred, slot, acc, rng, [(int(acc.argmax()), int(acc.max()), U.EOS if rng.random() < 0.5 else U.PAD)] if ends else [])
        dev.bufs["drafts"].set(s.drafts)
        s = X.sample_accept_step(s, pred)
        launch(native, dev, s, pred)
        steps += 1
        U.check_loop(dev, s, f"B {B}, step {steps}")
    print(f"B {B}: {steps} steps, accepted {s.words['accepted'] - 0}, width {s.words['width']}")
    assert steps >= 4 and (s.out[:, 0] == U.BOS).all() and s.words["n_active"] == 0
    assert (s.out != U.SENTINEL[torch.int64]).all()


@pytest.mark.parametrize("d,Ld", [(64, 1), (256, 3)])
def test_kvcopy_commits_the_records(native, d, Ld):
    s, pred = case("lengths-N3-D2")
    dev = U.DeviceLoop(s, DEV)
    launch(native, dev, s, pred)
    want = X.sample_accept_step(s, pred)
    U.check_loop(dev, want, "the accept step the records come from")
    rec, n_copy, Lc = want.rec, want.words["n_copy"], s.max_len + s.D + 1
    live = rec[:n_copy]
    assert n_copy < s.B and {0, s.D} <= set(live[:, 2]) and {0, s.N - 1} <= set(live[:, 1])
    ops = U.kv_operands(rec, n_copy, s.B, s.N, s.D, d, Ld, Lc, seed=d + Ld)
    qkv = U.Buf(ops["qkv"].shape, torch.float32, DEV, ops["qkv"])
    kc, vc = U.Buf(ops["k0"].shape, torch.float32, DEV), U.Buf(ops["v0"].shape, torch.float32, DEV)
    native.debug_kvcopy(dev.bufs["rec"].v, n_copy, qkv.v, kc.v, vc.v, s.N, s.D, d, s.B)
    torch.cuda.synchronize()
    wk, wv = U.kv_commit(rec, n_copy, ops["qkv"], ops["k0"], ops["v0"], s.N, s.D)
    U.check_buf(kc, wk, f"K cache, d {d} Ld {Ld}")
    U.check_buf(vc, wv, f"V cache, d {d} Ld {Ld}")


def test_the_last_commit_fits_the_cache(native):
    """A row at front max_len - 2 that accepts D tokens commits K/V up to position max_len - 2 + D < Lc = max_len + D + 1."""
    s, pred = case("limit-N2-D5")
    want = X.sample_accept_step(s, pred)
    n = want.words["n_copy"]
    assert (want.rec[:n, 3] + want.rec[:n, 2] + 1).max() == s.max_len - 1 + s.D <= s.max_len + s.D + 1
    ops = U.kv_operands(want.rec, n, s.B, s.N, s.D, 64, 1, s.max_len + s.D + 1, seed=1)
    qkv = U.Buf(ops["qkv"].shape, torch.float32, DEV, ops["qkv"])
    kc, vc = U.Buf(ops["k0"].shape, torch.float32, DEV), U.Buf(ops["v0"].shape, torch.float32, DEV)
    rec = U.Buf(want.rec.shape, torch.int32, DEV, want.rec)
    native.debug_kvcopy(rec.v, n, qkv.v, kc.v, vc.v, s.N, s.D, 64, s.B)
    torch.cuda.synchronize()
    wk, wv = U.kv_commit(want.rec, n, ops["qkv"], ops["k0"], ops["v0"], s.N, s.D)
    U.check_buf(kc, wk, "K cache")
    U.check_buf(vc, wv, "V cache")


def test_invalid_arguments_are_refused(native):
    import translation_transformer_amd as tta
    s, pred = case("retire-120-of-300")
    dev = U.DeviceLoop(s, DEV)

    def refused(**kw):
        dev.pred.set(pred)
        a = dict(B=s.B, n=s.N, d=s.D, Ls=s.Ls, max_len=s.max_len, pad=s.pad, bos=s.bos, eos=s.eos, gen_ld=s.gen_ld, threads=0,
                 pred=dev.pred.v, **dev.tensors())
        a.update(kw)
        with pytest.raises(tta.TtxError) as e:
            native.debug_sample_accept(dev.entry_words(), **a)
        assert e.value.code == -1

    refused(threads=256)
    refused(threads=512)
    refused(gen_ld=s.max_len - 1)
    refused(front=None)
    refused(haspad=None)
    dev.words["n_active"] = 301
    refused()
    dev.load(s)
    launch(native, dev, s, pred)                                         # and nothing was launched in between
    U.check_loop(dev, X.sample_accept_step(s, pred), "after the refusals")
