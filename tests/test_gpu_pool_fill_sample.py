"""One admission of the sampling slot pool (k_pool_admit + k_pool_fill, csrc/ttx_loop_kernels.hip.h) through
ttx_debug_pool_fill_sample, against tests/util_sample_pool.admit: S_chunk = 3 staged sources x n samples into 12 slots of which 3 are
occupied (at least 9 stay free).  key, sample, row_of, front, src_len, the gen rows, the drafts, the validity bytes and the cross
K/V of every new slot must be exactly those of source i / n, the caller rows read BOS then PAD, occupied slots and unrelated caller
rows keep what they held, n_active / m_rows are right, and rows beyond the free slots raise error 4 with nothing filled.
"""
import numpy as np
import pytest
import torch

import util_loop_checks as U
import util_sample_pool as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
C, N, D, MAX_LEN, LS_CAP, LS_NEW, KV_ROW, S_CHUNK = 12, 3, 2, 9, 11, 7, 24, 3
DT = {"key": torch.int64, "src_valid": torch.uint8, "memkv": torch.float32, "out": torch.int64}


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


def setup(n: int, occupied, first_src: int, seed: int):
    rng = np.random.default_rng(seed)
    pool = P.Pool(C, N, D, MAX_LEN, LS_CAP, KV_ROW, out_rows=(first_src + S_CHUNK) * n + 4, rng=rng)
    pool.act_idx[:len(occupied)] = occupied
    pool.n_active = len(occupied)
    drafts_new = rng.integers(3, 40, size=(S_CHUNK, N * D), dtype=np.int32)
    valid_new = (rng.random((S_CHUNK, LS_NEW)) < 0.8).astype(np.uint8)
    memkv_new = rng.standard_normal((S_CHUNK, LS_NEW, KV_ROW)).astype(np.float32)
    keys = rng.integers(-2 ** 62, 2 ** 62, size=first_src + S_CHUNK, dtype=np.int64)
    return pool, drafts_new, valid_new, memkv_new, keys


def run(native, pool: P.Pool, drafts_new, valid_new, memkv_new, n: int, first_src: int, keys, over=None):
    bufs = {name: U.Buf(getattr(pool, name).shape, DT.get(name, torch.int32), DEV, getattr(pool, name)) for name in P.Pool.ARRAYS}
    staged = dict(drafts_new=U.Buf(drafts_new.shape, torch.int32, DEV, drafts_new), valid_new=U.Buf(valid_new.shape, torch.uint8, DEV, valid_new),
                  memkv_new=U.Buf(memkv_new.shape, torch.float32, DEV, memkv_new))
    if keys is not None:
        staged["row_keys"] = U.Buf(keys.shape, torch.int64, DEV, keys)
    a = dict(B=C, n=N, d=D, n_active=pool.n_active, n_sources=S_CHUNK, per_src=n, first_src=first_src, Ls_new=LS_NEW, Ls_cap=LS_CAP,
             gen_ld=pool.gen_ld, kv_row=KV_ROW, max_len=MAX_LEN, out_rows=pool.out.shape[0], bos=U.BOS, pad=U.PAD)
    a.update(over or {})
    arrays = {k: b.v for k, b in {**bufs, **staged}.items()}
    arrays["src_valid"], arrays["valid_new"] = bufs["src_valid"].v, staged["valid_new"].v
    res = native.debug_pool_fill_sample(**a, **arrays)
    torch.cuda.synchronize()
    return res, bufs, staged


def check(bufs, staged, want: P.Pool, what: str) -> None:
    for name in P.Pool.ARRAYS:
        U.check_buf(bufs[name], getattr(want, name), f"{what}: {name}")
    for name, b in staged.items():
        assert b.margins() is None, f"{what}: {name}: {b.margins()}"


@pytest.mark.parametrize("with_keys", [True, False])
@pytest.mark.parametrize("n", [1, 3])
def test_admission_equals_the_restatement(native, n, with_keys):
    occupied = [7, 0, 4]                                                # a non-identity list: the new rows take 1, 2, 3, 5, 6, 8, ...
    first_src = 5
    pool, drafts_new, valid_new, memkv_new, keys = setup(n, occupied, first_src, seed=n)
    want = pool.clone()
    wres = P.admit(want, drafts_new, valid_new, memkv_new, n, first_src, keys if with_keys else None)
    res, bufs, staged = run(native, pool, drafts_new, valid_new, memkv_new, n, first_src, keys if with_keys else None)
    assert res == wres and res["n_active"] == 3 + S_CHUNK * n and res["m_rows"] == res["n_active"] * (1 + N * D) and res["error"] == 0
    check(bufs, staged, want, f"n {n} keys {with_keys}")
    new = want.act_idx[3:3 + S_CHUNK * n]
    assert new.tolist() == [b for b in range(C) if b not in occupied][:S_CHUNK * n]
    assert want.sample[new].tolist() == [i % n for i in range(S_CHUNK * n)]
    assert want.row_of[new].tolist() == [first_src * n + i for i in range(S_CHUNK * n)]
    rows = want.out[first_src * n:(first_src + S_CHUNK) * n]
    assert (rows[:, 0] == U.BOS).all() and (rows[:, 1:] == U.PAD).all()
    assert (want.out[:first_src * n] == -7).all() and (want.out[(first_src + S_CHUNK) * n:] == -7).all()
    for b in occupied:                                                  # occupied slots keep what they held
        assert (want.gen[b] == pool.gen[b]).all() and want.key[b] == pool.key[b] and (want.memkv[b] == pool.memkv[b]).all()


def test_more_rows_than_free_slots_is_error_4_and_fills_nothing(native):
    occupied = [7, 0, 4, 1, 9]                                          # 7 free slots, 9 rows
    pool, drafts_new, valid_new, memkv_new, keys = setup(3, occupied, 0, seed=9)
    want = pool.clone()
    wres = P.admit(want, drafts_new, valid_new, memkv_new, 3, 0, keys)
    res, bufs, staged = run(native, pool, drafts_new, valid_new, memkv_new, 3, 0, keys)
    assert res == wres and res["error"] == 4
    check(bufs, staged, want, "error 4")
    assert (want.gen == pool.gen).all() and (want.out == pool.out).all()


def test_refused_arguments(native):
    from translation_transformer_amd._native import TtxError
    pool, drafts_new, valid_new, memkv_new, keys = setup(3, [7, 0, 4], 0, seed=2)
    for kw in (dict(B=0), dict(n_active=C + 1), dict(n_sources=0), dict(per_src=0), dict(first_src=-1), dict(Ls_new=LS_CAP + 1), dict(kv_row=6),
               dict(out_rows=8), dict(max_len=0), dict(d=0)):
        with pytest.raises(TtxError) as e:
            run(native, pool, drafts_new, valid_new, memkv_new, 3, 0, keys, over=kw)
        assert e.value.code == -1, kw
    dup = pool.clone()
    dup.act_idx[:3] = [7, 7, 4]
    with pytest.raises(TtxError):
        run(native, dup, drafts_new, valid_new, memkv_new, 3, 0, keys)
    res, bufs, staged = run(native, pool, drafts_new, valid_new, memkv_new, 3, 0, keys)      # and the session still works
    assert res["error"] == 0 and res["n_active"] == 12
