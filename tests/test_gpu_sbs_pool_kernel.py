"""The kernels of the stochastic beam pool (csrc/ttx_sbs_pool.hip.h) one launch at a time.

Step kernels (ttx_debug_sbs_step_pool).  One launch over C = 4 slots: slot 0 fresh (level 1, one live parent), slot 1 at level 2 and
slot 2 at level 9 or 23 with K parents (about a fifth finished), slot 3 free and full of sentinels.  Every output array must equal,
bit for bit, what ttx_debug_sbs_step (no filter, no prefix) or ttx_debug_sbs_step_ex writes when launched per source (B = 1) with that
slot's own scalars; the free slot's outputs keep their sentinels, the guard margins stay intact and no input is written.  No
tolerance anywhere: the per-batch kernels are the oracle (tests/test_gpu_sbs_kernel.py and test_gpu_sbs_mask_kernel.py hold THEM to
float64).

Bookkeeping kernels (ttx_debug_sbs_pool).  A pool of C = 3 slots walked launch by launch beside the NumPy restatement
(tests/util_sbs_pool_checks.py, in float32): init, admit + fill, a step (the restatement's, uploaded), retire, publish, and a slot
retired and re-admitted in consecutive launches; after each launch every array and word equals the restatement's.
"""
import numpy as np
import pytest
import torch

import util_beam_checks as B
import util_sbs_checks as S
import util_sbs_pool_checks as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32, I64, F32, U8 = np.int32, np.int64, np.float32, np.uint8
PAD, EOS = 0, 2
C_SLOTS, LD = 4, 26
STEP_IN = ["logits", "slot_of", "finished", "phi", "g", "gen", "row_of", "level", "nlive", "key"]
STEP_OUT = ["new_cand", "new_phi", "new_g", "parent", "new_len", "new_finished", "parent_draft", "nfin"]
PFX = ["pfx_tok", "pfx_len", "pfx_src"]


@pytest.fixture(scope="module")
def native():
    import translation_transformer_amd as t
    from util_models import tiny_state
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    st, cfg = tiny_state()
    return t.NativeTransformer(st, cfg["num_heads"], 0, device=0)      # any model gives a session; the shapes are arguments


# -- step kernels ---------------------------------------------------------------------------------------------------------------------
def pool_case(V: int, K: int, deep: int, salt: int) -> dict:
    """The operands of one launch: slot states from util_sbs_checks.make_state, logits rows compacted in an order of their own."""
    rng = np.random.default_rng([V, K, deep, salt, 2024])
    n = C_SLOTS * K
    level = np.array([1, 2, deep, 5], I32)
    nlive = np.array([1, K, K, K], I32)
    row_of = np.array([3, 0, 7, -1], I32)
    fin = np.ones(n, U8)
    phi, G = B.sent(n, F32), B.sent(n, F32)
    gen = B.sent((n, LD), I32)
    for s in range(3):
        beam = int(nlive[s])
        p, g, f, rows = S.make_state(rng, beam, int(level[s]), V, PAD, EOS)
        c0 = s * K
        phi[c0:c0 + beam], G[c0:c0 + beam], fin[c0:c0 + beam] = p, g, f
        gen[c0:c0 + beam] = PAD
        gen[c0:c0 + beam, :level[s]] = rows
    if K > 1:
        fin[2 * K + 1] = 1                                                # slot 2 always has a finished parent
        if K >= 5:
            G[1 * K + K - 1] = -np.inf                                    # and slot 1 a -inf parent (a masked child selected earlier)
            phi[1 * K + K - 1] = -np.inf
            fin[1 * K + K - 1] = 1
    live = np.nonzero(fin == 0)[0]
    slot_of = np.full(n, -1, I32)
    slot_of[live] = rng.permutation(len(live)).astype(I32)
    logits = np.zeros((len(live), V), F32)
    logits[slot_of[live]] = S.make_logits(rng, len(live), V)              # a tenth of the entries -inf
    key = rng.integers(-2 ** 62, 2 ** 62, C_SLOTS).astype(I64)
    return dict(V=V, K=K, logits=logits, slot_of=slot_of, finished=fin, phi=phi, g=G, gen=gen, row_of=row_of, level=level, nlive=nlive,
                key=key, seed=int(rng.integers(0, 2 ** 63)), temperature=float(rng.choice([0.5, 1.0, 3.0])))


def outputs(K: int) -> dict:
    n = C_SLOTS * K
    return dict(new_cand=B.sent((n, LD), I64), new_phi=B.sent(n, F32), new_g=B.sent(n, F32), parent=B.sent(n, I32), new_len=B.sent(n, I32),
                new_finished=B.sent(n, U8), parent_draft=B.sent(n, I32), nfin=B.sent(C_SLOTS, I32))


def prefix_table(c: dict, mode):
    """The table by slot for prefix lengths 0, 3, or longer than the slot's level (None: no table)."""
    if mode is None:
        return None
    rng = np.random.default_rng([c["V"], c["K"], 77])
    ld = LD - 1
    tok = rng.integers(0, c["V"], (C_SLOTS, ld)).astype(I32)
    src = np.array([2, 0, 3, 1], I32)                                    # the slots' rows of the table, not in slot order
    tok[src[1], 1] = c["V"] + 5                                          # slot 1 at level 2: an id outside the vocabulary reads as 0
    tok[src[0], 0] = EOS                                                 # a forced EOS ends the fresh slot's rows
    n = {"0": np.zeros(C_SLOTS, I32), "3": np.full(C_SLOTS, 3, I32), "long": np.minimum(c["level"] + 2, ld).astype(I32)}[mode]
    return dict(pfx_tok=tok, pfx_len=n, pfx_src=src)


def launch_pool(native, c: dict, masked: bool, top_k: int, top_p: float, pfx) -> dict:
    arrays = {k: c[k] for k in STEP_IN}
    arrays.update(outputs(c["K"]))
    extra = {}
    if pfx is not None:
        arrays.update(pfx)
        extra = dict(pfx_ld=pfx["pfx_tok"].shape[1], pfx_sources=C_SLOTS)
    bufs = B.upload(arrays, DEV)
    native.debug_sbs_step_pool(V=c["V"], ld=LD, C_=C_SLOTS, K=c["K"], pad=PAD, eos=EOS, seed=c["seed"],
                               inv_T=float(np.float32(1.0) / np.float32(c["temperature"])), masked=masked, top_k=top_k, top_p=top_p,
                               **extra, **{k: B.dev(bufs[k]) for k in bufs})
    torch.cuda.synchronize()
    B.check_margins(bufs)
    B.check_inputs(bufs, arrays, STEP_IN + (PFX if pfx is not None else []))
    return B.download(bufs, STEP_OUT)


def launch_source(native, c: dict, s: int, masked: bool, top_k: int, top_p: float, pfx) -> dict:
    """Slot s as a per-batch launch of one source with the slot's own scalars."""
    K, beam, width = c["K"], int(c["nlive"][s]), int(c["level"][s])
    cs = slice(s * K, s * K + beam)
    live = np.nonzero(c["slot_of"][cs] >= 0)[0]
    slot_of = np.full(beam, -1, I32)
    slot_of[live] = np.arange(len(live), dtype=I32)
    logits = np.zeros((max(len(live), 1), c["V"]), F32)
    logits[:len(live)] = c["logits"][c["slot_of"][cs][live]]
    arrays = dict(logits=logits, slot_of=slot_of, finished=c["finished"][cs], phi=c["phi"][cs], g=c["g"][cs], gen=c["gen"][cs],
                  key=c["key"][s:s + 1], new_cand=B.sent((K, LD), I64), new_phi=B.sent(K, F32), new_g=B.sent(K, F32), parent=B.sent(K, I32),
                  new_len=B.sent(K, I32), new_finished=B.sent(K, U8), parent_draft=B.sent(K, I32), summary=np.zeros(5, I32))
    kw = dict(V=c["V"], ld=LD, width=width, B=1, beam=beam, K=K, pad=PAD, eos=EOS, pos=width, seed=c["seed"],
              inv_T=float(np.float32(1.0) / np.float32(c["temperature"])))
    if not masked:
        bufs = B.upload(arrays, DEV)
        native.debug_sbs_step(**kw, **{k: B.dev(bufs[k]) for k in bufs})
    else:
        if pfx is not None:
            row = int(pfx["pfx_src"][s])
            arrays.update(pfx_tok=pfx["pfx_tok"][row:row + 1], pfx_len=pfx["pfx_len"][s:s + 1], pfx_src=np.zeros(1, I32))
            kw.update(pfx_ld=pfx["pfx_tok"].shape[1], pfx_sources=1)
        bufs = B.upload(arrays, DEV)
        native.debug_sbs_step_ex(**kw, top_k=top_k, top_p=top_p, **{k: B.dev(bufs[k]) for k in bufs})
    torch.cuda.synchronize()
    B.check_margins(bufs)
    return B.download(bufs, ["new_cand", "new_phi", "new_g", "parent", "new_len", "new_finished", "parent_draft", "summary"])


def shapes():
    out = []
    vk = [(V, K) for V in (7, 64, 256, 1000) for K in (1, 5, 32) if K <= V and K * V * 4 <= 150 * 1024]
    for i, (V, K) in enumerate(vk):
        deep = 9 if i % 2 == 0 else 23
        out.append((V, K, deep, False, 0, 1.0, None))                    # k_sbs_step_pool against k_sbs_step
        out.append((V, K, deep, True, 8, 0.9, "3"))                      # filter and prefixes of length 3
    for K in (1, 5, 32):
        out.append((64, K, 23, True, 0, 1.0, "long"))                    # every live slot forced
    out.append((256, 5, 9, True, 8, 0.9, "0"))                           # a table that forces nothing
    out.append((1000, 5, 23, True, 0, 1.0, None))                        # the masked kernel with nothing to mask
    return out


SHAPES = shapes()


@pytest.mark.parametrize("V,K,deep,masked,top_k,top_p,pfx_mode", SHAPES,
                         ids=[f"V{v}-K{k}-L{d}-{'masked' if m else 'plain'}-k{tk}-p{tp}-pfx{pm}" for v, k, d, m, tk, tp, pm in SHAPES])
def test_step_pool_equals_the_per_source_launches(native, V, K, deep, masked, top_k, top_p, pfx_mode):
    c = pool_case(V, K, deep, 0)
    pfx = prefix_table(c, pfx_mode)
    got = launch_pool(native, c, masked, top_k, top_p, pfx)
    blank = outputs(K)
    for s in range(C_SLOTS):
        ks = slice(s * K, (s + 1) * K)
        if c["row_of"][s] < 0:
            for name in STEP_OUT[:-1]:
                B.same(got[name][ks], blank[name][ks], f"free slot {s}: {name} was written")
            B.same(got["nfin"][s:s + 1], blank["nfin"][s:s + 1], f"free slot {s}: nfin was written")
            continue
        ref = launch_source(native, c, s, masked, top_k, top_p, pfx)
        for name in ("new_cand", "new_phi", "new_g", "new_len", "new_finished", "parent_draft"):
            B.same(got[name][ks], ref[name], f"slot {s} (level {c['level'][s]}, {c['nlive'][s]} parents): {name}")
        B.same(got["parent"][ks], ref["parent"] + I32(s * K), f"slot {s}: parent")
        assert got["nfin"][s] == ref["summary"][0] == int(ref["new_finished"].sum()), f"slot {s}: nfin"
        assert (ref["new_len"] == c["level"][s] + 1).all()
    if pfx_mode in ("3", "long"):
        assert (got["new_cand"][0, 1] == EOS) and got["new_finished"][0] == 1, "the fresh slot's forced EOS"


def test_step_pool_refusals(native):
    import translation_transformer_amd as t
    c = pool_case(64, 5, 9, 0)
    for change in (dict(level=np.array([1, 2, LD, 5], I32)), dict(level=np.array([0, 2, 9, 5], I32)), dict(nlive=np.array([1, 6, 5, 5], I32)),
                   dict(nlive=np.array([0, 5, 5, 5], I32))):
        with pytest.raises(t.TtxError) as e:
            launch_pool(native, {**c, **change}, False, 0, 1.0, None)
        assert e.value.code == -1, change
    for kw in (dict(masked=False, top_k=8, top_p=1.0), dict(masked=True, top_k=33, top_p=1.0), dict(masked=True, top_k=0, top_p=0.0)):
        with pytest.raises(t.TtxError) as e:
            launch_pool(native, c, kw["masked"], kw["top_k"], kw["top_p"], None)
        assert e.value.code == -1, kw


# -- bookkeeping kernels ----------------------------------------------------------------------------------------------------------------
BK = dict(C_=3, K=3, max_len=6, ld=8, Ls_cap=6, pad=PAD, bos=1)
KV_ROW, N_SRC = 8, 5
SLOT_ARRAYS = ["row_of", "level", "nlive", "nfin", "key", "pfx_len", "pfx_src", "run_acc"]
CAND_ARRAYS = ["cand_next", "len_next", "fin_next", "phi_next", "parent", "parent_draft", "cand_src_len", "g_in", "g_out"]
CALL_ARRAYS = ["out", "out_logp", "out_gumbel"]


class Device:
    """The pool's arrays on the device, and a NumPy image of what they must hold."""

    def __init__(self, native, keys, src_len, pfx_len_src):
        C_, K, L, ld, Ls = BK["C_"], BK["K"], BK["max_len"], BK["ld"], BK["Ls_cap"]
        n = C_ * K
        self.native = native
        a = dict(row_of=B.sent(C_, I32), level=B.sent(C_, I32), nlive=B.sent(C_, I32), nfin=B.sent(C_, I32), key=B.sent(C_, I64),
                 pfx_len=B.sent(C_, I32), pfx_src=B.sent(C_, I32), run_acc=B.sent(C_, I32), src_running=B.sent(N_SRC, I32), cand_next=B.sent((n, ld), I64), len_next=B.sent(n, I32),
                 fin_next=B.sent(n, U8), phi_next=B.sent(n, F32), parent=B.sent(n, I32), parent_draft=B.sent(n, I32),
                 cand_src_len=B.sent(n, I32), g_in=B.sent(n, F32), g_out=B.sent(n, F32), len_all=src_len.astype(I32),
                 row_keys=keys.astype(I64), pfx_len_src=pfx_len_src.astype(I32), out=B.sent((N_SRC, K, L), I64),
                 out_logp=B.sent((N_SRC, K), F32), out_gumbel=B.sent((N_SRC, K), F32), dev_summary=B.sent(4, I32), src_of=B.sent(n, I32),
                 new_slot=B.sent(C_, I32), valid_new=np.zeros((C_, Ls), U8), src_valid=B.sent((C_, Ls), U8),
                 memkv=B.sent((C_, Ls, KV_ROW), F32), memkv_new=np.zeros((C_, Ls, KV_ROW), F32))
        self.a = a
        self.bufs = B.upload(a, DEV)
        self.words = [5, 0, 0, 0, 0, 0, 9, 0, 4, 3, 2, 1]               # junk counters and pinned words for init to clear
        self.flip = False                                                # g_in / g_out swapped (odd iterations)

    def launch(self, op, **kw):
        bufs = dict(self.bufs)
        if self.flip:
            bufs["g_in"], bufs["g_out"] = bufs["g_out"], bufs["g_in"]
        self.words = self.native.debug_sbs_pool(op, self.words, **BK, **kw, **{k: B.dev(bufs[k]) for k in bufs})
        torch.cuda.synchronize()
        B.check_margins(self.bufs)

    def get(self, name):
        x = self.bufs[name].get()
        return x.view(F32) if self.bufs[name].dtype == torch.float32 else x

    def put(self, name, value):
        self.bufs[name].set(value)

    def compare(self, want: dict, what: str):
        for name, v in want.items():
            B.same(self.get(name), np.ascontiguousarray(v), f"{what}: {name}")


def image(pool: P.Pool, dev: Device) -> dict:
    """What the restatement says the device arrays hold (g by the buffer names of the device, whatever the parity)."""
    w = dict(row_of=pool.row_of, level=pool.level, nlive=pool.nlive, nfin=pool.nfin, key=pool.key, run_acc=pool.run_acc, cand_next=pool.cand_next,
             len_next=pool.len_next, fin_next=pool.fin_next, phi_next=pool.phi_next, parent=pool.parent, parent_draft=pool.parent_draft,
             cand_src_len=pool.cand_src_len, g_in=pool.g[0], g_out=pool.g[1])
    return w


def test_bookkeeping_kernels_follow_the_restatement(native):
    C_, K, L, Ls = BK["C_"], BK["K"], BK["max_len"], BK["Ls_cap"]
    rng = np.random.default_rng(5)
    keys = np.array([5, 1 << 40, -3, 0, (1 << 33) + 1], I64)
    src_len = np.array([6, 5, 4, 3, 2], I32)
    pfx_len_src = np.array([0, 2, 0, 4, 1], I32)

    def model_of(i):
        def model(rows):
            out = np.empty((len(rows), 6), F32)
            for j, r in enumerate(rows):
                x = np.random.default_rng(hash((i,) + tuple(int(t) for t in r)) % 2 ** 32).uniform(-1, 1, 6).astype(F32)
                x[PAD] = -np.inf
                x[EOS] += F32(3.0 if i == 1 else -1.0)                   # source 1 finishes early: its slot is reused
                out[j] = x
            return out
        return model
    pool = P.Pool([model_of(i) for i in range(N_SRC)], keys, C_, K, L, 11, 1.0, PAD, BK["bos"], EOS, dtype=F32, src_len=src_len)
    dev = Device(native, keys, src_len, pfx_len_src)
    pfx_len, pfx_src = np.zeros(C_, I32), np.zeros(C_, I32)
    src_valid, memkv = dev.a["src_valid"].copy(), dev.a["memkv"].copy()
    out, out_logp, out_gumbel = dev.a["out"].copy(), dev.a["out_logp"].copy(), dev.a["out_gumbel"].copy()
    src_running = dev.a["src_running"].copy()

    # init: every slot free, every candidate finished, counters and pinned words zero
    dev.launch("init")
    assert dev.words == [0] * 12
    dev.compare({**image(pool, dev), "pfx_len": pfx_len, "pfx_src": pfx_src, "src_of": np.arange(C_ * K, dtype=I32) // K,
                 "dev_summary": np.zeros(4, I32)}, "init")

    def admit(first_row, R, what):
        Ls_new = int(src_len[first_row:first_row + R].max())
        valid_new = (np.arange(Ls_new)[None, :] < src_len[first_row:first_row + R, None]).astype(U8)
        kv_new = rng.standard_normal((R, Ls_new, KV_ROW)).astype(F32)
        stage_v, stage_kv = np.zeros((C_, Ls), U8), np.zeros((C_, Ls, KV_ROW), F32)
        stage_v.reshape(-1)[:R * Ls_new] = valid_new.reshape(-1)
        stage_kv.reshape(-1)[:R * Ls_new * KV_ROW] = kv_new.reshape(-1)
        dev.put("valid_new", stage_v)
        dev.put("memkv_new", stage_kv)
        dev.flip = bool(pool.iteration & 1)                              # g_in: the buffer the next iteration reads
        slots = pool.admit(first_row, R)
        dev.launch("admit", R=R, first_row=first_row)
        B.same(dev.get("new_slot")[:R], slots, f"{what}: new_slot")
        B.same(dev.get("row_of"), pool.row_of, f"{what}: row_of after admit")
        dev.launch("fill", R=R, first_row=first_row, Ls_new=Ls_new, kv_row=KV_ROW)
        for i, s in enumerate(slots):
            pfx_len[s], pfx_src[s] = pfx_len_src[first_row + i], first_row + i
            src_valid[s] = 0
            src_valid[s, :Ls_new] = valid_new[i]
            memkv[s, :Ls_new] = kv_new[i]
        assert not P.check_admission(pool, first_row, slots)
        dev.flip = False
        dev.compare({**image(pool, dev), "pfx_len": pfx_len, "pfx_src": pfx_src, "src_valid": src_valid, "memkv": memkv, "out": out,
                     "out_logp": out_logp, "out_gumbel": out_gumbel, "src_running": src_running}, what)
        return slots

    def iterate(what):
        """The restatement's step uploaded, then retire and publish on the device."""
        pool.step()
        for name, v in image(pool, dev).items():
            dev.put(name, v)
        dev.words[0] = pool.iteration                                    # BeamCounters.model_calls, as k_bs_list counts it
        before = pool.row_of.copy()
        pool.retire()
        pool.publish()
        dev.flip = bool((pool.iteration - 1) & 1)                        # g_out: the buffer this iteration's step wrote
        dev.launch("retire")
        dev.launch("publish")
        dev.flip = False
        for s in np.nonzero((before >= 0) & (pool.row_of < 0))[0]:
            r = before[s]
            out[r], out_logp[r], out_gumbel[r] = pool.out[r], pool.out_logp[r], pool.out_gumbel[r]
            src_running[r] = pool.src_running[r]
        dev.compare({**image(pool, dev), "out": out, "out_logp": out_logp, "out_gumbel": out_gumbel, "src_running": src_running, "pfx_len": pfx_len, "pfx_src": pfx_src,
                     "src_valid": src_valid, "memkv": memkv}, what)
        assert dev.words[8:] == [pool.host["steps_done"], pool.host["n_live"], pool.host["n_running"], 0], what
        return np.nonzero((before >= 0) & (pool.row_of < 0))[0]

    admit(0, 3, "first admission")
    cursor, reused = 3, False
    for it in range(40):
        freed = iterate(f"iteration {it + 1}")
        take = min(int((pool.row_of < 0).sum()), N_SRC - cursor)
        if take > 0:
            slots = admit(cursor, take, f"admission after iteration {it + 1}")        # retired and re-admitted in consecutive launches
            reused |= bool(set(slots.tolist()) & set(freed.tolist())) and (pool.row_of >= 0).sum() > take
            cursor += take
        if not (pool.row_of >= 0).any():
            break
    assert cursor == N_SRC and not (pool.row_of >= 0).any(), "the walk did not drain the list"
    assert reused, "no slot was reused beside a running source: the case shows nothing"
    assert (out != dev.a["out"]).all() and not (pool.out == -7).any()
    assert src_running.sum() == pool.running_rows and (src_running >= 1).all(), "the per-source counts sum to the pool's running rows"

    # more sources than free slots: slot -1 for the rest, the error word set, and fill skips them
    dev.launch("init")
    dev.launch("admit", R=3, first_row=0)
    dev.launch("admit", R=2, first_row=3)
    assert dev.words[11] == 1 and (dev.get("new_slot")[:2] == -1).all()
    before = {k: dev.get(k).copy() for k in ("cand_next", "level", "memkv", "src_valid")}
    dev.launch("fill", R=2, first_row=3, Ls_new=2, kv_row=KV_ROW)
    dev.compare(before, "fill of sources without a slot")


def test_bookkeeping_refusals(native):
    import translation_transformer_amd as t
    dev = Device(native, np.zeros(N_SRC, I64), np.full(N_SRC, 2, I32), np.zeros(N_SRC, I32))
    for op, kw in (("admit", dict(R=0)), ("admit", dict(R=4)), ("fill", dict(R=1, Ls_new=7, kv_row=8)), ("fill", dict(R=1, Ls_new=2, kv_row=6)),
                   ("fill", dict(R=1, Ls_new=0, kv_row=8)), (7, dict())):
        with pytest.raises(t.TtxError) as e:
            dev.launch(op, **kw)
        assert e.value.code == -1, (op, kw)
