"""util_attn_checks with the head dimension as a parameter (tests/test_gpu_attn_hd64.py, tests/test_attn_hd_checks_host.py).

util_attn_checks fixes DH = 32 in a module global that the existing attention tests share within one process, so nothing here
changes it.  What does not depend on the head dimension is imported from it: the mode and kernel ids, the step visibility
rules, the token patterns, the per-group key views, the operand layout, check_bits and the structure check.  What does is
restated with ``dh`` as an argument: the case (d = dh * H), the float64 / fp32 rule, the score distributions, the case
builders and the value check.  The tolerance is util_attn_checks' derived one, unchanged:
    tol = 4 e32 + (ln nk + 2) 2^-23 max |V over visible keys|
(neither term knows the head dimension: e32 is measured on the case itself, the second term bounds __expf's error per
normalised sum).

One score distribution is added to the five of util_attn_checks: ``upper``, in which q and k are zero in dims 0 .. 31 of every
head, so that only dims 32 .. dh - 1 decide the scores (a contraction that stops after 32 dims sees uniform scores).

``standin`` evaluates a case in fp32 on the CPU the way a kernel would, optionally with ONE defect of the kind a head-dimension
port can have; the host test shows that the checks reject each of them.
"""
from __future__ import annotations

import math

import torch

import util_attn_checks as A
import util_gemm_checks as G
from util_attn_checks import (ENC, FULL_SELF, FULL_CROSS, STEP_SELF, STEP_CROSS, MODE_NAMES, K_PROD, K_ATTN, K_ATTN2, K_ATTN3,   # noqa: F401
                              K_ATTN3S, KERNEL_NAMES, PAD, LOUD, check_bits, check_structure, step_visibility_direct,
                              step_visibility_expanded)

DISTS = A.DISTS + ["upper"]
DEFECTS = ["first_32_dims", "upper_half_unwritten", "upper_half_copied", "head_offset_32", "next_head_v"]


def scale_of(dh: int) -> float:
    return 1.0 / math.sqrt(dh)


class Case(A.Case):
    """A.Case at head dimension ``dh``: d = dh * H."""

    def __init__(self, dh, **kw):
        super().__init__(**kw)
        self.dh = dh
        self.d = dh * self.H


def _kw(case: Case) -> dict:
    return {k: v for k, v in case.__dict__.items() if k not in ("_ref", "d")}


# ---- arithmetic ---------------------------------------------------------------------------------------------------------
def attend(q, k, v, vis, H, dh, defect=None):
    """A.attend at head dimension dh.  ``defect`` (host test only) breaks it in one way, see DEFECTS."""
    nq, nk = vis.shape
    heads = lambda t: t.reshape(-1, H, dh).transpose(0, 1)
    if defect == "head_offset_32":                               # head h taken from columns 32 h .. 32 h + dh - 1
        take = lambda t: torch.stack([t[:, 32 * h:32 * h + dh] for h in range(H)])
        qh, kh, vh = take(q), take(k), take(v)
    else:
        qh, kh, vh = heads(q), heads(k), heads(v)
    if defect == "next_head_v":
        vh = vh.roll(-1, 0)
    if defect == "first_32_dims":
        qh, kh = qh[..., :32], kh[..., :32]
    s = (qh @ kh.transpose(-1, -2)) * scale_of(dh)
    s = s.masked_fill(~vis[None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m)
    den = p.sum(-1, keepdim=True)
    o = (p @ vh) / torch.where(den > 0, den, torch.ones_like(den))
    if defect == "upper_half_copied":
        o = torch.cat([o[..., :dh // 2], o[..., :dh // 2]], -1)
    return o.transpose(0, 1).reshape(nq, H * dh)


def evaluate(case: Case, dtype, step_direct: bool = False, defect=None):
    """A.evaluate at the case's head dimension."""
    out = torch.zeros(case.out_rows, case.d, dtype=dtype)
    nk_max, vmax = 1, 0.0
    for row0, scatter, q, k, v, vis in A._group_views(case, dtype, step_direct):
        o = attend(q, k, v, vis, case.H, case.dh, defect)
        if scatter is None:
            out[row0:row0 + o.shape[0]] = o
        else:
            rows, skip = scatter
            out[rows] = o[skip:]
        nk_max = max(nk_max, int(vis.sum(-1).max()))
        seen = vis.any(0)
        if bool(seen.any()):
            vmax = max(vmax, float(v[seen].abs().max()))
    return out, nk_max, vmax


def reference(case: Case) -> dict:
    """ref (float64), t32 (stock fp32), e32, tol of a case: computed once, shared by every test that runs the case."""
    if case._ref is None:
        ref, nk, vmax = evaluate(case, torch.float64)
        t32, _, _ = evaluate(case, torch.float32)
        assert not torch.isnan(ref).any() and not torch.isnan(t32).any(), f"{case}: the reference reads a never-read region"
        e32 = float((t32.to(torch.float64) - ref).abs().max()) if ref.numel() else 0.0
        tol = 4.0 * e32 + (math.log(nk) + 2.0) * 2.0 ** -23 * vmax          # util_attn_checks.reference, unchanged
        case._ref = dict(ref=ref, t32=t32, e32=e32, tol=tol, nk=nk, vmax=vmax)
    return case._ref


def standin(case: Case, defect=None) -> G.Arena:
    """The case evaluated in fp32 on the CPU into a guarded output the way a launch would leave it (step modes by the direct
    rule over [prefix | all step rows]); ``defect``: one of DEFECTS or None."""
    out = G.Arena(case.out_rows, case.d, fill=G.OUT_FILL)
    res, _, _ = evaluate(case, torch.float32, step_direct=True, defect=None if defect == "upper_half_unwritten" else defect)
    n = case.live_rows
    if defect == "upper_half_unwritten":
        cols = (torch.arange(case.d) % case.dh) < case.dh // 2
        out.m[:n, cols] = res[:n, cols]
    else:
        out.m[:n] = res[:n]
    return out


# ---- operands -----------------------------------------------------------------------------------------------------------
def _shape_scores(q, k, pos, n_pos, dist, H, dh):
    """A._shape_scores at head dimension dh, plus ``upper``."""
    if dist == "peaked":
        q *= 8.0
        return
    if dist in ("ordinary", "upper"):                            # upper: see _upper_only, applied to the finished operands
        return
    u = torch.full((H * dh,), 1.0 / math.sqrt(dh))               # unit vector per head
    if dist == "offset":                                          # scale * a^2 = 100: every score sits near +100
        a = math.sqrt(100.0 / scale_of(dh))
        q += a * u
        k += a * u
    else:                                                         # scale * 4 * pos / 8: +-2.8 per 32-key tile at dh = 32, +-2 at 64
        amp = (pos if dist == "ascending" else (n_pos - pos)).to(torch.float32) / 8.0
        if q is not None:
            q += 4.0 * u
        k += amp[:, None] * u


def _upper_only(dh, *tensors):
    """Zeroes dims 0 .. 31 of every head in place where a value is there to be read (never-read NaN stays NaN)."""
    for t in tensors:
        if t is None:
            continue
        cols = (torch.arange(t.shape[-1]) % dh) < 32
        low = t[..., cols]
        t[..., cols] = torch.where(torch.isnan(low), low, torch.zeros_like(low))


def full_case(dh, mode, L, Lk=0, groups=1, H=2, dist="ordinary", seed=0, shared_mem=False, patterns=None, name=None) -> Case:
    """A.full_case at head dimension dh."""
    gen = torch.Generator().manual_seed(1000 + seed)
    d = H * dh
    default = {1: ["mid"], 3: ["tail", "none", "mid"]}.get(groups, ["mid"] * groups)
    q = torch.randn(groups * L, d, generator=gen)
    c = dict(mode=mode, H=H, groups=groups, L=L, Lk=Lk, dist=dist)
    if mode == FULL_CROSS:
        rm = 3 if shared_mem else groups                        # shared: rows 1, 0, 1 are used, row 2 is never read
        pats = patterns or (["tail", "mid", "full"] if shared_mem else default)
        real = torch.stack([A._pattern(pats[r], Lk, gen) for r in range(rm)])
        n_key_rows, key_real = rm * Lk, real.reshape(-1)
        pos = torch.arange(Lk).repeat(rm)
        c.update(key_pad=(~real).to(torch.uint8), mem_row=torch.tensor([1, 0, 1][:groups], dtype=torch.int32) if shared_mem else None,
                 max_keys=Lk)
    else:
        pats = patterns or default
        real = torch.stack([A._pattern(pats[g], L, gen) for g in range(groups)])
        n_key_rows, key_real = groups * L, real.reshape(-1)
        pos = torch.arange(L).repeat(groups)
        c.update(tok=A._tokens(real, gen), max_keys=L)
    k = torch.randn(n_key_rows, d, generator=gen)
    v = torch.randn(n_key_rows, d, generator=gen)
    _shape_scores(q, k, pos, Lk if mode == FULL_CROSS else L, dist, H, dh)
    k[~key_real] = A._loud(gen, int((~key_real).sum()), d)
    v[~key_real] = A._loud(gen, int((~key_real).sum()), d)
    if mode == FULL_CROSS and shared_mem:
        k[2 * Lk:], v[2 * Lk:] = float("nan"), float("nan")
    if dist == "upper":
        _upper_only(dh, q, k)
    nm = name or (f"dh{dh}-{MODE_NAMES[mode]}-L{L}" + (f"-Lk{Lk}" if mode == FULL_CROSS else "") + f"-g{groups}-H{H}-{dist}"
                  + ("-shared" if shared_mem else ""))
    return Case(dh, q=q, k=k, v=v, name=nm, **c)


def step_case(dh, mode, N, D, slots, H=2, dist="ordinary", seed=0, extra_groups=0, n_active=None, cache_slot=False, src_of=False,
              src_len=False, name=None, cache_len=None) -> Case:
    """A.step_case at head dimension dh.  ``cache_len``: capacity of the cache (max_keys of the launch) when it is to exceed the
    largest front + 3."""
    gen = torch.Generator().manual_seed(2000 + seed)
    d, rps = H * dh, 1 + N * D
    n_act = len(slots) if n_active is None else n_active
    groups = len(slots) + extra_groups
    B = groups + 2
    act_idx = ((torch.arange(groups) * 1 + 2) % B).flip(0).to(torch.int32)          # slot -> sequence, a permutation, never the identity
    max_f = max([s["f"] for s in slots[:max(n_act, 1)]] + [0])
    Lc = max(max_f + 3, cache_len or 0)
    Lk = max([s["src"] for s in slots] + [1])
    q = torch.full((groups * rps, d), float("nan"))
    k, v = q.clone(), q.clone()
    front = torch.zeros(B, dtype=torch.int32)
    c = dict(mode=mode, H=H, groups=groups, n_active=n_act, N=N, D=D, dist=dist, act_idx=act_idx, front=front, specs=slots)
    if mode == STEP_SELF:
        gen_ld = Lc + D + 2
        n_cache = B + (1 if cache_slot else 0)
        cslot = ((torch.arange(B) * 1 + 3) % n_cache).to(torch.int32) if cache_slot else None
        # never-read token columns: PAD and real ids alternate, so that a read one column off the front changes the mask
        tok = (torch.arange(gen_ld)[None, :] + torch.arange(B)[:, None]) % 2 * 7
        tok = tok.to(torch.int32)
        kc = torch.full((n_cache, Lc, d), float("nan"))
        vc = kc.clone()
    else:
        perm = ((torch.arange(B) + 1) % B).to(torch.int32) if src_of else None
        key_pad = torch.full((B, Lk), 1, dtype=torch.uint8)                         # behind a source's end: "real", never to be read
        mk = torch.full((B * Lk, d), float("nan"))
        mv = mk.clone()
        slen = torch.full((B,), 1, dtype=torch.int32)
    for g, s in enumerate(slots):
        if g >= n_act:
            break
        b = int(act_idx[g])
        rows = slice(g * rps, (g + 1) * rps)
        q[rows] = torch.randn(rps, d, generator=gen)
        if mode == STEP_SELF:
            f = s["f"]
            front[b] = f
            real = A._pattern("mid" if s.get("prefix_pads") else "full", f, gen)
            tok[b, :f] = A._tokens(real, gen)
            tok[b, f] = PAD if s.get("front_pad") else 5
            tok[b, f + 1:f + 1 + D] = (torch.arange(D) + (1 if s.get("front_pad") else 0)) % 2 * 9   # column f + 1: real iff the front is PAD
            cb = int(cslot[b]) if cslot is not None else b
            kk, vv = torch.randn(f + rps, d, generator=gen), torch.randn(f + rps, d, generator=gen)
            pos = torch.cat([torch.arange(f + 1), f + 1 + torch.arange(N * D) % max(D, 1)])
            _shape_scores(q[rows], kk, pos, f + 1 + D, dist, H, dh)
            masked = torch.cat([~real, torch.tensor([bool(s.get("front_pad"))]), torch.zeros(N * D, dtype=torch.bool)])
            kk[masked] = A._loud(gen, int(masked.sum()), d)
            vv[masked] = A._loud(gen, int(masked.sum()), d)
            kc[cb, :f], vc[cb, :f] = kk[:f], vv[:f]
            k[rows], v[rows] = kk[f:], vv[f:]
        else:
            src = int(perm[b]) if perm is not None else b
            n = s["src"]
            slen[b] = n
            real = A._pattern("mid" if s.get("prefix_pads") else "full", n, gen)
            kk, vv = torch.randn(n, d, generator=gen), torch.randn(n, d, generator=gen)
            _shape_scores(q[rows], kk, torch.arange(n), n, dist, H, dh)
            kk[~real] = A._loud(gen, int((~real).sum()), d)
            vv[~real] = A._loud(gen, int((~real).sum()), d)
            mk[src * Lk:src * Lk + n], mv[src * Lk:src * Lk + n] = kk, vv
            key_pad[src, :n] = real.to(torch.uint8)
            if not src_len:                       # every key of the row is read: the tail is masked and loud
                key_pad[src, n:] = 0
                mk[src * Lk + n:(src + 1) * Lk] = A._loud(gen, Lk - n, d)
                mv[src * Lk + n:(src + 1) * Lk] = A._loud(gen, Lk - n, d)
    if mode == STEP_SELF:
        if dist == "upper":
            _upper_only(dh, q, k, kc)
        c.update(tok=tok, gen_ld=gen_ld, kcache=kc, vcache=vc, cache_slot=cslot, Lc=Lc, max_keys=Lc)
    else:
        if dist == "upper":
            _upper_only(dh, q, mk)
        c.update(key_pad=key_pad, Lk=Lk, src_of=perm, src_len=slen if src_len else None, max_keys=Lk)
        k, v = mk, mv
    nm = name or (f"dh{dh}-{MODE_NAMES[mode]}-N{N}-D{D}-g{groups}-a{n_act}-H{H}-{dist}" + ("-cslot" if cache_slot and mode == STEP_SELF else "")
                  + ("-srcof" if src_of and mode == STEP_CROSS else "") + ("-srclen" if src_len and mode == STEP_CROSS else ""))
    return Case(dh, q=q, k=k, v=v, name=nm, **c)


def subcase(case: Case, order) -> Case:
    """A.subcase: the slots ``order`` of a step case as a launch of their own."""
    rps = case.rps
    rows = torch.cat([torch.arange(g * rps, (g + 1) * rps) for g in order])
    kw = _kw(case)
    kw.update(groups=len(order), n_active=len(order), act_idx=case.act_idx[list(order)].clone(), q=case.q[rows].clone(),
              name=f"{case.name}[slots {list(order)}]")
    if case.mode == STEP_SELF:
        kw.update(k=case.k[rows].clone(), v=case.v[rows].clone())
    return Case(**kw)


def repad(case: Case, L2: int) -> Case:
    """A.repad: the same real tokens padded further (new key rows PAD and LOUD, new query rows random)."""
    gen = torch.Generator().manual_seed(77)
    d = case.d
    kw = _kw(case)
    cross = case.mode == FULL_CROSS
    L1 = case.Lk if cross else case.L
    assert not case.step and L2 >= L1

    def grow(t, n_rows, fresh):
        out = fresh(n_rows * L2, d).reshape(n_rows, L2, d)
        out[:, :L1] = t.reshape(n_rows, L1, d)
        return out.reshape(-1, d)

    loud = lambda r, c_: A._loud(gen, r, c_)
    if cross:
        rm = case.key_pad.shape[0]
        kp = torch.ones(rm, L2, dtype=torch.uint8)
        kp[:, :L1] = case.key_pad
        kw.update(Lk=L2, key_pad=kp, k=grow(case.k, rm, loud), v=grow(case.v, rm, loud), max_keys=L2)
    else:
        tok = torch.full((case.groups, L2), PAD, dtype=torch.int32)
        tok[:, :L1] = case.tok
        kw.update(L=L2, tok=tok, q=grow(case.q, case.groups, lambda r, c_: torch.randn(r, c_, generator=gen)),
                  k=grow(case.k, case.groups, loud), v=grow(case.v, case.groups, loud), max_keys=L2)
    kw["name"] = f"{case.name}-padded-to-{L2}"
    return Case(**kw)


class Operands(A.Operands):
    """A.Operands (guarded allocations; self modes a packed QKV buffer with ldq = ldkv = 3d, cross modes K / V interleaved in a
    [rows, 4d] buffer) with the case's head dimension and scale among the keyword arguments of debug_attn."""

    def __init__(self, case: Case, device="cpu"):
        super().__init__(case, device)
        self.kw.update(scale=scale_of(case.dh), head_dim=case.dh)


# ---- checkers -----------------------------------------------------------------------------------------------------------
def _where(case: Case, row: int, col: int) -> str:
    g, qi = divmod(row, case.q_per_group)
    return f"group {g} head {col // case.dh} query {qi} dim {col % case.dh}"


def check_values(got: torch.Tensor, case: Case, what: str) -> float:
    """max |got - float64| over the live rows within the case's tolerance (a NaN fails).  Returns the error."""
    r = reference(case)
    n = case.live_rows
    err = (got[:n].cpu().to(torch.float64) - r["ref"][:n]).abs()
    ok = err <= r["tol"]
    if not bool(ok.all()):
        row, col = (int(i) for i in torch.nonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {err.numel()} values outside the tolerance {r['tol']:.3e} (e32 {r['e32']:.3e}); "
                             f"first at {_where(case, row, col)}: got {got[row, col].item()!r} expected {r['ref'][row, col].item()!r}")
    return float(err.max()) if err.numel() else 0.0


def staged_keys(case: Case) -> int:
    """Keys one k_attn2 workgroup stages for the case, as the launcher counts them from max_keys."""
    if case.mode != STEP_SELF:
        return case.max_keys
    draft = min(case.N, (64 + case.D - 2) // case.D + 1) * case.D if case.D > 0 else 0
    return case.max_keys + 1 + draft


def kernels_for(case: Case, key_limit: int):
    """The kernels that can serve a case at head dimension 64 (k_attn3 / k_attn3s never; k_attn2 up to ``key_limit`` staged keys)."""
    return [K_ATTN] + ([K_ATTN2] if staged_keys(case) <= key_limit else [])
