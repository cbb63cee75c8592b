"""Reference, tolerance, case builders and checkers of the kernel-level attention tests (tests/test_gpu_attn_kernels.py), kept
free of any GPU call so that tests/test_attn_checks_host.py can show on the CPU that each checker fails when it should.

A ``Case`` holds the logical operands of ONE attention launch on the CPU (ttx_debug_attn's arguments) and ``Operands`` places
them in guarded allocations (util_gemm_checks.Arena) on a device.  Three kinds of memory surround the live data:

  never read      NaN: cache positions >= front, memory rows >= src_len, Q/K/V rows of slots >= n_active, the second layer's
                  columns of the interleaved cross K/V buffer, guard bands; token columns past the front hold a pattern of PAD and
                  real ids that changes the result when it is read in place of the front token
  read, masked    finite values of magnitude 1e4 (``LOUD``): PAD keys, the masked front row, source positions behind a source's
                  end when no src_len is given.  Finite, because a masked key's V enters 0 * V in every kernel
  everything else seeded random, q / k / v about N(0, 1), shaped by the case's score distribution

The reference ``attn_ref64`` is the documented rule in float64, per head softmax(scale q k^T + mask) v, a query without a
visible key giving exactly 0.  The step modes expand every draft into its own dense sequence [prefix | front | draft rows] and
run plain causal attention on it (the reference model's shape); ``step_visibility_direct`` states the same rule as one matrix
over [prefix | all step rows] and is what the CPU stand-in kernel of the host test evaluates.

Tolerance, derived and not tuned: with e32 = max |attn_torch32 - attn_ref64| (the same formula, stock fp32 torch ops),
    tol = 4 e32 + (ln nk + 2) 2^-23 max |V over visible keys|.
The factor 4 is finish_tolerance's allowance for a different reduction tree.  The second term is what stock torch does not
share: __expf rounds x log2(e) before the hardware exponential, a relative error of about (|x| + 2) 2^-24 per probability;
weighted by the probabilities (sum p |x| <= ln nk for x = score - max) that is (ln nk + 2) 2^-24 per normalised sum, doubled for
numerator and denominator.  nk = the largest number of keys any query of the case sees.
"""
from __future__ import annotations

import math

import torch

import util_gemm_checks as G

ENC, FULL_SELF, FULL_CROSS, STEP_SELF, STEP_CROSS = range(5)
MODE_NAMES = ["ENC", "FULL_SELF", "FULL_CROSS", "STEP_SELF", "STEP_CROSS"]
K_PROD, K_ATTN, K_ATTN2, K_ATTN3, K_ATTN3S = range(5)
KERNEL_NAMES = ["production", "k_attn", "k_attn2", "k_attn3", "k_attn3s"]
DH = 32
SCALE = 1.0 / math.sqrt(DH)
PAD = 0
LOUD = 1.0e4
DISTS = ["ordinary", "peaked", "offset", "ascending", "descending"]

# the grids of the GPU module (the host test walks the step grid too)
SELF_LS = [1, 16, 17, 31, 32, 33, 64, 65, 130]
CROSS_LKS = [1, 31, 32, 33, 255, 256, 257, 290, 384, 385]
F_VALUES = [0, 1, 30, 31, 32, 33, 63, 64, 65, 200]
SRC_LENS = [1, 31, 32, 33, 64, 70]
STEP_ND = [(1, 0), (1, 1), (3, 10), (2, 16), (7, 10), (5, 13), (64, 1), (4, 3)]


class Case:
    """Logical operands of one launch (CPU tensors).  Rows of q / k / v: [rows, d]; see the builders below."""

    def __init__(self, **kw):
        self.tok = self.key_pad = self.mem_row = self.act_idx = self.front = self.src_of = self.src_len = None
        self.kcache = self.vcache = self.cache_slot = None
        self.L = self.Lk = self.gen_ld = self.D = self.n_active = self.Lc = 0
        self.N = 1
        self.__dict__.update(kw)
        self.d = DH * self.H
        self._ref = None

    @property
    def step(self):
        return self.mode in (STEP_SELF, STEP_CROSS)

    @property
    def rps(self):
        return 1 + self.N * self.D

    @property
    def q_per_group(self):
        return self.rps if self.step else self.L

    @property
    def live_rows(self):
        return (self.n_active if self.step else self.groups) * self.q_per_group

    @property
    def out_rows(self):
        return self.groups * self.q_per_group

    def __repr__(self):
        return self.name


# ---- arithmetic ---------------------------------------------------------------------------------------------------------
def attend(q, k, v, vis, H):
    """softmax(scale q k^T + mask) v per head in the dtype of q, from stock torch ops.  q [nq, d], k / v [nk, d], vis [nq, nk]
    bool.  A query that sees nothing gives exactly 0."""
    nq, nk = vis.shape
    qh, kh, vh = (t.reshape(-1, H, DH).transpose(0, 1) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * SCALE
    s = s.masked_fill(~vis[None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m)
    den = p.sum(-1, keepdim=True)
    o = (p @ vh) / torch.where(den > 0, den, torch.ones_like(den))
    return o.transpose(0, 1).reshape(nq, H * DH)


def step_visibility_direct(N, D, f, prefix_real, front_real):
    """[RPS, f + RPS] bool over the keys [cached prefix | step rows]: the rule as the issue of the tests states it."""
    rps = 1 + N * D
    vis = torch.zeros(rps, f + rps, dtype=torch.bool)
    vis[:, :f] = prefix_real[None, :f]
    vis[:, f] = front_real
    for n in range(N):
        for j in range(1, D + 1):              # key row of token j of draft n
            for j2 in range(j, D + 1):         # seen by the later tokens of the same draft
                vis[1 + n * D + (j2 - 1), f + 1 + n * D + (j - 1)] = True
    return vis


def step_visibility_expanded(N, D, f, prefix_real, front_real):
    """The same matrix read off the dense sequences: draft n is the sequence [prefix | front | its D rows] under the causal rule
    with PAD keys masked; a step row sees exactly the keys of its own sequence at positions up to its own."""
    rps = 1 + N * D
    vis = torch.zeros(rps, f + rps, dtype=torch.bool)
    for n in range(max(N, 1)):
        key_of_pos = list(range(f + 1)) + [f + 1 + n * D + j for j in range(D)]        # position -> column of the direct layout
        real = torch.cat([prefix_real[:f], torch.tensor([bool(front_real)]), torch.ones(D, dtype=torch.bool)])
        row_of_pos = {f: 0, **{f + 1 + j: 1 + n * D + j for j in range(D)}}
        for pos, row in row_of_pos.items():
            for p2 in range(pos + 1):
                if real[p2]:
                    vis[row, key_of_pos[p2]] = True
    return vis


def _group_views(case: Case, dtype, step_direct: bool):
    """Yields (first output row, q, k, v, vis) per live group / slot / draft with the keys a kernel may read for it."""
    c, d = case, case.d
    cast = lambda t: t.to(dtype)
    if not c.step:
        for g in range(c.groups):
            rows = slice(g * c.L, (g + 1) * c.L)
            if c.mode == FULL_CROSS:
                mr = int(c.mem_row[g]) if c.mem_row is not None else g
                kr = slice(mr * c.Lk, (mr + 1) * c.Lk)
                vis = (c.key_pad[mr] == 0)[None, :].expand(c.L, c.Lk)
            else:
                kr = rows
                vis = (c.tok[g] != PAD)[None, :].expand(c.L, c.L)
                if c.mode == FULL_SELF:
                    vis = vis & torch.ones(c.L, c.L, dtype=torch.bool).tril()
            yield g * c.L, None, cast(c.q[rows]), cast(c.k[kr]), cast(c.v[kr]), vis
        return
    rps = c.rps
    for g in range(c.n_active):
        b = int(c.act_idx[g])
        rows = slice(g * rps, (g + 1) * rps)
        if c.mode == STEP_CROSS:
            s = int(c.src_of[b]) if c.src_of is not None else b
            nk = int(c.src_len[b]) if c.src_len is not None else c.Lk
            kr = slice(s * c.Lk, s * c.Lk + nk)
            vis = (c.key_pad[s, :nk] != 0)[None, :].expand(rps, nk)
            yield g * rps, None, cast(c.q[rows]), cast(c.k[kr]), cast(c.v[kr]), vis
            continue
        f = int(c.front[b])
        cb = int(c.cache_slot[b]) if c.cache_slot is not None else b
        real = c.tok[b] != PAD
        if step_direct:
            k = torch.cat([c.kcache[cb, :f], c.k[rows]])
            v = torch.cat([c.vcache[cb, :f], c.v[rows]])
            yield g * rps, None, cast(c.q[rows]), cast(k), cast(v), step_visibility_direct(c.N, c.D, f, real, bool(real[f]))
            continue
        for n in range(c.N):
            # the dense sequence of draft n: positions 0 .. f + D, queries at f .. f + D
            dr = [g * rps] + [g * rps + 1 + n * c.D + j for j in range(c.D)]
            k = torch.cat([c.kcache[cb, :f], c.k[dr]])
            v = torch.cat([c.vcache[cb, :f], c.v[dr]])
            key_real = torch.cat([real[:f + 1], torch.ones(c.D, dtype=torch.bool)])
            causal = torch.ones(f + 1 + c.D, f + 1 + c.D, dtype=torch.bool).tril()[f:]
            take = dr if n == 0 else dr[1:]                  # row 0 is the same in every draft: stored once
            yield None, (take, 0 if n == 0 else 1), cast(c.q[dr]), cast(k), cast(v), causal & key_real[None, :]


def evaluate(case: Case, dtype, step_direct: bool = False):
    """(out [out_rows, d] in ``dtype`` with rows of inactive slots 0, largest visible key count, max |V| over visible keys)."""
    out = torch.zeros(case.out_rows, case.d, dtype=dtype)
    nk_max, vmax = 1, 0.0
    for row0, scatter, q, k, v, vis in _group_views(case, dtype, step_direct):
        o = attend(q, k, v, vis, case.H)
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


def attn_ref64(case: Case) -> torch.Tensor:
    return reference(case)["ref"]


def attn_torch32(case: Case) -> torch.Tensor:
    return reference(case)["t32"]


def reference(case: Case) -> dict:
    """ref (float64), t32 (stock fp32), e32, tol of a case: computed once, shared by every test that runs the case."""
    if case._ref is None:
        ref, nk, vmax = evaluate(case, torch.float64)
        t32, _, _ = evaluate(case, torch.float32)
        assert not torch.isnan(ref).any() and not torch.isnan(t32).any(), f"{case}: the reference reads a never-read region"
        e32 = float((t32.to(torch.float64) - ref).abs().max()) if ref.numel() else 0.0
        tol = 4.0 * e32 + (math.log(nk) + 2.0) * 2.0 ** -23 * vmax
        case._ref = dict(ref=ref, t32=t32, e32=e32, tol=tol, nk=nk, vmax=vmax)
    return case._ref


# ---- operands -----------------------------------------------------------------------------------------------------------
def _loud(gen, *shape):
    return LOUD * (torch.randint(0, 2, shape, generator=gen).to(torch.float32) * 2.0 - 1.0)


def _shape_scores(q, k, pos, n_pos, dist, H):
    """Applies a score distribution: q [nq, d] in place, k [nk, d] in place with ``pos`` [nk] the keys' positions among n_pos."""
    if dist == "peaked":
        q *= 8.0
        return
    if dist == "ordinary":
        return
    u = torch.full((H * DH,), 1.0 / math.sqrt(DH))             # unit vector per head
    if dist == "offset":                                        # scale * a^2 = 100: every score sits near +100
        a = math.sqrt(100.0 / SCALE)
        q += a * u
        k += a * u
    else:                                                       # scale * 4 * pos / 8: +-2.8 per 32-key tile, far above the noise
        amp = (pos if dist == "ascending" else (n_pos - pos)).to(torch.float32) / 8.0
        if q is not None:
            q += 4.0 * u
        k += amp[:, None] * u


def _pattern(kind, n, gen):
    """Real-token mask of n positions: 'full', 'none', 'tail' (ragged end), 'mid' (PADs at 0 and in the middle, last one real)."""
    real = torch.ones(n, dtype=torch.bool)
    if kind == "none":
        real[:] = False
    elif kind == "tail":
        real[max(1, (2 * n + 2) // 3):] = False
    elif kind == "mid" and n >= 4:
        real[0] = False
        real[n // 3:n // 2 + 1] = False
    return real


def _tokens(real, gen):
    t = torch.randint(1, 30, real.shape, generator=gen, dtype=torch.int32)
    return torch.where(real, t, torch.full_like(t, PAD))


def full_case(mode, L, Lk=0, groups=1, H=4, dist="ordinary", seed=0, shared_mem=False, patterns=None, name=None) -> Case:
    """ENC / FULL_SELF (keys = the group's own L rows) or FULL_CROSS (L queries, Lk keys of a memory row)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    d = H * DH
    default = {1: ["mid"], 3: ["tail", "none", "mid"]}.get(groups, ["mid"] * groups)
    q = torch.randn(groups * L, d, generator=gen)
    c = dict(mode=mode, H=H, groups=groups, L=L, Lk=Lk, dist=dist)
    if mode == FULL_CROSS:
        rm = 3 if shared_mem else groups                        # shared: rows 1, 0, 1 are used, row 2 is never read
        pats = patterns or (["tail", "mid", "full"] if shared_mem else default)
        real = torch.stack([_pattern(pats[r], Lk, gen) for r in range(rm)])
        n_key_rows, key_real = rm * Lk, real.reshape(-1)
        pos = torch.arange(Lk).repeat(rm)
        c.update(key_pad=(~real).to(torch.uint8), mem_row=torch.tensor([1, 0, 1][:groups], dtype=torch.int32) if shared_mem else None,
                 max_keys=Lk)
    else:
        pats = patterns or default
        real = torch.stack([_pattern(pats[g], L, gen) for g in range(groups)])
        n_key_rows, key_real = groups * L, real.reshape(-1)
        pos = torch.arange(L).repeat(groups)
        c.update(tok=_tokens(real, gen), max_keys=L)
    k = torch.randn(n_key_rows, d, generator=gen)
    v = torch.randn(n_key_rows, d, generator=gen)
    _shape_scores(q, k, pos, Lk if mode == FULL_CROSS else L, dist, H)
    k[~key_real] = _loud(gen, int((~key_real).sum()), d)
    v[~key_real] = _loud(gen, int((~key_real).sum()), d)
    if mode == FULL_CROSS and shared_mem:
        k[2 * Lk:], v[2 * Lk:] = float("nan"), float("nan")
    nm = name or f"{MODE_NAMES[mode]}-L{L}" + (f"-Lk{Lk}" if mode == FULL_CROSS else "") + f"-g{groups}-H{H}-{dist}" + ("-shared" if shared_mem else "")
    return Case(q=q, k=k, v=v, name=nm, **c)


def step_case(mode, N, D, slots, H=4, dist="ordinary", seed=0, extra_groups=0, n_active=None, cache_slot=False, src_of=False,
              src_len=False, name=None) -> Case:
    """One verify-step launch.  ``slots``: per slot a dict f, src (source length), front_pad, prefix_pads.  Sequences live in a
    batch of B = slots + 2 rows reached through a non-identity act_idx; slots past n_active hold NaN."""
    gen = torch.Generator().manual_seed(2000 + seed)
    d, rps = H * DH, 1 + N * D
    n_act = len(slots) if n_active is None else n_active
    groups = len(slots) + extra_groups
    B = groups + 2
    act_idx = ((torch.arange(groups) * 1 + 2) % B).flip(0).to(torch.int32)          # slot -> sequence, a permutation, never the identity
    max_f = max([s["f"] for s in slots[:max(n_act, 1)]] + [0])
    Lc = max_f + 3
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
            real = _pattern("mid" if s.get("prefix_pads") else "full", f, gen)
            tok[b, :f] = _tokens(real, gen)
            tok[b, f] = PAD if s.get("front_pad") else 5
            tok[b, f + 1:f + 1 + D] = (torch.arange(D) + (1 if s.get("front_pad") else 0)) % 2 * 9   # column f + 1: real iff the front is PAD
            cb = int(cslot[b]) if cslot is not None else b
            kk, vv = torch.randn(f + rps, d, generator=gen), torch.randn(f + rps, d, generator=gen)
            pos = torch.cat([torch.arange(f + 1), f + 1 + torch.arange(N * D) % max(D, 1)])
            _shape_scores(q[rows], kk, pos, f + 1 + D, dist, H)
            masked = torch.cat([~real, torch.tensor([bool(s.get("front_pad"))]), torch.zeros(N * D, dtype=torch.bool)])
            kk[masked] = _loud(gen, int(masked.sum()), d)
            vv[masked] = _loud(gen, int(masked.sum()), d)
            kc[cb, :f], vc[cb, :f] = kk[:f], vv[:f]
            k[rows], v[rows] = kk[f:], vv[f:]
        else:
            src = int(perm[b]) if perm is not None else b
            n = s["src"]
            slen[b] = n
            real = _pattern("mid" if s.get("prefix_pads") else "full", n, gen)
            kk, vv = torch.randn(n, d, generator=gen), torch.randn(n, d, generator=gen)
            _shape_scores(q[rows], kk, torch.arange(n), n, dist, H)
            kk[~real] = _loud(gen, int((~real).sum()), d)
            vv[~real] = _loud(gen, int((~real).sum()), d)
            mk[src * Lk:src * Lk + n], mv[src * Lk:src * Lk + n] = kk, vv
            key_pad[src, :n] = real.to(torch.uint8)
            if not src_len:                       # every key of the row is read: the tail is masked and loud
                key_pad[src, n:] = 0
                mk[src * Lk + n:(src + 1) * Lk] = _loud(gen, Lk - n, d)
                mv[src * Lk + n:(src + 1) * Lk] = _loud(gen, Lk - n, d)
    if mode == STEP_SELF:
        c.update(tok=tok, gen_ld=gen_ld, kcache=kc, vcache=vc, cache_slot=cslot, Lc=Lc, max_keys=Lc)
    else:
        c.update(key_pad=key_pad, Lk=Lk, src_of=perm, src_len=slen if src_len else None, max_keys=Lk)
        k, v = mk, mv
    nm = name or (f"{MODE_NAMES[mode]}-N{N}-D{D}-g{groups}-a{n_act}-H{H}-{dist}" + ("-cslot" if cache_slot and mode == STEP_SELF else "")
                  + ("-srcof" if src_of and mode == STEP_CROSS else "") + ("-srclen" if src_len and mode == STEP_CROSS else ""))
    return Case(q=q, k=k, v=v, name=nm, **c)


def grid_slots(i, n):
    """Slot specs of grid case i: fronts and source lengths walk their value lists, slot 1 has a PAD front token (case 0: at
    f = 0), slot 2 PADs inside its prefix and source."""
    out = []
    for j in range(n):
        f = F_VALUES[(5 * i + 3 * j) % len(F_VALUES)]
        if j == 1 and i % 4 == 0:
            f = 0
        out.append(dict(f=f, src=SRC_LENS[(5 * i + j) % len(SRC_LENS)], front_pad=(j == 1), prefix_pads=(j == 2)))
    return out


def step_grid(mode):
    """The step cases of the GPU module: every (N, D) with five slots of mixed f / source length in one launch, the null and
    non-identity indirections alternating, plus one slot alone, inactive trailing slots, H = 8 and H = 2."""
    cases = []
    for i, (N, D) in enumerate(STEP_ND):
        cases.append(step_case(mode, N, D, grid_slots(i, 5), dist=DISTS[i % 5], seed=i, extra_groups=i % 2, cache_slot=bool(i % 2),
                               src_of=bool((i // 2) % 2), src_len=bool(i % 3)))
    cases.append(step_case(mode, 3, 10, [dict(f=33, src=33)], dist="offset", seed=20, name=f"{MODE_NAMES[mode]}-one-slot"))
    cases.append(step_case(mode, 5, 13, grid_slots(9, 5), n_active=3, dist="ascending", seed=21, cache_slot=True, src_len=True,
                           name=f"{MODE_NAMES[mode]}-3-of-5-active"))
    cases.append(step_case(mode, 7, 10, grid_slots(10, 3), H=8, dist="descending", seed=22, src_of=True, name=f"{MODE_NAMES[mode]}-H8"))
    # k_attn3 tile counts of 5 and 9 (waves with shares of 2,1,1,1 and 3,2,2,2 tiles) need fronts between those of F_VALUES:
    # 110 + 1 + 40 draft keys = 151 keys, 230 + 1 + 40 = 271 keys
    cases.append(step_case(mode, 7, 10, [dict(f=110, src=70), dict(f=230, src=33, prefix_pads=True), dict(f=64, src=1)], dist="ordinary",
                           seed=24, cache_slot=True, name=f"{MODE_NAMES[mode]}-tiles-5-9"))
    cases.append(step_case(mode, 5, 13, grid_slots(11, 3), H=2, dist="peaked", seed=23, src_len=True, name=f"{MODE_NAMES[mode]}-H2"))
    return cases


def full_grid(mode):
    cases = []
    if mode == FULL_CROSS:
        for i, Lk in enumerate(CROSS_LKS):
            groups = 3 if i % 2 else 1
            cases.append(full_case(mode, 3, Lk, groups, dist=DISTS[i % 5], seed=100 + i, shared_mem=(i % 4 == 1)))
        cases.append(full_case(mode, 3, 33, 3, H=8, dist="offset", seed=120))
        cases.append(full_case(mode, 3, 257, 1, H=2, dist="ascending", seed=121))
    else:
        for i, L in enumerate(SELF_LS):
            cases.append(full_case(mode, L, 0, 1 if i % 2 else 3, dist=DISTS[(i + mode) % 5], seed=10 * mode + i))
        cases.append(full_case(mode, 65, 0, 3, H=8, dist="ascending", seed=10 * mode + 50))
        cases.append(full_case(mode, 33, 0, 1, H=2, dist="offset", seed=10 * mode + 51))
    return cases


def subcase(case: Case, order) -> Case:
    """The slots ``order`` of a step case as a launch of their own (same sequences, caches and sources; only the slot-indexed
    operands move): slot i of the result is slot order[i] of ``case``."""
    rps = case.rps
    rows = torch.cat([torch.arange(g * rps, (g + 1) * rps) for g in order])
    kw = {k: v for k, v in case.__dict__.items() if k not in ("_ref", "d")}
    kw.update(groups=len(order), n_active=len(order), act_idx=case.act_idx[list(order)].clone(), q=case.q[rows].clone(),
              name=f"{case.name}[slots {list(order)}]")
    if case.mode == STEP_SELF:
        kw.update(k=case.k[rows].clone(), v=case.v[rows].clone())
    return Case(**kw)


class Operands:
    """The operands of a case inside guarded allocations on ``device`` and the keyword arguments of NativeTransformer.debug_attn.
    Self modes: one packed QKV buffer (ldq = ldkv = 3d); cross modes: ldq = d and K / V as the first of two layers interleaved
    in a [rows, 4d] buffer, the way production lays memkv out."""

    def __init__(self, case: Case, device="cpu"):
        c, d = case, case.d
        self.case = c
        dev = lambda t: None if t is None else t.to(device)
        if c.mode in (FULL_CROSS, STEP_CROSS):
            self.qa = G.Arena(c.q.shape[0], d, device=device)
            self.kva = G.Arena(c.k.shape[0], 4 * d, device=device)
            self.qa.m[:] = dev(c.q)
            self.kva.m[:, :d], self.kva.m[:, d:2 * d] = dev(c.k), dev(c.v)
            q, k, v = self.qa.m, self.kva.m[:, :d], self.kva.m[:, d:2 * d]
        else:
            self.qa = G.Arena(c.q.shape[0], 3 * d, device=device)
            self.qa.m[:, :d], self.qa.m[:, d:2 * d], self.qa.m[:, 2 * d:] = dev(c.q), dev(c.k), dev(c.v)
            q, k, v = self.qa.m[:, :d], self.qa.m[:, d:2 * d], self.qa.m[:, 2 * d:]
        self.out = G.Arena(c.out_rows, d, device=device, fill=G.OUT_FILL)
        self.kw = dict(mode=c.mode, q=q, k=k, v=v, out=self.out.m, heads=c.H, scale=SCALE, groups=c.groups, max_keys=c.max_keys,
                       L=c.L, Lk=c.Lk, tok=dev(c.tok), pad=PAD, key_pad=dev(c.key_pad), mem_row=dev(c.mem_row), act_idx=dev(c.act_idx),
                       front=dev(c.front), src_of=dev(c.src_of), src_len=dev(c.src_len), cache_slot=dev(c.cache_slot),
                       gen_ld=c.gen_ld, n=c.N, d=c.D, n_active=c.n_active)
        if c.mode == STEP_SELF:
            n_cache = c.kcache.shape[0]
            self.kc = G.Arena(n_cache * c.Lc, d, device=device)
            self.vc = G.Arena(n_cache * c.Lc, d, device=device)
            self.kc.m[:], self.vc.m[:] = dev(c.kcache.reshape(-1, d)), dev(c.vcache.reshape(-1, d))
            self.kw.update(kcache=self.kc.m, vcache=self.vc.m, cache_seq_stride=c.Lc * d)


# ---- checkers -----------------------------------------------------------------------------------------------------------
def _where(case: Case, row: int, col: int) -> str:
    g, qi = divmod(row, case.q_per_group)
    return f"group {g} head {col // DH} query {qi} dim {col % DH}"


def check_structure(out: G.Arena, case: Case, what: str) -> None:
    """Rows of slots >= n_active (the rows behind the live ones) and the guard bands keep their fill; no live word is the fill."""
    G.check_untouched(out, case.live_rows, what)
    live = out.m[:case.live_rows]
    left = torch.nonzero(live.contiguous().view(torch.int32) == G.OUT_FILL)
    assert left.numel() == 0, f"{what}: {left.shape[0]} live output words were never written; first at {_where(case, int(left[0, 0]), int(left[0, 1]))}"


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


def check_bits(a: torch.Tensor, b: torch.Tensor, case: Case, what: str) -> None:
    """Two results of the same rows agree bit for bit (a NaN never agrees)."""
    assert a.shape == b.shape, (a.shape, b.shape)
    same = (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) & ~torch.isnan(a)
    if not bool(same.all()):
        row, col = (int(i) for i in torch.nonzero(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {a.numel()} values differ in their bits; first at {_where(case, row, col)}: "
                             f"{a[row, col].item()!r} against {b[row, col].item()!r}")


def kernels_for(case: Case):
    """The kernels that can serve a case (ttx_debug_attn refuses the others)."""
    ks = [K_ATTN]
    if not (case.mode == FULL_CROSS and case.Lk > 384):
        ks.append(K_ATTN2)
    if case.step and case.H % 4 == 0:
        ks += [K_ATTN3, K_ATTN3S]
    return ks


def repad(case: Case, L2: int) -> Case:
    """The same real tokens padded further: ENC / FULL_SELF to L2 positions per group, FULL_CROSS to L2 keys per memory row.  The
    new key rows are PAD (masked, LOUD), the new query rows random; every row of ``case`` keeps its values."""
    gen = torch.Generator().manual_seed(77)
    d = case.d
    kw = {k: v for k, v in case.__dict__.items() if k not in ("_ref", "d")}
    cross = case.mode == FULL_CROSS
    L1 = case.Lk if cross else case.L
    assert not case.step and L2 >= L1

    def grow(t, n_rows, fresh):
        out = fresh(n_rows * L2, d).reshape(n_rows, L2, d)
        out[:, :L1] = t.reshape(n_rows, L1, d)
        return out.reshape(-1, d)

    loud = lambda r, c_: _loud(gen, r, c_)
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


def stream_case(mode, n_cu: int) -> Case:
    """A k_attn3s launch with more units than the grid has waves (8 per CU): about 1.5 x 8 n_cu units plus a remainder, H = 8 and
    (N, D) = (2, 16), two 32-row tiles per slot, so 16 units per slot.  A wave's consecutive units lie 8 n_cu units = n_cu / 2
    slots apart; fronts walk a list of 9 values and source lengths one of 6 with strides that never bring the same value back at
    that distance, so they differ in f, in the tile count and in the source length."""
    H, N, D = 8, 2, 16
    units = 12 * n_cu + 37
    n_slots = -(-units // (H * 2))
    fs = F_VALUES[:9]
    step = max(1, n_cu // 2)
    slots = [dict(f=fs[(g + g // step) % 9] if step % 9 == 0 else fs[g % 9],
                  src=SRC_LENS[(g + g // step) % 6] if step % 6 == 0 else SRC_LENS[g % 6],
                  front_pad=(g % 11 == 3), prefix_pads=(g % 7 == 2)) for g in range(n_slots)]
    return step_case(mode, N, D, slots, H=H, dist="ordinary", seed=31, extra_groups=1, cache_slot=True, src_len=True,
                     name=f"{MODE_NAMES[mode]}-stream-{n_slots}-slots")
