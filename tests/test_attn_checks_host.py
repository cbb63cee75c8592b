"""The checks of tests/test_gpu_attn_kernels.py can fail: a CPU stand-in "kernel" (the fp32 evaluation of the direct visibility
rule, written into the guarded allocations of util_attn_checks.Operands) passes every checker, and the same stand-in with one
defect an attention kernel could have is flagged by the checker that claims to catch it, under the derived tolerance.  Also:
the two formulations of the step visibility agree on the whole (N, D, f) grid of the GPU module, and the float64 reference
agrees with the oracle's multi-head attention in float64.  No GPU."""
import pytest
import torch

import util_attn_checks as A
import util_gemm_checks as G

_CASES = {}


def host_case(mode, dist="ordinary"):
    """One small case per mode and distribution with every edge the defects need: PAD keys, an all-PAD group, a PAD front
    token (one at f = 0), several drafts, more than one 32-key tile, every indirection given and not the identity."""
    key = (mode, dist)
    if key not in _CASES:
        if mode == A.FULL_CROSS:
            c = A.full_case(mode, 3, 65, 3, dist=dist, seed=7, shared_mem=True)
            c2 = A.full_case(mode, 3, 65, 3, dist=dist, seed=8)                     # memory rows tail / none / mid: a fully masked group
            _CASES[key] = [c, c2]
        elif mode in (A.ENC, A.FULL_SELF):
            _CASES[key] = [A.full_case(mode, 65, 0, 3, dist=dist, seed=7)]
        else:
            _CASES[key] = [A.step_case(mode, 3, 10, A.grid_slots(0, 5), dist=dist, seed=7, extra_groups=1, cache_slot=True, src_of=True,
                                       src_len=True)]
    return _CASES[key]


def attend_online(q, k, v, vis, H, no_max=False, no_rescale=False):
    """The online-softmax evaluation over 32-key tiles in fp32 (what k_attn3 / k_attn3s are defined as), with its two classic
    mistakes on request."""
    nq, nk = vis.shape
    qh, kh, vh = (t.reshape(-1, H, A.DH).transpose(0, 1) for t in (q, k, v))
    s = ((qh @ kh.transpose(-1, -2)) * A.SCALE).masked_fill(~vis[None], float("-inf"))
    M = torch.full((H, nq, 1), float("-inf"))
    Lsum = torch.zeros(H, nq, 1)
    O = torch.zeros(H, nq, A.DH)
    for k0 in range(0, nk, 32):
        st = s[:, :, k0:k0 + 32]
        mi = st.amax(-1, keepdim=True)
        Mn = torch.maximum(M, mi)
        base = torch.zeros_like(Mn) if no_max else torch.where(torch.isinf(Mn), torch.zeros_like(Mn), Mn)
        a = torch.where(torch.isinf(M), torch.zeros_like(M), torch.exp(M - base))
        if no_max:
            a = torch.ones_like(a)
        p = torch.exp(st - base)
        Lsum = Lsum * a + p.sum(-1, keepdim=True)
        O = O * (torch.ones_like(a) if no_rescale else a) + p @ vh[:, k0:k0 + 32]
        M = Mn
    o = O / torch.where(Lsum > 0, Lsum, torch.ones_like(Lsum))
    return o.transpose(0, 1).reshape(nq, H * A.DH)


def mutated(case, defect):
    """Defects that are a wrong index or a wrong mask word: the stand-in evaluates a case whose index / mask arrays are what the
    defective kernel would effectively use (the data stays where it is)."""
    kw = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in case.__dict__.items() if k not in ("_ref", "d")}
    real_tok = lambda t: torch.where(t == A.PAD, torch.full_like(t, 5), t)
    if defect == "PAD key visible":
        if case.mode in (A.ENC, A.FULL_SELF):
            kw["tok"] = real_tok(kw["tok"])
        elif case.mode == A.STEP_SELF:
            for b in range(kw["tok"].shape[0]):
                f = int(case.front[b])
                kw["tok"][b, :f] = real_tok(kw["tok"][b, :f])
        else:
            kw["key_pad"] = torch.full_like(kw["key_pad"], 0 if case.mode == A.FULL_CROSS else 1)
    elif defect in ("PAD front token visible", "real front token masked"):
        for b in range(kw["tok"].shape[0]):
            f = int(case.front[b])
            if defect == "PAD front token visible" and kw["tok"][b, f] == A.PAD:
                kw["tok"][b, f] = 5
            elif defect == "real front token masked" and kw["tok"][b, f] != A.PAD:
                kw["tok"][b, f] = A.PAD
    elif defect == "key_pad polarity swapped":
        kw["key_pad"] = 1 - kw["key_pad"]
    elif defect == "act_idx taken as the identity":
        kw["act_idx"] = torch.arange(case.groups, dtype=torch.int32)
    elif defect == "cache_slot taken as the identity":
        kw["cache_slot"] = None
    elif defect == "src_of taken as the identity":
        kw["src_of"] = None
    elif defect == "mem_row taken as the identity":
        kw["mem_row"] = None
    return A.Case(**kw)


def standin(case, ops, defect=None):
    """A stand-in for a kernel: the direct rule in fp32 on the CPU, written into the live rows of the output arena."""
    c = mutated(case, defect)
    ops.out.reset()
    res = torch.zeros(case.out_rows, case.d)
    for row0, _, q, k, v, vis in A._group_views(c, torch.float32, True):
        vis = vis.clone()
        nq, nk = vis.shape
        f = nk - nq if case.mode == A.STEP_SELF else 0
        if defect == "causal off by one":
            for i in range(nq - 1):
                if case.mode == A.FULL_SELF:
                    vis[i, i + 1] = vis[nq - 1, i + 1]                   # the last query sees every real key
                elif i >= 1 and i % case.D != 0:                         # step row i: token of a draft with a successor in it
                    vis[i, f + i + 1] = True
        elif defect == "draft sees the previous draft":
            for n in range(1, case.N):
                vis[1 + n * case.D, f + 1 + (n - 1) * case.D] = True
        elif defect == "last key dropped":
            vis[:, nk - 1] = False
        elif defect == "clamped duplicate of the last key counted":
            k, v, vis = torch.cat([k, k[-1:]]), torch.cat([v, v[-1:]]), torch.cat([vis, vis[:, -1:]], 1)
        elif defect == "V of the next head":
            v = v.reshape(-1, case.H, A.DH).roll(-1, 1).reshape(-1, case.d)
        if defect in ("no max subtraction", "fold without rescaling"):
            o = attend_online(q, k, v, vis, case.H, no_max=defect == "no max subtraction", no_rescale=defect == "fold without rescaling")
        else:
            o = A.attend(q, k, v, vis, case.H)
        if defect == "NaN for a fully masked query":
            o[~vis.any(1)] = float("nan")
        res[row0:row0 + nq] = o
    ops.out.m[:case.live_rows] = res[:case.live_rows]
    if defect == "row of an inactive slot written":
        ops.out.m[case.live_rows] = 0.0
    elif defect == "guard overwritten":
        ops.out.buf[G.GUARD + ops.out.rows * ops.out.ld] = 0.0
    return ops.out.m.clone()


def flagged_by(case, defect):
    ops = A.Operands(case)
    got = standin(case, ops, defect)
    flagged = []
    for name, check in (("structure", lambda: A.check_structure(ops.out, case, "host")), ("values", lambda: A.check_values(got, case, "host"))):
        try:
            check()
        except AssertionError as e:
            assert "group" in str(e) or "row" in str(e) or "guard" in str(e), str(e)
            flagged.append(name)
    return flagged


ALL = [A.ENC, A.FULL_SELF, A.FULL_CROSS, A.STEP_SELF, A.STEP_CROSS]
STEP = [A.STEP_SELF, A.STEP_CROSS]
DEFECTS = [  # (defect, modes, distribution, the checker that must flag it)
    ("PAD key visible", ALL, "ordinary", "values"),
    ("causal off by one", [A.FULL_SELF, A.STEP_SELF], "ordinary", "values"),
    ("draft sees the previous draft", [A.STEP_SELF], "ordinary", "values"),
    ("PAD front token visible", [A.STEP_SELF], "ordinary", "values"),
    ("real front token masked", [A.STEP_SELF], "ordinary", "values"),
    ("last key dropped", ALL, "ordinary", "values"),
    ("clamped duplicate of the last key counted", ALL, "ordinary", "values"),
    ("no max subtraction", ALL, "offset", "values"),
    ("fold without rescaling", ALL, "ascending", "values"),
    ("V of the next head", ALL, "ordinary", "values"),
    ("act_idx taken as the identity", STEP, "ordinary", "values"),
    ("cache_slot taken as the identity", [A.STEP_SELF], "ordinary", "values"),
    ("src_of taken as the identity", [A.STEP_CROSS], "ordinary", "values"),
    ("mem_row taken as the identity", [A.FULL_CROSS], "ordinary", "values"),
    ("key_pad polarity swapped", [A.FULL_CROSS, A.STEP_CROSS], "ordinary", "values"),
    ("NaN for a fully masked query", [A.ENC, A.FULL_SELF, A.FULL_CROSS, A.STEP_SELF], "ordinary", "values"),
    ("row of an inactive slot written", STEP, "ordinary", "structure"),
    ("guard overwritten", ALL, "ordinary", "structure"),
]


@pytest.mark.parametrize("mode", ALL, ids=A.MODE_NAMES)
@pytest.mark.parametrize("dist", A.DISTS)
def test_correct_standin_passes_every_check(mode, dist):
    for case in host_case(mode, dist):
        assert flagged_by(case, None) == [], case.name
        r = A.reference(case)
        assert 0.0 < r["e32"] < r["tol"] < 1e-2 * max(r["vmax"], 1.0), (case.name, r["e32"], r["tol"])


@pytest.mark.parametrize("defect,modes,dist,checker", DEFECTS, ids=[d[0].replace(" ", "-") for d in DEFECTS])
def test_each_defect_is_flagged(defect, modes, dist, checker):
    for mode in modes:
        hits = [flagged_by(case, defect) for case in host_case(mode, dist)]
        assert any(checker in h for h in hits), f"{defect} in {A.MODE_NAMES[mode]}: flagged by {hits}, expected {checker}"
        if checker == "values":
            assert all("structure" not in h for h in hits), f"{defect}: the structure check has no business flagging it"


def test_checkers_name_the_first_offender():
    case = host_case(A.FULL_SELF)[0]
    ops = A.Operands(case)
    got = standin(case, ops)
    bad = got.clone()
    bad[case.L + 5, 2 * A.DH + 3] += 1.0
    with pytest.raises(AssertionError, match="group 1 head 2 query 5 dim 3"):
        A.check_values(bad, case, "host")
    with pytest.raises(AssertionError, match="group 1 head 2 query 5 dim 3"):
        A.check_bits(bad, got, case, "host")
    A.check_bits(got, got.clone(), case, "host")
    nan = got.clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        A.check_bits(nan, nan.clone(), case, "host")                           # a NaN never agrees, not even with itself


def test_step_visibility_formulations_agree():
    """The dense-sequence expansion and the direct matrix give the same visibility for every (N, D, f) of the GPU grid, with PADs
    in the prefix and both states of the front token; and the two float64 evaluations built on them agree to rounding."""
    for N, D in A.STEP_ND:
        for f in A.F_VALUES:
            real = A._pattern("mid", f + 1, None)
            for front_real in (True, False):
                a = A.step_visibility_direct(N, D, f, real, front_real)
                b = A.step_visibility_expanded(N, D, f, real, front_real)
                assert torch.equal(a, b), (N, D, f, front_real, torch.nonzero(a != b)[0].tolist())
                assert a[0, f + 1:].sum() == 0 and a[:, :f].sum() == (1 + N * D) * int(real[:f].sum())
    for case in A.step_grid(A.STEP_SELF):
        x, _, _ = A.evaluate(case, torch.float64, step_direct=True)
        assert float((x - A.attn_ref64(case)).abs().max()) <= 1e-12 * max(A.reference(case)["vmax"], 1.0), case.name


def test_reference_agrees_with_the_oracle_attention():
    """ENC, FULL_SELF and FULL_CROSS: attn_ref64 against oracle/model.py's _mha in float64 (identity output projection) wherever
    a query sees a key (torch's softmax gives NaN for the others, the kernels' convention is 0)."""
    from oracle.model import NEG_INF, OracleConfig, OracleTransformer
    H, E = 4, 128
    gen = torch.Generator().manual_seed(3)
    st = {"a.in_proj_weight": torch.randn(3 * E, E, generator=gen) / E ** 0.5, "a.in_proj_bias": torch.randn(3 * E, generator=gen),
          "a.out_proj.weight": torch.eye(E), "a.out_proj.bias": torch.zeros(E)}
    orc = OracleTransformer(OracleConfig(vocab_size=30, embedding_dim=E, num_heads=H, max_positions=8), st, dtype=torch.float64)
    w, bias = orc.w["a.in_proj_weight"], orc.w["a.in_proj_bias"]
    for mode in (A.ENC, A.FULL_SELF, A.FULL_CROSS):
        case = A.full_case(mode, 17 if mode != A.FULL_CROSS else 5, 33 if mode == A.FULL_CROSS else 0, 3, seed=40 + mode)
        L, Lkv = case.L, case.Lk or case.L
        xq = torch.randn(3, L, E, generator=gen, dtype=torch.float64)
        xkv = torch.randn(3, Lkv, E, generator=gen, dtype=torch.float64) if mode == A.FULL_CROSS else xq
        case.q = (xq @ w[:E].T + bias[:E]).reshape(-1, E)
        case.k = (xkv @ w[E:2 * E].T + bias[E:2 * E]).reshape(-1, E)
        case.v = (xkv @ w[2 * E:].T + bias[2 * E:]).reshape(-1, E)
        masked = case.key_pad != 0 if mode == A.FULL_CROSS else case.tok == A.PAD
        add = torch.zeros(3, Lkv, dtype=torch.float64).masked_fill(masked, NEG_INF)[:, None, None, :]
        if mode == A.FULL_SELF:
            add = add + torch.full((L, L), NEG_INF, dtype=torch.float64).triu(1)[None, None]
        want = orc._mha("a", xq, xkv, add).reshape(-1, E)
        got, _, _ = A.evaluate(case, torch.float64)
        seen = ~torch.isnan(want).any(-1)
        assert 0 < int(seen.sum()) < seen.numel() or mode == A.FULL_SELF
        assert float((got[seen] - want[seen]).abs().max()) < 1e-12, A.MODE_NAMES[mode]
        assert float(got[~seen].abs().max() if (~seen).any() else 0.0) == 0.0
