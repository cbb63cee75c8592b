"""CPU checks of tests/util_beam_checks.py: the restatement of the beam kernels against the oracle's formulations (the torch
expressions of oracle/spec_beam.py:142-257, oracle.drafting.make_drafts, the reference's own top-k goldens), the derived score bound
on every input the GPU test launches (a numpy fp32 evaluation in the kernel's order stays inside it; four bounds of error are
caught), the exemption cap of k_bs_hits on the float64 reference alone, and for every checker a correct output with one wrong
element, which must fail."""
import numpy as np
import pytest
import torch

import util_beam_checks as B
from oracle.drafting import make_drafts
from oracle.spec_beam import nucleus_mask, topk_per_group
from util_models import load_npz


def fails(fn, *args, **kw) -> bool:
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


# -- the port of ttxsel::topk1_index -----------------------------------------------------------------------------------------
def test_topk1_port_matches_torch_topk():
    rng = np.random.default_rng(0)
    for n in range(1, 131):
        for _ in range(12):
            x = rng.integers(-1, 4, size=n)
            assert B.topk1_index(x) == int(torch.from_numpy(x).topk(1).indices[0]), (n, x.tolist())


# -- leaves ------------------------------------------------------------------------------------------------------------------
def torch_leaves(c):
    """spec_beam.py:220-241 on the case's operands: leaves in torch.nonzero order with their fp32 scores."""
    cands = [cc for cc in range(c.n_cand) if not c.pool or c.live[cc]]
    best = [B.best_draft(c, cc) for cc in cands]
    dl, R = c.dl, B.rps(c.N, c.dl)
    cl = torch.zeros((len(cands), dl + 1, c.V))
    for t, cc in enumerate(cands):
        if c.finished[cc]:
            cl[t, :, B.PAD] = 35.0
        else:
            rows = [c.slot_of[cc] * R + (0 if p == 0 else 1 + best[t][0] * dl + (p - 1)) for p in range(dl + 1)]
            cl[t] = torch.from_numpy(c.logits[rows])
    best_n = torch.tensor([b[1] for b in best])
    chosen = torch.from_numpy(np.stack([c.drafts32[cc, b[0]] for cc, b in zip(cands, best)]).astype(np.int64)).reshape(len(cands), dl)
    tree = nucleus_mask(cl, 20.0, c.K, 0.0)
    pos = torch.arange(dl + 1)
    tree = tree * (pos.unsqueeze(0) <= best_n.unsqueeze(1)).unsqueeze(-1)
    marked = chosen.clone()
    short = best_n != dl
    marked[short, best_n[short]] = B.BOS
    tree[:, :-1, :].scatter_(2, marked.unsqueeze(-1), 0.0)
    leaf_c, leaf_p, leaf_t = torch.nonzero(tree, as_tuple=True)
    lp = cl.softmax(-1).log()
    scores = []
    for t, p, tok in zip(leaf_c.tolist(), leaf_p.tolist(), leaf_t.tolist()):
        seq = torch.cat([chosen[t], torch.zeros(1, dtype=torch.long)])
        seq[p] = tok
        step = torch.gather(lp[t], 1, seq.unsqueeze(-1)).squeeze(-1).masked_fill(pos > p, 0.0).cumsum(-1)
        scores.append(float(torch.tensor(c.logp[cands[t]]) + step[-1]))
    return [(cands[t], p, tok) for t, p, tok in zip(leaf_c.tolist(), leaf_p.tolist(), leaf_t.tolist())], scores


@pytest.mark.parametrize("kw", [k for k in B.leaves_cases() if not (k["pool"] and k["dl"] > 4) and k["V"] * k["n_cand"] < 20000],
                         ids=lambda k: f"V{k['V']}-K{k['K']}-N{k['N']}-dl{k['dl']}")
def test_leaves_match_the_torch_formulation(kw):
    c = B.leaves_case(**kw)
    if c.pool:
        c.dl_of[:] = c.dl                                                  # the reference has one draft length
    ref = B.bs_leaves(c)
    want, scores = torch_leaves(c)
    mine = [(cc, p, int(ref.out["leaf_tok"][cc, p, i])) for cc in range(c.n_cand) for p in range(c.dl + 1)
            for i in range(max(int(ref.out["leaf_cnt"][cc, p]), 0)) if not c.pool or c.live[cc]]
    assert mine == want                                                    # tokens, order and counts
    for (cc, p, tok), s in zip(want, scores):
        i = list(ref.out["leaf_tok"][cc, p, :ref.out["leaf_cnt"][cc, p]]).index(tok)
        assert abs(s - ref.score[cc, p, i]) <= ref.bound[cc, p, i], (cc, p, tok)


@pytest.mark.parametrize("kw", list(B.leaves_cases()), ids=lambda k: f"V{k['V']}-K{k['K']}-N{k['N']}-dl{k['dl']}")
def test_leaf_score_bound_holds_for_fp32_and_catches_four_bounds(kw):
    c = B.leaves_case(**kw)
    worst = 0.0
    for vpl in B.vpls_for(c.V):
        c.vpl = vpl
        ref, f32 = B.bs_leaves(c), B.bs_leaves(c, fp32=True)
        worst = max(worst, B.check_leaves(f32.out, c, ref, "fp32 evaluation"))
    assert 0.0 < worst <= 1.0
    real = np.argwhere(~np.isnan(ref.score))
    at = tuple(real[len(real) // 2])
    bad = {k: v.copy() for k, v in f32.out.items()}
    bad["leaf_score"][at] = np.float32(ref.score[at] + 4 * ref.bound[at])
    assert fails(B.check_leaves, bad, c, ref, "four bounds")
    assert {"bos_excluded", "zero_logit"} <= c.features or c.dl == 0
    run = [cc for cc in range(c.n_cand) if (not c.pool or c.live[cc]) and not c.finished[cc]]
    assert sorted({int(ref.out["best_n"][cc]) for cc in run}) == list(range(c.dl + 1))      # every accepted length 0 .. dl


def test_leaves_checker_fails_on_wrong_elements():
    c = B.leaves_case(V=65, K=5, N=3, dl=10, n_cand=12, max_cand=13, seed=3)
    ref, good = B.bs_leaves(c), B.bs_leaves(c, fp32=True).out
    B.check_leaves(good, c, ref, "good")
    cc, p = [tuple(v) for v in np.argwhere(ref.out["leaf_cnt"] >= 2)][0]
    n = int(ref.out["leaf_cnt"][cc, p])
    bad = {k: v.copy() for k, v in good.items()}                           # a segment in descending token order
    bad["leaf_tok"][cc, p, :n] = good["leaf_tok"][cc, p, :n][::-1]
    bad["leaf_score"][cc, p, :n] = good["leaf_score"][cc, p, :n][::-1]
    assert fails(B.check_leaves, bad, c, ref, "descending")
    bad = {k: v.copy() for k, v in good.items()}                           # a leaf written beyond the candidates of the launch
    bad["leaf_cnt"][c.n_cand, 0] = 0
    assert fails(B.check_leaves, bad, c, ref, "tail")
    bad = {k: v.copy() for k, v in good.items()}                           # a score beyond the count
    bad["leaf_score"][cc, p, c.K - 1 if n < c.K else 0] = 0.0
    assert n == c.K or fails(B.check_leaves, bad, c, ref, "beyond")
    bad = {k: v.copy() for k, v in good.items()}                           # another of the equally long drafts
    bad["best_slot"][cc] = (good["best_slot"][cc] + 1) % c.N
    assert fails(B.check_leaves, bad, c, ref, "slot")


# -- hits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", list(B.hits_cases()), ids=lambda k: f"V{k['V']}-K{k['K']}-N{k['N']}-dl{k['dl']}")
def test_hits_reference_alone_stays_under_the_exemption_cap(kw):
    c = B.hits_case(**kw)
    ref = B.bs_hits(c)
    n, inside = int(ref.written.sum()), int((ref.near & ~c.planted & ref.written).sum())
    assert inside <= B.HIT_CAP * n, (inside, n)
    assert B.check_hits(ref.want.copy(), c, ref, "reference") == 0
    if c.dl == 0:
        return
    assert len(c.plans) >= 4 and (ref.margin[c.planted] >= B.PLANT_MARGIN).all()
    for r, at, dup, cc, i, j in c.plans:                                   # the planted token's rank decides the flag
        assert ref.want[cc, i * c.dl + j] == (1 if at < r else 0), (r, at, dup)
    cc, p = [tuple(v) for v in np.argwhere(c.planted)][0]
    bad = ref.want.copy()                                                  # a flag flipped outside the margin
    bad[cc, p] ^= 1
    assert fails(B.check_hits, bad, c, ref, "flipped")
    bad = ref.want.copy()                                                  # a flag of a pair that does not exist
    un = np.argwhere(~ref.written)
    if len(un):
        bad[tuple(un[0])] = 0
        assert fails(B.check_hits, bad, c, ref, "unwritten")


def test_hits_reference_is_the_oracle_nucleus():
    g = load_npz("helpers.npz")
    x = g["nuc_in"].reshape(-1, g["nuc_in"].shape[-1])
    for K, tag in ((5, "a"), (10, "c")):
        kept, _, _ = B.nucleus64(x, K)
        want = np.isfinite(g[f"nuc_out_{tag}"].reshape(x.shape))
        got = np.zeros(x.shape, bool)
        for r in range(len(x)):
            got[r, kept[r][kept[r] >= 0]] = True
        assert (got == want).all()


# -- selection ---------------------------------------------------------------------------------------------------------------
def as_segments(scores: np.ndarray, K: int, rng):
    """One group's scores laid into segments of capacity K with random counts, enumeration order = the flat order."""
    cnt, left = [], len(scores)
    while left:
        n = int(rng.integers(0, min(K, left) + 1))
        cnt.append(n)
        left -= n
    sc = np.full((len(cnt), K), np.nan, np.float32)
    flat, at = [], 0
    for s, n in enumerate(cnt):
        sc[s, :n] = scores[at:at + n]
        flat += [(s, i) for i in range(n)]
        at += n
    return sc, np.array(cnt), flat


def test_selection_matches_topk_per_group():
    rng = np.random.default_rng(1)
    g = load_npz("helpers.npz")
    jobs = [(g["topk_score_in"][:23].reshape(-1), g["topk_lens"], 3, g["topk_score_out"], g["topk_idx_out"]),
            (g["topk_score_in"][:18].reshape(-1), g["topk2_lens"], 2, g["topk2_score_out"], g["topk2_idx_out"])]
    for K in (1, 2, 10, 32):
        lens = rng.integers(K, 3 * K + 5, size=4)
        score = rng.permutation(int(lens.sum())).astype(np.float32) / 7                 # tie-free
        top, idx = topk_per_group(torch.from_numpy(score), lens, K, pad=float("-inf"))
        jobs.append((score, lens, K, top.numpy(), idx.numpy()))
    for score, lens, K, top, idx in jobs:
        start = 0
        for gi, n in enumerate(int(v) for v in lens):
            sc, cnt, flat = as_segments(score[start:start + n], K, rng)
            win = B.best_leaves(sc, cnt, K)
            assert [start + flat.index(w) for w in win] == idx.reshape(len(lens), K)[gi].tolist()
            assert [sc[w] for w in win] == top[gi].tolist()
            start += n


def test_select_checker_fails_on_wrong_elements():
    c = B.select_case(B=2, beam=3, K=3, dl=2, pattern="ties", ld_extra=2, seed=4)
    good = B.beam_select(c)
    B.check_exact(good, B.beam_select(c), "good")
    r = [r for r in range(c.K - 1) if good["new_logp"][r] == good["new_logp"][r + 1]
         and (good["parent"][r], good["mark"][r]) != (good["parent"][r + 1], good["mark"][r + 1])][0]
    bad = {k: v.copy() for k, v in good.items()}                           # a swapped tie
    for k in ("new_cand", "new_logp", "parent", "parent_draft", "mark", "new_len", "new_finished"):
        bad[k][[r, r + 1]] = good[k][[r + 1, r]]
    assert fails(B.check_exact, bad, good, "swapped tie")
    bad = {k: v.copy() for k, v in good.items()}                           # a column beyond the logical width
    bad["new_cand"][0, c.width] = B.PAD
    assert fails(B.check_exact, bad, good, "beyond width")
    short = B.select_case(B=2, beam=3, K=3, dl=2, pattern="short", seed=4)
    out = B.beam_select(short)
    assert out["summary"][4] == 1 and (out["parent"][:3] == B.sent(3, np.int32)).all() and out["parent"][3] >= 0
    for pattern in ("one_quarter", "sparse", "neg_inf", "exact"):          # the patterns are what they claim
        s = B.select_case(B=1, beam=10, K=10, dl=10, pattern=pattern, seed=2)
        per_wave = (s.beam * (s.dl + 1) * s.K + 3) // 4
        out = B.beam_select(s)
        seg = [int(np.flatnonzero((s.leaf_score.reshape(-1) == v))[0]) // per_wave for v in out["new_logp"][:s.K] if np.isfinite(v)]
        if pattern == "one_quarter":
            assert set(seg) == {3}
        if pattern == "sparse":
            assert s.leaf_cnt.reshape(-1)[:-(-per_wave // s.K)].sum() < s.K and 0 in seg
        if pattern == "neg_inf":
            assert np.isneginf(out["new_logp"][1:s.K]).all() and np.isfinite(out["new_logp"][0])
        if pattern == "exact":
            assert s.leaf_cnt[:s.beam].sum() == s.K and out["summary"][4] == 0


# -- k_beam_step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", list(B.step_cases()), ids=lambda k: "-".join(f"{a}{v}" for a, v in k.items() if a != "seed"))
def test_step_bound_holds_for_fp32_and_catches_four_bounds(kw):
    c = B.step_case(**kw)
    good = B.step_fp32(c)
    exact = c.kind != "random"
    assert 0.0 < B.check_step(good, c, "fp32 evaluation", exact) <= 1.0
    tot, bnd = B.step_totals(c)
    k, tok = int(good["parent"][0]), int(good["new_cand"][0, c.width])
    bad = {k_: v.copy() for k_, v in good.items()}
    bad["new_score"][0] = np.float32(tot[k, tok] + 4 * bnd[k, tok])
    assert fails(B.check_step, bad, c, "four bounds", exact)
    if c.kind.startswith("tie"):                                           # a swapped tie
        bad = {k_: v.copy() for k_, v in good.items()}
        assert good["new_score"][0] == good["new_score"][1]
        for name in ("new_cand", "parent"):
            bad[name][[0, 1]] = good[name][[1, 0]]
        assert fails(B.check_step, bad, c, "swapped tie", exact)
    bad = {k_: v.copy() for k_, v in good.items()}                         # the same pair twice
    for name in ("new_cand", "parent", "new_score", "new_finished"):
        bad[name][1] = good[name][0]
    assert c.K == 1 or fails(B.check_step, bad, c, "twice", exact)


def test_step_checker_sees_a_missed_candidate():
    c = B.step_case(B=1, beam=3, K=3, V=65, kind="random", seed=9)
    good = B.step_fp32(c)
    tot, _ = B.step_totals(c)
    flat = np.argsort(-tot.reshape(-1))
    k, tok = divmod(int(flat[c.K + 2]), c.V)                               # a total well below the K best takes the last place
    bad = {k_: v.copy() for k_, v in good.items()}
    bad["parent"][c.K - 1], bad["new_cand"][c.K - 1, :c.width] = k, c.gen[k, :c.width]
    bad["new_cand"][c.K - 1, c.width], bad["new_score"][c.K - 1] = tok, np.float32(tot[k, tok])
    bad["new_finished"][c.K - 1] = 1 if c.finished[k] or tok == B.EOS else 0
    assert fails(B.check_step, bad, c, "missed", False)


# -- k_bs_prep ---------------------------------------------------------------------------------------------------------------
def test_prep_matches_make_drafts_and_the_matching_rule():
    rng = np.random.default_rng(2)
    Bn, Ls, N, K = 3, 40, 4, 3
    src = rng.integers(5, 12, size=(Bn, Ls)).astype(np.int64)              # few symbols: keys with many windows
    src[:, 0], src[:, -1] = B.BOS, B.EOS
    for draft_len in (5, 8):
        lib = make_drafts(src, draft_len + 1, Ls - 5, 5, 200, B.EOS, B.PAD, 4)
        dl = lib.shape[2] - 1
        c = B.prep_case(B=Bn, beam=K, n_cand=Bn * K, max_cand=Bn * K + 1, dl=dl, N=N, smart=True, n_lib=lib.shape[1], seed=draft_len)
        c.lib = lib.astype(np.int32)
        for cc in range(c.n_cand):
            c.cand_next[cc, c.len_next[cc] - 1] = [src[cc // K, 3 + cc], 99, src[cc // K, 1]][cc % 3]
        out = B.bs_prep(c)
        for cc in range(c.n_cand):
            row, b = c.cand_next[cc], cc // K
            last = row[int((row != B.PAD).sum()) - 1]                      # spec_beam.py:147-153
            match = np.flatnonzero(lib[b, :, 0] == last)
            if match.size == 0:
                match = np.array([0])
            rows = [lib[b, j, 1:dl + 1] for j in match[:N]]
            assert out["per_cand"][cc] == len(rows)
            want = rows + [rows[0]] * (N - len(rows))
            assert (out["drafts32"][cc] == np.stack(want)).all()
        assert {1, N} <= set(out["per_cand"][:c.n_cand])
        allc = B.prep_case(B=Bn, beam=K, n_cand=Bn * K, max_cand=Bn * K, dl=draft_len - 2, N=N, smart=False, D0=draft_len, seed=1)
        allc.drafts_all = make_drafts(src[:, 1:], draft_len, N, 5, 200, B.EOS, B.PAD, 4).astype(np.int32)
        out = B.bs_prep(allc)
        for cc in range(allc.n_cand):                                      # spec_beam.py:155-157
            assert (out["drafts32"][cc] == allc.drafts_all[cc // K, :, :allc.dl]).all() and out["per_cand"][cc] == N


def test_prep_and_list_checkers_fail_on_wrong_elements():
    c = B.prep_case(B=2, beam=4, n_cand=6, max_cand=8, dl=5, N=3, smart=True, n_lib=300, seed=5)
    good = B.bs_prep(c)
    bad = {k: v.copy() for k, v in good.items()}                           # a write into a candidate beyond n_cand
    bad["len"][7] = 1
    assert fails(B.check_exact, bad, good, "tail")
    bad = {k: v.copy() for k, v in good.items()}                           # an unused slot that does not repeat the first draft
    cc = int(np.flatnonzero(good["per_cand"][:c.n_cand] < c.N)[0])
    bad["drafts32"][cc, c.N - 1, 0] += 1
    assert fails(B.check_exact, bad, good, "slot")
    rng = np.random.default_rng(3)
    active = (rng.random(70) < 0.5).astype(np.uint8)
    per_cand, length = rng.integers(1, 4, size=70).astype(np.int32), rng.integers(1, 9, size=70).astype(np.int32)
    good, cnt, state = B.bs_list(active, per_cand, length, 67, 3, 4, [0] * 8, 70)
    act = np.flatnonzero(active[:67])
    assert state[:3] == [len(act), 3 * len(act), 13 * len(act)] and cnt[0] == 1 and cnt[6] == len(act)
    assert cnt[3] == len(act) + 4 * int(per_cand[act].sum()) and cnt[5] == int((length[act] - 1).sum()) and cnt[7] == per_cand[:67].max()
    assert (good["slot_of"][67:] == B.sent(3, np.int32)).all() and (good["act_idx"][len(act):] == B.sent(70 - len(act), np.int32)).all()
    bad = {k: v.copy() for k, v in good.items()}                           # two neighbours of the compact list swapped
    bad["act_idx"][[0, 1]] = good["act_idx"][[1, 0]]
    assert fails(B.check_exact, bad, good, "order")


# -- k_tree_cache ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [False, True])
def test_tree_cache_is_the_concatenation(slots):
    c = B.tree_case(d=64, layers=2, n_cand=11, prev_N=3, prev_D=4, slots=slots, seed=6)
    kn, vn = B.tree_cache(c)
    R = B.rps(c.prev_N, c.prev_D)
    qkv = c.qkv.reshape(c.layers, c.max_cand, R, 3, c.d)                   # [layer, slot, step row, q/k/v, d]
    before_k = c.k_old if slots else B.sent(c.k_old.shape, np.float32)
    written = np.zeros(c.k_old.shape[1], bool)
    seen = set()
    for cc in range(c.max_cand):
        p = int(c.parent[cc])
        if not c.active[cc] or p < 0:
            continue
        sp, sc = (int(c.slot_parent[cc]), int(c.slot_self[cc])) if slots else (p, cc)
        written[sc] = True
        slot, n_new = int(c.prev_slot_of[p]), int(c.len[cc] - c.prev_len[p])
        seen.add((n_new, slot >= 0, sp == sc))
        for l in range(c.layers):
            front = qkv[l, slot, :1, 1] if slot >= 0 and n_new > 0 else np.zeros((0, c.d), np.float32)
            first = 1 + int(c.parent_draft[cc]) * c.prev_D
            draft = qkv[l, slot, first:first + n_new - 1, 1] if slot >= 0 and n_new > 1 else np.zeros((0, c.d), np.float32)
            want = np.concatenate([c.k_old[l, sp, :c.prev_len[p] - 1], front, draft])
            B.same(kn[l, sc, :len(want)], want, f"candidate {cc} layer {l}")
            B.same(kn[l, sc, len(want):], before_k[l, sc, len(want):], f"candidate {cc} layer {l}: rows beyond its length")
    B.same(kn[:, ~written], before_k[:, ~written], "slots of candidates the rule skips")
    assert {n for n, _, _ in seen} >= {0, 1, 1 + c.prev_D} and any(not s for _, s, _ in seen)
    assert not slots or {t for _, _, t in seen} == {False, True}
    cc = [cc for cc in range(c.max_cand) if c.active[cc] and c.parent[cc] >= 0 and c.prev_slot_of[c.parent[cc]] >= 0
          and c.len[cc] - c.prev_len[c.parent[cc]] >= 2][0]
    p = int(c.parent[cc])
    sc = int(c.slot_self[cc]) if slots else cc
    bad = kn.copy()                                                        # the source row 1 + best * dl + (j - 1), off by one
    bad[0, sc, c.prev_len[p]] = qkv[0, c.prev_slot_of[p], 1 + int(c.parent_draft[cc]) * c.prev_D + 1, 1]
    assert fails(B.same, bad, kn, "off by one")
    idle = int(np.flatnonzero(c.active == 0)[0])
    bad = kn.copy()                                                        # a write into an inactive candidate
    bad[0, int(c.slot_self[idle]) if slots else idle, 0, 0] = 1.0
    assert fails(B.same, bad, kn, "inactive")
