"""Plain restatement of k_beam_step_masked (csrc/ttx_beam_mask.hip.h; include/ttx.h states the rule under
ttx_beam_generate_constrained), the operands of its kernel-level tests, a stand-in kernel with planted defects and the checker.  No
GPU call in here: tests/test_beam_mask_checks_host.py does the restatement by hand and shows on the CPU that the checker fails when
it should; tests/test_gpu_beam_mask_kernel.py holds the kernel to it, one launch at a time (ttx_debug_beam_step_masked).

The rule, for parent k of source b (candidate cc = b * beam + k) whose row holds ``width`` tokens:
  live, free      total[v] = score + log softmax(row)[v] over the row's finite logits; a -inf logit is a -inf child; no finite logit:
                  every child -inf
  finished        one child, PAD, with the artificial row's total (35 on PAD, 0 elsewhere); every other child -inf; score -inf (a
                  dead parent): every child -inf
  live, forced    (width <= pfx_len[b])  the token pfx_tok[pfx_src[b]][width - 1] (outside [0, V): 0) has total = score exactly, every
                  other child is -inf
  selection       the K largest totals, largest first, equal values (all the -inf children among them) by ascending flat index
                  k * V + v, none twice
  dead row        a selected -inf child: the parent's tokens then PAD, score -inf, finished, counted in summary[0]
A case is a util_beam_checks step case (same field names) plus ``pfx_tok`` / ``pfx_len`` / ``pfx_src`` (None: no table).

SCORES.  The bound is util_beam_checks' (lsm64 over the finite logits of the row, one addition): masked ids add exact
zeros to z, so the bound of the unmasked evaluation holds.  A forced child's score is the parent's on the bits, a dead row's is -inf.
The cases are drawn so that the finite totals among the best K + 1 of every source lie GAP = 1e-3 apart or are equal by construction
(identical rows under identical scores), two orders of magnitude above the bound, so the float64 order is the kernel's.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

import util_beam_checks as B

PAD, BOS, EOS = B.PAD, B.BOS, B.EOS
I32, I64, F32, U8 = B.I32, B.I64, B.F32, B.U8
GAP = B.GAP
NEG = -np.inf
STEP_IN, STEP_OUT = B.STEP_IN, B.STEP_OUT
PFX_IN = ["pfx_tok", "pfx_len", "pfx_src"]
FIELDS = ["parent", "token", "new_cand", "new_score", "new_len", "new_finished", "parent_draft"]
DEFECTS = ("inf_twice", "inf_first", "dead_token", "dead_unfinished", "nan_row", "forced_logp", "forced_other_source", "tie_high")


def forced_token(c, b: int):
    """The token source b is forced to at column ``width``, or None where the position is free."""
    if getattr(c, "pfx_len", None) is None or c.width > int(c.pfx_len[b]):
        return None
    tok = int(c.pfx_tok[int(c.pfx_src[b]), c.width - 1])
    return tok if 0 <= tok < c.V else 0


def artificial(c) -> np.ndarray:
    x = np.zeros(c.V, F32)
    x[c.pad] = 35.0
    return x


def totals(c):
    """(tot, bnd) float64 [n_cand, V]: every child's total under the rule (-inf: no such child) and the bound on its fp32 value
    (0 where the rule gives the value exactly)."""
    n_cand, n_l = c.B * c.beam, -(-c.V // 64)
    tot, bnd = np.full((n_cand, c.V), NEG), np.zeros((n_cand, c.V))
    for cc in range(n_cand):
        sc = float(c.score[cc])
        ftok = forced_token(c, cc // c.beam)
        if not c.finished[cc] and ftok is not None:
            tot[cc, ftok] = sc
            continue
        x = artificial(c) if c.finished[cc] else c.logits[c.slot_of[cc]]
        ok = np.isfinite(x)
        if not ok.any() or sc == NEG:
            continue
        l, T = B.lsm64(x[ok], n_l)
        tot[cc, ok] = sc + l
        bnd[cc, ok] = T + (B.EPS32 / 2) * (abs(sc) + np.abs(l))
        if c.finished[cc]:
            keep = np.arange(c.V) == c.pad
            tot[cc, ~keep], bnd[cc, ~keep] = NEG, 0.0
    return tot, bnd


def lsm32_masked(x: np.ndarray, n_l: int) -> np.ndarray:
    """util_beam_checks.lsm32 on a row that may hold -inf (expf(-inf) = 0, logf(0) = -inf); a row without a finite logit: all -inf."""
    if not np.isfinite(x).any():
        return np.full(len(x), NEG, F32)
    with np.errstate(divide="ignore"):
        return B.lsm32(x, n_l)


def select(t: np.ndarray, K: int, high: bool = False) -> list:
    """Flat indices of the K largest entries of ``t``, largest first, equal values the lower (``high``: the higher) index first."""
    return sorted(range(len(t)), key=lambda i: (-t[i], -i if high else i))[:K]


def exact_order(c) -> list:
    """picks[b] = [(parent, token)] in the float64 order; asserts that the finite totals among the best K + 1 of every source are
    GAP apart or planted ties (identical rows, scores and logits)."""
    tot, _ = totals(c)
    picks = []
    for b in range(c.B):
        t = tot[b * c.beam:(b + 1) * c.beam].reshape(-1)
        order = select(t, min(c.K + 1, len(t)))
        for u, w in zip(order[:-1], order[1:]):
            if t[w] == NEG:
                break
            cu, cw = b * c.beam + u // c.V, b * c.beam + w // c.V
            rows = [artificial(c) if c.finished[x] else c.logits[c.slot_of[x]] for x in (cu, cw)]
            tied = (c.finished[cu] == c.finished[cw] and np.array_equal(rows[0], rows[1]) and c.score[cu] == c.score[cw]
                    and rows[0][u % c.V] == rows[1][w % c.V] and (c.finished[cu] or forced_token(c, b) is None))
            assert tied or t[u] - t[w] >= GAP, f"source {b}: totals {t[u]!r} and {t[w]!r} are neither planted ties nor {GAP} apart"
        picks.append([(i // c.V, i % c.V) for i in order[:c.K]])
    return picks


def outputs(c, picks, scores, dead_token: bool = False, dead_unfinished: bool = False) -> dict:
    """The arrays a launch leaves behind that selected ``picks[b]`` = [(parent, token)] with ``scores[b]`` (sentinels elsewhere).
    The two flags plant the defects of that name."""
    Bn, beam, K = c.B, c.beam, c.K
    o = dict(new_cand=B.sent((Bn * K, c.ld), I64), new_score=B.sent(Bn * K, F32), parent=B.sent(Bn * K, I32), new_len=B.sent(Bn * K, I32),
             new_finished=B.sent(Bn * K, U8), parent_draft=B.sent(Bn * K, I32), summary=c.summary.copy())
    for b in range(Bn):
        for r, (k, tok) in enumerate(picks[b]):
            cc, out = b * beam + k, b * K + r
            dead = scores[b][r] == NEG
            o["new_cand"][out] = PAD
            o["new_cand"][out, :c.width] = c.gen[cc, :c.width]
            if not dead or dead_token:
                o["new_cand"][out, c.width] = tok
            o["new_score"][out] = scores[b][r]
            o["parent"][out], o["parent_draft"][out], o["new_len"][out] = cc, 0, c.width + 1
            fin = bool(c.finished[cc]) or tok == c.eos or (dead and not dead_unfinished)
            o["new_finished"][out] = 1 if fin else 0
            o["summary"][0] += 1 if fin else 0
    return o


def standin(c, defect: str | None = None) -> dict:
    """A correct fp32 evaluation of the rule in the kernel's order, or one with ``defect`` (one of DEFECTS) planted."""
    assert defect is None or defect in DEFECTS, defect
    n_cand, n_l = c.B * c.beam, -(-c.V // 64)
    tot = np.full((n_cand, c.V), NEG, F32)
    for cc in range(n_cand):
        b, sc = cc // c.beam, F32(c.score[cc])
        ftok = forced_token(c, b)
        if not c.finished[cc] and ftok is not None:
            if defect == "forced_other_source":
                tok = int(c.pfx_tok[(int(c.pfx_src[b]) + 1) % len(c.pfx_tok), c.width - 1])
                ftok = tok if 0 <= tok < c.V else 0
            tot[cc, ftok] = sc
            if defect == "forced_logp":
                tot[cc, ftok] = sc + lsm32_masked(c.logits[c.slot_of[cc]], n_l)[ftok]
            continue
        x = artificial(c) if c.finished[cc] else c.logits[c.slot_of[cc]]
        if defect == "nan_row" and not np.isfinite(x).any():
            tot[cc] = np.nan
            continue
        with np.errstate(invalid="ignore"):
            tot[cc] = (sc + lsm32_masked(x, n_l)).astype(F32) if sc != NEG else NEG
        if c.finished[cc]:
            tot[cc, np.arange(c.V) != c.pad] = NEG
    picks, scores = [], []
    for b in range(c.B):
        t = tot[b * c.beam:(b + 1) * c.beam].reshape(-1)
        key = np.where(np.isnan(t), NEG, t)
        order = select(key, c.K, high=defect == "tie_high")
        n_fin = int(np.isfinite(key[order]).sum())
        if defect == "inf_twice" and n_fin < c.K:       # k_beam_step's fallback: flat index 0 again and again, as an ordinary row
            order = order[:n_fin] + [0] * (c.K - n_fin)
        if defect == "inf_first" and 0 < n_fin < c.K:
            order[n_fin - 1], order[n_fin] = order[n_fin], order[n_fin - 1]
        picks.append([(i // c.V, i % c.V) for i in order])
        scores.append([t[i] for i in order])
    return outputs(c, picks, scores, dead_token=defect in ("dead_token", "inf_twice"),
                   dead_unfinished=defect in ("dead_unfinished", "inf_twice"))


def check(got: dict, c, what: str) -> float:
    """The arrays ``got`` of a launch against the restatement: the selection is the float64 order (exact_order), every integer is what
    that selection implies, a finite score lies within its bound (a forced child's and a dead row's on the bits).  Raises an
    AssertionError that names the first differing (source, rank, field); ``summary`` and the untouched elements come last.  Returns
    the largest error / bound."""
    Bn, beam, K, V = c.B, c.beam, c.K, c.V
    tot, bnd = totals(c)
    picks = exact_order(c)
    want_sc = [[tot[b * beam + k, t] for k, t in picks[b]] for b in range(Bn)]
    want = outputs(c, picks, want_sc)
    worst = 0.0
    for b in range(Bn):
        for r, (k, tok) in enumerate(picks[b]):
            out, cc = b * K + r, b * beam + k
            w = want_sc[b][r]
            for f in FIELDS:
                if f == "token":
                    g, x = int(got["new_cand"][out, c.width]), int(want["new_cand"][out, c.width])
                    bad = g != x
                elif f == "new_cand":
                    g, x = got[f][out].tolist(), want[f][out].tolist()
                    bad = g != x
                elif f == "new_score":
                    g, x = float(got[f][out]), w
                    if w == NEG or bnd[cc, tok] == 0.0:
                        bad = not (F32(g).view(I32) == F32(x).view(I32))
                    else:
                        ratio = abs(g - x) / bnd[cc, tok] if np.isfinite(g) else np.inf
                        bad = not ratio <= 1.0
                        worst = max(worst, ratio) if not bad else worst
                else:
                    g, x = int(got[f][out]), int(want[f][out])
                    bad = g != x
                assert not bad, f"{what}: source {b} rank {r} field {f}: got {g!r}, the rule gives {x!r}"
    g0, x0 = int(got["summary"][0]), int(want["summary"][0])
    assert g0 == x0, f"{what}: summary[0] is {g0}, the rule gives {x0}"
    for f in STEP_OUT:
        if f != "new_score":
            B.same(got[f], want[f], f"{what}: {f}")
    return worst


def case(*, B_: int = 3, beam: int, K: int, V: int, kind: str, width: int = 3, ld: int = 0, seed: int = 0):
    """Operands of one k_beam_step_masked launch.  kind:
      finite   finite logits, finished parents (beam >= 3), no table: k_beam_step's own case
      tenth    a tenth of the logits -inf; beam >= 3: a finished parent, a dead parent (finished, score -inf) and an all -inf live
               row per source, beside live ones
      few      no finished parent; source b has exactly (K, K - 1, 1)[b % 3] finite children
      few0     the same with (0, 1, K - 1)
      forced   tenth plus a table: prefix lengths (width + 1, width - 1, width) by source, so the middle source is free; the sources'
               rows of the table permuted; one forced id outside [0, V)
      tie      tenth with parents 0 and 1 of every source identical (rows and scores) and two planted maxima: ties across parents"""
    assert kind in ("finite", "tenth", "few", "few0", "forced", "tie"), kind
    for attempt in range(200):
        rng = np.random.default_rng(seed + 1000 * attempt)
        n_cand = B_ * beam
        c = NS(B=B_, beam=beam, K=K, V=V, kind=kind, pad=PAD, eos=EOS, width=width, ld=ld or width + 2,
               pfx_tok=None, pfx_len=None, pfx_src=None)
        c.finished = np.zeros(n_cand, U8)
        c.score = (-rng.random(n_cand) * 9).astype(F32)
        rich = beam >= 3 and kind in ("tenth", "forced", "tie")
        if beam >= 3 and kind not in ("few", "few0"):
            for b in range(B_):
                c.finished[b * beam + beam - 1] = 1                       # a finished parent
                if rich:
                    c.finished[b * beam + beam - 2] = 1                   # a dead parent
                    c.score[b * beam + beam - 2] = NEG
        run = np.flatnonzero(c.finished == 0)
        c.slot_of = np.full(n_cand, -1, I32)
        c.slot_of[run] = rng.permutation(len(run))
        c.logits = (rng.standard_normal((len(run), V)) * 4).astype(F32)
        c.gen = rng.integers(3, 90, size=(n_cand, c.ld)).astype(I32)
        c.summary = np.array([3, B.BIG, 0, 0, 0], I32)
        if kind in ("tenth", "forced", "tie"):
            c.logits[rng.random(c.logits.shape) < 0.1] = NEG
            if beam >= 5:
                for b in range(B_):
                    c.logits[c.slot_of[b * beam + 2]] = NEG               # a live row without a finite logit
        if kind in ("few", "few0"):
            counts = (K, K - 1, 1) if kind == "few" else (0, 1, K - 1)
            for b in range(B_):
                slots = c.slot_of[b * beam:(b + 1) * beam]
                keep = rng.permutation(beam * V)[:counts[b % 3]]
                mask = np.ones(beam * V, bool)
                mask[keep] = False
                rows = c.logits[slots].reshape(-1)
                rows[mask] = NEG
                c.logits[slots] = rows.reshape(beam, V)
        if kind == "tie":
            assert beam >= 5, "parents 0 and 1 live, 2 without a finite logit, then the dead and the finished one"
            for b in range(B_):
                a0, a1 = b * beam, b * beam + 1
                row = c.logits[c.slot_of[a0]]
                v1, v2 = rng.permutation(V)[:2]
                top = row[np.isfinite(row)].max()
                row[v1], row[v2] = top + 12.0, top + 6.0
                c.logits[c.slot_of[a1]] = row
                c.score[a1] = c.score[a0]
                c.score[b * beam + 2:(b + 1) * beam] -= F32(60.0)
        if kind == "forced":
            lens = np.array([(width + 1, width - 1, width)[b % 3] for b in range(B_)], I32)
            c.pfx_ld = width + 2
            c.pfx_src = rng.permutation(B_).astype(I32)
            c.pfx_tok = rng.integers(3, V, size=(B_, c.pfx_ld)).astype(I32)
            c.pfx_tok[c.pfx_src[0], width - 1] = V + 5                     # read as 0
            c.pfx_len = lens
        try:
            exact_order(c)
            return c
        except AssertionError:
            if kind == "tie":
                raise
    raise AssertionError("no case with separated totals found")


def arrays(c) -> dict:
    a = B.step_arrays(c)
    if c.pfx_len is not None:
        a.update(pfx_tok=c.pfx_tok, pfx_len=c.pfx_len, pfx_src=c.pfx_src)
    return a
