"""Top-N accuracy of a prediction CSV — what src/score_predictions.py:15-57 reports, without
requiring RDKit at run time.

The CSV is what the PredictionWriter appends (src/callbacks.py:55-64): ``source,target,prediction_1..N`` per line,
split on commas exactly like the reference does (:20-24; a header line, if present, is scored as a row by the
reference too — pass ``skip_header=True`` to drop it).  A prediction counts as a hit when it equals the target
after canonicalisation.  With RDKit importable the canonical form is RDKit's (invalid SMILES -> "!", :7-13), which is
the reference's definition; without it strings are compared as they are (exact-string top-N: a lower bound of the
RDKit figure, since two spellings of one molecule do not match) and the invalid-SMILES rate is reported as None.
`score_tokens` does the same on token ids, on the device, straight from a generator's output.

Parity: RDKit is absent from the build image and the reference's own script cannot run there — the RDKit branch
is "parity unpinned"; the exact-string branch is checked against a plain per-row restatement in
tests/test_scoring.py.
"""
from __future__ import annotations

import argparse

TOP_N = (1, 3, 5, 10, 15, 20, 50)


def _rdkit_canonicalizer():
    try:
        from rdkit import Chem, RDLogger
    except Exception:
        return None
    RDLogger.DisableLog("rdApp.*")

    def canon(s: str) -> str:
        if s == "":
            return s
        m = Chem.MolFromSmiles(s)
        return "!" if m is None else Chem.MolToSmiles(m)
    return canon


def score_rows(targets: list, predictions: list, canonicalize=None) -> dict:
    """targets: list[str]; predictions: list[list[str]] (ragged; missing ranks count as empty strings, :25)."""
    n = len(targets)
    width = max((len(p) for p in predictions), default=0)
    canon = canonicalize or (lambda s: s)
    cache: dict = {}

    def c(s):
        v = cache.get(s)
        if v is None:
            v = cache[s] = canon(s)
        return v

    first_hit = []                                   # rank (1-based) of the first matching prediction, 0 = none
    invalid = [0] * width
    empty = [0] * width
    for t, ps in zip(targets, predictions):
        ct = c(t)
        rank = 0
        for i in range(width):
            cp = c(ps[i]) if i < len(ps) else ""
            if cp == "!":
                invalid[i] += 1
            if cp == "":
                empty[i] += 1
            if rank == 0 and cp == ct:
                rank = i + 1
        first_hit.append(rank)
    ks = [k for k in TOP_N if k <= width]
    acc = {f"top {k}": 100.0 * sum(1 for r in first_hit if 0 < r <= k) / max(n, 1) for k in ks}
    inv = {f"prediction {k}": (100.0 * invalid[k - 1] / max(n, 1)) if canonicalize else None for k in ks}
    emp = {f"prediction {k}": 100.0 * empty[k - 1] / max(n, 1) for k in ks}
    return {"n_queries": n, "n_preds": width, "accuracy": acc, "invalid_smiles": inv, "empty_smiles": emp,
            "canonicalizer": "rdkit" if canonicalize else "exact string"}


def score_csv(filename: str, skip_header: bool = False, canonicalize="auto") -> dict:
    with open(filename) as f:
        lines = [ln.strip() for ln in f.readlines()]
    if skip_header and lines and lines[0].startswith("source,target"):
        lines = lines[1:]
    targets, preds = [], []
    for line in lines:
        _, t, *ps = line.split(",")
        targets.append(t)
        preds.append(ps)
    canon = _rdkit_canonicalizer() if canonicalize == "auto" else canonicalize
    return score_rows(targets, preds, canon)


def score_tokens(pred, tgt, pad: int, bos: int, eos: int) -> dict:
    """Exact token-id top-N on tensors: pred Long[B,N,L] (hypotheses best-first), tgt Long[B,Lt].  A hypothesis is
    compared on its tokens up to the first EOS with BOS/PAD skipped, like GenericTokenizer.decode
    (src/data_handling/tokenizer_base.py:80-91).  Runs on whatever device the tensors are on."""
    import torch

    def clean(x):                                    # [..., L] -> same shape, tokens kept in order, rest = -1
        after = (x == eos).cumsum(-1) > 0            # from the first EOS on (EOS itself is dropped too)
        keep = ~after & (x != bos) & (x != pad)
        # stable compaction: kept tokens first, in their original order
        order = torch.argsort((~keep).to(torch.int8), dim=-1, stable=True)
        return torch.where(keep.gather(-1, order), x.gather(-1, order), torch.full_like(x, -1))

    B, N, L = pred.shape
    W = max(L, tgt.shape[1])
    p = torch.full((B, N, W), pad, dtype=pred.dtype, device=pred.device)
    p[:, :, :L] = pred
    t = torch.full((B, W), pad, dtype=pred.dtype, device=pred.device)
    t[:, :tgt.shape[1]] = tgt.to(pred.device)
    hit = (clean(p) == clean(t).unsqueeze(1)).all(-1)                  # [B, N]
    top = hit.cumsum(1) > 0
    ks = [k for k in TOP_N if k <= N]
    return {"n_queries": B, "n_preds": N, "accuracy": {f"top {k}": 100.0 * float(top[:, k - 1].float().mean()) for k in ks}}


def rank_by_score(pred, scores):
    """The hypotheses of every source reordered by descending score, unfinished ones last, equal scores in their given order.
    ``pred`` Long[B,N,L]; ``scores``: a HypothesisScores (or anything with ``score`` / ``length`` / ``finished`` [B,N] and an
    optional ``token_logp`` [B,N,L-1]).  Returns ``(pred, scores, perm)`` reordered, with ``perm`` Long[B,N]: rank -> index of the
    hypothesis in the input.  Runs on whatever device the tensors are on."""
    import torch
    order = torch.argsort(scores.score, dim=1, descending=True, stable=True)         # by score ...
    fin = scores.finished.bool().gather(1, order)
    perm = order.gather(1, torch.argsort((~fin).to(torch.int8), dim=1, stable=True))  # ... then finished first, order kept
    tok = getattr(scores, "token_logp", None)
    out = type(scores)(scores.score.gather(1, perm), scores.length.gather(1, perm), scores.finished.gather(1, perm),
                       None if tok is None else tok.gather(1, perm[:, :, None].expand(-1, -1, tok.shape[2])))
    return pred.gather(1, perm[:, :, None].expand(-1, -1, pred.shape[2])), out, perm


def unique_samples(samples, scores, eos: int = 2):
    """The distinct hypotheses among each source's samples.  ``samples`` Long[B, N, L] as
    ``TranslationInferenceSampling.generate`` returns it; ``scores`` Float[B, N] (or anything with ``score`` [B, N], such as a
    HypothesisScores).  Two samples are the same hypothesis when their tokens agree up to and including the first ``eos`` (whatever
    follows it is ignored).  Returns one list per source of ``(tokens Long[L], count, score)``:
    the first occurrence of each hypothesis, how many of the N samples equal it, and its score, ordered by descending score
    (equal scores: first occurrence first).  Plain torch, on whatever device the tensors are on."""
    import torch
    sc = getattr(scores, "score", scores)
    B, N, L = samples.shape
    if tuple(sc.shape) != (B, N):
        raise ValueError(f"scores must be [B, N] = [{B}, {N}], got {tuple(sc.shape)}")
    after = ((samples == eos).cumsum(-1) - (samples == eos).long()) > 0          # strictly after the first EOS
    canon = torch.where(after, torch.full_like(samples, -1), samples).cpu()
    rows, vals = samples.cpu(), sc.detach().cpu().tolist()
    out = []
    for b in range(B):
        first: dict = {}
        for j in range(N):
            key = tuple(canon[b, j].tolist())
            if key in first:
                first[key][1] += 1
            else:
                first[key] = [j, 1]
        uniq = sorted(first.values(), key=lambda e: (-vals[b][e[0]], e[0]))
        out.append([(rows[b, j], cnt, vals[b][j]) for j, cnt in uniq])
    return out


def fold_samples(samples, scores=None, order: str = "score", unfinished: str = "keep", gather: bool = True, with_logmass=None,
                 pad: int = 0, eos: int = 2):
    """``unique_samples`` on the device, with no model at hand: the distinct hypotheses of every source, counted and ranked by
    one kernel launch (ttx_fold_hypotheses without a session).  ``samples`` Long[B, N, L] on the GPU, ``scores`` Float[B, N] (or
    anything with ``.score``) or None; the keywords and the ``FoldedHypotheses`` returned are those of
    ``NativeTransformer.fold_hypotheses``.  With ``order="score"`` and ``unfinished="keep"`` the live ranks are
    ``unique_samples``' list, in its order.  A CPU tensor raises ValueError: there is no CPU fallback, ``unique_samples`` folds on
    the host."""
    from .model import fold_on_device
    if hasattr(samples, "is_cuda") and not samples.is_cuda:
        raise ValueError("fold_samples runs on the GPU and has no CPU fallback: pass device tensors, or fold host tensors with "
                         "scoring.unique_samples")
    return fold_on_device(None, None, samples, scores, order, unfinished, gather, with_logmass, pad, eos)


def write_folds(filename: str, folds, append: bool = True) -> None:
    """The fold side file of the prediction CSV: one line per source, ``n_unique,logmass,count_1,...,count_U`` with the counts in
    the order of the CSV's ``prediction_1..N`` columns (logmass with 9 significant digits: fp32 round-trips; ``nan`` when the fold
    carried none).  ``folds``: a FoldedHypotheses, or ``(count, n_unique, logmass)`` as ``predict_folds`` keeps it."""
    if hasattr(folds, "n_unique"):
        folds = (folds.count, folds.n_unique, folds.logmass)
    count, n_unique, logmass = folds
    cnt, nu = count.detach().cpu().tolist(), n_unique.detach().cpu().tolist()
    lm = [float("nan")] * len(nu) if logmass is None else logmass.detach().cpu().tolist()
    with open(filename, "a" if append else "w") as f:
        for c_row, u, m in zip(cnt, nu, lm):
            print(",".join([str(int(u)), f"{m:.9g}"] + [str(int(c)) for c in c_row[:int(u)]]), file=f)


def read_folds(filename: str) -> list:
    """What ``write_folds`` wrote: per source ``(n_unique, logmass, [count_1, ..., count_U])``."""
    rows = []
    with open(filename) as f:
        for line in f:
            v = line.strip().split(",")
            rows.append((int(v[0]), float(v[1]), [int(c) for c in v[2:]]))
    return rows


def sbs_weights(logp, gumbel):
    """Importance weights of a stochastic-beam-search sample (Kool, van Hoof & Welling, ICML 2019, §4.2).  ``logp`` and ``gumbel``
    are [..., K + 1] as ``TranslationInferenceStochasticBeamSearch(beam_size=K + 1).generate(.., return_details=True)`` returns
    them in sampling order.  kappa is the last row's ``gumbel``, the threshold the first K rows exceeded.  The last row is
    dropped: the result is float64 [..., K], computed on the host.

    The paper's weight is ``p_i / (1 - exp(-exp(logp_i - kappa)))``, p_i = exp(logp_i): the probability of hypothesis i over the
    probability that its perturbed value exceeds kappa.  That holds for perturbed values whose maximum is itself a Gumbel draw
    M.  The search here fixes the maximum at 0 (``gumbel[..., 0] == 0``), and with these values the formula is biased (its
    estimate of the total mass averages 0.92 on the test's toy model).  Moving the maximum from 0 to M moves every perturbed
    value by the same amount in exp(-G): exp(-kappa_M) = exp(-kappa) - 1 + exp(-M), with exp(-M) a unit exponential and the
    sample unchanged.  The weight returned is the paper's averaged over M,
    ``w_i = p_i * int_0^inf e^-e / (1 - exp(-p_i (a + e))) de`` with ``a = exp(-kappa) - 1``, evaluated as
    ``e^a E1(a) + p_i * int e^-e h(p_i (a + e)) de``, h(s) = 1 / (1 - e^-s) - 1 / s (Gauss-Laguerre, 64 nodes).

    With the K hypotheses y_i, ``sum_i w_i f(y_i)`` is an unbiased estimate of ``E_{y ~ p} f(y)``: ``sum_i w_i 1[y_i == y*]``
    estimates the mass the model gives an answer y*, ``sum_i w_i`` estimates 1, and ``sum_i w_i 1[..]`` over any set of answers
    its total mass.  A kappa of -inf (fewer than K + 1 hypotheses exist) gives ``w_i = p_i``: the sample is the support.

    Under the generator's ``top_k`` / ``top_p`` filter ``logp`` is the log-probability under the filtered, renormalised model and
    the weights estimate masses of that distribution; under a ``prefix`` they estimate masses of the conditional distribution
    given source and prefix.  Rows with ``logp = -inf`` (ranks that do not exist) get weight 0."""
    import numpy as np

    def host(x):
        x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
        return x.astype(np.float64)
    lp, g = host(logp), host(gumbel)
    if lp.shape != g.shape or lp.ndim < 1 or lp.shape[-1] < 2:
        raise ValueError(f"logp and gumbel must share a shape [..., K + 1] with K >= 1, got {lp.shape} and {g.shape}")
    p = np.exp(lp[..., :-1])
    with np.errstate(over="ignore"):
        a = np.broadcast_to(np.expm1(-g[..., -1:]), p.shape)      # exp(-kappa) - 1 >= 0
    # the first part: (1 / p) * e^a E1(a) = (1 / p) * int e^-e / (a + e) de
    first = _exp_e1(a)
    # the second part: int e^-e h(p (a + e)) de with the smooth h(s) = 1 / (1 - e^-s) - 1 / s, by Gauss-Laguerre
    nodes, wts = np.polynomial.laguerre.laggauss(64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s = p[..., None] * (a[..., None] + nodes)
        small = s < 1e-4
        h = np.where(small, 0.5 + s / 12.0, -1.0 / np.expm1(-np.where(small, 1.0, s)) - 1.0 / np.where(small, 1.0, s))
        h = np.where(np.isinf(s), 1.0, h)
        second = (h * wts).sum(-1)
    return np.where(p == 0.0, 0.0, first + p * second)


def _exp_e1(a):
    """e^a E1(a) = int_0^inf e^-e / (a + e) de for a >= 0 (inf at 0, 0 at inf), float64: the power series of E1 up to 1, the
    continued fraction 1 / (a + 1 - 1 / (a + 3 - 4 / (a + 5 - ...))) above."""
    import numpy as np
    a = np.asarray(a, dtype=np.float64)
    out = np.zeros_like(a)
    lo = a <= 1.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = np.where(lo, a, 0.5)
        total, term = np.zeros_like(x), np.ones_like(x)
        for k in range(1, 40):
            term = term * (-x) / k
            total -= term / k
        series = np.exp(x) * (-np.euler_gamma - np.log(x) + total)
        y = np.where(lo | np.isinf(a), 2.0, a)
        cf = np.zeros_like(y)
        for k in range(200, 0, -1):                               # backward evaluation, 200 levels: 1e-15 at a = 1
            cf = k * k / (y + 2 * k + 1 - cf)
        cf = 1.0 / (y + 1 - cf)
    out = np.where(lo, series, cf)
    return np.where(np.isinf(a), 0.0, out)


def importance_weights(scores, logq, normalize: bool = True):
    """Importance weights ``p(y) / q(y)`` of hypotheses drawn from a sampling distribution q (temperature, top-k, top-p), float64
    [B, N] on the host.  ``scores``: a HypothesisScores (or log p as an array [B, N]); ``logq``: a ProposalScores (or log q as an
    array [B, N]) of the same rows.  The weight is ``exp(logp - logq)``; a row with ``logq = -inf`` (the sampler cannot emit it:
    its ratio is undefined and it is no draw from q) and a row that is not finished (where ``finished`` is known: an object was
    passed) get weight 0.  ``normalize=True`` divides every source's weights by their sum (self-normalised importance sampling);
    a source without a finite row gets zeros.

    What they estimate.  For N independent draws y_i ~ q of one source, ``(1 / N) sum_i w_i f(y_i)`` with ``normalize=False`` is
    an unbiased estimate of ``sum_{y in supp q} p(y) f(y)``: expectations under the model p RESTRICTED to q's support.  Without a
    filter (temperature only) the supports agree and this is ``E_p f``.  Under ``top_k`` / ``top_p`` the support of p exceeds
    that of q, the mass of p outside it is never seen, and the estimate is biased low by exactly that mass; ``(1 / N) sum_i w_i``
    estimates the mass p gives q's support, not 1.  ``normalize=True`` gives ``sum_i w_i f(y_i)``, the self-normalised
    estimate of ``E_p[f | supp q]``: consistent, biased at finite N (order 1 / N), and usable when p or q is known up to a
    constant only.  Rows must be independent draws; the K distinct rows of stochastic beam search are a sample without
    replacement, for which ``sbs_weights`` is the estimator."""
    import numpy as np

    def host(x):
        x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
        return x.astype(np.float64)
    fin = None
    for obj in (scores, logq):
        f = getattr(obj, "finished", None)
        if f is not None:
            f = host(f) != 0
            fin = f if fin is None else (fin & f)
    lp = host(scores.score if hasattr(scores, "score") else scores)
    lq = host(logq.logq if hasattr(logq, "logq") else logq)
    if lp.ndim != 2 or lp.shape != lq.shape or (fin is not None and fin.shape != lp.shape):
        raise ValueError(f"scores and logq must share a shape [B, N], got {lp.shape} and {lq.shape}")
    ok = np.isfinite(lq) & np.isfinite(lp)
    if fin is not None:
        ok &= fin
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.where(ok, np.exp(np.where(ok, lp - lq, 0.0)), 0.0)
    if normalize:
        tot = w.sum(axis=1, keepdims=True)
        w = np.divide(w, tot, out=np.zeros_like(w), where=tot > 0)
    return w


def check_logit_bias(logit_bias, B: int, vocab_size: int):
    """The per-source logit bias of a sampling call as the library takes it: a floating-point tensor [B, V], ``V`` the model's
    vocabulary, one row per source, every value finite or ``-inf`` (``-inf`` forbids the token).  Returns it as float32, on the
    device it came on; ``None`` for ``None``.  ValueError, naming the first offending source: a shape that is not [B, V], a
    dtype that is not floating point, a ``NaN`` or a ``+inf``.  Pure: CPU tensors are checked as they are (a device tensor's
    verdict is read back)."""
    import torch
    if logit_bias is None:
        return None
    b = torch.as_tensor(logit_bias)
    if not b.dtype.is_floating_point:
        raise ValueError(f"logit_bias must be a floating-point tensor [B, V], got {b.dtype}")
    if b.dim() != 2 or tuple(b.shape) != (B, vocab_size):
        raise ValueError(f"logit_bias must have shape [{B}, {vocab_size}] (one row per source, one value per token of the model's "
                         f"vocabulary), got {tuple(b.shape)}")
    b = b.detach().to(torch.float32)
    bad = (torch.isnan(b) | (b == float("inf"))).any(dim=1)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        v = int(torch.nonzero(torch.isnan(b[i]) | (b[i] == float("inf")))[0])
        raise ValueError(f"logit_bias of source {i} holds {float(b[i, v])!r} at token {v}: values must be finite or -inf")
    return b


def bias_from_allowed(allowed):
    """The logit bias of an allow-list: ``allowed`` Bool[B, V] -> Float32[B, V], ``0`` where a token is allowed and ``-inf`` where
    it is not, on the device of ``allowed``.  ValueError for anything but a two-dimensional bool tensor."""
    import torch
    a = torch.as_tensor(allowed)
    if a.dtype != torch.bool or a.dim() != 2:
        raise ValueError(f"allowed must be a bool tensor [B, V], got {tuple(a.shape)} {a.dtype}")
    out = torch.zeros(a.shape, dtype=torch.float32, device=a.device)
    return out.masked_fill_(~a, float("-inf"))


def combine_bias(logit_bias, allowed, B: int, vocab_size: int):
    """``logit_bias`` and / or ``allowed`` of a call as ONE checked bias (``check_logit_bias``), or ``None`` for neither: the
    allow-list is added as ``-inf`` onto the bias."""
    import torch
    if allowed is None:
        return check_logit_bias(logit_bias, B, vocab_size)
    mask = check_logit_bias(bias_from_allowed(allowed), B, vocab_size)
    if logit_bias is None:
        return mask
    b = check_logit_bias(logit_bias, B, vocab_size)
    return torch.where(torch.isinf(mask).to(b.device), mask.to(b.device), b)


def allowlist_from_source(src, always, vocab_size: int, pad: int):
    """The "product tokens come from the reactants" constraint: Bool[B, V], true for every token id that occurs in the source row
    ``src[b]`` (Long[B, Ls], right-padded with ``pad``, which itself is not allowed on that ground) and for every id in ``always``
    (the structure tokens, EOS).  One scatter on the device of ``src``.  Source ids outside [0, V) are ignored."""
    import torch
    src = torch.as_tensor(src)
    if src.dim() != 2 or src.dtype.is_floating_point or src.dtype == torch.bool:
        raise ValueError(f"src must be an integer tensor [B, Ls], got {tuple(src.shape)} {src.dtype}")
    src = src.to(torch.int64)
    ok = (src != pad) & (src >= 0) & (src < vocab_size)
    out = torch.zeros((src.shape[0], vocab_size + 1), dtype=torch.bool, device=src.device)
    out.scatter_(1, torch.where(ok, src, torch.full_like(src, vocab_size)), True)          # the spare column takes what is ignored
    out = out[:, :vocab_size].contiguous()
    ids = torch.as_tensor(list(always) if not hasattr(always, "shape") else always, dtype=torch.int64).reshape(-1)
    if ids.numel():
        if int(ids.min()) < 0 or int(ids.max()) >= vocab_size:
            raise ValueError(f"always holds an id outside the vocabulary [0, {vocab_size})")
        out[:, ids.to(src.device)] = True
    return out


def write_logq(filename: str, logq, append: bool = True) -> None:
    """The log q side file of the prediction CSV: one line per source, ``logq_1,length_1,finished_1,first_outside_1,...`` in the
    order of the CSV's ``prediction_1..N`` columns (log q with 9 significant digits: fp32 round-trips; ``-inf`` for a row outside
    the support).  ``logq``: a ProposalScores.  The prediction CSV itself is left as it is."""
    lq, ln, fin, fo = (t.detach().cpu().tolist() for t in (logq.logq, logq.length, logq.finished, logq.first_outside))
    with open(filename, "a" if append else "w") as f:
        for q_row, l_row, f_row, o_row in zip(lq, ln, fin, fo):
            print(",".join(f"{q:.9g},{int(n)},{int(bool(d))},{int(o)}" for q, n, d, o in zip(q_row, l_row, f_row, o_row)), file=f)


def read_logq(filename: str) -> list:
    """What ``write_logq`` wrote: per source a list of ``(logq, length, finished, first_outside)``."""
    rows = []
    with open(filename) as f:
        for line in f:
            v = line.strip().split(",")
            rows.append([(float(v[i]), int(v[i + 1]), bool(int(v[i + 2])), int(v[i + 3])) for i in range(0, len(v) - 3, 4)])
    return rows


def write_scores(filename: str, scores, append: bool = True) -> None:
    """The side file of the prediction CSV: one line per source, ``score_1,length_1,finished_1,...,score_N,length_N,finished_N``
    in the order of the CSV's ``prediction_1..N`` columns (scores with 9 significant digits: fp32 round-trips).  The prediction
    CSV itself, which ``score_csv`` reads, is left as it is."""
    sc, ln, fin = (t.detach().cpu().tolist() for t in (scores.score, scores.length, scores.finished))
    with open(filename, "a" if append else "w") as f:
        for s_row, l_row, f_row in zip(sc, ln, fin):
            print(",".join(f"{s:.9g},{int(n)},{int(bool(d))}" for s, n, d in zip(s_row, l_row, f_row)), file=f)


def read_scores(filename: str) -> list:
    """What ``write_scores`` wrote: per source a list of ``(score, length, finished)``."""
    rows = []
    with open(filename) as f:
        for line in f:
            v = line.strip().split(",")
            rows.append([(float(v[i]), int(v[i + 1]), bool(int(v[i + 2]))) for i in range(0, len(v) - 2, 3)])
    return rows


def write_alignments(filename: str, maps, append: bool = True) -> None:
    """The alignment side file of the prediction CSV: one line per source, the hypotheses separated by commas in the order of
    the CSV's ``prediction_1..N`` columns, each the source positions of its live query positions separated by spaces (position
    ``t`` aligns the token ``t + 1`` of the hypothesis; a hypothesis of length 0 gives an empty field).  ``maps``: an
    AttentionMaps (or anything with ``alignment`` [B,N,T] and ``length`` [B,N]).  The prediction CSV itself is left as it is."""
    al, ln = (t.detach().cpu().tolist() for t in (maps.alignment, maps.length))
    with open(filename, "a" if append else "w") as f:
        for a_row, l_row in zip(al, ln):
            print(",".join(" ".join(str(int(j)) for j in a[:int(n)]) for a, n in zip(a_row, l_row)), file=f)


def read_alignments(filename: str) -> list:
    """What ``write_alignments`` wrote: per source a list of per-hypothesis lists of source positions."""
    with open(filename) as f:
        return [[[int(j) for j in field.split()] for field in line.rstrip("\n").split(",")] for line in f]


def write_alternatives(filename: str, alts, append: bool = True) -> None:
    """The alternatives side file of the prediction CSV: one line per source, the hypotheses separated by commas in the order of
    the CSV's ``prediction_1..N`` columns, the live positions of a hypothesis separated by ``;``, each position as
    ``id_1:logp_1 .. id_k:logp_k|rank|entropy`` (9 significant digits: fp32 round-trips; a hypothesis of length 0 gives an empty
    field).  ``alts``: an Alternatives (or anything with its fields).  The prediction CSV itself is left as it is."""
    ids, lps, rk, en, ln = (t.detach().cpu().tolist() for t in (alts.top_id, alts.top_logp, alts.rank, alts.entropy, alts.length))
    with open(filename, "a" if append else "w") as f:
        for i_row, p_row, r_row, e_row, l_row in zip(ids, lps, rk, en, ln):
            print(",".join(";".join(" ".join(f"{int(v)}:{lp:.9g}" for v, lp in zip(i_row[h][p], p_row[h][p]))
                                    + f"|{int(r_row[h][p])}|{e_row[h][p]:.9g}" for p in range(int(n)))
                           for h, n in enumerate(l_row)), file=f)


def read_alternatives(filename: str) -> list:
    """What ``write_alternatives`` wrote: per source a list of hypotheses, each a list of positions
    ``([(id, logp), ...], rank, entropy)``."""
    def position(text):
        pairs, rank, entropy = text.split("|")
        return [(int(i), float(lp)) for i, lp in (pair.split(":") for pair in pairs.split())], int(rank), float(entropy)

    with open(filename) as f:
        return [[[position(t) for t in field.split(";")] if field else [] for field in line.rstrip("\n").split(",")] for line in f]


def near_ties(alts, eps: float):
    """bool [..., T]: the live positions of every hypothesis whose top-1 / top-2 ``margin`` is below ``eps`` — where an fp32
    near-tie decided which token ranks first.  ``alts``: an Alternatives with k >= 2."""
    import torch
    margin = alts.margin
    return (torch.arange(margin.shape[-1], device=margin.device) < alts.length.unsqueeze(-1)) & (margin < eps)


def _fmt(d: dict) -> str:
    w = max(len(k) for k in d)
    return "\n".join(f"{k.ljust(w)}    {'n/a' if v is None else round(v, 6)}" for k, v in d.items())


def main(argv=None):
    ap = argparse.ArgumentParser(description="top-N accuracy of a prediction CSV")
    ap.add_argument("--filename", "-f", type=str, required=True)
    ap.add_argument("--skip-header", action="store_true")
    a = ap.parse_args(argv)
    r = score_csv(a.filename, skip_header=a.skip_header)
    print(f"({r['n_queries']} queries, {r['n_preds']} predictions each, match on {r['canonicalizer']})")
    print("Accuracy, %")
    print(_fmt(r["accuracy"]))
    print()
    print("Invalid SMILES, %")
    print(_fmt(r["invalid_smiles"]))
    print()
    print("Empty SMILES, %")
    print(_fmt(r["empty_smiles"]))
    return r


if __name__ == "__main__":
    main()
