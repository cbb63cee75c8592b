"""Syntax-constrained sampling: the syntax table of a SMILES vocabulary and the host-side checks that go with it.

The samplers (``TranslationInferenceSampling``, ``TranslationInferenceSamplingSpeculative`` and its ``generate_many``) take
``syntax=SmilesSyntax(...)``: a row can then only ever hold tokens after which it can still end balanced: every ``(`` closed, every
ring-bond label used an even number of times, EOS inside ``max_len``.  include/ttx.h ("Syntax-constrained sampling") states the rule;
k_syntax_mask (csrc/ttx_syntax.hip.h) applies it on the GPU.  This is a NECESSARY condition for a parseable SMILES string, not
validity: valence, aromaticity, ``()``, ``C11`` and ring bonds across ``.`` are outside it.  No GPU is involved in this module."""
from __future__ import annotations

import re
from typing import NamedTuple

import numpy as np
import torch

FORBID, NEUTRAL, OPEN, CLOSE, RING0, MAX_RINGS = -1, 0, 1, 2, 3, 64

_RING = re.compile(r"^(?:([0-9])|%([0-9]{2}))$")


class SyntaxCheck(NamedTuple):
    """``SmilesSyntax.check``: per row ``balanced`` (depth 0 and no open ring label at its end), ``finished`` (it holds EOS) and
    ``first_offending`` (the first column whose token the rule forbids there, -1 for none)."""
    balanced: np.ndarray
    finished: np.ndarray
    first_offending: np.ndarray


class SmilesSyntax:
    """The syntax table: one int8 class per vocabulary id (-1 FORBID, 0 neutral, 1 OPEN, 2 CLOSE, 3 + l ring label l < 64)."""

    def __init__(self, cls):
        t = torch.as_tensor(cls)
        if t.dim() != 1 or t.numel() < 1:
            raise ValueError(f"a syntax table is one class per vocabulary id, [V]; got shape {tuple(t.shape)}")
        if t.dtype != torch.int8:
            raise ValueError(f"a syntax table is int8; got {t.dtype}")
        t = t.detach().cpu().contiguous()
        if int(t.min()) < FORBID or int(t.max()) >= RING0 + MAX_RINGS:
            raise ValueError(f"syntax classes lie in [-1, {RING0 + MAX_RINGS - 1}]; got [{int(t.min())}, {int(t.max())}]")
        self.cls = t

    @classmethod
    def from_vocab(cls, vocab, forbid=("<PAD>", "<BOS>", "?")) -> "SmilesSyntax":
        """From the token strings: ``(`` opens, ``)`` closes, a digit ``d`` and ``%nn`` are ring-bond labels (numbered in ascending
        order of their value), the tokens of ``forbid`` are never emitted, everything else is neutral.  ``vocab``: a tokenizer (its
        ``decoder_dict``), a token -> id dict, or an id -> token dict (ids as integers or digit strings, as a vocabulary file holds
        them).  More than 64 ring labels are refused."""
        d = getattr(vocab, "decoder_dict", vocab)
        if not isinstance(d, dict) or not d:
            raise ValueError("from_vocab needs a tokenizer or a non-empty vocabulary dict")
        if all(isinstance(v, (int, np.integer)) for v in d.values()):
            by_id = {int(i): str(tok) for tok, i in d.items()}
        else:
            by_id = {int(i): str(tok) for i, tok in d.items()}
        V = max(by_id) + 1
        if min(by_id) < 0:
            raise ValueError("a vocabulary id is negative")
        rings = {}
        for i, tok in by_id.items():
            m = _RING.match(tok)
            if m:
                rings[i] = int(m.group(1) if m.group(1) is not None else m.group(2))
        numbers = sorted(set(rings.values()))
        if len(numbers) > MAX_RINGS:
            raise ValueError(f"the vocabulary holds {len(numbers)} ring-bond labels; the constraint tracks at most {MAX_RINGS}")
        label = {n: l for l, n in enumerate(numbers)}
        out = np.zeros(V, dtype=np.int8)
        for i, tok in by_id.items():
            if tok in forbid:
                out[i] = FORBID
            elif tok == "(":
                out[i] = OPEN
            elif tok == ")":
                out[i] = CLOSE
            elif i in rings:
                out[i] = RING0 + label[rings[i]]
        return cls(torch.from_numpy(out))

    def __len__(self) -> int:
        return int(self.cls.numel())

    def table(self, V: int, device) -> torch.Tensor:
        """The table as a contiguous int8 tensor [V] on ``device``; a table of another length than the vocabulary is refused."""
        if len(self) != int(V):
            raise ValueError(f"the syntax table holds {len(self)} classes, the vocabulary {int(V)} tokens")
        return self.cls.to(device).contiguous()

    # -- the rule on the host ------------------------------------------------------------------------
    def _step(self, tok: int, depth: int, ring: int) -> tuple:
        c = int(self.cls[tok]) if 0 <= tok < len(self) else NEUTRAL
        if c == OPEN:
            depth += 1
        elif c == CLOSE:
            depth -= 1
        elif c >= RING0:
            ring ^= 1 << (c - RING0)
        return depth, ring

    def _allowed(self, tok: int, depth: int, ring: int, left: int, eos: int) -> bool:
        need = max(depth, 0) + bin(ring).count("1")
        if tok == eos:
            return depth == 0 and ring == 0
        c = int(self.cls[tok]) if 0 <= tok < len(self) else NEUTRAL
        if c == FORBID:
            return False
        if c == OPEN:
            return need + 2 <= left
        if c == CLOSE:
            return depth > 0
        if c >= RING0:
            return bool((ring >> (c - RING0)) & 1) or need + 2 <= left
        return need + 1 <= left

    def check(self, rows, eos_token_idx: int = 2, max_len: int | None = None) -> SyntaxCheck:
        """For rows Long[..., L] as ``generate`` returns them (BOS in column 0): ``balanced``, ``finished`` and ``first_offending``
        of every row, arrays of the leading shape.  Columns after the first EOS are not read.  ``max_len``: the length the rows were
        generated under (default L)."""
        a = np.asarray(rows.detach().cpu() if isinstance(rows, torch.Tensor) else rows, dtype=np.int64)
        if a.ndim < 1 or a.shape[-1] < 1:
            raise ValueError("check needs rows [..., L >= 1]")
        lead, L = a.shape[:-1], a.shape[-1]
        max_len = L if max_len is None else int(max_len)
        flat = a.reshape(-1, L)
        bal = np.zeros(len(flat), dtype=bool)
        fin = np.zeros(len(flat), dtype=bool)
        off = np.full(len(flat), -1, dtype=np.int64)
        for r, row in enumerate(flat):
            depth, ring = 0, 0
            for pos in range(1, L):
                tok = int(row[pos])
                if off[r] < 0 and not self._allowed(tok, depth, ring, (max_len - 1) - pos, eos_token_idx):
                    off[r] = pos
                if tok == eos_token_idx:
                    fin[r] = True
                    break
                depth, ring = self._step(tok, depth, ring)
            bal[r] = depth == 0 and ring == 0
        return SyntaxCheck(bal.reshape(lead), fin.reshape(lead), off.reshape(lead))

    def check_prefix(self, prefix, pad_token_idx: int = 0) -> None:
        """Refuse (ValueError) a forced prefix (Long[B, Lp], right-padded with PAD, no BOS) whose running depth goes negative: a ``)``
        with nothing to close can never be balanced.  A prefix that already needs more columns than remain is NOT refused: the rule
        then allows closers only and the row may end unfinished."""
        if prefix is None:
            return
        a = np.asarray(prefix.detach().cpu() if isinstance(prefix, torch.Tensor) else prefix, dtype=np.int64)
        if a.ndim != 2:
            return                       # the generator's own prefix check names the shape
        for b, row in enumerate(a):
            depth, ring = 0, 0
            for c, tok in enumerate(row):
                if int(tok) == pad_token_idx:
                    break
                depth, ring = self._step(int(tok), depth, ring)
                if depth < 0:
                    raise ValueError(f"prefix {b} closes a branch that was never opened (column {c}): its depth goes negative")


def as_syntax(syntax) -> SmilesSyntax | None:
    """``None``, a ``SmilesSyntax``, or an int8 tensor / array [V] (the raw table)."""
    if syntax is None or isinstance(syntax, SmilesSyntax):
        return syntax
    return SmilesSyntax(syntax)
