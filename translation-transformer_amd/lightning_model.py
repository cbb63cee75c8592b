"""Lightning surface of the reference kept for the inference path:

    VanillaEncoderDecoderTransformerLightning   <- src/model/lightning_model.py:22-243

Same ``init_args`` (lightning_model.py:24-51), same ``predict_step`` / ``on_predict_start`` /
``on_predict_end`` hooks and JSON report keys, same ``validation_step`` / ``test_step`` (teacher-forced loss, token and
sequence accuracy logged under the reference's names and flags; the outputs DecodingCallback reads), same attributes the
PredictionWriter callback reads (``tgt_tokenizer``; src/callbacks.py:49-64), same checkpoint key layout (``model.`` + the
names of SURVEY §8(b) B6) — so ``main.py predict|validate|test -c cfg.yaml --ckpt_path ...`` runs unchanged once the YAML's
``model.class_path`` points here.  Training is out of scope: ``training_step`` raises.

``self.model`` is a parameter container with the reference's module names (so Lightning's checkpoint loading
fills it); its torch ``forward`` is never called — all arithmetic runs in libttx_hip.so through the
NativeTransformer built from those parameters when prediction starts (or at the first validation / test step).  The
module imports without pytorch_lightning (absent in the build container); then a minimal stand-in base class is used and
``run_predict`` / ``run_evaluate`` below drive the hooks.
"""
from __future__ import annotations

import datetime
import json
import os
from pathlib import Path
from timeit import default_timer as timer
from types import SimpleNamespace
from typing import Any

import torch
from torch import nn

try:  # pragma: no cover - depends on the environment
    from pytorch_lightning import LightningModule
    HAVE_LIGHTNING = True
except Exception:  # pragma: no cover
    HAVE_LIGHTNING = False

    class LightningModule(nn.Module):  # minimal stand-in: hparams + the hooks this file uses
        def __init__(self):
            super().__init__()
            self.hparams = SimpleNamespace()
            self.trainer = None

        def save_hyperparameters(self, ignore=()):
            import inspect
            frame = inspect.currentframe().f_back
            args = {k: v for k, v in frame.f_locals.items() if k not in ("self", "__class__") and k not in ignore}
            self.hparams = SimpleNamespace(**args)

        def log(self, name, value, batch_size=None, **flags):
            """Records what Lightning's ``self.log`` would reduce: the value (kept on the device), the batch size and the
            flags.  ``batch_size`` defaults to the one run_evaluate set for the current batch, as Lightning infers it."""
            if batch_size is None:
                batch_size = getattr(self, "_current_batch_size", None)
            self.__dict__.setdefault("logged", []).append((name, value, batch_size, flags))

from ._native import activation_code
from .model import NativeTransformer
from . import decoding as D


class _Emb(nn.Module):
    def __init__(self, vocab, d, pad):
        super().__init__()
        self.embedding = nn.Embedding(vocab, d, padding_idx=pad)


class WeightContainer(nn.Module):
    """Parameters only, named exactly like the reference's VanillaTransformer (src/model/modules.py:40-84)."""

    def __init__(self, src_vocab, tgt_vocab, n_enc, n_dec, d, heads, ff, share, src_pad, tgt_pad, activation="relu"):
        super().__init__()
        self.src_pad_token_i, self.tgt_pad_token_i = src_pad, tgt_pad
        self.emb_dim, self.num_heads = d, heads
        self.src_token_featurizer = _Emb(src_vocab, d, src_pad)
        self.tgt_token_featurizer = self.src_token_featurizer if share else _Emb(tgt_vocab, d, tgt_pad)
        enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(d, heads, ff, 0.0, activation, 1e-5, True, False), n_enc,
                                    nn.LayerNorm(d, eps=1e-5), enable_nested_tensor=False)
        dec = nn.TransformerDecoder(nn.TransformerDecoderLayer(d, heads, ff, 0.0, activation, 1e-5, True, False), n_dec,
                                    nn.LayerNorm(d, eps=1e-5))
        self.transformer = nn.Transformer(d_model=d, nhead=heads, batch_first=True, custom_encoder=enc, custom_decoder=dec)
        self.next_token_classifier = nn.Linear(d, tgt_vocab)

    def forward(self, *a, **k):
        raise RuntimeError("the torch modules here only hold parameters; the forward pass runs in libttx_hip.so")


class _PredictAhead:
    """Decodes windows of the predict dataloader ahead of ``predict_step`` so that the rows of many batches share the
    GPU (slot pools for greedy-speculative: generate_many(reorder=True); batches in flight for beam-speculative), while
    ``Trainer.predict`` / ``main.py`` keep calling ``predict_step(batch, batch_idx)`` one batch at a time.

    The reference's loop decodes batch i inside predict_step(i) (src/model/lightning_model.py:209-212).  Here the module
    walks a second iterator over the same (unshuffled: src/data_handling/seq2seq_wrappers.py:168-175) dataloader, `window`
    batches at a time; predict_step(i) checks that the batch it was handed holds exactly the tokens that were decoded for
    index i and returns that tensor — identical to generate(batch) (row-scheduled decoding replays the reference's loop per
    given batch).  Any mismatch (a sampler that reorders) switches the look-ahead off for the rest of the run, the counters of
    the batches that were decoded ahead but not served are taken back, and the batch is decoded on the spot.  A batch on which
    the reference raises (or the max_steps guard trips) is left to generate() so that the error surfaces at the same
    predict_step as in the reference — for every generator: the window is decoded with on_error="skip".  Only dataloaders that
    can be iterated again are looked ahead on (a one-shot iterator would be consumed: the module then decodes per batch)."""

    def __init__(self, generator, loader, window: int, in_flight: int):
        self.generator, self.window, self.in_flight = generator, max(1, int(window)), max(1, int(in_flight))
        self.it = iter(loader)
        self.next_idx = 0            # index of the next batch the iterator yields
        self.ready = {}              # batch index -> (src tokens on the device, prediction or None, its counter shares)
        self.enabled = True
        self.served = self.fallbacks = self.windows = 0
        self.decode_seconds = 0.0
        self.rows = 0                # sources decoded ahead so far: the running index the sampling generators key their rows by
        self.prefixes = {}           # batch index -> the batch's "prefix_tokens" it was decoded with (sampling generators; None: none)
        self.syntax = None           # the module's syntax table (sampling generators under predict_syntax_constraint)
        self.biases = {}             # batch index -> the batch's ("logit_bias", "allowed_tokens") it was decoded with (None: none)
        self.score_ahead = False     # also score every decoded window in one bucketed pass (generator.score_many)
        self.scores = {}             # batch index -> the HypothesisScores of the prediction kept in `ready`
        self.score_seconds = 0.0     # time of the windows' scoring passes that the module has not yet added to its report
        self.kept_scores = None      # set by take(): the scores of the prediction it returned

    def _decode_window(self, device) -> None:
        pending, prefixes, proposals, biases, allowed = [], [], [], [], []
        for _ in range(self.window):
            try:
                b = next(self.it)
            except StopIteration:
                break
            pending.append(b["src_tokens"].to(device))
            prefixes.append(b.get("prefix_tokens") if hasattr(b, "get") else None)
            proposals.append(b.get("proposal_tokens") if hasattr(b, "get") else None)
            biases.append(b.get("logit_bias") if hasattr(b, "get") else None)
            allowed.append(b.get("allowed_tokens") if hasattr(b, "get") else None)
        if not pending:
            self.enabled = False
            return
        g = self.generator
        prompted = any(q is not None for q in prefixes)
        keyed = isinstance(g, (D.TranslationInferenceSamplingSpeculative, D.TranslationInferenceStochasticBeamSearch))
        if prompted and not keyed:
            raise ValueError(f'"prefix_tokens" in a batch: only generation="sampling", "sampling_speculative" and '
                             f'"stochastic_beam_search" take forced prefixes, not {type(g).__name__}')
        proposed = any(q is not None for q in proposals)     # offered drafts: they change no row, so take() does not compare them
        if proposed and not isinstance(g, D.TranslationInferenceSamplingSpeculative):
            raise ValueError(f'"proposal_tokens" in a batch: only generation="sampling_speculative" takes proposals, '
                             f"not {type(g).__name__}")
        biased = any(q is not None for q in biases) or any(q is not None for q in allowed)
        if biased and not keyed:
            raise ValueError(f'"logit_bias" / "allowed_tokens" in a batch: only generation="sampling", "sampling_speculative" and '
                             f'"stochastic_beam_search" take a logit bias, not {type(g).__name__}')
        if biased and not isinstance(g, D.TranslationInferenceSamplingSpeculative):
            self.enabled = False     # the stochastic beam pool takes no bias: these batches are decoded one by one (take() falls back)
            return
        t0 = timer()
        if isinstance(g, D.TranslationInferenceGreedySpeculative):      # slot pools over all rows of the window
            preds = g.generate_many(pending, in_flight=self.in_flight, reorder=True, on_error="skip")
        elif keyed:                 # pools over all sources of the window, keyed as predict_step keys them: the running source index
            keys, r0 = [], self.rows
            for b in pending:
                keys.append(torch.arange(r0, r0 + int(b.shape[0])))
                r0 += int(b.shape[0])
            more = {"proposals": proposals} if proposed else {}
            if biased:
                more.update(logit_biases=biases, allowed=allowed)
            if self.syntax is not None and isinstance(g, D.TranslationInferenceSamplingSpeculative):
                more.update(syntax=self.syntax)
            preds = g.generate_many(pending, row_keys=keys, in_flight=self.in_flight, prefixes=prefixes if prompted else None, **more)
            self.rows = r0
        else:                                                           # source pools over all sources of the window
            preds = g.generate_many(pending, in_flight=self.in_flight, on_error="skip")
        shares = list(getattr(g, "last_batch_counters", [])) or [None] * len(pending)
        self.decode_seconds += timer() - t0
        self.windows += 1
        if self.score_ahead:        # the whole window in length buckets; timed like the module's per-batch pass, idle on both sides
            torch.cuda.synchronize()
            t0 = timer()
            scored = g.score_many(pending, preds)
            torch.cuda.synchronize()
            self.score_seconds += timer() - t0
            for k, sc in enumerate(scored):
                self.scores[self.next_idx + k] = sc
        for k, (src, pred) in enumerate(zip(pending, preds)):
            self.ready[self.next_idx + k] = (src, pred, shares[k])
            self.prefixes[self.next_idx + k] = prefixes[k]
            self.biases[self.next_idx + k] = (biases[k], allowed[k])
        self.next_idx += len(pending)

    def _take_back(self, entries) -> None:
        """The generator's counters without the batches that were decoded ahead but will be decoded again by generate()."""
        for _, pred, share in entries:
            if pred is not None and share:
                for name, v in share.items():
                    setattr(self.generator, name, getattr(self.generator, name) - v)

    @staticmethod
    def _same_prefix(a, b) -> bool:
        if a is None or b is None:
            return a is None and b is None
        return a.shape == b.shape and torch.equal(a.cpu(), b.cpu())

    def take(self, src: torch.Tensor, batch_idx: int, prefix=None, logit_bias=None, allowed=None):
        """The prediction prepared for batch `batch_idx` (and its forced prefixes `prefix`, its `logit_bias` and `allowed`
        list), or None (decode it now)."""
        self.kept_scores = None
        if not self.enabled:
            return None
        if batch_idx not in self.ready and batch_idx == self.next_idx:
            self._decode_window(src.device)
        hit = self.ready.pop(batch_idx, None)
        had = self.prefixes.pop(batch_idx, None)
        had_bias = self.biases.pop(batch_idx, (None, None))
        self.kept_scores = self.scores.pop(batch_idx, None)       # of the prediction returned below; None when it is not served
        if hit is None or hit[0].shape != src.shape or not torch.equal(hit[0], src.to(hit[0].device)) \
                or not self._same_prefix(had, prefix) or not self._same_prefix(had_bias[0], logit_bias) \
                or not self._same_prefix(had_bias[1], allowed):
            self.enabled = False                       # not the batch that was decoded for this index: stop looking ahead
            self._take_back(([hit] if hit is not None else []) + list(self.ready.values()))
            self.ready.clear()
            self.prefixes.clear()
            self.biases.clear()
            self.scores.clear()
            self.kept_scores = None
            self.fallbacks += 1
            return None
        if hit[1] is None:                             # the reference raises on this batch: let generate() raise it here
            self.fallbacks += 1
            return None
        self.served += 1
        return hit[1]


class VanillaEncoderDecoderTransformerLightning(LightningModule):
    def __init__(self,
                 src_tokenizer=None, tgt_tokenizer=None,
                 embedding_dim: int = 128, feedforward_dim: int = 256, num_encoder_layers: int = 3,
                 num_decoder_layers: int = 3, num_heads: int = 4, dropout_rate: float = 0.0, activation: str = "relu",
                 share_embeddings: bool = False,
                 learning_rate: float = 3e-4, weight_decay: float = 0., scheduler: str = "const", warmup_steps: int = 0,
                 generation: str = "beam_search", beam_size: int = 0, max_len: int = 0, n_drafts: int = 0,
                 draft_len: int = 0, smart_drafts_mode: bool = True,
                 sampling_temperature: float = 1.0, sampling_top_k: int = 0, sampling_top_p: float = 1.0, sampling_seed: int = 0,
                 report_prediction_time: bool = True, report_prediction_file: str | None = None):
        super().__init__()
        self.save_hyperparameters(ignore=["src_tokenizer", "tgt_tokenizer"])
        assert src_tokenizer is not None, "source tokenizer not provided"
        assert tgt_tokenizer is not None, "target tokenizer not provided"
        activation_code(activation)                  # ValueError for anything but "relu" / "gelu" (the reference passes a string)
        self.src_tokenizer, self.tgt_tokenizer = src_tokenizer, tgt_tokenizer
        self.src_vocab_size, self.tgt_vocab_size = src_tokenizer.n_tokens, tgt_tokenizer.n_tokens
        self.src_pad_token_i, self.src_bos_token_i, self.src_eos_token_i = (
            src_tokenizer.pad_token_idx, src_tokenizer.bos_token_idx, src_tokenizer.eos_token_idx)
        self.tgt_pad_token_i, self.tgt_bos_token_i, self.tgt_eos_token_i = (
            tgt_tokenizer.pad_token_idx, tgt_tokenizer.bos_token_idx, tgt_tokenizer.eos_token_idx)
        self.model = WeightContainer(self.src_vocab_size, self.tgt_vocab_size, num_encoder_layers, num_decoder_layers,
                                     embedding_dim, num_heads, feedforward_dim, share_embeddings,
                                     self.src_pad_token_i, self.tgt_pad_token_i, activation)
        if generation not in ("greedy", "beam_search", "greedy_speculative", "beam_search_speculative", "sampling",
                              "sampling_speculative", "stochastic_beam_search", "beam_search_constrained"):
            options = ", ".join(["beam_search", "greedy", "greedy_speculative", "beam_search_speculative", "sampling",
                                 "sampling_speculative", "stochastic_beam_search", "beam_search_constrained"])
            raise ValueError(f'Unknown generation option {generation}. Options are {options}.')
        if generation in ("greedy_speculative", "sampling_speculative"):
            assert draft_len > 0, "Number of speculative tokens must be a positive integer."
        self.native: NativeTransformer | None = None
        self.generator = None
        self._ahead = None
        self._scores_on = False
        # generation="sampling" and "sampling_speculative": reactions predicted so far in this predict run; a reaction's running index is its row key, so
        # its samples do not depend on the batch size or on what shares its batch
        self._predict_rows = 0
        # batches decoded ahead of predict_step (0: decode every batch inside its own predict_step like the reference);
        # not an init_arg, so the reference's YAML files load unchanged — set the attribute or TTX_PREDICT_WINDOW
        self.predict_window = 256
        # speculative sampling: decode the look-ahead windows through generate_many (slot pools over the sources of a window, the
        # reactions' running indices as row keys); like predict_window no init_arg — set the attribute or TTX_PREDICT_SAMPLE_POOL=1
        self.predict_sample_pool = False
        # predict_step also scores its hypotheses (NativeTransformer.score_hypotheses) into self.predict_scores[batch_idx];
        # like predict_window no init_arg — set the attribute or TTX_PREDICT_SCORES=1
        self.predict_with_scores = False
        self.predict_scores: dict = {}
        # predict_step also keeps the source alignment of its hypotheses (NativeTransformer.attention_maps, last layer) as
        # self.predict_alignments[batch_idx] = (alignment, length) — the alignment, not the maps: a window of 256 batches of
        # maps does not belong in memory.  No init_arg either — set the attribute or TTX_PREDICT_ATTENTION=1
        self.predict_with_attention = False
        self.predict_alignments: dict = {}
        self._attention_on = False
        # predict_step also keeps what the model considered at every position of its hypotheses (NativeTransformer.alternatives)
        # as self.predict_alternatives[batch_idx]: k > 0 switches it on and is the number of alternatives per position.  With
        # predict_with_scores on too, both come from one decoder pass.  No init_arg either — set the attribute or
        # TTX_PREDICT_ALTERNATIVES=k
        self.predict_with_alternatives = 0
        self.predict_alternatives: dict = {}
        # predict_step also evaluates the hypotheses under the distribution they were drawn from (generator.logq: the
        # generator's temperature and filter, the batch's prefix as forced positions) into self.predict_logq[batch_idx], a
        # ProposalScores; generation "sampling", "sampling_speculative" and "stochastic_beam_search" only.  No init_arg either —
        # set the attribute or TTX_PREDICT_LOGQ=1
        self.predict_with_logq = False
        # hold the samplers to rows that can still end balanced (branches closed, ring labels paired, EOS inside max_len): the
        # syntax table is built from the target tokenizer (syntax.SmilesSyntax.from_vocab); generation "sampling",
        # "sampling_speculative" and "beam_search_constrained" only.  No init_arg either — set the attribute or TTX_PREDICT_SYNTAX=1
        self.predict_syntax_constraint = False
        self.predict_logq: dict = {}
        self._logq_on = False
        # predict_step scores its samples, folds them on the device (generator.fold: order="score", unfinished="last") and
        # RETURNS the folded rows: each reaction's distinct hypotheses best first, all-PAD rows after, so that the writer's
        # prediction_1..N columns hold no duplicate and top-N accuracy means something for a sampling run.
        # self.predict_folds[batch_idx] = (count, n_unique, logmass).  With predict_with_scores on, the kept scores are those of
        # the folded rows.  generation "sampling" and "sampling_speculative" only; refused together with the per-sample records
        # (attention, alternatives, log q).  No init_arg either — set the attribute or TTX_PREDICT_FOLD=1
        self.predict_fold_samples = False
        self.predict_folds: dict = {}
        self._fold_on = False
        self._fold_seconds, self._distinct = 0.0, 0
        self._logq_seconds, self._outside = 0.0, 0
        self._alternatives_k = 0
        self.report_prediction_time = report_prediction_time
        self.prediction_start_time = None

    # -- native path ------------------------------------------------------------------------------
    def _weights_fingerprint(self) -> tuple:
        """Content checksum of the parameters (sum and absolute sum per tensor, float64, computed where the weights live): also
        sees writes through ``p.data`` / optimiser swaps that bump no version counter."""
        ps = list(self.model.parameters())
        if not ps:
            return ()
        with torch.no_grad():
            sums = torch.stack([torch.stack((p.detach().double().sum(), p.detach().double().abs().sum())) for p in ps]).cpu()
        return tuple((tuple(p.shape), float(a), float(b)) for p, (a, b) in zip(ps, sums.tolist()))

    def build_native(self, device: int | str | torch.device | None = None, force: bool = False) -> None:
        """(Re)build the HIP model + generator from the current parameters (call after loading a checkpoint).  A second
        call with unchanged parameter VALUES (content checksum) keeps the HIP model and its warm sessions and only makes a
        fresh generator (zeroed counters); ``force=True`` rebuilds regardless."""
        fp = self._weights_fingerprint()
        if not force and self.native is not None and fp == getattr(self, "_native_fp", None) and device is None:
            self.generator = self._create_generator()
            print(self.generator)
            return
        if device is None:
            p = next(self.model.parameters())
            device = p.device if p.is_cuda else torch.device("cuda:0")
        if self.src_pad_token_i != self.tgt_pad_token_i:
            # the reference keeps the two apart (modules.py:44-47); ttx_config carries one pad id, which masks source keys
            # AND target keys, so a source tokenizer with another pad index would be masked wrongly: refuse it loudly
            raise ValueError(f"source pad id {self.src_pad_token_i} != target pad id {self.tgt_pad_token_i}: the HIP path "
                             "supports one shared pad index (the reference's tokenizers fix PAD=0, tokenizer_base.py:27)")
        self.native = NativeTransformer(self.model.state_dict(), self.hparams.num_heads, self.tgt_pad_token_i, device=device,
                                        activation=self.hparams.activation)
        self._native_fp = fp
        self.generator = self._create_generator()
        print(self.generator)

    def _create_generator(self):
        h, m = self.hparams, self.native
        common = dict(pad_token=self.tgt_pad_token_i, bos_token=self.tgt_bos_token_i, eos_token=self.tgt_eos_token_i)
        if h.generation == "greedy":
            return D.TranslationInferenceGreedy(m, max_len=h.max_len, **common)
        if h.generation == "beam_search":
            return D.TranslationInferenceBeamSearch(m, beam_size=h.beam_size, max_len=h.max_len, **common)
        if h.generation == "beam_search_constrained":   # beam search under the batch's bias / allow-list / prefixes and the syntax table
            return D.TranslationInferenceBeamSearchConstrained(m, beam_size=h.beam_size, max_len=h.max_len, **common)
        if h.generation == "greedy_speculative":
            return D.TranslationInferenceGreedySpeculative(m, max_len=h.max_len, draft_len=h.draft_len, n_drafts=h.n_drafts,
                                                           replace_token=self.tgt_tokenizer.encoder_dict["c"], **common)
        if h.generation == "stochastic_beam_search":  # beam_size distinct draws per reaction (sampling without replacement)
            return D.TranslationInferenceStochasticBeamSearch(m, beam_size=h.beam_size, max_len=h.max_len,
                                                              temperature=h.sampling_temperature, seed=h.sampling_seed,
                                                              top_k=h.sampling_top_k, top_p=h.sampling_top_p, **common)
        if h.generation == "sampling":               # beam_size samples per reaction, as the reference uses it for n_best
            return D.TranslationInferenceSampling(m, max_len=h.max_len, temperature=h.sampling_temperature, top_k=h.sampling_top_k,
                                                  top_p=h.sampling_top_p, num_samples=max(1, h.beam_size), seed=h.sampling_seed,
                                                  **common)
        if h.generation == "sampling_speculative":   # the same samples from the speculative loop
            return D.TranslationInferenceSamplingSpeculative(
                m, max_len=h.max_len, draft_len=h.draft_len, n_drafts=h.n_drafts, replace_token=self.tgt_tokenizer.encoder_dict["c"],
                temperature=h.sampling_temperature, top_k=h.sampling_top_k, top_p=h.sampling_top_p, num_samples=max(1, h.beam_size),
                seed=h.sampling_seed, **common)
        return D.TranslationInferenceBeamSearchSpeculative(
            m, vocab_size=self.tgt_vocab_size, max_len=h.max_len, n_best=h.beam_size, draft_len=h.draft_len,
            n_drafts=h.n_drafts, C_token=self.tgt_tokenizer.encoder_dict["c"], smart_drafts_mode=h.smart_drafts_mode, **common)

    # -- hooks kept from the reference ---------------------------------------------------------------
    def predict_step(self, batch: Any, batch_idx: int, dataloader_idx: int = 0) -> Any:
        if self.generator is None:
            self.build_native()
        ahead = self._ahead
        pred = None
        sampling = self.hparams.generation in ("sampling", "sampling_speculative")
        beams = ("stochastic_beam_search", "beam_search_constrained")              # the beam loops that take prefixes and a bias
        prefix = batch["prefix_tokens"] if "prefix_tokens" in batch else None      # forced target prefixes: Long[B, Lp], no BOS
        if prefix is not None and not sampling and self.hparams.generation not in beams:
            raise ValueError(f'"prefix_tokens" in a batch: only generation="sampling", "sampling_speculative", '
                             f'"stochastic_beam_search" and "beam_search_constrained" take forced prefixes, not '
                             f'"{self.hparams.generation}"')
        proposal = batch["proposal_tokens"] if "proposal_tokens" in batch else None  # offered drafts: Long[B, Lq], no BOS
        if proposal is not None and self.hparams.generation != "sampling_speculative":
            raise ValueError(f'"proposal_tokens" in a batch: only generation="sampling_speculative" takes proposals, '
                             f'not "{self.hparams.generation}"')
        # per-source logit bias Float[B, V] and / or allow-list Bool[B, V]: which tokens a source may produce
        bias = {k: batch[name] for k, name in (("logit_bias", "logit_bias"), ("allowed", "allowed_tokens")) if name in batch}
        if bias and not sampling and self.hparams.generation not in beams:
            raise ValueError(f'"logit_bias" / "allowed_tokens" in a batch: only generation="sampling", "sampling_speculative", '
                             f'"stochastic_beam_search" and "beam_search_constrained" take a logit bias, not '
                             f'"{self.hparams.generation}"')
        kept = None                  # the batch's HypothesisScores when its window was scored ahead
        if ahead is not None and dataloader_idx == 0:
            pred = ahead.take(batch["src_tokens"], batch_idx, prefix, bias.get("logit_bias"), bias.get("allowed"))
            kept = ahead.kept_scores if pred is not None else None
            if self._scores_on:      # the windows' scoring passes count where the per-batch passes count
                self._scoring_seconds += ahead.score_seconds
            ahead.score_seconds = 0.0
        if pred is not None and self.hparams.generation in ("sampling", "sampling_speculative", "stochastic_beam_search"):
            self._predict_rows += int(batch["src_tokens"].shape[0])        # served ahead under these keys: a fallback goes on from here
        elif pred is None and self.hparams.generation in ("sampling", "sampling_speculative"):
            B = int(batch["src_tokens"].shape[0])
            more = dict(bias) if proposal is None else dict(bias, proposal=proposal)
            if getattr(self, "_syntax", None) is not None:
                more["syntax"] = self._syntax
            pred = self.generator.generate(batch["src_tokens"], row_keys=torch.arange(self._predict_rows, self._predict_rows + B),
                                           prefix=prefix, **more)
            self._predict_rows += B
        elif pred is None and self.hparams.generation == "stochastic_beam_search":   # keyed like the samplers: the running index
            B = int(batch["src_tokens"].shape[0])
            pred = self.generator.generate(batch["src_tokens"], row_keys=torch.arange(self._predict_rows, self._predict_rows + B),
                                           prefix=prefix, **bias)
            self._predict_rows += B
        elif pred is None and self.hparams.generation == "beam_search_constrained":
            more = dict(bias)
            if getattr(self, "_syntax", None) is not None:
                more["syntax"] = self._syntax
            pred = self.generator.generate(batch["src_tokens"], prefix=prefix, **more)
        elif pred is None:
            pred = self.generator.generate(batch["src_tokens"])
        if self._fold_on:
            return self._fold_batch(batch["src_tokens"], pred, batch_idx, kept)
        both = self._logq_on and self._scores_on and self._alternatives_k <= 0     # scores and log q from ONE decoder pass
        if self._alternatives_k > 0:
            self._alternatives_batch(batch["src_tokens"], pred, batch_idx)
        elif self._scores_on and not both:
            self._score_batch(batch["src_tokens"], pred, batch_idx, kept)
        if self._attention_on:
            self._align_batch(batch["src_tokens"], pred, batch_idx)
        if self._logq_on:
            self._logq_batch(batch["src_tokens"], pred, batch_idx, prefix, with_scores=both, bias=bias)
        return pred

    def _logq_batch(self, src: torch.Tensor, pred: torch.Tensor, batch_idx: int, prefix, with_scores: bool = False,
                    bias: dict | None = None) -> None:
        """The batch's ProposalScores under the generator's own distribution, whether it was decoded ahead or on the spot; the
        token tensor predict_step returns stays what it was.  ``with_scores``: the batch's HypothesisScores come from the same
        decoder pass (its time then counts as scoring_seconds too, as _alternatives_batch counts its own).  Timed like
        _score_batch."""
        torch.cuda.synchronize()
        t0 = timer()
        more = dict(bias or {})
        if getattr(self, "_syntax", None) is not None:
            more["syntax"] = self._syntax
        q = self.generator.logq(src, pred, prefix=prefix, with_scores=with_scores, **more)
        torch.cuda.synchronize()
        dt = timer() - t0
        self._logq_seconds += dt
        if with_scores:
            sc = q.scores
            self._scoring_seconds += dt
            self._keep_scores(type(sc)(sc.score, sc.length, sc.finished, None), batch_idx)
            q = q._replace(scores=None)
        self.predict_logq[batch_idx] = q
        self._outside = self._outside + (q.first_outside >= 0).sum()      # kept on the device until the report

    def _fold_batch(self, src: torch.Tensor, pred: torch.Tensor, batch_idx: int, kept=None) -> torch.Tensor:
        """The batch's samples scored and folded, whether they were decoded ahead or on the spot: returns the folded rows
        (distinct, best first, all-PAD rows after) and keeps (count, n_unique, logmass); with scores on, the kept
        HypothesisScores are those of the folded rows, gathered by ``perm``, and hold what the scoring rule gives an all-PAD row
        (score 0, length 0, unfinished) beyond ``n_unique``.  Timed like _score_batch.  ``kept``: the samples' scores when the
        look-ahead scored their window (the same values; their time is counted already)."""
        torch.cuda.synchronize()
        t0 = timer()
        sc = kept if kept is not None else self.generator.score(src, pred)
        torch.cuda.synchronize()
        t1 = timer()
        f = self.generator.fold(src, pred, scores=sc, order="score", unfinished="last")
        torch.cuda.synchronize()
        self._fold_seconds += timer() - t1
        self.predict_folds[batch_idx] = (f.count, f.n_unique, f.logmass)
        self._distinct = self._distinct + f.n_unique.sum()                 # kept on the device until the report
        if self._scores_on:
            self._scoring_seconds += t1 - t0
            live = f.perm >= 0
            idx = f.perm.clamp(min=0).long()
            zero = torch.zeros((), dtype=sc.score.dtype, device=sc.score.device)
            self._keep_scores(type(sc)(torch.where(live, sc.score.gather(1, idx), zero),
                                       torch.where(live, sc.length.gather(1, idx), torch.zeros_like(sc.length)),
                                       live & sc.finished.gather(1, idx), None), batch_idx)
        return f.pred

    def _score_batch(self, src: torch.Tensor, pred: torch.Tensor, batch_idx: int, kept=None) -> None:
        """The batch's HypothesisScores, whether it was decoded ahead or on the spot; the token tensor predict_step returns
        stays what it was.  Timed with a synchronisation on both sides, so scoring_seconds is the pass's own time.  ``kept``: the
        scores the look-ahead computed with the batch's window (generator.score_many: the same values bit for bit), served as
        they are; their time was counted when the window was scored."""
        if kept is not None:
            self._keep_scores(kept, batch_idx)
            return
        torch.cuda.synchronize()
        t0 = timer()
        sc = self.generator.score(src, pred)
        torch.cuda.synchronize()
        self._scoring_seconds += timer() - t0
        self._keep_scores(sc, batch_idx)

    def _keep_scores(self, sc, batch_idx: int) -> None:
        self.predict_scores[batch_idx] = sc
        self._top1_sum = self._top1_sum + sc.score[:, 0].double().sum()      # kept on the device until the report
        self._top1_n += int(sc.score.shape[0])
        self._unfinished = self._unfinished + (~sc.finished).sum()

    def _alternatives_batch(self, src: torch.Tensor, pred: torch.Tensor, batch_idx: int) -> None:
        """The batch's Alternatives and, with scores on, its HypothesisScores from the same decoder pass (its time then counts
        as scoring_seconds too); the token tensor predict_step returns stays what it was.  Timed like _score_batch."""
        torch.cuda.synchronize()
        t0 = timer()
        out = self.generator.alternatives(src, pred, k=self._alternatives_k, with_scores=self._scores_on)
        torch.cuda.synchronize()
        dt = timer() - t0
        self._alternatives_seconds += dt
        if not self._scores_on:
            self.predict_alternatives[batch_idx] = out
            return
        alts, sc = out
        self._scoring_seconds += dt
        self.predict_alternatives[batch_idx] = alts
        self._keep_scores(type(sc)(sc.score, sc.length, sc.finished, None), batch_idx)

    def _align_batch(self, src: torch.Tensor, pred: torch.Tensor, batch_idx: int) -> None:
        """The batch's source alignments, whether it was decoded ahead or on the spot; the token tensor predict_step returns
        stays what it was.  Timed like _score_batch."""
        torch.cuda.synchronize()
        t0 = timer()
        maps = self.generator.attention(src, pred)
        torch.cuda.synchronize()
        self._attention_seconds += timer() - t0
        self.predict_alignments[batch_idx] = (maps.alignment, maps.length)

    def _predict_loader(self):
        """The (first) predict dataloader Trainer.predict iterates, or None."""
        tr = self.trainer
        if tr is None:
            return None
        loaders = getattr(tr, "predict_dataloaders", None)
        if loaders is None:
            dm = getattr(tr, "datamodule", None)
            loaders = dm.predict_dataloader() if dm is not None and hasattr(dm, "predict_dataloader") else None
        if loaders is None:
            return None
        if isinstance(loaders, (list, tuple)):
            if len(loaders) == 0:
                return None
            return loaders if isinstance(loaders[0], dict) else loaders[0]     # a list of batches is a loader itself
        return loaders

    def on_predict_start(self) -> None:
        self.build_native()                      # weights are final here (Trainer.predict has loaded --ckpt_path)
        self._ahead = None
        self._predict_rows = 0
        self._scores_on = bool(self.predict_with_scores) or os.environ.get("TTX_PREDICT_SCORES") == "1"
        self.predict_scores = {}
        self._attention_on = bool(self.predict_with_attention) or os.environ.get("TTX_PREDICT_ATTENTION") == "1"
        self.predict_alignments = {}
        try:
            self._alternatives_k = int(self.predict_with_alternatives) or int(os.environ.get("TTX_PREDICT_ALTERNATIVES", "0"))
        except ValueError:
            raise ValueError("predict_with_alternatives / TTX_PREDICT_ALTERNATIVES must be an integer k (0: off), got "
                             f"{self.predict_with_alternatives!r} / {os.environ.get('TTX_PREDICT_ALTERNATIVES')!r}") from None
        self.predict_alternatives = {}
        self._logq_on = bool(self.predict_with_logq) or os.environ.get("TTX_PREDICT_LOGQ") == "1"
        if self._logq_on and self.hparams.generation not in ("sampling", "sampling_speculative", "stochastic_beam_search"):
            raise ValueError('predict_with_logq / TTX_PREDICT_LOGQ: only generation="sampling", "sampling_speculative" and '
                             f'"stochastic_beam_search" draw from a sampling distribution, not "{self.hparams.generation}"')
        self.predict_logq = {}
        self._fold_on = bool(self.predict_fold_samples) or os.environ.get("TTX_PREDICT_FOLD") == "1"
        if self._fold_on and self.hparams.generation not in ("sampling", "sampling_speculative"):
            raise ValueError('predict_fold_samples / TTX_PREDICT_FOLD: only generation="sampling" and "sampling_speculative" '
                             f'return repeated rows to fold, not "{self.hparams.generation}"')
        if self._fold_on and (self._attention_on or self._alternatives_k > 0 or self._logq_on):
            raise ValueError("predict_fold_samples / TTX_PREDICT_FOLD returns the folded rows; predict_with_attention, "
                             "predict_with_alternatives and predict_with_logq keep one record per sample and cannot be combined "
                             "with it (predict_with_scores can)")
        self.predict_folds = {}
        self._fold_seconds, self._distinct = 0.0, 0
        self._syntax = None
        if bool(self.predict_syntax_constraint) or os.environ.get("TTX_PREDICT_SYNTAX") == "1":
            if self.hparams.generation not in ("sampling", "sampling_speculative", "beam_search_constrained"):
                raise ValueError('predict_syntax_constraint / TTX_PREDICT_SYNTAX: only generation="sampling", '
                                 '"sampling_speculative" and "beam_search_constrained" take the syntax constraint, not '
                                 f'"{self.hparams.generation}"')
            from .syntax import SmilesSyntax
            self._syntax = SmilesSyntax.from_vocab(self.tgt_tokenizer)
        self._logq_seconds, self._outside = 0.0, 0
        self._alternatives_seconds = 0.0
        self._attention_seconds = 0.0
        self._scoring_seconds, self._top1_n, self._top1_sum, self._unfinished = 0.0, 0, 0.0, 0
        window = int(os.environ.get("TTX_PREDICT_WINDOW", str(self.predict_window)))
        # speculative sampling and stochastic beam search decode per batch unless asked to pool: predict_sample_pool /
        # TTX_PREDICT_SAMPLE_POOL=1
        per_batch = (D.TranslationInferenceSamplingSpeculative, D.TranslationInferenceStochasticBeamSearch)
        pooled = not isinstance(self.generator, per_batch) or bool(self.predict_sample_pool) \
            or os.environ.get("TTX_PREDICT_SAMPLE_POOL") == "1"
        if window > 0 and pooled and hasattr(self.generator, "generate_many"):
            loader = self._predict_loader()
            # a second pass over the loader must not consume it: one-shot iterators (iter(x) is x) are decoded per batch
            if loader is not None and iter(loader) is not loader:
                self._ahead = _PredictAhead(self.generator, loader, window, int(os.environ.get("TTX_INFLIGHT", "8")))
                self._ahead.syntax = self._syntax
                # scores alone (for themselves or for the fold): score every window ahead too, in one bucketed pass; log q,
                # alternatives and attention keep their per-batch passes (TTX_SCORE_LIST=0: so do the scores)
                self._ahead.score_ahead = (self._scores_on or self._fold_on) and not self._logq_on and self._alternatives_k <= 0 \
                    and not self._attention_on and os.environ.get("TTX_SCORE_LIST", "1") != "0"
        if self.report_prediction_time:
            self.prediction_start_time = timer()

    def on_predict_end(self) -> None:
        if not self.report_prediction_time:
            return
        torch.cuda.synchronize()
        elapsed = datetime.timedelta(seconds=timer() - self.prediction_start_time)
        h = self.hparams
        dm = getattr(self.trainer, "datamodule", None)
        report = {
            "algorithm": h.generation,
            "batch_size": getattr(dm, "batch_size", None),
            "tgt_test_path": str(getattr(dm, "tgt_test_path", None)),
            "max_len": h.max_len,
            "total_seconds": round(elapsed.total_seconds(), 4),
            "model_calls": self.generator.model_calls_num,
            "seconds_per_model_call": round(elapsed.total_seconds() / max(1, self.generator.model_calls_num), 4),
        }
        if h.generation in ("greedy_speculative", "beam_search_speculative"):
            report["n_drafts"] = h.n_drafts
            report["draft_len"] = h.draft_len
            if h.generation == "beam_search_speculative":
                report["accepted_tokens"] = self.generator.accepted_tokens_num
                report["acceptance_rate"] = round(self.generator.accepted_tokens_num /
                                                  max(1, self.generator.produced_non_pad_tokens), 4)
        if h.generation == "sampling_speculative":
            report["n_drafts"] = h.n_drafts
            report["draft_len"] = h.draft_len
            report["accepted_tokens"] = self.generator.accepted_tokens_num
            report["acceptance_rate"] = round(self.generator.accepted_tokens_num /
                                              max(1, self.generator.stats_total["produced_tokens"]), 4)
        if self._scores_on:
            report["scoring_seconds"] = round(self._scoring_seconds, 6)
            report["mean_top1_logprob"] = round(float(self._top1_sum) / max(1, self._top1_n), 6)
            report["unfinished_hypotheses"] = int(self._unfinished)
        if self._alternatives_k > 0:
            report["alternatives_seconds"] = round(self._alternatives_seconds, 6)
        if self._attention_on:
            report["attention_seconds"] = round(self._attention_seconds, 6)
        if self._fold_on:
            report["fold_seconds"] = round(self._fold_seconds, 6)
            report["distinct_hypotheses"] = int(self._distinct)
        if self._logq_on:
            report["logq_seconds"] = round(self._logq_seconds, 6)
            report["hypotheses_outside_support"] = int(self._outside)
        text = json.dumps(report)
        print(text)
        if h.report_prediction_file is not None:
            Path(h.report_prediction_file).parent.mkdir(exist_ok=True)
            with open(h.report_prediction_file, "a") as f:
                print(text, file=f)

    # -- teacher-forced evaluation (lightning_model.py:174-207) ---------------------------------------
    def _teacher_forced(self, batch: Any, return_logits: bool):
        if self.native is None:
            self.build_native()
        return self.native.teacher_forced(batch["src_tokens"], batch["tgt_tokens"], return_logits=return_logits,
                                          eos_token_idx=self.tgt_eos_token_i)

    def _log_metrics(self, stage: str, r, batch_size: int) -> None:
        # the reference's names and flags; batch_size is what Lightning infers from the batch (its first tensor, src_tokens)
        self.log(f"{stage}/loss", r.loss, on_step=False, on_epoch=True, prog_bar=True, batch_size=batch_size)
        self.log(f"{stage}/acc_single_tok", r.token_acc, on_step=False, on_epoch=True, prog_bar=False, batch_size=batch_size)
        self.log(f"{stage}/acc_sequence", r.seq_acc, on_step=False, on_epoch=True, prog_bar=False, batch_size=batch_size)

    def validation_step(self, batch: Any, batch_idx: int) -> Any:
        r = self._teacher_forced(batch, return_logits=False)
        self._log_metrics("val", r, batch["src_tokens"].shape[0])
        return {"pred_tokens": r.pred_tokens, "target_ahead": batch["tgt_tokens"][:, 1:]}

    def test_step(self, batch: Any, batch_idx: int) -> Any:
        r = self._teacher_forced(batch, return_logits=True)
        self._log_metrics("test", r, batch["src_tokens"].shape[0])
        return {"source_token_ids": batch["src_tokens"], "pred_logits": r.logits, "target_token_ids": batch["tgt_tokens"]}

    # -- out of scope ------------------------------------------------------------
    def training_step(self, *a, **k):
        raise NotImplementedError("training is outside the MI355X inference path; train with the reference")


def run_predict(module: VanillaEncoderDecoderTransformerLightning, batches, writer=None, datamodule=None,
                schedule: str = "rows", window: int = 256, in_flight: int = 8) -> list:
    """Stand-in for ``Trainer.predict`` when pytorch_lightning is absent: the same hook order and nothing else
    (on_predict_start -> predict_step per batch -> writer.write_on_batch_end -> on_predict_end), with a trainer object that
    exposes ``predict_dataloaders`` and ``datamodule`` like Lightning's.  ``schedule="batches"`` switches the module's
    look-ahead off (every batch is decoded inside its own predict_step, as in the reference)."""
    if schedule not in ("batches", "rows"):
        raise ValueError("schedule must be 'batches' or 'rows'")
    batches = list(batches)
    module.trainer = SimpleNamespace(datamodule=datamodule, predict_dataloaders=batches)
    module.predict_window = window if schedule == "rows" else 0
    old_inflight = os.environ.get("TTX_INFLIGHT")
    os.environ["TTX_INFLIGHT"] = str(in_flight)
    outs = []
    try:
        with torch.inference_mode():
            module.on_predict_start()
            for i, batch in enumerate(batches):
                pred = module.predict_step(batch, i)
                if writer is not None:
                    writer.write_on_batch_end(module.trainer, module, pred, None, batch, i, 0)
                outs.append(pred)
            module.on_predict_end()
    finally:
        if old_inflight is None:
            os.environ.pop("TTX_INFLIGHT", None)
        else:
            os.environ["TTX_INFLIGHT"] = old_inflight
    return outs


def run_evaluate(module: VanillaEncoderDecoderTransformerLightning, batches, stage: str = "validate", callbacks=()) -> dict:
    """Stand-in for ``Trainer.validate`` / ``Trainer.test`` when pytorch_lightning is absent: Lightning's hook order
    (on_{stage}_start, on_{stage}_epoch_start, then per batch on_{stage}_batch_start -> {stage}_step -> the callbacks'
    on_{stage}_batch_end, then the callbacks' on_{stage}_epoch_end, on_{stage}_epoch_end, on_{stage}_end; hooks the module does
    not define are skipped) and Lightning's reduction of ``on_epoch=True`` logs: the mean over the batches weighted by each
    batch's size (``src_tokens.shape[0]``).  Returns {name: epoch value} as floats; metrics the callbacks send to
    ``trainer.logger.log_metrics`` are kept in ``module.trainer.logger.metrics``."""
    if stage not in ("validate", "test"):
        raise ValueError("stage must be 'validate' or 'test'")
    hook = "validation" if stage == "validate" else "test"
    step = getattr(module, f"{hook}_step")
    logger = SimpleNamespace(metrics={})
    logger.log_metrics = lambda metrics, step=None: logger.metrics.update(metrics)
    module.trainer = SimpleNamespace(logger=logger, datamodule=None)

    def call(obj, name, *args):
        fn = getattr(obj, name, None)
        if fn is not None:
            fn(*args)

    module.logged = []
    with torch.inference_mode():
        call(module, f"on_{hook}_start")
        call(module, f"on_{hook}_epoch_start")
        for i, batch in enumerate(batches):
            module._current_batch_size = int(batch["src_tokens"].shape[0])
            call(module, f"on_{hook}_batch_start", batch, i)
            out = step(batch, i)
            for cb in callbacks:
                call(cb, f"on_{hook}_batch_end", module.trainer, module, out, batch, i)
        for cb in callbacks:
            call(cb, f"on_{hook}_epoch_end", module.trainer, module)
        call(module, f"on_{hook}_epoch_end")
        call(module, f"on_{hook}_end")
    module._current_batch_size = None
    sums, sizes = {}, {}
    for name, value, bs, flags in module.logged:
        if not flags.get("on_epoch", False):
            continue
        v = torch.as_tensor(value).detach().double().cpu().item()
        sums[name] = sums.get(name, 0.0) + v * bs
        sizes[name] = sizes.get(name, 0) + bs
    return {name: sums[name] / sizes[name] for name in sums}
