"""Teacher-forced evaluation on the MI355X (ttx_token_metrics / ttx_teacher_forced_eval, NativeTransformer.teacher_forced,
validation_step / test_step / run_evaluate) against the reference's own metrics (tests/golden/eval_metrics.npz, made by
tests/golden/make_golden_eval.py) and a torch restatement of them."""
import json

import numpy as np
import pytest
import torch

from util_models import GOLDEN, PAD, EOS, fixture_tokens, full_state, tiny_state, load_npz
from util_eval import golden_cases, reference_metrics, same_float

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-4     # a position whose argmax differs must have a reference top-2 gap below this (the parity checks' rule)


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def tiny(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)


def exact_loss(logits: np.ndarray, tgt: np.ndarray) -> float:
    """The mean cross-entropy in float64 (what the fp32 evaluations approximate)."""
    x = torch.from_numpy(np.asarray(logits)).double()
    t = torch.from_numpy(np.asarray(tgt))[:, 1:]
    return float((torch.logsumexp(x, -1) - x.gather(-1, t.unsqueeze(-1)).squeeze(-1)).mean())


def _check_metrics(r, ref: dict, label: str, logits: np.ndarray, tgt: np.ndarray) -> None:
    """Accuracies bit-exact; loss within 1e-6 relative of the reference's.  The reference's fp32 value carries its own rounding
    (1.8e-6 relative on the tiny model's confident positions, where every nll is log of a softmax sum next to 1.0): the kernel
    is held to 1e-6 relative of the float64 value, and to the reference's within 1e-6 relative plus the reference's own error."""
    loss, tok, seq = (float(v) for v in torch.stack([r.loss, r.token_acc, r.seq_acc]).cpu())
    exact = exact_loss(logits, tgt)
    ref_loss = float(ref["loss"])
    print(f"{label}: loss {loss:.9g} (ref {ref_loss:.9g}, float64 {exact:.9g})  token_acc {tok} (ref {ref['token_acc']})  "
          f"seq_acc {seq} (ref {ref['seq_acc']})")
    assert same_float(tok, ref["token_acc"]), label
    assert same_float(seq, ref["seq_acc"]), label
    assert abs(loss - exact) <= 1e-6 * abs(exact), label
    assert abs(loss - ref_loss) <= 1e-6 * abs(ref_loss) + abs(ref_loss - exact), label


@pytest.mark.parametrize("name", list(golden_cases()))
def test_token_metrics_on_golden_logits(tiny, name):
    c = golden_cases()[name]
    logits, tgt = torch.from_numpy(c["logits"]).cuda(), torch.from_numpy(c["tgt"]).cuda()
    r = tiny.token_metrics(logits, tgt, int(c["eos"]))
    pred = r.pred_tokens.cpu()
    assert r.pred_tokens.dtype == torch.int64 and pred.shape == tgt[:, 1:].shape
    assert torch.equal(pred, torch.from_numpy(c["pred"]))
    assert torch.equal(pred, torch.from_numpy(c["logits"]).argmax(-1))
    _check_metrics(r, c, name, c["logits"], c["tgt"])
    nll_ref = torch.nn.functional.cross_entropy(torch.from_numpy(c["logits"]).flatten(0, 1), torch.from_numpy(c["tgt"])[:, 1:].flatten(),
                                                reduction="none").reshape(pred.shape)
    assert (r.token_nll.cpu() - nll_ref).abs().max().item() <= 1e-5 * max(1.0, nll_ref.abs().max().item())


@pytest.mark.parametrize("name", ["ties_v64", "v1024", "example_v12"])
def test_token_metrics_unaligned_logits_take_the_scalar_path_with_equal_results(tiny, name):
    """V % 4 == 0 but a base that is not 16-byte aligned: the per-column loop instead of float4 loads, same results."""
    c = golden_cases()[name]
    x = torch.from_numpy(c["logits"]).cuda()
    tgt = torch.from_numpy(c["tgt"]).cuda()
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")
    buf[1:] = x.reshape(-1)
    shifted = buf[1:].view(x.shape)
    assert shifted.data_ptr() % 16 != 0
    a = tiny.token_metrics(x, tgt, int(c["eos"]))
    b = tiny.token_metrics(shifted, tgt, int(c["eos"]))
    assert torch.equal(a.pred_tokens, b.pred_tokens)
    # the lanes see the columns in another grouping: the sums may differ in the last bits, the accuracies may not
    assert torch.equal(torch.stack([a.token_acc, a.seq_acc]).nan_to_num(-1.0), torch.stack([b.token_acc, b.seq_acc]).nan_to_num(-1.0))
    assert abs(float(a.loss) - float(b.loss)) <= 1e-6 * abs(float(a.loss))
    assert torch.allclose(a.token_nll, b.token_nll, rtol=1e-6, atol=1e-7)


def _near_tie_pred_check(pred: torch.Tensor, ref_logits: torch.Tensor, label: str) -> int:
    """pred equals the reference argmax except at positions whose reference top-2 gap is below NEAR_TIE."""
    ref_pred = ref_logits.argmax(-1)
    diff = pred != ref_pred
    if diff.any():
        top2 = ref_logits[diff].topk(2, dim=-1).values
        gaps = (top2[:, 0] - top2[:, 1]).abs()
        print(f"{label}: {int(diff.sum())} positions differ at near-ties, gaps {gaps.tolist()}")
        assert (gaps < NEAR_TIE).all(), label
    return int(diff.sum())


def _check_teacher_forced(native, src, tgt, ref_logits, eos, label, loss_tol=1e-4):
    r = native.teacher_forced(src.cuda(), tgt.cuda(), return_logits=True, eos_token_idx=eos)
    pred = r.pred_tokens.cpu()
    _near_tie_pred_check(pred, ref_logits, label)
    ref = reference_metrics(ref_logits, tgt, eos)
    loss = float(r.loss)
    print(f"{label}: loss {loss:.7g} ref {ref['loss']:.7g}")
    assert abs(loss - ref["loss"]) <= loss_tol
    # accuracies: exactly the reference's metrics of the native prediction (= of the reference argmax where none differs)
    mine = reference_metrics(ref_logits, tgt, eos, pred=pred)
    assert same_float(float(r.token_acc), mine["token_acc"]) and same_float(float(r.seq_acc), mine["seq_acc"]), label
    # the logits handed out are those of the forward pass: ttx_forward(src, tgt[:, :-1]), bit for bit
    fwd = native(src.cuda(), tgt[:, :-1].contiguous().cuda())
    assert torch.equal(r.logits, fwd)
    assert (r.logits.cpu() - ref_logits).abs().max().item() < 1e-3
    return r, ref


def test_teacher_forced_tiny_matches_reference(tiny):
    c = golden_cases()["tiny"]
    src, tgt, _, _ = fixture_tokens()
    assert np.array_equal(tgt.numpy(), c["tgt"])
    r, ref = _check_teacher_forced(tiny, src, tgt, torch.from_numpy(c["logits"]), EOS, "tiny")
    assert same_float(ref["token_acc"], c["token_acc"]) and same_float(ref["seq_acc"], c["seq_acc"])
    # without return_logits: the same results, no logits
    r2 = tiny.teacher_forced(src.cuda(), tgt.cuda())
    assert r2.logits is None
    assert torch.equal(r2.pred_tokens, r.pred_tokens) and torch.equal(r2.token_nll, r.token_nll)
    assert torch.equal(torch.stack([r2.loss, r2.token_acc, r2.seq_acc]), torch.stack([r.loss, r.token_acc, r.seq_acc]))


def test_teacher_forced_full_size_matches_oracle(tta, trained_full_state):
    from oracle.model import OracleTransformer, config_from_state
    st = trained_full_state(4)
    native = tta.NativeTransformer(st, 8, 0, device=0)
    oracle = OracleTransformer(config_from_state(st, 8), st)
    src, tgt, _, _ = fixture_tokens()
    with torch.inference_mode():
        ref_logits = oracle(src, tgt[:, :-1]).float()
    _check_teacher_forced(native, src, tgt, ref_logits, EOS, "full 4+4")


def test_teacher_forced_is_bit_identical_from_call_to_call(tiny):
    src, tgt, _, _ = fixture_tokens()
    a = tiny.teacher_forced(src.cuda(), tgt.cuda())
    b = tiny.teacher_forced(src.cuda(), tgt.cuda())
    assert torch.equal(a.token_nll, b.token_nll) and torch.equal(a.pred_tokens, b.pred_tokens)
    assert torch.equal(torch.stack([a.loss, a.token_acc, a.seq_acc]), torch.stack([b.loss, b.token_acc, b.seq_acc]))


def test_bench_shaped_batch_matches_forward_plus_torch_metrics(tta):
    """bs = 32 MIT-shaped synthetic reactions (tools/synth.py) on the 4+4 d=256 model with V = 256 (float4 path): the metrics of
    teacher_forced equal the reference's metrics restated in torch over the logits of __call__."""
    from tools.synth import SynthReactions, pad_batch, V
    native = tta.NativeTransformer(full_state(V, 77), 8, 0, device=0)
    src_rows, tgt_rows = SynthReactions(seed=2024).dataset(32)
    src, tgt = torch.from_numpy(pad_batch(src_rows)), torch.from_numpy(pad_batch(tgt_rows))
    r = native.teacher_forced(src.cuda(), tgt.cuda())
    logits = native(src.cuda(), tgt[:, :-1].contiguous().cuda()).cpu()
    ref = reference_metrics(logits, tgt, EOS)
    assert torch.equal(r.pred_tokens.cpu(), ref["pred"])
    _check_metrics(r, ref, f"synth bs=32 Lt={tgt.shape[1]}", logits.numpy(), tgt.numpy())
    assert tgt.shape[0] == 32 and not np.isnan(ref["seq_acc"])      # every synthetic target ends in EOS


def test_rejects_bad_inputs(tiny, tta):
    src, tgt, _, V = fixture_tokens()
    bad = tgt.clone()
    bad[0, 3] = V
    with pytest.raises(IndexError):
        tiny.teacher_forced(src.cuda(), bad.cuda())
    with pytest.raises(ValueError):
        tiny.teacher_forced(src.cuda(), tgt[:, :1].cuda())
    N = tta._native
    out = torch.empty(3, device="cuda")
    s, t = src.cuda(), tgt.cuda()
    stream = tiny._stream()
    assert tiny._lib.ttx_teacher_forced_eval(tiny.session, s.data_ptr(), 10, s.shape[1], t.data_ptr(), 1, EOS, None, None, None,
                                             out.data_ptr(), stream) == N.TTX_ERR_INVALID
    logits = torch.zeros((2, 3, 1025), device="cuda")
    assert tiny._lib.ttx_token_metrics(tiny.session, logits.data_ptr(), t.data_ptr(), 2, 4, 1025, EOS, None, None,
                                       out.data_ptr(), stream) == N.TTX_ERR_INVALID
    assert tiny._lib.ttx_teacher_forced_eval(tiny.session, s.data_ptr(), 10, s.shape[1], t.data_ptr(), 5002, EOS, None, None,
                                             None, out.data_ptr(), stream) == N.TTX_ERR_INVALID


# -- Lightning surface ------------------------------------------------------------------------------------------------
class FixtureTokenizer:
    """Shape of the reference's GenericTokenizer that the module and DecodingCallback use (tokenizer_base.py:16-94)."""
    pad_token_idx, bos_token_idx, eos_token_idx, unk_token_idx = 0, 1, 2, 3

    def __init__(self):
        self.decoder_dict = {int(k): v for k, v in json.loads((GOLDEN / "fixture_vocab.json").read_text()).items()}
        self.encoder_dict = {v: k for k, v in self.decoder_dict.items()}

    @property
    def n_tokens(self):
        return len(self.encoder_dict)

    def decode(self, tokens):
        out = []
        for i in tokens:
            i = int(i)
            if i not in (self.bos_token_idx, self.eos_token_idx, self.pad_token_idx):
                out.append(self.decoder_dict[i])
            if i == self.eos_token_idx:
                break
        return "".join(out)


class DecodingCallback:
    """What src/callbacks.py:9-38 does with validation_step's outputs."""

    def __init__(self):
        self.validation_step_outputs = []

    def on_validation_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, dataloader_idx=0):
        self.validation_step_outputs.append(outputs)

    def on_validation_epoch_end(self, trainer, pl_module):
        tkz = pl_module.tgt_tokenizer
        total_correct, total = 0, 0
        for o in self.validation_step_outputs:
            pred_tokens = o["pred_tokens"].cpu().numpy()
            target_ahead = o["target_ahead"].cpu().numpy()
            for i in range(pred_tokens.shape[0]):
                total_correct += int(tkz.decode(pred_tokens[i]) == tkz.decode(target_ahead[i]))
                total += 1
        trainer.logger.log_metrics({"val/whole_seq_exact_match_acc_total": total_correct / total})
        self.validation_step_outputs.clear()


def _module(tta, st, cfg):
    tkz = FixtureTokenizer()
    mod = tta.VanillaEncoderDecoderTransformerLightning(
        src_tokenizer=tkz, tgt_tokenizer=tkz, embedding_dim=cfg["embedding_dim"], feedforward_dim=cfg["feedforward_dim"],
        num_encoder_layers=cfg["num_encoder_layers"], num_decoder_layers=cfg["num_decoder_layers"],
        num_heads=cfg["num_heads"], share_embeddings=True, generation="greedy", max_len=150)
    missing, unexpected = mod.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    assert not missing and not unexpected
    return mod


def test_validation_and_test_step_surface(tta):
    st, cfg = tiny_state()
    mod = _module(tta, st, cfg)
    src, tgt, _, V = fixture_tokens()
    batch = {"src_tokens": src[:4].cuda(), "tgt_tokens": tgt[:4].cuda()}
    mod.logged = []
    out = mod.validation_step(batch, 0)                      # builds the native model on first use
    assert mod.native is not None
    assert set(out) == {"pred_tokens", "target_ahead"}
    assert out["pred_tokens"].shape == (4, tgt.shape[1] - 1) and out["pred_tokens"].dtype == torch.int64
    assert torch.equal(out["target_ahead"], batch["tgt_tokens"][:, 1:])
    logged = {name: (value, bs, flags) for name, value, bs, flags in mod.logged}
    assert list(logged) == ["val/loss", "val/acc_single_tok", "val/acc_sequence"]
    assert logged["val/loss"][2] == dict(on_step=False, on_epoch=True, prog_bar=True)
    assert logged["val/acc_single_tok"][2] == dict(on_step=False, on_epoch=True, prog_bar=False)
    assert logged["val/acc_sequence"][2] == dict(on_step=False, on_epoch=True, prog_bar=False)
    assert all(bs == 4 for _, bs, _ in logged.values())
    c = golden_cases()["tiny"]
    ref = reference_metrics(torch.from_numpy(c["logits"][:4]), tgt[:4], EOS)
    assert abs(float(logged["val/loss"][0]) - ref["loss"]) < 1e-4
    assert same_float(float(logged["val/acc_single_tok"][0]), ref["token_acc"])
    assert same_float(float(logged["val/acc_sequence"][0]), ref["seq_acc"])

    mod.logged = []
    out = mod.test_step(batch, 0)
    assert set(out) == {"source_token_ids", "pred_logits", "target_token_ids"}
    assert out["pred_logits"].shape == (4, tgt.shape[1] - 1, V)
    assert torch.equal(out["source_token_ids"], batch["src_tokens"]) and torch.equal(out["target_token_ids"], batch["tgt_tokens"])
    assert (out["pred_logits"].cpu() - torch.from_numpy(c["logits"][:4])).abs().max().item() < 1e-3
    assert [n for n, _, _, _ in mod.logged] == ["test/loss", "test/acc_single_tok", "test/acc_sequence"]
    assert float(mod.logged[0][1]) == float(logged["val/loss"][0])

    with pytest.raises(NotImplementedError):
        mod.training_step(batch, 0)


@pytest.mark.parametrize("stage", ["validate", "test"])
def test_run_evaluate_weights_batches_like_lightning(tta, trained_full_state, stage):
    """Batches of unequal size: the epoch value is the batch-size-weighted mean of the per-batch values (Lightning's
    on_epoch=True reduction); DecodingCallback's exact-match rate over validation_step's outputs."""
    st = trained_full_state(4)
    cfg = dict(embedding_dim=256, feedforward_dim=2048, num_encoder_layers=4, num_decoder_layers=4, num_heads=8)
    mod = _module(tta, {k: v.numpy() for k, v in st.items()}, cfg)
    src, tgt, _, _ = fixture_tokens()
    cuts = [(0, 3), (3, 8), (8, 10)]
    batches = []
    for a, b in cuts:
        s, t = src[a:b], tgt[a:b]
        s = s[:, :int((s != PAD).sum(1).max())]       # each batch padded to its own longest row, like the collate
        t = t[:, :int((t != PAD).sum(1).max())]
        batches.append({"src_tokens": s.cuda(), "tgt_tokens": t.cuda()})
    cb = DecodingCallback()
    epoch = tta.run_evaluate(mod, batches, stage=stage, callbacks=[cb])
    prefix = "val" if stage == "validate" else "test"
    per = [mod.native.teacher_forced(b["src_tokens"], b["tgt_tokens"]) for b in batches]
    sizes = [b - a for a, b in cuts]
    for key, attr in (("loss", "loss"), ("acc_single_tok", "token_acc"), ("acc_sequence", "seq_acc")):
        want = sum(float(getattr(r, attr)) * n for r, n in zip(per, sizes)) / sum(sizes)
        assert abs(epoch[f"{prefix}/{key}"] - want) <= 1e-12 * max(1.0, abs(want)), key
    assert set(epoch) == {f"{prefix}/loss", f"{prefix}/acc_single_tok", f"{prefix}/acc_sequence"}
    if stage == "validate":
        tkz = mod.tgt_tokenizer
        want = np.mean([tkz.decode(r.pred_tokens[i].cpu().numpy()) == tkz.decode(b["tgt_tokens"][i, 1:].cpu().numpy())
                        for r, b in zip(per, batches) for i in range(b["tgt_tokens"].shape[0])])
        assert mod.trainer.logger.metrics["val/whole_seq_exact_match_acc_total"] == want
        print("exact-match rate", want, "epoch", epoch)
