#!/usr/bin/env python3
"""Generate the GELU fixtures under tests/golden/ from the REFERENCE implementation: a 2+2-layer model with d = 64, 2 heads,
F = 128 and activation="gelu" (the exact erf GELU of nn.TransformerEncoderLayer / nn.TransformerDecoderLayer), trained here on the
ten fixture pairs, and what the reference's model and its four generators give on it.  The model is constructed here:
make_golden.py's build_ref_model hard-codes "relu".

Runs ONLY in the build container, where the reference is mounted read-only; like make_golden_hd64.py, which it is modelled on, and
make_golden.py (imported for its loaders and its reference imports) it stores nothing but token ids, weights trained by this script and output arrays:

  gelu_config.json            the model's hyper-parameters ("activation": "gelu")
  gelu_weights_{0,...}.npz    the state dict, split by tensor so that every file stays below 1 MiB (tests/util_gelu.py joins them)
  gelu_model_io.npz           encode_src / decode_tgt / forward outputs (the arrays of tiny_model_io.npz)
  gelu_gen.npz                tokens and counters of the generators on make_golden.py's settings for the tiny model, on a reduced
                              grid: greedy__ (B in {1, 4, 10}, max_len 150 and 40), beam__ (beam 5), spec_greedy__ (N in {1, 3, 7},
                              D in {5, 10}, and the max_len 30 / 45 runs whose unfinished rows stay PAD), spec_beam__ (both draft
                              modes, fixture rows on which the reference's loop terminates)

Before it writes, the script asserts what the GPU tests rely on: the float32 GELU oracle (tests/util_gelu.py: the oracle
with F.gelu in its feed-forward) reproduces every reference token and every counter exactly (so no beam hypothesis needs the near-tie rule of tests/test_gpu_beam_native.py), and the float64 oracle's
smallest lead between its two best logits along the ten target paths is printed and stored (gelu_model_io.npz: min_lead).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gelu.py
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import make_golden as MG  # noqa: E402  (puts the reference's src/ on sys.path)
from make_golden import (PAD, BOS, EOS, TranslationInferenceGreedy, TranslationInferenceBeamSearch,  # noqa: E402
                         TranslationInferenceGreedySpeculative, TranslationInferenceBeamSearchSpeculative, trim_np)

GELU = dict(num_encoder_layers=2, num_decoder_layers=2, embedding_dim=64, num_heads=2, feedforward_dim=128)
PART_BYTES = 900 * 1024
BATCHES, NS, DS, BEAM = (1, 4, 10), (1, 3, 7), (5, 10), 5
# beam-speculative: (first rows that terminate, batch size, n_best, n_drafts, draft_len)
SPEC_BEAM = [(4, 4, 5, 7, 10), (8, 4, 5, 3, 10), (10, 2, 3, 2, 5), (3, 3, 2, 1, 3)]


def train():
    src, tgt, _, V = MG.fixture_tokens()
    torch.manual_seed(123456)
    model = MG.VanillaTransformer(V, V, GELU["num_encoder_layers"], GELU["num_decoder_layers"], GELU["embedding_dim"],
                                  GELU["num_heads"], GELU["feedforward_dim"], 0.0, "gelu", True, PAD, PAD)
    opt = torch.optim.Adam(model.parameters(), lr=2e-3)
    crit = torch.nn.CrossEntropyLoss(reduction="mean")
    model.train()
    for step in range(4000):
        logits = model(src, tgt[:, :-1])
        loss = crit(logits.reshape(-1, V), tgt[:, 1:].reshape(-1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        if float(loss) < 2e-3:
            break
    model.eval()
    with torch.inference_mode():
        g = TranslationInferenceGreedy(model, 150, PAD, BOS, EOS).generate(src)
    ok = sum(int(torch.equal(g[i, 0, :int((tgt[i] != PAD).sum())], tgt[i, :int((tgt[i] != PAD).sum())])) for i in range(src.size(0)))
    n = sum(v.numel() for v in model.state_dict().values())
    print("gelu: final loss", float(loss), "steps", step, "greedy exact", ok, "/ 10,", n, "floats", flush=True)
    assert ok == 10
    return model, V


def write_weights(model, V):
    sd = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in model.state_dict().items()}
    parts, size = [{}], 0
    for k, v in sd.items():
        if size + v.nbytes > PART_BYTES and parts[-1]:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    for old in HERE.glob("gelu_weights_*.npz"):
        old.unlink()
    for i, p in enumerate(parts):
        np.savez_compressed(HERE / f"gelu_weights_{i}.npz", **p)
        assert (HERE / f"gelu_weights_{i}.npz").stat().st_size < 1024 * 1024
    (HERE / "gelu_config.json").write_text(json.dumps(dict(GELU, activation="gelu", vocab_size=V, share_embeddings=True, weight_parts=len(parts))))
    return sd


def oracles(sd):
    from oracle.model import config_from_state
    from util_gelu import GeluOracleTransformer
    cfg = config_from_state(sd, GELU["num_heads"])
    return GeluOracleTransformer(cfg, sd), GeluOracleTransformer(cfg, sd, dtype=torch.float64)


def model_io(m, o32, o64):
    src, tgt, _, V = MG.fixture_tokens()
    with torch.inference_mode():
        mask = src == PAD
        memory = m.encode_src(src, mask)
        logits = m.decode_tgt(tgt[:, :-1], memory, memory_pad_mask=mask)
        fwd = m(src, tgt[:, :1])
        tgt2 = tgt[:, :24].clone()                   # ragged decoder input, as the speculative loop feeds it
        for i in range(tgt2.size(0)):
            tgt2[i, 8 + i:] = PAD
        logits2 = m.decode_tgt(tgt2, memory, memory_pad_mask=mask)
    # the float64 oracle's lead along the target paths: what exact token identity of the greedy paths rests on
    lg64 = o64.decode_tgt(tgt[:, :-1], o64.encode_src(src, mask), mask)
    top2 = lg64.topk(2, -1).values
    real = tgt[:, 1:] != PAD
    assert torch.equal(lg64.argmax(-1)[real], tgt[:, 1:][real])
    min_lead = float((top2[..., 0] - top2[..., 1])[real].min())
    err32 = float((o32.decode_tgt(tgt[:, :-1], memory, mask) - logits).abs().max())
    print(f"model: memory {tuple(memory.shape)} logits {tuple(logits.shape)}; float32 oracle against the reference {err32:.2e}; "
          f"float64 oracle's smallest lead along the target paths {min_lead:.3f}", flush=True)
    assert err32 < 5e-5 and min_lead > 1.0
    np.savez_compressed(HERE / "gelu_model_io.npz", src=src.numpy(), tgt_in=tgt[:, :-1].numpy(), memory=memory.numpy(),
                        logits=logits.numpy(), fwd_bos=fwd.numpy(), tgt_ragged=tgt2.numpy(), logits_ragged=logits2.numpy(),
                        min_lead=np.float64(min_lead))


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    w = min(a.shape[-1], b.shape[-1])
    assert a.shape[:-1] == b.shape[:-1] and np.array_equal(a[..., :w], b[..., :w]) and not a[..., w:].any() and not b[..., w:].any(), what


def generators(m, o32, o64):
    from oracle.decoding import GreedyOracle, BeamSearchOracle, GreedySpeculativeOracle
    from oracle.spec_beam import BeamSearchSpeculativeOracle
    src, _, c_tok, V = MG.fixture_tokens()
    out = {}
    with torch.inference_mode():
        for bsz in BATCHES:
            for max_len in (150, 40):
                g, o = TranslationInferenceGreedy(m, max_len, PAD, BOS, EOS), GreedyOracle(o32, max_len, PAD, BOS, EOS)
                toks = [g.generate(src[i:i + bsz]) for i in range(0, 10, bsz)]
                for i, t in zip(range(0, 10, bsz), toks):
                    same(o.generate(src[i:i + bsz]).numpy(), t.numpy(), ("greedy", bsz, max_len, i))
                w = max(t.size(2) for t in toks)
                out[f"greedy__b{bsz}_m{max_len}_tokens"] = np.concatenate([np.pad(trim_np(t), ((0, 0), (0, 0), (0, w - t.size(2)))) for t in toks])
                out[f"greedy__b{bsz}_m{max_len}_calls"] = np.int64(g.model_calls_num)
                assert o.model_calls_num == g.model_calls_num
            g, o = TranslationInferenceBeamSearch(m, BEAM, 150, PAD, BOS, EOS), BeamSearchOracle(o32, BEAM, 150, PAD, BOS, EOS)
            for bi, i in enumerate(range(0, 10, bsz)):
                t = g.generate(src[i:i + bsz])
                assert np.array_equal(o.generate(src[i:i + bsz]).numpy(), t.numpy()), ("beam", bsz, bi)
                out[f"beam__b{bsz}_k{BEAM}_batch{bi}"] = trim_np(t)
            out[f"beam__b{bsz}_k{BEAM}_calls"] = np.int64(g.model_calls_num)
            assert o.model_calls_num == g.model_calls_num
            for N in NS:
                for D in DS:
                    g = TranslationInferenceGreedySpeculative(m, 150, D, N, PAD, BOS, EOS, c_tok)
                    toks = np.concatenate([trim_np(g.generate(src[i:i + bsz])) for i in range(0, 10, bsz)])
                    for oo in (o32, o64):
                        o = GreedySpeculativeOracle(oo, 150, D, N, PAD, BOS, EOS, c_tok)
                        assert np.array_equal(np.concatenate([o.generate(src[i:i + bsz]).numpy() for i in range(0, 10, bsz)]), toks), (bsz, N, D)
                        assert o.model_calls_num == g.model_calls_num
                    out[f"spec_greedy__b{bsz}_n{N}_d{D}_tokens"] = toks
                    out[f"spec_greedy__b{bsz}_n{N}_d{D}_calls"] = np.int64(g.model_calls_num)
        print("greedy, beam, greedy-speculative: the oracle reproduces every token and counter", flush=True)
        for max_len in (30, 45):                     # some rows never finish (quirk: they stay all-PAD)
            g = TranslationInferenceGreedySpeculative(m, max_len, 10, 3, PAD, BOS, EOS, c_tok)
            t = g.generate(src)
            o = GreedySpeculativeOracle(o32, max_len, 10, 3, PAD, BOS, EOS, c_tok)
            assert np.array_equal(o.generate(src).numpy(), t.numpy()) and o.model_calls_num == g.model_calls_num
            out[f"spec_greedy__short_m{max_len}_tokens"] = trim_np(t)
            out[f"spec_greedy__short_m{max_len}_calls"] = np.int64(g.model_calls_num)

        # beam-speculative: the reference loop does not terminate on every row of an overfit model (make_golden.py:
        # section_spec_beam), so it runs under a cap on decoder calls and the cases take the rows on which it ends
        real_decode, calls = m.decode_tgt, [0]

        class NotTerminating(Exception):
            pass

        def capped(*a, **k):
            calls[0] += 1
            if calls[0] >= 400:
                raise NotTerminating()
            return real_decode(*a, **k)

        m.decode_tgt = capped

        def make(smart, nbest, N, D):
            return TranslationInferenceBeamSearchSpeculative(m, max_len=150, n_best=nbest, draft_len=D, n_drafts=N, vocab_size=V,
                                                             smart_drafts_mode=smart, pad_token=PAD, bos_token=BOS, eos_token=EOS, C_token=c_tok)

        good = []
        for r in range(src.size(0)):
            ok = True
            for smart in (False, True):
                for _, _, nbest, N, D in SPEC_BEAM:
                    calls[0] = 0
                    sel = src[r:r + 1]
                    try:
                        make(smart, nbest, N, D).generate(sel[:, :int((sel != PAD).sum())])
                    except NotTerminating:
                        ok = False
            print("row", r, "terminates" if ok else "does NOT terminate", flush=True)
            if ok:
                good.append(r)
        assert len(good) >= 4, good
        n_hyp = 0
        for smart in (False, True):
            for ci, (n_rows, bsz, nbest, N, D) in enumerate(SPEC_BEAM):
                rows = good[:n_rows]
                g = make(smart, nbest, N, D)
                o = BeamSearchSpeculativeOracle(o32, 150, nbest, D, N, V, smart, PAD, BOS, EOS, c_tok, max_steps=400)
                key = f"spec_beam__smart{int(smart)}_case{ci}"
                out[f"{key}_rows"] = np.array(rows, dtype=np.int64)
                out[f"{key}_params"] = np.array([bsz, nbest, N, D], dtype=np.int64)
                nb = 0
                for bi, i in enumerate(range(0, len(rows), bsz)):
                    calls[0] = 0
                    sel = src[rows[i:i + bsz]]
                    sel = sel[:, :int((sel != PAD).sum(1).max())]
                    t = g.generate(sel)
                    # every hypothesis, exactly: no rank of any source needs the near-tie rule
                    assert np.array_equal(o.generate(sel).numpy(), t.numpy()), (key, bi)
                    n_hyp += t.shape[0] * t.shape[1]
                    out[f"{key}_batch{bi}"] = trim_np(t)
                    nb += 1
                out[f"{key}_nbatches"] = np.int64(nb)
                out[f"{key}_calls"] = np.int64(g.model_calls_num)
                out[f"{key}_accepted"] = np.int64(g.accepted_tokens_num)
                out[f"{key}_produced"] = np.int64(g.produced_non_pad_tokens)
                assert (o.model_calls_num, o.accepted_tokens_num, o.produced_non_pad_tokens) == \
                    (g.model_calls_num, g.accepted_tokens_num, g.produced_non_pad_tokens), key
                print(key, rows, (bsz, nbest, N, D), "calls", g.model_calls_num, "acc", g.accepted_tokens_num, g.produced_non_pad_tokens,
                      flush=True)
        m.decode_tgt = real_decode
        print("beam-speculative:", n_hyp, "hypotheses, the float32 oracle reproduces every one and every counter", flush=True)
    np.savez_compressed(HERE / "gelu_gen.npz", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    model, V = train()
    sd = write_weights(model, V)
    o32, o64 = oracles(sd)
    model_io(model, o32, o64)
    generators(model, o32, o64)
