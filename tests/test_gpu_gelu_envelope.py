"""The model envelope of tests/test_gpu_envelope.py under activation="gelu": its six seeded models (d64-F64, d128-F192,
d256-F2304, d256-F8192, d512-F512, d1024-F4096), its inputs, helpers and bars — logits within 1e-3 of the float64 oracle, encoder
memory within 1e-4, the same argmax where the oracle's lead exceeds 2e-3, at most 1 % of the positions left out — with the float64
GELU oracle (tests/util_gelu.py) as the yardstick.  The FFN1 launches of these models reach every GELU instantiation of the GEMM
kernels (F = 64 ... 8192 columns, K = d = 64 ... 1024).

The seeds are that module's: with each of them the float32 GELU oracle meets the bars (test_fp32_gelu_oracle_meets_the_bars, no
GPU) and the speculative decode of the last test runs 24 to 35 verify steps under GELU, so none had to be replaced.  On these
models GELU and ReLU logits differ by 0.2 to 0.6, hundreds of bars.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_envelope as E
from util_gelu import GeluOracleTransformer
from util_models import PAD, BOS, EOS

MODELS, IDS = E.MODELS, E.IDS


@functools.lru_cache(maxsize=None)
def oracle_of(name, dtype):
    from oracle.model import config_from_state
    st, heads, _ = E.state_of(name)
    return GeluOracleTransformer(config_from_state(st, heads), st, dtype=dtype)


@functools.lru_cache(maxsize=None)
def io_of(name):
    """The tokens of test_gpu_envelope.io_of and the float64 GELU oracle's outputs on them."""
    src, tgt, mask, _, _ = E.io_of(name)
    o64 = oracle_of(name, torch.float64)
    memory = o64.encode_src(src, mask)
    return src, tgt, mask, memory, o64.decode_tgt(tgt, memory, mask)


@pytest.mark.parametrize("name", IDS)
def test_fp32_gelu_oracle_meets_the_bars(name):
    src, tgt, mask, mem64, lg64 = io_of(name)
    o32 = oracle_of(name, torch.float32)
    d_mem = float((o32.encode_src(src, mask).double() - mem64)[~mask].abs().max())
    err, left_out = E.compare_logits(o32.decode_tgt(tgt, mem64.float(), mask), lg64, f"{name} float32 GELU oracle")
    relu = float((E.io_of(name)[4] - lg64).abs().max())
    print(f"{name}: float32 GELU oracle against float64: memory {d_mem:.3e}, logits {err:.3e}, positions left out {left_out:.1%}; "
          f"the ReLU logits differ by {relu:.2f}")
    assert d_mem < E.MEMORY_TOL
    assert relu > 100 * E.LOGIT_TOL            # a model that ran ReLU instead could not pass the tests below


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_encode_and_decode_match_the_fp64_gelu_oracle(tta, name):
    st, heads, _ = E.state_of(name)
    src, tgt, mask, mem64, lg64 = io_of(name)
    native = tta.NativeTransformer(st, heads, PAD, device=0, activation="gelu")
    mem = native.encode_src(src.cuda(), mask.cuda()).cpu()
    d_mem = float((mem.double() - mem64)[~mask].abs().max())
    assert float(mem[mask].abs().max()) == 0.0
    lg = native.decode_tgt(tgt.cuda(), mem64.float().cuda(), memory_pad_mask=mask.cuda()).cpu()
    err, left_out = E.compare_logits(lg, lg64, name)
    print(f"{name}: memory error {d_mem:.3e}, logits error {err:.3e}, logits absmax {float(lg64.abs().max()):.2f}, "
          f"positions left out {left_out:.1%}")
    assert d_mem < E.MEMORY_TOL
    native.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_speculative_decode_is_one_arithmetic_under_every_variant(tta, name, monkeypatch):
    """test_gpu_envelope's check of the same name on GELU models: snapshot logits, fronts and output tokens are bit-identical
    across the four step policies (every GEMM variant carries FFN1 once), and the snapshot logits of verify steps 1 and 3 lie within
    LOGIT_TOL of the float64 GELU oracle's full-prefix decode_tgt of the same token rows."""
    from oracle.drafting import make_drafts
    N_DRAFTS, DRAFT_LEN = E.N_DRAFTS, E.DRAFT_LEN
    st, heads, V = E.state_of(name)
    gen = torch.Generator().manual_seed(1 + sum(map(ord, name)))
    src = E.ragged(gen, [9, 6, 12, 7, 10], V, 12, eos=True)
    mask = src == PAD
    o64 = oracle_of(name, torch.float64)
    memory = o64.encode_src(src, mask)
    drafts = make_drafts(src[:, 1:], DRAFT_LEN, N_DRAFTS, 1, 200, EOS, PAD, E.C_TOKEN).numpy()
    first, worst = {}, 0.0
    for policy, (qkv_small, small, ffn2_slab) in E.POLICIES.items():
        monkeypatch.setenv("TTX_QKV_SMALL_ROWS", str(qkv_small))
        monkeypatch.setenv("TTX_SMALL_ROWS", str(small))
        monkeypatch.setenv("TTX_FFN2_SLAB_ROWS", str(ffn2_slab))
        native = tta.NativeTransformer(st, heads, PAD, device=0, activation="gelu")     # the variables are read when the session is created
        for step in (1, 3):
            g = tta.TranslationInferenceGreedySpeculative(native, E.MAX_LEN, DRAFT_LEN, N_DRAFTS, PAD, BOS, EOS, E.C_TOKEN)
            g.record_step = step
            out = g.generate(src.cuda()).cpu()
            snap = g.step_snapshot()
            assert snap["step"] == step and snap["logits"].shape[1] == 1 + N_DRAFTS * DRAFT_LEN
            if step not in first:
                first[step] = (policy, snap, out)
                for slot, b in enumerate(snap["rows"].tolist()):
                    f = int(snap["front"][b])
                    prefix = snap["gen"][b, :f + 1].astype(np.int64)
                    rows = torch.from_numpy(np.stack([np.concatenate([prefix, drafts[b, n]]) for n in range(N_DRAFTS)]))
                    ref = o64.decode_tgt(rows, memory[b:b + 1].expand(N_DRAFTS, -1, -1), mask[b:b + 1].expand(N_DRAFTS, -1))
                    for n in range(N_DRAFTS):
                        got = np.concatenate([snap["logits"][slot, :1], snap["logits"][slot, 1 + n * DRAFT_LEN:1 + (n + 1) * DRAFT_LEN]])
                        worst = max(worst, float(np.abs(got - ref[n, f:f + DRAFT_LEN + 1].numpy()).max()))
            else:
                p0, s0, out0 = first[step]
                for key in ("logits", "rows", "front", "gen"):
                    assert np.array_equal(snap[key].view(np.int32), s0[key].view(np.int32)), f"{name} step {step}: {key} under {policy} differs from {p0}"
                assert torch.equal(out, out0), f"{name}: output tokens under {policy} differ from {p0}"
        native.close()
    print(f"{name}: GELU verify-step logits (steps 1 and 3) against the float64 full-prefix oracle: max abs diff {worst:.3e}; "
          f"bit-identical under {', '.join(E.POLICIES)}")
    assert worst < E.LOGIT_TOL
