"""CPU-side checks of what the GELU tests on the GPU rest on (tests/util_gelu.py): the float64 yardstick gelu64 and the
element-wise bound A(x) = 4 * 2^-23 * max(1, |x|) admit a correct fp32 evaluation of the exact GELU — torch's own, the
hand-written 0.5 x (1 + erf(x / sqrt 2)), and the order the kernels pin (csrc/ttx_common.hip.h: gelu_erf) — and reject the
functions a wrong epilogue would compute instead.  And: an activation the library does not have is a ValueError, not a GPU call.

fp32 loses its RELATIVE accuracy in the negative tail: 1 + erf is formed on the grid of 2^-24 below 1, so gelu(-5) = -1.43e-6 comes
out as a multiple of 2.5 * 2^-24 = 1.49e-7, per cent away from the true value.  That is why the bound is absolute in max(1, |x|)."""
import math

import pytest
import torch
import torch.nn.functional as F

from util_gelu import act_bound, gelu64

SQRT1_2 = 0.70710678118654752440


def sweep() -> torch.Tensor:
    return torch.arange(-12 * 4096, 12 * 4096 + 1, dtype=torch.float64).div(4096).to(torch.float32)


def big_sweep() -> torch.Tensor:
    """3 million points: 2 million normal samples with sigma = 3 and 1 million points on [-12, 12]."""
    gen = torch.Generator().manual_seed(20261017)
    return torch.cat([torch.randn(2_000_000, generator=gen, dtype=torch.float32) * 3.0,
                      torch.linspace(-12.0, 12.0, 1_000_000, dtype=torch.float64).to(torch.float32)])


def used(y: torch.Tensor, x: torch.Tensor) -> float:
    """Largest |y - gelu64(x)| / A(x); NaN and Inf count as infinitely far."""
    err = (y.to(torch.float64) - gelu64(x)).abs()
    err = torch.where(torch.isfinite(y.to(torch.float64)), err, torch.full_like(err, float("inf")))
    return float((err / act_bound(x)).max())


def handwritten32(x: torch.Tensor) -> torch.Tensor:
    """0.5 * x * (1 + erf(x / sqrt 2)), every operation rounded to fp32."""
    return 0.5 * x * (1.0 + torch.erf(x * SQRT1_2))


def pinned32(x: torch.Tensor) -> torch.Tensor:
    """The kernels' order: t = x * fl(1 / sqrt 2); e = erf(t); h = 0.5 x; y = fma(h, e, h) — the fma emulated in float64 (the
    product of two fp32 numbers is exact there)."""
    e = torch.erf(x * SQRT1_2)
    h = 0.5 * x
    return (h.to(torch.float64) * e.to(torch.float64) + h.to(torch.float64)).to(torch.float32)


def test_yardstick_agrees_with_the_definition():
    """gelu64 (written with erfc) against 0.5 x (1 + erf(x / sqrt 2)) in float64 where that form is itself accurate, and against
    known values."""
    x = sweep().to(torch.float64)
    direct = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pos = x >= -1.0
    assert float((gelu64(x) - direct)[pos].abs().max()) < 1e-15 * 12
    assert abs(float(gelu64(torch.tensor(1.0))) - 0.8413447460685429) < 1e-15
    assert abs(float(gelu64(torch.tensor(-5.0))) - (-1.4332578589e-06)) < 1e-15
    assert float(gelu64(torch.tensor(0.0))) == 0.0


def test_torch_fp32_gelu_is_inside_the_bound():
    x = sweep()
    u = used(F.gelu(x), x)
    print(f"torch fp32 F.gelu on [-12, 12] in steps of 1/4096: used fraction of A {u:.3f}")
    assert u <= 1.0


def test_handwritten_and_pinned_fp32_are_inside_the_bound():
    x = big_sweep()
    uh, up = used(handwritten32(x), x), used(pinned32(x), x)
    print(f"3M-point sweep: hand-written fp32 uses {uh:.3f} of A, the kernels' pinned order {up:.3f}")
    assert uh <= 1.0 and up <= 1.0
    x = sweep()
    assert used(handwritten32(x), x) <= 1.0 and used(pinned32(x), x) <= 1.0


def test_relative_accuracy_is_lost_in_the_negative_tail():
    x = torch.tensor([-5.0])
    y, want = float(F.gelu(x)), float(gelu64(x))
    # thousands of fp32 roundoffs away in relative terms, yet a small fraction of A
    assert abs(y - want) / abs(want) > 1e-3 and used(F.gelu(x), x) <= 0.1


DEFECTS = {
    "tanh approximation": lambda x: F.gelu(x, approximate="tanh"),
    "x * sigmoid(1.702 x)": lambda x: x * torch.sigmoid(1.702 * x),
    "ReLU": torch.relu,
    "erf(x) without the 1 / sqrt 2": lambda x: 0.5 * x * (1.0 + torch.erf(x)),
    "no activation": lambda x: x,
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_defective_activations_are_outside_the_bound(name):
    x = sweep()
    u = used(DEFECTS[name](x), x)
    print(f"{name}: {u:.0f} x the bound")
    assert u > 100.0


def test_nan_and_inf_fail():
    x = torch.tensor([1.0, 2.0])
    assert used(torch.tensor([float("nan"), 1.9545]), x) == float("inf")
    assert used(torch.tensor([0.8413447, float("inf")]), x) == float("inf")


class _Tok:
    n_tokens, pad_token_idx, bos_token_idx, eos_token_idx = 30, 0, 1, 2
    encoder_dict = {"c": 5}


def test_unknown_activation_is_a_value_error_without_a_gpu():
    import translation_transformer_amd as tta
    from translation_transformer_amd import _native as N
    with pytest.raises(ValueError, match="relu.*gelu"):
        tta.VanillaEncoderDecoderTransformerLightning(_Tok(), _Tok(), embedding_dim=64, feedforward_dim=128, num_encoder_layers=1,
                                                      num_decoder_layers=1, num_heads=2, activation="swish")
    with pytest.raises(ValueError, match="relu.*gelu"):
        tta.NativeTransformer({}, 2, activation="swish")
    with pytest.raises(ValueError, match="relu.*gelu"):
        tta.dist.broadcast_model({}, 2, 0, 0, activation="tanh")
    assert (N.activation_code("relu"), N.activation_code("gelu")) == (N.TTX_ACT_RELU, N.TTX_ACT_GELU) == (1, 2)


def test_lightning_class_accepts_gelu_and_builds_gelu_layers():
    import translation_transformer_amd as tta
    m = tta.VanillaEncoderDecoderTransformerLightning(_Tok(), _Tok(), embedding_dim=64, feedforward_dim=128, num_encoder_layers=1,
                                                      num_decoder_layers=1, num_heads=2, activation="gelu")
    assert m.hparams.activation == "gelu"
    assert m.model.transformer.encoder.layers[0].activation is F.gelu and m.model.transformer.decoder.layers[0].activation is F.gelu
    r = tta.VanillaEncoderDecoderTransformerLightning(_Tok(), _Tok(), embedding_dim=64, feedforward_dim=128, num_encoder_layers=1,
                                                      num_decoder_layers=1, num_heads=2)
    assert r.model.transformer.encoder.layers[0].activation is F.relu
