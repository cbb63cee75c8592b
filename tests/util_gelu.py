"""The GELU side of the test suite: the float64 yardstick and the element-wise bound of the exact (erf) GELU, an oracle whose
feed-forward uses it, and the loaders of the GELU fixtures (tests/golden/gelu_*, written by tests/golden/make_golden_gelu.py:
the reference's own 2+2-layer model with d = 64, 2 heads, F = 128 and activation="gelu", trained on the ten fixture pairs)."""
from __future__ import annotations

import functools
import json
import math

import torch
import torch.nn.functional as F

from oracle.model import OracleTransformer
from util_models import GOLDEN, load_npz

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2       # enum ttx_activation (include/ttx.h)
GELU_MAX_SLOPE = 1.13                        # the largest |gelu'(x)| is 1.129 (at x = sqrt 2)


def gelu64(x: torch.Tensor) -> torch.Tensor:
    """The yardstick: 0.5 x (1 + erf(x / sqrt 2)) in float64 — written as 0.5 x erfc(-x / sqrt 2), the same function without the
    cancellation of 1 + erf in the negative tail, so that the yardstick itself is good to a few float64 ulps everywhere."""
    x = x.to(torch.float64)
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))


def act_bound(x: torch.Tensor) -> torch.Tensor:
    """A(x) = 4 * 2^-23 * max(1, |x|): what one fp32 evaluation of the exact GELU may differ from gelu64 by.  ABSOLUTE in
    max(1, |x|), not relative to gelu(x): 1 + erf(x / sqrt 2) is formed near 1, so in the negative tail (gelu(-5) = -1.4e-6) fp32
    keeps little relative accuracy — its results there are multiples of |x| 2^-25 — while the absolute error stays at the size of an
    ulp of x."""
    return 4.0 * 2.0 ** -23 * x.to(torch.float64).abs().clamp_min(1.0)


class GeluOracleTransformer(OracleTransformer):
    """OracleTransformer with the exact GELU in the feed-forward (the only place the activation occurs)."""

    def _ffn(self, prefix: str, x: torch.Tensor) -> torch.Tensor:
        h = F.gelu(x @ self.w[prefix + ".linear1.weight"].T + self.w[prefix + ".linear1.bias"])
        return h @ self.w[prefix + ".linear2.weight"].T + self.w[prefix + ".linear2.bias"]


@functools.lru_cache(maxsize=None)
def gelu_state() -> tuple[dict, dict]:
    """(state dict joined from its parts, config)."""
    cfg = json.loads((GOLDEN / "gelu_config.json").read_text())
    st = {}
    for i in range(cfg["weight_parts"]):
        st.update(load_npz(f"gelu_weights_{i}.npz"))
    assert cfg["activation"] == "gelu"
    return st, cfg


def gelu_gen(prefix: str) -> dict:
    """The arrays of one generator in gelu_gen.npz ('greedy', 'beam', 'spec_greedy', 'spec_beam'), prefix stripped."""
    z = load_npz("gelu_gen.npz")
    return {k[len(prefix) + 2:]: v for k, v in z.items() if k.startswith(prefix + "__")}


BATCHES, NS, DS, BEAM = (1, 4, 10), (1, 3, 7), (5, 10), 5
