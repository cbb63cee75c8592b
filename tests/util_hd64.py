"""Loaders of the head-dimension-64 fixtures (tests/golden/hd64_*, written by tests/golden/make_golden_hd64.py): the reference's
own 2+2-layer model with d = 128 and 2 heads, trained on the ten fixture pairs."""
from __future__ import annotations

import functools
import json

from util_models import GOLDEN, load_npz


@functools.lru_cache(maxsize=None)
def hd64_state() -> tuple[dict, dict]:
    """(state dict joined from its parts, config)."""
    cfg = json.loads((GOLDEN / "hd64_config.json").read_text())
    st = {}
    for i in range(cfg["weight_parts"]):
        st.update(load_npz(f"hd64_weights_{i}.npz"))
    assert cfg["embedding_dim"] // cfg["num_heads"] == 64 and sum(v.size for v in st.values()) == 543006
    return st, cfg


def hd64_gen(prefix: str) -> dict:
    """The arrays of one generator in hd64_gen.npz ('greedy', 'beam', 'spec_greedy', 'spec_beam'), prefix stripped."""
    z = load_npz("hd64_gen.npz")
    return {k[len(prefix) + 2:]: v for k, v in z.items() if k.startswith(prefix + "__")}


BATCHES, NS, DS, BEAM = (1, 4, 10), (1, 3, 7), (5, 10), 5
