"""bench.py's plain run on one GPU: the headline alone (one run of the K timed steps, nothing beside it) and --dump-outputs
(the timed call's predictions, which must equal a per-batch decode of the same rows with the same weights)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_plain_run_times_the_steps_and_dumps_the_outputs(tmp_path):
    import translation_transformer_amd as tta
    sys.path.insert(0, str(ROOT))
    from tools.synth import SynthReactions, batches, PAD, BOS, EOS, C_TOK
    from tools.train_synth import train
    weights = ROOT / ".weights_cache" / "synth_mit_1500.pt"       # bench.py's own cache (made by build() on a GPU machine)
    if not weights.exists():                                      # no cache: a short training run gives usable weights
        weights = tmp_path / "w.pt"
        torch.save(train("mit", steps=200, device="cuda", verbose=False, n_train=4000), weights)
    steps, warmup, bs = 3, 1, 32
    out = tmp_path / "out"
    env = dict(os.environ, TTX_WEIGHTS=str(weights))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.strip().split("\n") if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["unit"] == "reactions/s" and line["higher_is_better"] is True and line["dtype"] == "f32" and line["value"] > 0
    assert line["steps"] == steps and line["warmup"] == warmup and line["config"]["reactions"] <= steps * bs
    assert line["repeats"]["n"] == 1
    assert line["ms_per_step"] == pytest.approx(1e3 * line["repeats"]["seconds_in_run_order"][0] / steps)
    for key in ("c3", "c4", "n_drafts_1", "one_batch_at_a_time", "batches_as_given_in_flight", "predict_step_surface",
                "smiles_pipeline", "roofline", "cpu_baseline", "parity"):
        assert key not in line, key                                  # --full only
    got, rows = np.load(out / "predictions.npy"), np.load(out / "rows.npy")
    assert got.dtype == np.float32 and rows.dtype == np.float64
    assert got.shape == (steps * bs, 1, 200) and np.array_equal(rows, np.arange(steps * bs))
    # the same rows, one batch at a time
    sd = torch.load(weights, weights_only=True, map_location="cpu")
    model = tta.NativeTransformer(sd, 8, PAD, device=0)
    src_all, _ = SynthReactions(123456, "mit").dataset((steps + warmup) * bs)
    exp = []
    for b in list(batches(src_all, bs))[warmup:]:
        g = tta.TranslationInferenceGreedySpeculative(model, 200, 10, 3, PAD, BOS, EOS, C_TOK)
        try:
            exp.append(g.generate(torch.from_numpy(b).cuda()).cpu().numpy())
        except tta.ReferenceError_:
            exp.append(np.full((b.shape[0], 1, 200), PAD, dtype=np.int64))
    model.close()
    np.testing.assert_array_equal(got, np.concatenate(exp).astype(np.float32))
