"""Native greedy-speculative generator (ttx_greedy_speculative_generate) against the reference's token
outputs (golden) and against the oracle on the same weights."""
import numpy as np
import pytest
import torch

from util_models import load_npz, tiny_state, fixture_tokens, PAD, BOS, EOS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1
    return t


@pytest.fixture(scope="module")
def tiny(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)


@pytest.mark.parametrize("bsz", [1, 4, 10])
def test_matches_reference_tokens(tta, tiny, bsz):
    gold = load_npz("gen_spec_greedy.npz")
    src, _, c, _ = fixture_tokens()
    for N in (1, 3, 7, 23):
        for D in (5, 10, 17):
            g = tta.TranslationInferenceGreedySpeculative(tiny, 150, D, N, PAD, BOS, EOS, c)
            out = np.concatenate([g.generate(src[i:i + bsz].cuda()).cpu().numpy() for i in range(0, 10, bsz)])
            np.testing.assert_array_equal(out, gold[f"b{bsz}_n{N}_d{D}_tokens"], err_msg=f"b{bsz} n{N} d{D}")
            assert g.model_calls_num == int(gold[f"b{bsz}_n{N}_d{D}_calls"])


def test_unfinished_rows_stay_pad(tta, tiny):
    gold = load_npz("gen_spec_greedy.npz")
    src, _, c, _ = fixture_tokens()
    for max_len in (30, 45):
        g = tta.TranslationInferenceGreedySpeculative(tiny, max_len, 10, 3, PAD, BOS, EOS, c)
        out = g.generate(src.cuda()).cpu().numpy()
        np.testing.assert_array_equal(out, gold[f"short_m{max_len}_tokens"])
        assert g.model_calls_num == int(gold[f"short_m{max_len}_calls"])


def test_many_batches_in_flight_equal_one_at_a_time(tta, tiny):
    src, _, c, _ = fixture_tokens()
    g1 = tta.TranslationInferenceGreedySpeculative(tiny, 150, 10, 3, PAD, BOS, EOS, c)
    batches = []
    for lo, hi in ((0, 3), (3, 4), (4, 8), (8, 10), (0, 10), (5, 9)):
        sel = src[lo:hi]
        batches.append(sel[:, :int((sel != PAD).sum(1).max())].cuda())
    ref = [g1.generate(b) for b in batches]
    for in_flight in (1, 2, 4):
        g2 = tta.TranslationInferenceGreedySpeculative(tiny, 150, 10, 3, PAD, BOS, EOS, c)
        out = g2.generate_many(batches, in_flight=in_flight)
        assert len(out) == len(ref)
        for a, b in zip(out, ref):
            assert torch.equal(a, b)
        assert g2.model_calls_num == g1.model_calls_num


def _random_sources(n, lo, hi, V, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        L = int(rng.integers(lo, hi + 1))
        body = rng.integers(4, V, size=L - 2)
        rows.append(np.concatenate([[BOS], body, [EOS]]))
    W = max(len(r) for r in rows)
    out = np.full((n, W), PAD, dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return torch.from_numpy(out)


def test_large_ragged_batch_matches_oracle(tta, tiny):
    """300 ragged random sources in ONE batch (more rows than one accept-kernel pass of 256 threads; rows that
    never reach EOS stay PAD; short max_len so the width rule ends the loop) against the oracle."""
    from oracle.model import OracleTransformer, config_from_state
    from oracle.decoding import GreedySpeculativeOracle
    st, cfg = tiny_state()
    oracle = OracleTransformer(config_from_state(st, cfg["num_heads"]), st)
    _, _, c, V = fixture_tokens()
    src = _random_sources(300, 6, 60, V, seed=3)
    outcomes = []
    for max_len, N, D in ((40, 3, 10), (150, 5, 6)):
        exp = GreedySpeculativeOracle(oracle, max_len, D, N, PAD, BOS, EOS, c)
        g = tta.TranslationInferenceGreedySpeculative(tiny, max_len, D, N, PAD, BOS, EOS, c)
        try:
            want = exp.generate(src)
        except RuntimeError:
            # the reference raises here (a row reaches EOS while the tensor is already wider than max_len,
            # speculative_decoding.py:158): the HIP path must report the same condition, not invent an output
            with pytest.raises(tta.ReferenceError_):
                g.generate(src.cuda())
            outcomes.append("raises")
            continue
        got = g.generate(src.cuda()).cpu()
        assert torch.equal(got, want)
        assert g.model_calls_num == exp.model_calls_num
        outcomes.append("equal")
    print("large ragged batch:", outcomes)
    assert "equal" in outcomes


def _sequential(tta, model, batches, max_len, D, N, c):
    """Per-batch `generate` calls: outputs (None where the reference raises), model calls of the batches that ran."""
    outs, calls = [], []
    for b in batches:
        g = tta.TranslationInferenceGreedySpeculative(model, max_len, D, N, PAD, BOS, EOS, c)
        try:
            outs.append(g.generate(b))
            calls.append(g.model_calls_num)
        except tta.ReferenceError_:
            outs.append(None)
            calls.append(None)
    return outs, calls


@pytest.mark.parametrize("max_len,D,N", [(150, 10, 3), (150, 4, 2), (45, 4, 2), (45, 10, 3), (40, 4, 2), (30, 10, 3), (27, 4, 2),
                                         (57, 4, 2), (20, 8, 2), (12, 6, 1)])
def test_row_scheduled_decoding_replays_the_given_batches(tta, tiny, max_len, D, N):
    """generate_many(reorder=True): rows decoded in length-sorted groups under the per-row width rule
    (ttx_greedy_speculative_generate_rows), then the reference's loop replayed over the batches as given —
    outputs, model_calls_num and the raise-or-not outcome equal per-batch `generate` calls."""
    src, _, c, _ = fixture_tokens()
    batches = []
    for lo, hi in ((0, 3), (3, 4), (4, 8), (8, 10), (0, 10), (5, 9), (6, 7)):
        sel = src[lo:hi]
        batches.append(sel[:, :int((sel != PAD).sum(1).max())].cuda())
    ref, calls = _sequential(tta, tiny, batches, max_len, D, N, c)
    ok = [i for i, o in enumerate(ref) if o is not None]
    bad = [i for i, o in enumerate(ref) if o is None]
    for group_size, in_flight in ((4, 3), (3, 1), (32, 2)):
        g = tta.TranslationInferenceGreedySpeculative(tiny, max_len, D, N, PAD, BOS, EOS, c)
        out = g.generate_many([batches[i] for i in ok], in_flight=in_flight, reorder=True, group_size=group_size)
        assert g.stats_total.get("device_model_calls", 0) > 0 or not ok        # the row path ran (no silent fallback)
        for i, o in zip(ok, out):
            assert torch.equal(o, ref[i]), f"batch {i} group_size {group_size}"
        assert g.model_calls_num == sum(calls[i] for i in ok)
        if bad:
            with pytest.raises(tta.ReferenceError_):
                g.generate_many(batches, in_flight=in_flight, reorder=True, group_size=group_size)
    print(f"max_len={max_len} D={D} N={N}: {len(ok)} batches equal, {len(bad)} raise as in the reference")


def test_row_scheduled_decoding_random_sources(tta, tiny):
    """320 ragged random sources in batches of 32.  Random token soup makes the tiny model emit PAD inside
    sequences now and then (reference quirk 2): the row path reports that and generate_many decodes the batches
    as given instead; either way the result equals per-batch generate."""
    _, _, c, V = fixture_tokens()
    src = _random_sources(320, 6, 60, V, seed=11)
    batches = []
    for i in range(0, 320, 32):
        sel = src[i:i + 32]
        batches.append(sel[:, :int((sel != PAD).sum(1).max())].cuda())
    for max_len, D, N in ((150, 10, 3), (64, 4, 2)):
        ref, calls = _sequential(tta, tiny, batches, max_len, D, N, c)
        ok = [i for i, o in enumerate(ref) if o is not None]
        g = tta.TranslationInferenceGreedySpeculative(tiny, max_len, D, N, PAD, BOS, EOS, c)
        out = g.generate_many([batches[i] for i in ok], in_flight=4, reorder=True)
        for i, o in zip(ok, out):
            assert torch.equal(o, ref[i])
        assert g.model_calls_num == sum(calls[i] for i in ok)
        print(f"random sources max_len={max_len}: {len(ok)}/10 batches decodable, row path used:",
              "device_model_calls" in g.stats_total)


def test_streaming_attention_fallback_matches(tta):
    """The long-sequence attention kernel (k_attn, used when the LDS images of k_attn2 do not fit) on the same
    inputs as the fast path."""
    import os
    gold = load_npz("gen_spec_greedy.npz")
    src, _, c, _ = fixture_tokens()
    st, cfg = tiny_state()
    os.environ["TTX_ATTN_FALLBACK"] = "1"
    try:
        slow = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    finally:
        os.environ.pop("TTX_ATTN_FALLBACK")
    g = tta.TranslationInferenceGreedySpeculative(slow, 150, 10, 3, PAD, BOS, EOS, c)
    np.testing.assert_array_equal(g.generate(src.cuda()).cpu().numpy(), gold["b10_n3_d10_tokens"])
    io = load_npz("tiny_model_io.npz")
    mem = slow.encode_src(torch.from_numpy(io["src"]).cuda()).cpu()
    mask = torch.from_numpy(io["src"]) == 0
    assert (mem - torch.from_numpy(io["memory"]))[~mask].abs().max() < 1e-4
    slow.close()


def test_reference_error_cases(tta, tiny):
    src, _, c, _ = fixture_tokens()
    with pytest.raises(tta.ReferenceError_):      # drafting.py:39 "The number of drafts must be greater than 0"
        tta.TranslationInferenceGreedySpeculative(tiny, 150, 10, 0, PAD, BOS, EOS, c).generate(src.cuda())
    with pytest.raises(tta.ReferenceError_):      # drafting.py:41 pad token == replace token
        tta.TranslationInferenceGreedySpeculative(tiny, 150, 10, 3, PAD, BOS, EOS, PAD).generate(src.cuda())
    out = tta.TranslationInferenceGreedySpeculative(tiny, 1, 1, 1, PAD, BOS, EOS, c).generate(src.cuda())
    assert out.shape == (10, 1, 1) and int((out != PAD).sum()) == 0     # `while size(1) < max_len` never entered


def test_generate_many_skip_mode(tta, tiny):
    """on_error="skip": batches on which the reference raises come back as None (both schedules), the others equal
    per-batch generate."""
    src, _, c, _ = fixture_tokens()
    batches = []
    for lo, hi in ((0, 3), (3, 4), (4, 8), (8, 10), (0, 10), (5, 9), (6, 7)):
        sel = src[lo:hi]
        batches.append(sel[:, :int((sel != PAD).sum(1).max())].cuda())
    max_len, D, N = 45, 4, 2                        # four of these batches raise in the reference (see the test above)
    ref, calls = _sequential(tta, tiny, batches, max_len, D, N, c)
    bad = [i for i, o in enumerate(ref) if o is None]
    assert bad and len(bad) < len(batches)
    for reorder in (True, False):
        g = tta.TranslationInferenceGreedySpeculative(tiny, max_len, D, N, PAD, BOS, EOS, c)
        out = g.generate_many(batches, in_flight=3, reorder=reorder, group_size=4, on_error="skip")
        assert sorted(g.last_failed_batches) == bad
        for i, o in enumerate(out):
            assert (o is None) == (i in bad)
            if o is not None:
                assert torch.equal(o, ref[i])


def test_slot_pool_randomised_partitions(tta, tiny):
    """Random batch partitions, pool capacities, session counts and decoding parameters: the row schedule (slot pool and
    fixed groups) returns, batch by batch, what per-batch `generate` returns — including which batches raise."""
    src, _, c, _ = fixture_tokens()
    rng = np.random.default_rng(42)
    checked = fell_back = 0
    for trial in range(12):
        max_len = int(rng.choice([150, 60, 45, 33, 27]))
        D = int(rng.choice([3, 4, 6, 10]))
        N = int(rng.choice([1, 2, 3, 5]))
        if D > max_len:
            continue
        # rows: fixture sources, some repeated, in random order, cut into random batches
        idx = rng.integers(0, src.shape[0], size=int(rng.integers(5, 40)))
        cuts = sorted(set(rng.integers(1, len(idx), size=int(rng.integers(1, 6))).tolist()))
        parts = np.split(idx, cuts)
        batches = []
        for p in parts:
            sel = src[torch.from_numpy(p)]
            batches.append(sel[:, :int((sel != PAD).sum(1).max())].cuda())
        ref, calls = _sequential(tta, tiny, batches, max_len, D, N, c)
        bad = [i for i, o in enumerate(ref) if o is None]
        for pool in (True, False):
            g = tta.TranslationInferenceGreedySpeculative(tiny, max_len, D, N, PAD, BOS, EOS, c)
            out = g.generate_many(batches, in_flight=int(rng.integers(1, 6)), reorder=True, group_size=int(rng.integers(1, 48)),
                                  on_error="skip", pool=pool)
            fell_back += "device" not in g.stats_total
            assert sorted(g.last_failed_batches) == bad, (trial, pool)
            for i, o in enumerate(out):
                if i in bad:
                    assert o is None
                else:
                    assert torch.equal(o, ref[i]), (trial, pool, i)
            assert g.model_calls_num == sum(calls[i] for i in range(len(batches)) if i not in bad)
            checked += 1
    print(f"{checked} randomised schedules checked, {fell_back} fell back to decoding as given")
    assert checked >= 16 and fell_back == 0


def test_out_of_range_token_ids_raise_like_torch_embedding(tta, tiny):
    src, _, c, V = fixture_tokens()
    bad = src[:3].clone()
    bad[1, 2] = V + 5
    g = tta.TranslationInferenceGreedySpeculative(tiny, 150, 10, 3, PAD, BOS, EOS, c)
    with pytest.raises(IndexError):
        g.generate(bad.cuda())
    with pytest.raises(IndexError):
        g.generate_many([src[:2].cuda(), bad.cuda()], reorder=True)
    with pytest.raises(IndexError):
        tiny.encode_src(bad.cuda())
    neg = src[:2].clone()
    neg[0, 1] = -1
    with pytest.raises(IndexError):
        tta.TranslationInferenceGreedy(tiny, 150, PAD, BOS, EOS).generate(neg.cuda())


def test_profiling_model_brackets_every_pool_session_and_changes_no_output(tta, tiny, monkeypatch):
    """The model bench.py builds for its roofline pass (TTX_PROFILE_GEMM=1 at construction): EVERY pool session it creates
    later brackets its GEMM launches (the count covers at least 6 launches per decoder layer + the classifier for every device
    step of every pool), the pools run one after another, and the outputs are those of an ordinary model."""
    fsrc, _, c, V = fixture_tokens()
    src = fsrc.repeat(8, 1)[torch.randperm(80, generator=torch.Generator().manual_seed(3))]       # 80 rows -> three pools
    batches = [src[i:i + 8] for i in range(0, 80, 8)]
    batches = [b[:, :int((b != PAD).sum(1).max())].cuda() for b in batches]
    g_ref = tta.TranslationInferenceGreedySpeculative(tiny, 150, 10, 3, PAD, BOS, EOS, c)
    ref = g_ref.generate_many(batches, in_flight=4, reorder=True, group_size=32, on_error="skip")
    assert "device" in g_ref.stats_total                     # the slot pools ran (no fallback to the batches as given)
    st, cfg = tiny_state()
    monkeypatch.setenv("TTX_PROFILE_GEMM", "1")
    pm = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    monkeypatch.delenv("TTX_PROFILE_GEMM")
    g = tta.TranslationInferenceGreedySpeculative(pm, 150, 10, 3, PAD, BOS, EOS, c)
    pm.kernel_profile()
    out = g.generate_many(batches, in_flight=4, reorder=True, group_size=32, on_error="skip")
    prof = pm.kernel_profile()
    for a, b in zip(out, ref):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)
    assert g.model_calls_num == g_ref.model_calls_num
    steps = g.stats_total["device"]["model_calls"]
    assert len(pm._pool) >= 2 and steps > 0
    assert prof["launches"] >= steps * (6 * pm.num_dec_layers + 1), (prof, steps)
    assert prof["gemm_ms"] > 0 and prof["pair_overhead_ms"] >= 0
    pm.close()


def test_one_batch_of_1200_rows_equals_its_three_sources(tta, tiny):
    """Three fixture sources, each 400 times, shuffled, decoded as ONE batch of 1 200 rows: k_accept runs with 1 024 threads in two
    rounds of its slot loop and of its ordered compaction, and 400 rows finish in the same step (more than its list of finished
    rows holds, so the output copy scans all slots).  The set of fronts is the same at every step as in the batch of the three
    sources alone, so the width rule is too: every row equals its source's row there, and so does model_calls_num."""
    src, _, c, _ = fixture_tokens()
    three = src[[0, 4, 8]]
    three = three[:, :int((three != PAD).sum(1).max())]
    g3 = tta.TranslationInferenceGreedySpeculative(tiny, 150, 10, 3, PAD, BOS, EOS, c)
    want = g3.generate(three.cuda()).cpu()
    assert bool((want == EOS).any(-1).all()), "every source finishes"
    which = torch.from_numpy(np.random.default_rng(5).permutation(np.repeat(np.arange(3), 400)))
    g = tta.TranslationInferenceGreedySpeculative(tiny, 150, 10, 3, PAD, BOS, EOS, c)
    got = g.generate(three[which].cuda()).cpu()
    assert got.shape == (1200,) + tuple(want.shape[1:])
    assert torch.equal(got, want[which])
    assert g.model_calls_num == g3.model_calls_num
