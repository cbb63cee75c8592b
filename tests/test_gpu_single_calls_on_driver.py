"""The single-session generate calls and standard beam search as one-session jobs of drive_sessions, on the tiny golden model:
a single call against the same batch as a one-batch generate_many, every loop in turn on one session against fresh sessions, and
inputs produced on a side stream immediately before the call.  Three ragged sources of 5, 7 and 9 tokens and max_len 12: rows
finish at different steps and the beam loop runs several iterations, in milliseconds."""
import pytest
import torch

from util_models import fixture_tokens, tiny_state, PAD, BOS, EOS

pytestmark = pytest.mark.gpu
MAX_LEN, DRAFT_LEN, N_DRAFTS, BEAM, N_SAMPLES, SEED = 12, 3, 2, 3, 2, 1234
COUNTERS = ("accepted_tokens", "produced_tokens", "verified_positions", "kv_prefix_positions")
LOOPS = ("greedy", "greedy_speculative", "sample", "sample_speculative", "beam", "beam_speculative")


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module")
def src():
    """[3, 9]: the first 4, 6 and 8 tokens of three fixture sources, each closed by EOS, right-padded."""
    rows = fixture_tokens()[0]
    out = torch.full((3, 9), PAD, dtype=torch.int64)
    for i, n in enumerate((5, 7, 9)):
        out[i, :n - 1] = rows[i, :n - 1]
        out[i, n - 1] = EOS
    return out


def new_model(tta):
    st, cfg = tiny_state()
    return tta.NativeTransformer(st, cfg["num_heads"], PAD, device=0)


def generators(tta, native):
    """name (LOOPS) -> generator on `native`."""
    c, V = fixture_tokens()[2:]
    sample = dict(temperature=1.0, top_k=8, num_samples=N_SAMPLES, seed=SEED)
    return {
        "greedy": tta.TranslationInferenceGreedy(native, MAX_LEN, PAD, BOS, EOS),
        "greedy_speculative": tta.TranslationInferenceGreedySpeculative(native, MAX_LEN, DRAFT_LEN, N_DRAFTS, PAD, BOS, EOS, c),
        "sample": tta.TranslationInferenceSampling(native, MAX_LEN, PAD, BOS, EOS, **sample),
        "sample_speculative": tta.TranslationInferenceSamplingSpeculative(native, MAX_LEN, DRAFT_LEN, N_DRAFTS, PAD, BOS, EOS, c, **sample),
        "beam": tta.TranslationInferenceBeamSearch(native, BEAM, MAX_LEN, PAD, BOS, EOS),
        "beam_speculative": tta.TranslationInferenceBeamSearchSpeculative(native, MAX_LEN, BEAM, DRAFT_LEN, N_DRAFTS, V, False, PAD, BOS,
                                                                          EOS, c, max_steps=100),
    }


@pytest.fixture(scope="module")
def fresh(tta, src):
    """name -> what the generator returns for `src` on a model (and session) created for that one call."""
    return {name: generators(tta, new_model(tta))[name].generate(src.cuda()).cpu() for name in LOOPS}


def test_single_call_equals_one_batch_many(tta, src):
    native = new_model(tta)
    c = fixture_tokens()[2]
    one = tta.TranslationInferenceGreedySpeculative(native, MAX_LEN, DRAFT_LEN, N_DRAFTS, PAD, BOS, EOS, c)
    many = tta.TranslationInferenceGreedySpeculative(native, MAX_LEN, DRAFT_LEN, N_DRAFTS, PAD, BOS, EOS, c)
    b = src.cuda()
    out_one = one.generate(b).cpu()
    out_many = many.generate_many([b], in_flight=1)
    assert len(out_many) == 1 and torch.equal(out_one, out_many[0].cpu())
    assert one.model_calls_num == many.model_calls_num and one.model_calls_num >= 2
    for k in COUNTERS:
        assert one.stats_total[k] == many.stats_total[k], k
    assert one.stats_total["produced_tokens"] > 0


def test_every_loop_in_turn_on_one_session(tta, src, fresh):
    gens = generators(tta, new_model(tta))                    # one model, one session for all of them
    b = src.cuda()
    for name in LOOPS + ("greedy_speculative",):
        assert torch.equal(gens[name].generate(b).cpu(), fresh[name]), name
    assert fresh["beam"].shape[:2] == (3, BEAM) and fresh["sample"].shape[:2] == (3, N_SAMPLES)


@pytest.mark.parametrize("name", ["greedy_speculative", "beam"])
def test_callers_stream_is_honoured(tta, src, fresh, name):
    gen = generators(tta, new_model(tta))[name]
    pinned = src.pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = pinned.to("cuda", non_blocking=True).clone() + 0          # produced on the side stream right before the call
        got = gen.generate(b).clone().cpu()                           # read on the side stream, nothing synchronised in between
    assert torch.equal(got, fresh[name])
