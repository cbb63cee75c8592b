"""translation-transformer_amd: MI355X-native speculative-decoding inference path of
Academich/translation-transformer.  Import as ``translation_transformer_amd`` through the
shim at the repository root (the directory name carries a hyphen)."""
from ._native import build, lib, TtxError, ReferenceError_  # noqa: F401
from .model import NativeTransformer, HypothesisScores, AttentionMaps, Alternatives, ProposalScores, FoldedHypotheses, reference_pe_table  # noqa: F401
from .decoding import (TranslationInferenceGreedySpeculative, TranslationInferenceGreedy,  # noqa: F401
                       TranslationInferenceBeamSearch, TranslationInferenceBeamSearchSpeculative,
                       TranslationInferenceSampling, TranslationInferenceSamplingSpeculative,
                       TranslationInferenceStochasticBeamSearch, SbsDetails, SbsTrace,
                       TranslationInferenceBeamSearchConstrained, ConstrainedBeamDetails)
from .lightning_model import VanillaEncoderDecoderTransformerLightning, run_predict, run_evaluate  # noqa: F401,E402
from . import dist  # noqa: F401,E402
from .tokenizer import NativeSmilesTokenizer  # noqa: F401,E402
from . import scheduling, scoring, syntax  # noqa: F401,E402
from .syntax import SmilesSyntax, SyntaxCheck  # noqa: F401,E402
