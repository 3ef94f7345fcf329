"""dlsg_amd -- MI355X-native implementation of the D-LSG (baiyang4/D-LSG-Video-Caption) per-clip
encoder/decoder hot path: CapGnnModel forward / train step / inference on hand-written gfx950 kernels."""
from .config import make_args, make_vocab, msvd_shaped, msrvtt_shaped, apply_dataset_overrides, Vocabulary  # noqa: F401
from .model import CapGnnModel, CapBaseline1, CapBaselineModel, Trainer, GreedyGraph, BeamGraph, NBestBeamGraph, SampleGraph, ss_epsilon, multistep_lr  # noqa: F401
from .gan import DiscV2, GanTrainer, GANLambdaHandler, save_checkpoint, load_checkpoint  # noqa: F401
from .data import H5File, CaptionSet, ResidentFeatures, StreamedFeatures, TrainLoader, EvalLoader, distributed_indices  # noqa: F401
from .scst import SCSTTrainer  # noqa: F401
from .mrt import MRTTrainer, risk_loss_reference  # noqa: F401
from .beam import beam_search, beam_nbest, stochastic_nbest, sample_without_replacement, importance_weights  # noqa: F401
from .beam import pack_exclusions, exclusions_hit, Exclusions, ExcludeNotCovered, BAD_ENDINGS  # noqa: F401
from .beam import pack_prefix, check_prefix, PrefixNotCovered  # noqa: F401
from .beam import sample, ensemble_sample, EnsembleSampleNotCovered  # noqa: F401
from .beam import constrained_beam_search, constrained_nbest, pack_constraints, pack_phrases, phrases_met  # noqa: F401
from .ensemble import Ensemble  # noqa: F401
from .graphs import EnsembleBeamGraph, EnsembleSampleGraph, ConsensusBeamGraph, StochasticBeamGraph, ConstrainedBeamGraph  # noqa: F401
from .consensus import consensus_rerank, consensus_search  # noqa: F401
from .rescore import score_captions, rescore, rescore_search  # noqa: F401
from .graphs import ScoreGraph, RescoreBeamGraph  # noqa: F401
from .scoring import DeviceCaptionMetrics, MixedReward, DeviceMixedReward  # noqa: F401
from .scoring import CiderD, DeviceCiderD, CaptionScorer, convert_data_to_coco_scorer_format, convert_prediction, evaluate, perplexity  # noqa: F401
