"""ttamm — MI355X-native training step for the two-tower model with an adaptive mimic
mechanism (drop-in for alperkartkaya2-afk/two-tower-augmented-with-adaptive-mimic-mechanism's
models + training hot loop).  Compute runs in libttamm.so (gfx950 HIP kernels); see
include/ttamm.h for the C ABI and DESIGN.md for the design."""

from .adaptive_mimic import AdaptiveMimicMechanism
from .data import DeviceInteractionLoader, load_features, load_interactions, save_features, save_interactions
from .encoders import (
    FeatureEncoderConfig,
    FeatureEncoderWrapper,
    FeatureFusionGate,
    TowerEncoder,
    build_feature_encoder,
    build_id_embedding,
    build_tower_encoder,
)
from .inbatch import inbatch_bce, inbatch_bce_loss, inbatch_softmax, inbatch_softmax_loss
from .metrics import RankingMetrics, compute_ranking_metrics, evaluate_metrics, ranking_metrics
from .retrieval import encode_item_embeddings, evaluate_model, prepare_faiss_resources, topk_merge
from .samplers import PositivesCSR, sample_negative_items
from .training import (
    DotProductSimilarity,
    FusedEvalLoss,
    FusedTrainStep,
    _collect_parameter_groups,
    compute_loss,
    train_one_epoch,
)
from .two_tower import TwoTowerModel

__all__ = [
    "AdaptiveMimicMechanism",
    "DeviceInteractionLoader",
    "DotProductSimilarity",
    "FeatureEncoderConfig",
    "FeatureEncoderWrapper",
    "FeatureFusionGate",
    "FusedEvalLoss",
    "FusedTrainStep",
    "PositivesCSR",
    "RankingMetrics",
    "TowerEncoder",
    "TwoTowerModel",
    "build_feature_encoder",
    "build_id_embedding",
    "build_tower_encoder",
    "compute_loss",
    "compute_ranking_metrics",
    "encode_item_embeddings",
    "evaluate_metrics",
    "evaluate_model",
    "inbatch_bce",
    "inbatch_bce_loss",
    "inbatch_softmax",
    "inbatch_softmax_loss",
    "load_features",
    "load_interactions",
    "prepare_faiss_resources",
    "ranking_metrics",
    "sample_negative_items",
    "save_features",
    "save_interactions",
    "topk_merge",
    "train_one_epoch",
]
