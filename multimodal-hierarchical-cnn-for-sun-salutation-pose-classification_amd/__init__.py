"""MI355X-native QuadtreeCNN hot path (forward/backward of the multimodal
Sun-Salutation pose classifier) behind the reference's nn.Module surface.

The directory name is not a Python identifier; import it with
    importlib.import_module("multimodal-hierarchical-cnn-for-sun-salutation-pose-classification_amd")
or put `<this dir>/quadtree_from_scratch` (or `/resnet`) on sys.path and keep the
reference's `from models import get_model`.
"""
from ._lib import LIB_PATH, QtError  # noqa: F401
from .augment import FrameAugmenter  # noqa: F401
from .loss import CrossEntropyLoss, FocalLoss, LossMeter  # noqa: F401
from .optim import FusedAdam, grad_norm  # noqa: F401
from .preprocess import FramePreprocessor, random_flips, random_resized_crop_boxes  # noqa: F401
from .quadtree import AttentionHierarchicalCNN, CnnLstm, QuadtreeCNN, StandardResNetCNN  # noqa: F401
from .video3d import Ji3DCNN, Quadtree3DCNN  # noqa: F401
from .gradcam import GradCAM, jet_lut  # noqa: F401
from .pose import FEATURE_NAMES, PoseFeatures, load_class_stats  # noqa: F401
from .pose_sequence import NUM_SEQUENCE_FEATURES, SEQUENCE_FEATURE_NAMES, SequencePoseFeatures  # noqa: F401
from .sequence_windows import SequenceWindows, WindowPlan, fit_class_stats  # noqa: F401
from .sequence_stream import CnnLstmStream  # noqa: F401
from .metrics import EvalMeter, predict  # noqa: F401
from .scores import ScoreMeter  # noqa: F401
from .annotate import MAJOR_SEGMENTS, POSE_CONNECTIONS, FrameAnnotator, caption_atlas  # noqa: F401
from .timeline import PoseTimeline  # noqa: F401
from .segments import SegmentMeter, segment_runs  # noqa: F401
from .pose_order import PoseLagDecoder, PoseLagSmoother  # noqa: F401
from .pose_order import PoseOrderDecoder, PoseOrderLearner, PosePosterior, cyclic_prior, prob_score  # noqa: F401
from .pose_order import PoseDurationDecoder, duration_prior, geometric_durations, hold_prior  # noqa: F401
from .pose_order import PoseDurationPosterior, expected_duration_prior  # noqa: F401
from .pose_order import PoseDurationLagDecoder, PoseDurationLagSmoother  # noqa: F401
from .pose_order import PoseDurationLearner  # noqa: F401

__all__ = ["QuadtreeCNN", "StandardResNetCNN", "AttentionHierarchicalCNN", "CnnLstm", "Quadtree3DCNN", "Ji3DCNN", "FusedAdam", "grad_norm",
           "CrossEntropyLoss", "FocalLoss", "LossMeter", "FramePreprocessor", "random_resized_crop_boxes", "random_flips", "FrameAugmenter",
           "GradCAM", "jet_lut", "PoseFeatures", "FEATURE_NAMES", "load_class_stats", "EvalMeter", "predict", "ScoreMeter",
           "SequencePoseFeatures", "SEQUENCE_FEATURE_NAMES", "NUM_SEQUENCE_FEATURES",
           "SequenceWindows", "WindowPlan", "fit_class_stats", "CnnLstmStream",
           "FrameAnnotator", "caption_atlas", "POSE_CONNECTIONS", "MAJOR_SEGMENTS", "PoseTimeline",
           "PoseOrderDecoder", "PosePosterior", "PoseOrderLearner", "PoseLagSmoother", "PoseLagDecoder", "cyclic_prior", "prob_score",
           "PoseDurationDecoder", "duration_prior", "hold_prior", "geometric_durations",
           "PoseDurationPosterior", "expected_duration_prior", "PoseDurationLagDecoder", "PoseDurationLagSmoother",
           "PoseDurationLearner",
           "SegmentMeter", "segment_runs",
           "QtError", "LIB_PATH"]
