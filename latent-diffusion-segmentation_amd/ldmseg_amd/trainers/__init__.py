from .losses import SegmentationLosses  # noqa: F401
from .sampler import TrainerDiffusion  # noqa: F401
from .trainer_ae import TrainerAE  # noqa: F401
