from .panoptic_evaluation_agnostic import PanopticEvaluatorAgnostic, pq_compute, id2rgb, rgb2id, get_table, pq_slots  # noqa: F401
from .semseg_evaluation import SemsegMeter, semseg_scores  # noqa: F401
