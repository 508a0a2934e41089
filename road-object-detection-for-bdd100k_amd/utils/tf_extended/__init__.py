"""Drop-in for the reference's utils/tf_extended (bboxes, metrics, math, tensors).

Evaluation bookkeeping (matching, TP/FP accumulation, precision/recall, VOC AP) runs on the
host in numpy, as the reference pins it to the CPU (evaluate.py:146, 164); the per-class
sort + NMS runs as the rod_select_topk_nms kernel (utils.net_tools.detected_bboxes).  Opt-in
(evaluate.py --match_on device / --ap_iou_sweep): the matching runs as rod_match_detections and
metrics.SweepTPFP keeps its per-threshold TP/FP masks on the GPU until the end of the run; the
precision/recall and AP arithmetic stays the host code below.  --ap_area_ranges: the matching runs
as rod_match_detections_area and SweepTPFP(area_ranges=...) keeps the per-range masks the same
way (metrics.sweep_average_precisions, metrics.mean_ap: a class without ground truth in a range
has no AP and the means skip it).
"""
from utils.tf_extended.bboxes import *  # noqa: F401,F403
from utils.tf_extended.math import *  # noqa: F401,F403
from utils.tf_extended.metrics import *  # noqa: F401,F403
from utils.tf_extended.tensors import *  # noqa: F401,F403
