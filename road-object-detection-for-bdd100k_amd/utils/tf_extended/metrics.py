"""utils/tf_extended/metrics.py — streaming TP/FP arrays, precision/recall, VOC07/VOC12 AP
(metrics.py:100-258), host numpy float64 as in the reference.  SweepTPFP (opt-in, not in the
reference) accumulates the device matcher's per-threshold TP/FP bit masks on the device and
applies the same host rules once, at the end of the run; with area_ranges it does so for the
per-range masks of the area matcher."""
import numpy as np

from utils.tf_extended.math import cummax

__all__ = ['streaming_tp_fp_arrays', 'StreamingTPFP', 'SweepTPFP', 'sweep_average_precisions', 'mean_ap',
           'precision_recall', 'average_precision_voc07', 'average_precision_voc12']


class StreamingTPFP(object):
    """Accumulator of (n_gt, n_det, tp, fp, scores) for one class (metrics.py:133-206)."""

    def __init__(self, remove_zero_scores=True):
        self.remove_zero_scores = remove_zero_scores
        self.num_gbboxes = 0
        self.num_detections = 0
        self.tp = np.zeros(0, bool)
        self.fp = np.zeros(0, bool)
        self.scores = np.zeros(0, np.float32)

    def update(self, num_gbboxes, tp, fp, scores):
        scores = np.asarray(scores, np.float32).reshape(-1)
        tp = np.asarray(tp, bool).reshape(-1)
        fp = np.asarray(fp, bool).reshape(-1)
        mask = np.logical_or(tp, fp)
        if self.remove_zero_scores:
            mask = np.logical_and(mask, scores > 1e-4)
        self.num_gbboxes += int(np.sum(num_gbboxes))
        self.num_detections += int(mask.sum())
        self.scores = np.concatenate([self.scores, scores[mask]])
        self.tp = np.concatenate([self.tp, tp[mask]])
        self.fp = np.concatenate([self.fp, fp[mask]])

    def value(self):
        return self.num_gbboxes, self.num_detections, self.tp, self.fp, self.scores


def streaming_tp_fp_arrays(num_gbboxes, tp, fp, scores, remove_zero_scores=True, state=None):
    """Dict-aware update: returns {c: StreamingTPFP} (created on first use) updated with
    this batch; `value()` of each gives the reference's metric tuple."""
    if isinstance(scores, dict) or isinstance(fp, dict):
        state = {} if state is None else state
        for c in num_gbboxes.keys():
            state[c] = streaming_tp_fp_arrays(num_gbboxes[c], tp[c], fp[c], scores[c], remove_zero_scores,
                                              state.get(c))
        return state
    st = StreamingTPFP(remove_zero_scores) if state is None else state
    st.update(num_gbboxes, tp, fp, scores)
    return st


class SweepTPFP(object):
    """Device-resident accumulator of rod.ops.match_detections outputs over a run, for every
    class slot c (label first_label + c) and every threshold t (bit t of the masks).

    One preallocated int32 buffer [capacity_images, C, 3 * N + 1] holds, per image and class,
    the N scores (their fp32 bits), the N tp masks, the N fp masks and n_gt.  update() copies a
    batch's tensors into the next rows on the current stream — no host synchronisation;
    value() makes ONE device -> host copy of the filled rows and then, per threshold and class,
    applies StreamingTPFP's rule (rows with tp or fp and score > 1e-4 are kept, in batch order)
    to give the reference's metric tuple for precision_recall / average_precision_voc07 / 12.
    Everything after the copy is host numpy, as in the reference.

    With area_ranges (fp32 [R, 2], the (lo, hi) pairs rod.ops.match_detections_area takes) the
    accumulator takes that op's outputs instead: the buffer is [capacity_images, C, N + R * (2 * N
    + 1)] — the N scores once, then per range the N tp masks, the N fp masks and n_gt — and
    value() / average_precisions() gain a leading per-range level.  A (range, class) without
    ground truth has no AP: None, which mean_ap skips."""

    def __init__(self, thresholds, num_classes, capacity_images, keep_top_k, device, first_label=1,
                 remove_zero_scores=True, area_ranges=None):
        import torch
        self.thresholds = np.array(thresholds, np.float32).reshape(-1)
        if not 1 <= self.thresholds.size <= 16:
            raise ValueError('SweepTPFP: 1 to 16 thresholds (the bits of the masks), got %d' % self.thresholds.size)
        self.C, self.N, self.capacity = int(num_classes), int(keep_top_k), int(capacity_images)
        self.first_label = int(first_label)
        self.remove_zero_scores = remove_zero_scores
        self.device = torch.device(device)
        self.thresholds_dev = torch.from_numpy(self.thresholds.copy()).to(self.device)
        self.area_ranges = None
        width = 3 * self.N + 1
        if area_ranges is not None:
            self.area_ranges = np.array(area_ranges, np.float32)
            if self.area_ranges.ndim != 2 or self.area_ranges.shape[1] != 2 or not len(self.area_ranges):
                raise ValueError('SweepTPFP: area_ranges must be [R, 2] with R >= 1, got shape %s'
                                 % (self.area_ranges.shape,))
            self.area_ranges_dev = torch.from_numpy(self.area_ranges.copy()).to(self.device)
            width = self.N + len(self.area_ranges) * (2 * self.N + 1)
        self.buf = torch.zeros((self.capacity, self.C, width), dtype=torch.int32, device=self.device)
        self.count = 0

    def update(self, scores, tp_mask, fp_mask, n_gt):
        """scores fp32 [B, C, N], tp_mask / fp_mask int32 [B, C, N], n_gt int32 [B, C]; with
        area_ranges tp_mask / fp_mask [R, B, C, N] and n_gt [R, B, C]."""
        import torch
        B, N = scores.shape[0], self.N
        lead = () if self.area_ranges is None else (len(self.area_ranges),)
        if tuple(scores.shape) != (B, self.C, N) or tuple(n_gt.shape) != lead + (B, self.C):
            raise ValueError('SweepTPFP.update: expected [B, %d, %d] scores, got %s' % (self.C, N, tuple(scores.shape)))
        if tuple(tp_mask.shape) != lead + (B, self.C, N) or tuple(fp_mask.shape) != lead + (B, self.C, N):
            raise ValueError('SweepTPFP.update: expected %s masks, got %s'
                             % (lead + (B, self.C, N), tuple(tp_mask.shape)))
        if scores.dtype != torch.float32:
            raise ValueError('SweepTPFP.update: scores must be float32')
        if self.count + B > self.capacity:
            raise ValueError('SweepTPFP.update: capacity of %d images exceeded' % self.capacity)
        rows = self.buf[self.count:self.count + B]
        rows[:, :, :N].copy_(scores.contiguous().view(torch.int32))
        if self.area_ranges is None:
            rows[:, :, N:2 * N].copy_(tp_mask)
            rows[:, :, 2 * N:3 * N].copy_(fp_mask)
            rows[:, :, 3 * N].copy_(n_gt)
        else:
            for r in range(len(self.area_ranges)):
                o = N + r * (2 * N + 1)
                rows[:, :, o:o + N].copy_(tp_mask[r])
                rows[:, :, o + N:o + 2 * N].copy_(fp_mask[r])
                rows[:, :, o + 2 * N].copy_(n_gt[r])
        self.count += B

    def _tuples(self, scores, tpm, fpm, n_gt):
        out = []
        for t in range(self.thresholds.size):
            per = {}
            for c in range(self.C):
                st = StreamingTPFP(self.remove_zero_scores)
                st.update(n_gt[:, c], (tpm[:, c] >> t) & 1, (fpm[:, c] >> t) & 1, scores[:, c])
                per[self.first_label + c] = st.value()
            out.append(per)
        return out

    def value(self):
        """[{label: (num_gbboxes, num_detections, tp, fp, scores)} for each threshold]: the
        tuples StreamingTPFP.value() gives after the same batches at that threshold.  With
        area_ranges: one such list per range."""
        N = self.N
        host = self.buf[:self.count].cpu().numpy()          # the run's only device -> host copy
        scores = np.ascontiguousarray(host[:, :, :N]).view(np.float32)
        if self.area_ranges is None:
            return self._tuples(scores, host[:, :, N:2 * N], host[:, :, 2 * N:3 * N], host[:, :, 3 * N])
        out = []
        for r in range(len(self.area_ranges)):
            o = N + r * (2 * N + 1)
            out.append(self._tuples(scores, host[:, :, o:o + N], host[:, :, o + N:o + 2 * N], host[:, :, o + 2 * N]))
        return out

    def average_precisions(self, value=None):
        """([{label: AP_VOC07}], [{label: AP_VOC12}]), one dict per threshold.  With area_ranges:
        one such list per range, and None in place of the AP of a class that has no ground
        truth in the range."""
        value = self.value() if value is None else value
        if self.area_ranges is not None:
            both = [sweep_average_precisions(per_t, True) for per_t in value]
            return [b[0] for b in both], [b[1] for b in both]
        return sweep_average_precisions(value)


def sweep_average_precisions(per_threshold, none_when_empty=False):
    """([{label: AP_VOC07}], [{label: AP_VOC12}]) of one SweepTPFP per-threshold list;
    none_when_empty: None in place of the AP of a class without ground truth."""
    ap07, ap12 = [], []
    for per in per_threshold:
        pr = {c: None if none_when_empty and v[0] == 0 else precision_recall(*v) for c, v in per.items()}
        ap07.append({c: None if v is None else average_precision_voc07(*v) for c, v in pr.items()})
        ap12.append({c: None if v is None else average_precision_voc12(*v) for c, v in pr.items()})
    return ap07, ap12


def mean_ap(aps):
    """Mean of {label: AP or None} over the labels that have one; None if none has."""
    vals = [v for v in aps.values() if v is not None]
    return sum(vals) / len(vals) if vals else None


def _safe_div(a, b):
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.asarray(a, np.float64) / np.asarray(b, np.float64)
    return np.where(np.asarray(b) > 0, q, 0.0)


def precision_recall(num_gbboxes, num_detections, tp, fp, scores, dtype=np.float64, scope=None):
    """Sort by score (top_k order: desc, ties by index), cumulative TP/FP -> P, R."""
    scores = np.asarray(scores)
    idx = np.argsort(-scores, kind='stable')[:num_detections]
    tp = np.cumsum(np.asarray(tp)[idx].astype(dtype))
    fp = np.cumsum(np.asarray(fp)[idx].astype(dtype))
    recall = _safe_div(tp, dtype(num_gbboxes))
    precision = _safe_div(tp, tp + fp)
    return precision, recall


def average_precision_voc12(precision, recall, name=None):
    """Area under the cummax precision envelope (metrics.py:212-234)."""
    p = np.concatenate([[0.], np.asarray(precision, np.float64), [0.]])
    r = np.concatenate([[0.], np.asarray(recall, np.float64), [1.]])
    p = cummax(p, reverse=True)
    return float(np.sum(p[1:] * (r[1:] - r[:-1])))


def average_precision_voc07(precision, recall, name=None):
    """11-point interpolated AP (metrics.py:237-258)."""
    p = np.concatenate([np.asarray(precision, np.float64), [0.]])
    r = np.concatenate([np.asarray(recall, np.float64), [np.inf]])
    ap = 0.
    for t in np.arange(0., 1.1, 0.1):
        v = p[r >= t]
        ap += (v.max() if v.size else -np.inf) / 11.
    return float(ap)
