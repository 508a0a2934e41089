"""Test infrastructure: numpy restatement of rod_match_detections_area (the semantics stated in
include/rod.h, ABI 31): the matching of tests/evalmatch_ref.py reported for R object-area ranges.

Two forms of one rule.  `match_one_area` is vectorised float32: the argmax, the IoU and the
"first detection that matches box idx at t" come from evalmatch_ref unchanged in meaning, and a
range only masks what is reported.  `match_one_area_sequential` is the rule as one would say it:
per range and per threshold, walk the detections in score order with an explicit "already
matched" bit per ground truth.  tests/test_areamatch_host.py holds the two against each other.

area(box) = (ymax - ymin) * (xmax - xmin), one float32 subtraction pair and one float32 multiply
(jaccard's area_g / area_d expression); in_r(a) = !(a < lo) && !(a >= hi), float32 against
float32: lo inclusive, hi exclusive, NaN inside."""
import numpy as np

from evalmatch_ref import jaccard

f32 = np.float32
ALL = (-np.inf, np.inf)


def area(boxes):
    b = np.asarray(boxes, f32)
    out = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    assert out.dtype == f32
    return out


def in_range(a, ranges):
    """a [...] float32, ranges [R, 2] -> bool [R, ...]."""
    a = np.asarray(a, f32)
    rg = np.asarray(ranges, f32).reshape(-1, 2)
    lo = rg[:, 0].reshape((-1,) + (1,) * a.ndim)
    hi = rg[:, 1].reshape((-1,) + (1,) * a.ndim)
    with np.errstate(invalid='ignore'):
        return ~(a[None] < lo) & ~(a[None] >= hi)


def normalised(px, image_size):
    """evaluate.py's conversion of pixel^2 bounds: np.float32(np.float64(px) / (H * W))."""
    h, w = image_size
    return np.float32(np.float64(px) / (h * w))


def _argmax(label, boxes, glabels, gboxes):
    same = (np.asarray(glabels) == label).astype(f32)
    jac = jaccard(boxes, gboxes) * same[None, :]
    idx = np.argmax(jac, axis=1)                      # first maximum; all zero -> ground truth 0
    return idx, jac[np.arange(len(boxes)), idx]


def match_one_area(label, boxes, glabels, gboxes, gdifficult, thresholds, ranges):
    """One (image, class), vectorised.  -> (n_gt [R], tp_mask [R, N], fp_mask [R, N]) int32."""
    thresholds = np.asarray(thresholds, f32).reshape(-1)
    ranges = np.asarray(ranges, f32).reshape(-1, 2)
    T, N, g, R = thresholds.size, len(boxes), len(glabels), len(ranges)
    all_bits = np.int32((1 << T) - 1)
    glabels = np.asarray(glabels)
    gdiff = np.asarray(gdifficult).astype(bool)
    d_in = in_range(area(np.asarray(boxes, f32).reshape(N, 4)), ranges)            # [R, N]
    g_in = in_range(area(np.asarray(gboxes, f32).reshape(g, 4)), ranges)           # [R, g]
    n_gt = np.count_nonzero(((glabels == label) & ~gdiff)[None] & g_in, axis=1).astype(np.int32)
    if g == 0:
        return n_gt, np.zeros((R, N), np.int32), np.where(d_in, all_bits, 0).astype(np.int32)
    idx, best = _argmax(label, boxes, glabels, gboxes)
    nd = ~gdiff[idx]
    tp = np.zeros(N, np.int32)
    match = np.zeros(N, np.int32)
    for t in range(T):
        cand = nd & (best > f32(thresholds[t]))       # float32 > float32, strict
        first = np.full(g, N, np.int64)
        np.minimum.at(first, idx[cand], np.nonzero(cand)[0])
        tp |= (cand & (first[idx] == np.arange(N))).astype(np.int32) << t
        match |= cand.astype(np.int32) << t
    gi = g_in[:, idx]                                                              # [R, N]
    tp_r = np.where(gi, tp[None], 0)
    fp_r = np.where(gi, (match & ~tp)[None], 0) | np.where(d_in, (all_bits & ~match)[None], 0)
    fp_r = np.where(nd[None], fp_r, 0)
    return n_gt, tp_r.astype(np.int32), fp_r.astype(np.int32)


def match_one_area_sequential(label, boxes, glabels, gboxes, gdifficult, thresholds, ranges):
    """The same, written straight from the rule: plain loops, one matched bit per ground truth."""
    thresholds = np.asarray(thresholds, f32).reshape(-1)
    ranges = np.asarray(ranges, f32).reshape(-1, 2)
    T, N, g, R = thresholds.size, len(boxes), len(glabels), len(ranges)
    boxes = np.asarray(boxes, f32).reshape(N, 4)
    gboxes = np.asarray(gboxes, f32).reshape(g, 4)
    n_gt = np.zeros(R, np.int32)
    tp = np.zeros((R, N), np.int32)
    fp = np.zeros((R, N), np.int32)
    if g:
        idx, best = _argmax(label, boxes, glabels, gboxes)
    for r in range(R):
        lo, hi = ranges[r]
        inside = lambda a: (not a < lo) and (not a >= hi)  # noqa: E731
        for j in range(g):
            if glabels[j] == label and not gdifficult[j] and inside(area(gboxes[j])):
                n_gt[r] += 1
        for t in range(T):
            matched = [False] * g
            for i in range(N):
                if g == 0:
                    fp[r, i] |= int(inside(area(boxes[i]))) << t
                    continue
                j = idx[i]
                if gdifficult[j]:
                    continue                              # neither, whatever the IoU
                if best[i] > thresholds[t]:
                    was, matched[j] = matched[j], True    # the box is taken, in the range or not
                    if not inside(area(gboxes[j])):
                        continue                          # matched to ignored ground truth: neither
                    if was:
                        fp[r, i] |= 1 << t
                    else:
                        tp[r, i] |= 1 << t
                elif inside(area(boxes[i])):
                    fp[r, i] |= 1 << t
    return n_gt, tp, fp


def match_detections_area(boxes, glabels, gboxes, gcount, thresholds, ranges, gdifficult=None, first_label=1,
                          one=match_one_area):
    """boxes [B, C, N, 4], glabels [B, G], gboxes [B, G, 4], gcount [B], ranges [R, 2] ->
    (tp_mask [R, B, C, N], fp_mask [R, B, C, N], n_gt [R, B, C]), int32."""
    boxes = np.asarray(boxes, f32)
    B, C, N = boxes.shape[:3]
    R = len(np.asarray(ranges).reshape(-1, 2))
    tp = np.zeros((R, B, C, N), np.int32)
    fp = np.zeros((R, B, C, N), np.int32)
    n_gt = np.zeros((R, B, C), np.int32)
    for b in range(B):
        g = int(gcount[b])
        gd = np.zeros(g, bool) if gdifficult is None else np.asarray(gdifficult)[b, :g]
        for c in range(C):
            n_gt[:, b, c], tp[:, b, c], fp[:, b, c] = one(first_label + c, boxes[b, c], glabels[b, :g], gboxes[b, :g],
                                                          gd, thresholds, ranges)
    return tp, fp, n_gt


def input_conditions(ranges, tp, fp, n_gt, tp_all, fp_all):
    """What keeps a multi-range case from passing while checking nothing, as the list of the
    conditions that FAIL (empty = fine).  tp_all / fp_all [B, C, N] are the all-range masks
    (evalmatch_ref.match_detections).  Every range must have a TP bit, an FP bit and a detection
    it ignores only because of the range (TP or FP in the all range, neither here) — but for a
    (-inf, +inf) row, which by the identity can ignore nothing — and some (range, class) must
    have no ground truth over the whole batch."""
    ranges = np.asarray(ranges, f32).reshape(-1, 2)
    seen = (tp_all | fp_all) != 0
    bad = []
    for r in range(len(ranges)):
        if not tp[r].any():
            bad.append('range %d has no TP bit' % r)
        if not fp[r].any():
            bad.append('range %d has no FP bit' % r)
        if tuple(ranges[r]) != ALL and not (seen & ((tp[r] | fp[r]) == 0)).any():
            bad.append('range %d ignores no detection' % r)
    if not (n_gt.sum(axis=1) == 0).any():
        bad.append('no (range, class) without ground truth')
    return bad


# ---------------------------------------------------------------------------- ranges for the cases
def hand_ranges(case):
    """Four ranges that cover the line for evalmatch_ref.hand_cases().  The 0.04 x 0.04 grid boxes
    of image 2 have three distinct float32 areas a0 < a1 < a2 (the subtraction rounds differently
    along the grid); a1 and a2 are used verbatim as bounds, so membership of every grid box of
    those two areas is decided on the equality edge: [-inf, a1) [a1, a2) [a2, 0.03) [0.03, inf)."""
    grid = np.unique(area(case[2][2, :60]))
    assert grid.size == 3, grid
    a1, a2 = grid[1], grid[2]
    return np.array([[-np.inf, a1], [a1, a2], [a2, 0.03], [0.03, np.inf]], f32)


def clustered_ranges(case, R, thresholds):
    """R rows for an evalmatch_ref.clustered_case: (-inf, +inf); a narrow range [s_k, s_k+w) between
    two ground-truth areas, the first (k, w) for which the whole set meets input_conditions (a
    narrow range is what leaves some class without ground truth); and R - 2 bins of equal count
    that cover the line.  R == 1: the (-inf, +inf) row alone."""
    from evalmatch_ref import match_detections
    boxes, gl, gb, gd, gcount = case
    if R == 1:
        return np.array([ALL], f32)
    assert R >= 3
    s = np.unique(np.concatenate([area(gb[b, :int(gcount[b])]) for b in range(len(gcount))]))
    cuts = s[np.linspace(0, s.size, R - 1).astype(int)[1:-1]]
    bins = np.stack([np.concatenate([[-np.inf], cuts]), np.concatenate([cuts, [np.inf]])], 1)
    tp_all, fp_all, _ = match_detections(boxes, gl, gb, gcount, thresholds, gd)
    for w in (1, 2, 3):
        for k in range(s.size - w):
            ranges = np.concatenate([[ALL], [[s[k], s[k + w]]], bins]).astype(f32)
            tp, fp, n_gt = match_detections_area(boxes, gl, gb, gcount, thresholds, ranges[:2], gd)
            if not input_conditions(ranges[:2], tp, fp, n_gt, tp_all, fp_all):
                return ranges
    raise AssertionError('no narrow range meets the input conditions')
