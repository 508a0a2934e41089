"""Test infrastructure: vectorised float32 numpy restatement of rod_match_detections (the
semantics stated in include/rod.h): oracle.post.bboxes_matching run once per threshold, for
every image and class slot, as bit masks.

The reference's loop carries one bit per ground truth ("already matched").  The ground truth a
detection competes for — the first argmax of IoU x same-label over the image's boxes — depends
on neither the threshold nor that bit, so the bit seen by detection i is "an earlier detection
with the same argmax, not difficult, matches at this threshold", and the detection is a TP when
it is the first such one.  Every float operation is one float32 numpy operation in the order of
oracle.post.bboxes_jaccard_one; the threshold comparison is float32 against float32."""
import numpy as np

f32 = np.float32


def jaccard(det, gt):
    """bboxes_jaccard_one of every detection det [N, 4] against every box gt [g, 4] -> [N, g]."""
    d = np.asarray(det, f32)[:, None, :]
    g = np.asarray(gt, f32)[None, :, :]
    h = np.maximum(np.minimum(g[..., 2], d[..., 2]) - np.maximum(g[..., 0], d[..., 0]), f32(0))
    w = np.maximum(np.minimum(g[..., 3], d[..., 3]) - np.maximum(g[..., 1], d[..., 1]), f32(0))
    inter = h * w
    area_g = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
    area_d = (d[..., 2] - d[..., 0]) * (d[..., 3] - d[..., 1])
    union = (-inter + area_g) + area_d
    with np.errstate(all='ignore'):
        q = inter / union
    out = np.where(union > 0, q, f32(0)).astype(f32)
    assert out.dtype == f32 and inter.dtype == f32 and union.dtype == f32
    return out


def match_one(label, boxes, glabels, gboxes, gdifficult, thresholds):
    """One (image, class): boxes [N, 4] in score order, the image's g ground-truth rows (already
    cut to gt_count).  Returns (n_gt, tp_mask [N] int32, fp_mask [N] int32)."""
    thresholds = np.asarray(thresholds, f32).reshape(-1)
    T, N, g = thresholds.size, len(boxes), len(glabels)
    all_bits = np.int32((1 << T) - 1)
    glabels = np.asarray(glabels)
    gdiff = np.asarray(gdifficult).astype(bool)
    n_gt = int(np.count_nonzero((glabels == label) & ~gdiff))
    if g == 0:
        return n_gt, np.zeros(N, np.int32), np.full(N, all_bits, np.int32)
    same = (glabels == label).astype(f32)
    jac = jaccard(boxes, gboxes) * same[None, :]
    idx = np.argmax(jac, axis=1)                      # first maximum
    best = jac[np.arange(N), idx]
    nd = ~gdiff[idx]
    tp = np.zeros(N, np.int32)
    for t in range(T):
        cand = nd & (best > f32(thresholds[t]))       # float32 > float32, strict
        first = np.full(g, N, np.int64)
        np.minimum.at(first, idx[cand], np.nonzero(cand)[0])
        tp |= (cand & (first[idx] == np.arange(N))).astype(np.int32) << t
    fp = np.where(nd, all_bits & ~tp, 0).astype(np.int32)
    return n_gt, tp, fp


def match_detections(boxes, glabels, gboxes, gcount, thresholds, gdifficult=None, first_label=1):
    """boxes [B, C, N, 4], glabels [B, G], gboxes [B, G, 4], gcount [B], gdifficult [B, G] or
    None -> (tp_mask [B, C, N], fp_mask [B, C, N], n_gt [B, C]), int32."""
    boxes = np.asarray(boxes, f32)
    B, C, N = boxes.shape[:3]
    tp = np.zeros((B, C, N), np.int32)
    fp = np.zeros((B, C, N), np.int32)
    n_gt = np.zeros((B, C), np.int32)
    for b in range(B):
        g = int(gcount[b])
        gd = np.zeros(g, bool) if gdifficult is None else np.asarray(gdifficult)[b, :g]
        for c in range(C):
            n_gt[b, c], tp[b, c], fp[b, c] = match_one(first_label + c, boxes[b, c], glabels[b, :g], gboxes[b, :g],
                                                       gd, thresholds)
    return tp, fp, n_gt


def from_oracle(label, boxes, glabels, gboxes, gdifficult, thresholds):
    """The same masks from oracle.post.bboxes_matching, one plain run per threshold."""
    from oracle.post import bboxes_matching
    N = len(boxes)
    tp = np.zeros(N, np.int32)
    fp = np.zeros(N, np.int32)
    n_gt = None
    for t, thr in enumerate(np.asarray(thresholds, f32).reshape(-1)):
        n, a, b = bboxes_matching(label, [1.0] * N, np.asarray(boxes, f32), list(glabels), np.asarray(gboxes, f32),
                                  list(gdifficult), f32(thr))
        assert n_gt in (None, n)
        n_gt = n
        tp |= np.array(a, bool).astype(np.int32) << t
        fp |= np.array(b, bool).astype(np.int32) << t
    return n_gt, tp, fp


# ---------------------------------------------------------------------------- hand-made cases
COCO = np.linspace(0.5, 0.95, 10).astype(f32)


def _box(y0, x0, y1, x1):
    return [y0, x0, y1, x1]


def hand_cases(N=70, G=130, C=3, seed=5):
    """One batch (B=4) packing the edge cases, per-image counts 0, 1, 65, 130; class slots are
    labels 1..C.  Returns (boxes [4, C, N, 4], glabels [4, G], gboxes [4, G, 4], gdifficult
    [4, G] uint8, gcount [4]).  Rows >= gcount hold NaN boxes and garbage labels."""
    rng = np.random.default_rng(seed)
    B = 4
    boxes = np.zeros((B, C, N, 4), f32)           # zero-padded detections everywhere not set
    gl = rng.integers(1, C + 1, (B, G)).astype(np.int32)   # garbage labels that LOOK valid
    gb = np.full((B, G, 4), np.nan, f32)
    gd = rng.integers(0, 2, (B, G)).astype(np.uint8)
    gcount = np.array([0, 1, 65, 130], np.int32)

    # image 0: no ground truth -> every detection FP in every bit
    boxes[0, :, :5] = rng.uniform(0, 1, (C, 5, 4)).astype(f32)

    # image 1: ONE ground truth, difficult and of class 2: class-1 detections overlap nothing of
    # their label -> argmax 0 -> that box -> difficult -> neither TP nor FP; a class-2 detection
    # that matches it records nothing either and n_gt stays 0
    gl[1, 0], gb[1, 0], gd[1, 0] = 2, _box(0.1, 0.1, 0.4, 0.4), 1
    boxes[1, 0, 0] = _box(0.6, 0.6, 0.9, 0.9)
    boxes[1, 0, 1] = _box(0.1, 0.1, 0.4, 0.4)
    boxes[1, 1, 0] = _box(0.1, 0.1, 0.4, 0.4)
    boxes[1, 1, 1] = _box(0.1, 0.1, 0.4, 0.35)

    # image 2 (65 rows): rows 0..59 a grid of small class-3 boxes, none difficult; the edge rows
    # sit at 60..64, past the 64 boundary for the last
    g2 = np.zeros((65, 4), f32)
    for j in range(60):
        y, x = (j // 10) * 0.05, (j % 10) * 0.05
        g2[j] = _box(2 + y, 2 + x, 2 + y + 0.04, 2 + x + 0.04)
    gl[2, :65], gd[2, :65] = 3, 0
    gl[2, 60], g2[60] = 1, _box(0, 0, 1, 1)            # unit box: exact IoU 0.5 and 0.75
    gl[2, 61], g2[61] = 1, _box(4, 4, 5, 5)            # twin ...
    gl[2, 62], g2[62] = 1, _box(4, 4, 5, 5)            # ... of it: the first index wins
    gl[2, 63], g2[63] = 1, _box(6, 6, 6, 7)            # zero-area ground truth
    gl[2, 64], g2[64] = 1, _box(8, 0, 9, 10)           # met by A (IoU 0.6) then B (0.9)
    gb[2, :65] = g2
    d = boxes[2, 0]
    d[0] = _box(8, 0, 9, 6)        # A: IoU 6/10 with row 64
    d[1] = _box(8, 0, 9, 9)        # B: IoU 9/10 with row 64
    d[2] = _box(0, 0, 1, 0.5)      # IoU exactly 0.5 with the unit box: no match at t = 0.5
    d[3] = _box(0, 0, 1, 0.75)     # IoU exactly 0.75
    d[4] = _box(4, 4, 5, 5)        # TP on row 61
    d[5] = _box(4, 4, 5, 5)        # duplicate detection: FP ("existing"), not a TP on the twin 62
    d[6] = _box(6, 6, 6, 7)        # on the zero-area ground truth: IoU 0
    d[7] = _box(5.9, 6, 6.1, 7)    # around it: inter 0
    d[66] = _box(8, 0, 9, 9.5)     # second wave: a later, better box on row 64 is still "existing"
    d[69] = _box(2, 2, 2.04, 2.04)  # class-1 detection on a class-3 box: argmax 0, not difficult -> FP
    boxes[2, 2, :60] = g2[:60][::-1]                   # class 3: every grid box once, reversed
    boxes[2, 2, 60:] = g2[:10]                         # and ten again: FP

    # image 3 (130 rows, > 2 x 64): random boxes, some difficult, detections jittered around them
    ctr = rng.uniform(0.1, 0.9, (130, 2))
    hw = rng.uniform(0.05, 0.3, (130, 2))
    g3 = np.concatenate([ctr - hw / 2, ctr + hw / 2], 1).astype(f32)
    gb[3, :130], gl[3, :130] = g3, rng.integers(1, C + 1, 130)
    gd[3, :130] = rng.random(130) < 0.2
    for c in range(C):
        src = g3[rng.integers(0, 130, N)]
        boxes[3, c] = (src + rng.normal(0, 0.02, (N, 4))).astype(f32)
        boxes[3, c, N - 6:] = 0                        # zero-padded tail
    return boxes, gl, gb, gd, gcount


def clustered_case(B, C, N, G, seed, difficult_rate=0.1):
    """Random ground truth with detections jittered around it (many contested boxes)."""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(0.1, 0.9, (B, G, 2))
    hw = rng.uniform(0.03, 0.3, (B, G, 2))
    gb = np.concatenate([ctr - hw / 2, ctr + hw / 2], -1).astype(f32)
    gl = rng.integers(1, C + 1, (B, G)).astype(np.int32)
    gd = (rng.random((B, G)) < difficult_rate).astype(np.uint8)
    gcount = rng.integers(max(G // 2, 0), G + 1, B).astype(np.int32)
    boxes = np.zeros((B, C, N, 4), f32)
    for b in range(B):
        g = max(int(gcount[b]), 1)
        for c in range(C):
            pick = rng.integers(0, g, N)
            scale = rng.choice([0.002, 0.01, 0.04], (N, 1))
            boxes[b, c] = (gb[b, pick] + rng.normal(0, 1, (N, 4)) * scale).astype(f32)
    return boxes, gl, gb, gd, gcount
