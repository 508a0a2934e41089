"""Test infrastructure: float32 numpy restatement of rod_select_topk_softnms (the semantics
stated in include/rod.h; Soft-NMS of Bodla et al., ICCV 2017, which the reference lacks).

Candidates as oracle.post.detected_bboxes takes them (select mask on scores and boxes, the
min(top_k, A) best by score, ties to the lower anchor index); then, until keep_top_k entries are
emitted: pick the live candidate with the largest working score (ties to the lower position),
stop unless it is > 0 and >= min_score, emit it, and rescore every live candidate by its IoU
with the pick (oracle.post._nms_iou_vec, the IoU of the hard NMS).  Every operation is one
float32 operation; exp is correctly rounded through float64 (oracle.targets.exp_cr)."""
import numpy as np

from oracle.post import _nms_iou_vec
from oracle.targets import exp_cr

f32 = np.float32

# why the loop of one (image, class) ended
FULL, MIN_SCORE, EXHAUSTED = 'keep_top_k', 'min_score', 'exhausted'


def soft_nms_candidates(w, cb, keep_top_k, nms_threshold, method, sigma, min_score):
    """The loop on an ordered candidate list: scores w [m] (>= 0), boxes cb [m, 4].
    Returns (emitted scores, emitted positions, stop reason)."""
    if method not in ('linear', 'gaussian'):
        raise ValueError(method)
    w = np.array(w, f32)
    cb = np.asarray(cb, f32)
    live = w > 0    # a zero score (below the select threshold) stays zero: never emitted
    thr, sg, ms = f32(nms_threshold), f32(sigma), f32(min_score)
    es, ep = [], []
    while len(es) < keep_top_k:
        if not live.any():
            return es, ep, EXHAUSTED
        p = int(np.argmax(np.where(live, w, f32(-1))))   # first maximum: the lower position
        wp = w[p]
        if not wp > 0:
            return es, ep, EXHAUSTED
        if not wp >= ms:
            return es, ep, MIN_SCORE
        es.append(wp)
        ep.append(p)
        live[p] = False
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            continue
        iou = _nms_iou_vec(cb[p], cb[idx])
        if method == 'linear':
            w[idx] = np.where(iou > thr, w[idx] * (f32(1.0) - iou), w[idx])
        else:
            t = iou * iou
            t = t / sg
            w[idx] = w[idx] * exp_cr(-t)
    return es, ep, FULL


def soft_detected_bboxes(probs, boxes, select_threshold, nms_threshold, top_k, keep_top_k, method, sigma=0.5,
                         min_score=0.001):
    """probs [B,A,K], corner boxes [B,A,4] -> rescored scores [B,K-1,keep], boxes [B,K-1,keep,4]
    in emission order, zero-padded, and {(b, c): (anchor indices emitted, stop reason)}."""
    probs = np.asarray(probs, f32)
    boxes = np.asarray(boxes, f32)
    B, A, K = probs.shape
    out_s = np.zeros((B, K - 1, keep_top_k), f32)
    out_b = np.zeros((B, K - 1, keep_top_k, 4), f32)
    info = {}
    for b in range(B):
        for c in range(1, K):
            p = probs[b, :, c]
            fm = (p >= f32(select_threshold)).astype(f32)
            s = p * fm
            bx = boxes[b] * fm[:, None]
            order = np.argsort(-s, kind='stable')[:min(top_k, A)]
            es, ep, why = soft_nms_candidates(s[order], bx[order], keep_top_k, nms_threshold, method, sigma,
                                              min_score)
            n = len(es)
            out_s[b, c - 1, :n] = es
            out_b[b, c - 1, :n] = bx[order[ep]] if n else 0
            info[(b, c)] = ([int(order[i]) for i in ep], why)
    return out_s, out_b, info
