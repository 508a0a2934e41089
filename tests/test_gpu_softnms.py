"""rod_select_topk_softnms (Soft-NMS, linear and gaussian) against its float32 numpy
restatement (tests/softnms_ref.py), bit for bit: both front ends, the candidate-list edge
cases, the degenerate identities with the hard entry, the output form, the host layers and
the captured predict graph."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import config
from oracle import post as op
from rod import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softnms_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32

METHODS = ['linear', 'gaussian']
# (select, nms, top_k, keep_top_k, sigma, min_score)
# min_score chosen on the restatement (the other figures are given): with these anchors the top
# 400 scores of a class lie in 0.59 .. 0.99 (the 200th near 0.73; of the top 64, the 16th near
# 0.94), a linear rescore by an IoU > 0.4 falls below the 200th and is never emitted, so only a
# min_score inside the score range makes linear differ from the hard NMS and ends loops early
CASES = [(0.1, 0.4, 400, 200, 0.5, 0.75), (0.3, 0.4, 400, 200, 0.5, 0.72), (0.02, 0.45, 64, 16, 0.3, 0.93)]
# crowded boxes (every candidate overlaps many others), keep_top_k up to top_k: rescored
# candidates are emitted, out of their original score order
CROWDED = [(0.1, 0.4, 400, 400, 0.5, 0.001), (0.1, 0.3, 300, 200, 0.2, 0.2)]
B, K = 2, 11


def _anchor_table():
    from utils import net_tools as nt
    config.img_size = (300, 300)
    anchors = nt.anchors_all_layer((300, 300), config.feat_sizes((300, 300)), nt.init_anchor(6))
    return nt.AnchorTable(anchors, 'cpu')


@functools.lru_cache(maxsize=None)
def _inputs(case='plain'):
    """The recipe of tests/test_gpu_detect.py (300x300 anchors, seed 5, B = 2, K = 11): logits
    N(0, 2) (or the candidate-list edge cases), offsets N(0, 0.2) -> (probs, corner boxes)."""
    rng = np.random.default_rng(5)
    if case == 'crowded':   # 1500 boxes of side 0.1 .. 0.4 centred in the middle third of the image
        A = 1500
        e, s, _ = op.softmax_rows(rng.normal(0, 2.0, (B, A, K)).astype(f32))
        probs = (e / s).astype(f32)
        ctr = rng.uniform(0.35, 0.65, (B, A, 2)).astype(f32)
        half = rng.uniform(0.05, 0.2, (B, A, 2)).astype(f32)
        boxes = np.concatenate([ctr - half, ctr + half], -1)
        probs.setflags(write=False)
        boxes.setflags(write=False)
        return probs, boxes
    tab = _anchor_table()
    A = tab.A
    if case == 'plain':
        logits = rng.normal(0, 2.0, (B, A, K)).astype(f32)
    elif case == 'many':    # most scores pass 0.1 in classes 1-2: lists far over 4096 (radix branch)
        logits = rng.normal(0, 0.3, (B, A, K)).astype(f32)
        logits[..., 1:3] += 2.0
    elif case == 'ties':    # quantised logits: massive exact ties in score
        logits = np.round(rng.normal(0, 1.5, (B, A, K))).astype(f32)
    elif case == 'few':
        logits = rng.normal(0, 1.0, (B, A, K)).astype(f32)
        logits[..., 0] += 4.0
    else:                   # 'none'
        logits = np.zeros((B, A, K), f32)
        logits[..., 0] = 10.0
    e, s, _ = op.softmax_rows(logits)
    probs = (e / s).astype(f32)
    off = rng.normal(0, 0.2, (B, A, 4)).astype(f32)
    boxes = op.decode_corner(tab.center_np, off)
    probs.setflags(write=False)
    boxes.setflags(write=False)
    return probs, boxes


@functools.lru_cache(maxsize=None)
def _ref(method, case, which='plain'):
    sel, nms, top_k, keep, sigma, min_score = case
    probs, boxes = _inputs(which)
    s, b, info = sr.soft_detected_bboxes(probs, boxes, sel, nms, top_k, keep, method, sigma, min_score)
    s.setflags(write=False)
    b.setflags(write=False)
    return s, b, info


@functools.lru_cache(maxsize=None)
def _hard(sel, nms, top_k, keep):
    return op.detected_bboxes(*_inputs(), sel, nms, top_k, keep)


def _run(dev, method, case, which='plain', compact=True):
    sel, nms, top_k, keep, sigma, min_score = case
    probs, boxes = _inputs(which)
    sd, bd = ops.select_topk_soft_nms(torch.tensor(probs).to(dev), torch.tensor(boxes).to(dev), sel, top_k,
                                      keep, nms, method, sigma, min_score, compact=compact)
    return sd.cpu().numpy(), bd.cpu().numpy()


def _check_form(s, b):
    """Scores non-increasing along the last axis; every slot after the first zero is zero."""
    assert (s[..., 1:] <= s[..., :-1]).all() and (s >= 0).all()
    empty = s == 0
    assert (np.logical_or.accumulate(empty, -1) == empty).all()
    assert not b[empty].any()


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'sel%g_top%d_keep%d' % (c[0], c[2], c[3]))
@pytest.mark.parametrize('method', METHODS)
def test_soft_nms_bit_exact(dev, method, case):
    sel, nms, top_k, keep, sigma, min_score = case
    probs, boxes = _inputs()
    s_ref, b_ref, info = _ref(method, case)
    # on the restatement alone: it is not the hard NMS, and over the parameter sets both ways of
    # ending the loop occur
    assert not np.array_equal(s_ref, _hard(sel, nms, top_k, keep)[0])
    why = [(len(idx), w, c[3]) for m in METHODS for c in CASES for idx, w in _ref(m, c)[2].values()]
    n_full = sum(1 for n, w, k in why if w == sr.FULL)
    n_min = sum(1 for n, w, k in why if w == sr.MIN_SCORE)
    print('stops: keep_top_k %d, min_score %d, exhausted %d of %d' % (n_full, n_min, len(why) - n_full - n_min,
                                                                   len(why)))
    assert n_full > 0 and n_min > 0
    assert all(n == k for n, w, k in why if w == sr.FULL) and all(n < k for n, w, k in why if w == sr.MIN_SCORE)
    _check_form(s_ref, b_ref)
    for compact in (True, False):   # candidate-list and direct front ends
        sd, bd = _run(dev, method, case, compact=compact)
        np.testing.assert_array_equal(sd, s_ref)
        np.testing.assert_array_equal(bd, b_ref)


@pytest.mark.parametrize('case', CROWDED, ids=lambda c: 'top%d_keep%d_min%g' % (c[2], c[3], c[5]))
@pytest.mark.parametrize('method', METHODS)
def test_soft_nms_crowded(dev, method, case):
    """Heavily overlapping boxes: rescored candidates are emitted (with a score other than their
    probability) and out of their position order — asserted on the restatement first."""
    probs, boxes = _inputs('crowded')
    s_ref, b_ref, info = _ref(method, case, 'crowded')
    rescored = sum(int((s_ref[b, c - 1, :len(idx)] != probs[b, idx, c]).sum()) for (b, c), (idx, _) in info.items())
    reordered = 0
    for (b, c), (idx, _) in info.items():
        emitted = probs[b, idx, c]      # the original scores in emission order
        reordered += int((emitted[1:] > emitted[:-1]).sum())
    print('emitted %d, rescored %d, out of score order %d' % (sum(len(i) for i, _ in info.values()), rescored,
                                                              reordered))
    assert rescored > 50 and reordered > 50
    _check_form(s_ref, b_ref)
    for compact in (True, False):
        sd, bd = _run(dev, method, case, 'crowded', compact=compact)
        np.testing.assert_array_equal(sd, s_ref)
        np.testing.assert_array_equal(bd, b_ref)


EDGE = (0.1, 0.4, 400, 200, 0.5, 0.001)


@pytest.mark.parametrize('which', ['many', 'ties', 'few', 'none'])
@pytest.mark.parametrize('method', METHODS)
def test_soft_nms_candidate_lists(dev, method, which):
    """The front-end edge cases of test_select_topk_nms_candidate_lists: the radix-select branch
    past 4096 candidates per class (and, in its other classes, fewer candidates than top_k),
    exact score ties (the position tie rule), a few hundred candidates, no candidate at all."""
    probs, _ = _inputs(which)
    s_ref, b_ref, info = _ref(method, EDGE, which)
    per_class = (probs[..., 1:] >= f32(0.1)).sum(1)
    n_sel = int(per_class.max())
    if which == 'many':     # classes 1-2 over 4096; the other classes have fewer candidates than top_k
        assert n_sel > 4096 and 0 < int(per_class.min()) < 400
    if which == 'ties':     # equal emitted scores do occur: the tie rule decides their order
        assert (np.diff(s_ref, axis=-1)[s_ref[..., 1:] > 0] == 0).any()
    if which == 'few':
        assert 400 < n_sel <= 4096      # more than top_k, sorted whole in LDS
    if which == 'none':
        assert n_sel == 0 and not s_ref.any()
    for compact in (True, False):
        sd, bd = _run(dev, method, EDGE, which, compact=compact)
        np.testing.assert_array_equal(sd, s_ref)
        np.testing.assert_array_equal(bd, b_ref)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'sel%g_top%d_keep%d' % (c[0], c[2], c[3]))
def test_soft_nms_degenerate_is_topk(dev, case):
    """Linear with nms_threshold = inf never rescores; gaussian with sigma = 1e30 multiplies by
    exp(-tiny) == 1.0f: both are the hard entry without suppression (pure top-k), with
    min_score = select_threshold (every candidate's score is >= it)."""
    sel, _, top_k, keep, _, _ = case
    probs, boxes = _inputs()
    pd, bxd = torch.tensor(probs).to(dev), torch.tensor(boxes).to(dev)
    inf = float('inf')
    for compact in (True, False):
        s_hard, b_hard = ops.select_topk_nms(pd, bxd, sel, top_k, keep, inf, compact=compact)
        assert s_hard.any()
        s_lin, b_lin = ops.select_topk_soft_nms(pd, bxd, sel, top_k, keep, inf, 'linear', 0.5, sel, compact=compact)
        s_gau, b_gau = ops.select_topk_soft_nms(pd, bxd, sel, top_k, keep, 0.4, 'gaussian', 1e30, sel,
                                                compact=compact)
        for s, b in ((s_lin, b_lin), (s_gau, b_gau)):
            assert torch.equal(s, s_hard) and torch.equal(b, b_hard)


@pytest.mark.parametrize('method', METHODS)
def test_soft_nms_output_form(dev, method):
    for case, which in ((CASES[0], 'plain'), (CASES[2], 'plain'), (EDGE, 'few'), (EDGE, 'ties')):
        sd, bd = _run(dev, method, case, which)
        _check_form(sd, bd)
        assert sd.any()


def test_soft_nms_host_surface(dev):
    from utils import net_tools
    from utils.tf_extended import bboxes as tfe_bboxes
    sel, nms, top_k, keep, sigma, min_score = CASES[0]
    probs, boxes = _inputs()
    pd, bxd = torch.tensor(probs).to(dev), torch.tensor(boxes).to(dev)
    s_ref, b_ref, _ = _ref('linear', CASES[0])
    rs, rb = net_tools.detected_bboxes(pd, bxd, select_threshold=sel, nms_threshold=nms, top_k=top_k,
                                       keep_top_k=keep, nms_method='linear', soft_nms_sigma=sigma,
                                       soft_nms_min_score=min_score)
    assert sorted(rs) == sorted(rb) == list(range(1, K))
    for c in range(1, K):
        np.testing.assert_array_equal(rs[c].cpu().numpy(), s_ref[:, c - 1])
        np.testing.assert_array_equal(rb[c].cpu().numpy(), b_ref[:, c - 1])
    # the default is still the hard NMS
    hs, hb = net_tools.detected_bboxes(pd, bxd, select_threshold=sel, nms_threshold=nms, top_k=top_k,
                                       keep_top_k=keep)
    s_hard, b_hard = ops.select_topk_nms(pd, bxd, sel, top_k, keep, nms)
    assert all(torch.equal(hs[c], s_hard[:, c - 1]) and torch.equal(hb[c], b_hard[:, c - 1]) for c in range(1, K))
    # bboxes_nms_batch on ONE class: its sorted, masked candidates (what bboxes_sort hands over)
    c = 3
    s_ref, b_ref, _ = _ref('gaussian', CASES[0])
    cs, cb = [], []
    for b in range(B):
        p = probs[b, :, c]
        fm = (p >= f32(sel)).astype(f32)
        order = np.argsort(-(p * fm), kind='stable')[:top_k]
        cs.append((p * fm)[order])
        cb.append((boxes[b] * fm[:, None])[order])
    gs, gb = tfe_bboxes.bboxes_nms_batch(torch.from_numpy(np.stack(cs)).to(dev), torch.from_numpy(np.stack(cb)).to(dev),
                                         nms_threshold=nms, keep_top_k=keep, nms_method='gaussian',
                                         soft_nms_sigma=sigma, soft_nms_min_score=min_score)
    np.testing.assert_array_equal(gs.cpu().numpy(), s_ref[:, c - 1])
    np.testing.assert_array_equal(gb.cpu().numpy(), b_ref[:, c - 1])
    with pytest.raises(ValueError, match='nms_method'):
        tfe_bboxes.bboxes_nms_batch(torch.from_numpy(np.stack(cs)).to(dev), torch.from_numpy(np.stack(cb)).to(dev),
                                    nms_method='bogus')


def test_soft_nms_in_the_predict_graph(dev):
    """The whole predict path with gaussian Soft-NMS captured as one HIP graph: the capture and
    a replay on another input equal the restatement applied to the eager probabilities and
    boxes of the same input; a hard Predictor on the same weights is still the oracle's NMS."""
    import predict
    from rod.data import detector_like_scores, synthetic_batch
    H = W = 300
    pr = predict.Predictor((H, W), dev, torch.float32, select_threshold=0.02, nms_method='gaussian', seed=71)
    # a detector-like score distribution (calibrated BatchNorm, shifted background logit), so that
    # the NMS has real work
    detector_like_scores(pr, synthetic_batch(1, H, W, dev, seed=72)[0], rate=0.05)
    imgs = [synthetic_batch(1, H, W, dev, seed=s)[0] for s in (73, 74)]
    kw = pr.kw
    refs, eager = [], []
    pr.keep_intermediates = True
    for img in imgs:
        pr(img)
        probs, boxes = pr.last[1].cpu().numpy(), pr.last[2].cpu().numpy()
        eager.append((probs, boxes))
        refs.append(sr.soft_detected_bboxes(probs, boxes, 0.02, kw['nms_threshold'], kw['top_k'], kw['keep_top_k'],
                                            'gaussian', kw['soft_nms_sigma'], kw['soft_nms_min_score']))
    assert not np.array_equal(refs[0][0], refs[1][0]) and refs[0][0].any()
    pr.keep_intermediates = False
    pr.use_graph = True
    graphs = []
    for img, (s_ref, b_ref, _) in zip(imgs, refs):
        scores, bboxes = pr(img)
        graphs.append(pr._graph[1])
        S = np.stack([scores[c].cpu().numpy() for c in sorted(scores)], 1)
        BX = np.stack([bboxes[c].cpu().numpy() for c in sorted(bboxes)], 1)
        np.testing.assert_array_equal(S, s_ref)
        np.testing.assert_array_equal(BX, b_ref)
    assert graphs[0] is graphs[1]          # the second call replayed the captured graph
    # changing the method re-captures
    pr.kw = dict(pr.kw, nms_method='linear')
    pr(imgs[0])
    assert pr._graph[1] is not graphs[0]
    hard = predict.Predictor((H, W), dev, torch.float32, select_threshold=0.02, seed=71)
    hard.net = pr.net
    hard.use_graph = True
    scores, bboxes = hard(imgs[0])
    assert hard._graph is not None
    s_ref, b_ref, _ = op.detected_bboxes(eager[0][0], eager[0][1], 0.02, kw['nms_threshold'], kw['top_k'],
                                         kw['keep_top_k'])
    np.testing.assert_array_equal(np.stack([scores[c].cpu().numpy() for c in sorted(scores)], 1), s_ref)
    np.testing.assert_array_equal(np.stack([bboxes[c].cpu().numpy() for c in sorted(bboxes)], 1), b_ref)
