"""Soft-NMS, the parts that need no GPU: the numpy restatement (tests/softnms_ref.py) on
hand-checked cases, the argument checks of rod_select_topk_softnms (they return before any HIP
call, as in tests/test_abi.py), the CLI defaults and the host layers' method check."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softnms_ref as sr  # noqa: E402

f32 = np.float32


def test_linear_two_boxes_iou_one_third():
    """[0,0,1,2] and [0,1,1,3]: intersection 1, union 2 + 2 - 1 = 3, IoU = fp32 1/3 > 0.3."""
    cb = np.array([[0, 0, 1, 2], [0, 1, 1, 3]], f32)
    w = np.array([0.9, 0.6], f32)
    es, ep, why = sr.soft_nms_candidates(w, cb, 2, 0.3, 'linear', 0.5, 0.001)
    iou = f32(1) / f32(3)
    assert ep == [0, 1] and why == sr.FULL
    assert es[0] == f32(0.9) and es[1] == f32(0.6) * (f32(1) - iou)
    assert es[1] != f32(0.6)
    # at a threshold the IoU does not exceed, linear leaves the score alone
    es, ep, _ = sr.soft_nms_candidates(w, cb, 2, 0.34, 'linear', 0.5, 0.001)
    assert es == [f32(0.9), f32(0.6)]
    # gaussian: t = iou*iou; t = t / sigma; w * exp(-t), each rounded to fp32, threshold unused
    es, ep, _ = sr.soft_nms_candidates(w, cb, 2, 123.0, 'gaussian', 0.5, 0.001)
    t = f32(f32(iou * iou) / f32(0.5))
    assert es[1] == f32(0.6) * f32(np.exp(-np.float64(t)))


def test_rescoring_changes_emission_order():
    """B overlaps A with IoU 0.5 and drops from 0.8 to 0.4, below the disjoint C (0.5)."""
    cb = np.array([[0, 0, 1, 2], [0, 0, 1, 1], [5, 5, 6, 6]], f32)
    w = np.array([0.9, 0.8, 0.5], f32)
    es, ep, why = sr.soft_nms_candidates(w, cb, 3, 0.3, 'linear', 0.5, 0.001)
    assert ep == [0, 2, 1] and why == sr.FULL
    assert es == [f32(0.9), f32(0.5), f32(0.8) * (f32(1) - f32(0.5))]
    assert all(a >= b for a, b in zip(es, es[1:]))


def test_ties_go_to_the_lower_position_and_anchor():
    cb = np.array([[0, 0, 1, 1], [2, 2, 3, 3], [4, 4, 5, 5], [6, 6, 7, 7]], f32)
    w = np.array([0.5, 0.5, 0.5, 0.5], f32)
    for method in ('linear', 'gaussian'):
        es, ep, why = sr.soft_nms_candidates(w, cb, 3, 0.3, method, 0.5, 0.001)
        assert ep == [0, 1, 2] and es == [f32(0.5)] * 3 and why == sr.FULL
    # a tie that rescoring creates: B (0.8, IoU 0.5 with A) becomes 0.4 == C, and B is the lower position
    cb = np.array([[0, 0, 1, 2], [0, 0, 1, 1], [5, 5, 6, 6]], f32)
    es, ep, _ = sr.soft_nms_candidates(np.array([0.9, 0.8, 0.4], f32), cb, 3, 0.3, 'linear', 0.5, 0.001)
    assert ep == [0, 1, 2] and es[1] == es[2] == f32(0.4)
    # through the candidate selection: equal probabilities -> the lower anchor index first
    probs = np.zeros((1, 5, 2), f32)
    probs[0, :, 1] = [0.2, 0.7, 0.7, 0.05, 0.7]
    boxes = np.array([[[i * 2, 0, i * 2 + 1, 1] for i in range(5)]], f32)
    s, b, info = sr.soft_detected_bboxes(probs, boxes, 0.1, 0.4, 4, 3, 'linear')
    assert info[(0, 1)][0] == [1, 2, 4]
    np.testing.assert_array_equal(s[0, 0], np.array([0.7, 0.7, 0.7], f32))
    np.testing.assert_array_equal(b[0, 0], boxes[0, [1, 2, 4]])


def test_stop_reasons_and_padding():
    cb = np.array([[0, 0, 1, 2], [0, 0, 1, 1.9], [5, 5, 6, 6]], f32)
    w = np.array([0.9, 0.3, 0.2], f32)
    # B is almost A: 0.3 * (1 - 0.95) < min_score 0.1 -> emitted A, C, then the stop on min_score
    es, ep, why = sr.soft_nms_candidates(w, cb, 3, 0.3, 'linear', 0.5, 0.1)
    assert ep == [0, 2] and why == sr.MIN_SCORE
    es, ep, why = sr.soft_nms_candidates(w, cb, 2, 0.3, 'linear', 0.5, 0.1)
    assert ep == [0, 2] and why == sr.FULL
    # candidates below the select threshold have score 0 and are never emitted
    probs = np.zeros((1, 3, 2), f32)
    probs[0, :, 1] = [0.05, 0.5, 0.09]
    boxes = np.array([[[0, 0, 1, 1], [2, 2, 3, 3], [4, 4, 5, 5]]], f32)
    s, b, info = sr.soft_detected_bboxes(probs, boxes, 0.1, 0.4, 3, 3, 'gaussian')
    assert info[(0, 1)] == ([1], sr.EXHAUSTED)
    np.testing.assert_array_equal(s[0, 0], np.array([0.5, 0, 0], f32))
    assert not b[0, 0, 1:].any()


def _call(method, sigma, min_score):
    from rod import _abi
    return _abi.call('rod_select_topk_softnms', None, None, 1, 10, 3, 0.1, 4, 2, 0.4, method, sigma, min_score,
                     None, None, None, None)


@pytest.mark.parametrize('method', [0, 3, -1])
def test_abi_rejects_bad_method(method):
    with pytest.raises(RuntimeError, match='method'):
        _call(method, 0.5, 0.001)


@pytest.mark.parametrize('sigma', [0.0, -1.0, float('inf'), float('nan')])
def test_abi_rejects_bad_sigma(sigma):
    with pytest.raises(RuntimeError, match='sigma'):
        _call(2, sigma, 0.001)


@pytest.mark.parametrize('min_score', [-0.5, float('inf'), float('nan')])
def test_abi_rejects_bad_min_score(min_score):
    for method in (1, 2):
        with pytest.raises(RuntimeError, match='min_score'):
            _call(method, 0.5, min_score)


def test_abi_limits_match_the_hard_entry():
    from rod import _abi
    with pytest.raises(RuntimeError, match='top_k'):
        _abi.call('rod_select_topk_softnms', None, None, 1, 10, 3, 0.1, 1025, 2, 0.4, 1, 0.5, 0.001, None, None,
                  None, None)
    with pytest.raises(RuntimeError, match='keep_top_k'):
        _abi.call('rod_select_topk_softnms', None, None, 1, 10, 3, 0.1, 4, 0, 0.4, 1, 0.5, 0.001, None, None,
                  None, None)
    with pytest.raises(RuntimeError, match='bad shape'):
        _abi.call('rod_select_topk_softnms', None, None, 1, 10, 1, 0.1, 4, 2, 0.4, 1, 0.5, 0.001, None, None,
                  None, None)


def test_cli_defaults_are_hard_nms():
    import evaluate
    import predict
    for mod in (predict, evaluate):
        F = mod.parse([])
        assert (F.nms_method, F.soft_nms_sigma, F.soft_nms_min_score) == ('hard', 0.5, 0.001)
        F = mod.parse(['--nms_method=gaussian', '--soft_nms_sigma=0.3', '--soft_nms_min_score=0.01'])
        assert (F.nms_method, F.soft_nms_sigma, F.soft_nms_min_score) == ('gaussian', 0.3, 0.01)
        with pytest.raises(SystemExit):
            mod.parse(['--nms_method=bogus'])


def test_host_layers_reject_an_unknown_method():
    import torch

    from rod import ops, roofline
    from utils import net_tools
    with pytest.raises(ValueError, match='nms_method'):
        net_tools.detected_bboxes(None, None, nms_method='bogus')
    with pytest.raises(ValueError, match='method'):
        ops.select_topk_soft_nms(torch.zeros(1, 4, 3), torch.zeros(1, 4, 4), 0.1, 4, 2, 0.4, 'hard')
    assert ops.SOFT_NMS_METHODS == {'linear': 1, 'gaussian': 2}
    args = (0, 0, 2, 1000, 11, 0.1, 400, 200, 0.4, 2, 0.5, 0.001, 0, 0, 0, 0)
    nbytes, flops = roofline.cost('rod_select_topk_softnms', args)
    assert nbytes == roofline.cost('rod_select_topk_nms', args[:9] + (0, 0, 0, 0))[0] and flops > 0
