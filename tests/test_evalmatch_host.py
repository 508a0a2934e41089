"""AP over an IoU-threshold sweep, the parts that need no GPU: the numpy restatement of
rod_match_detections (tests/evalmatch_ref.py) against oracle.post.bboxes_matching on the
hand-made cases, the entry's argument checks (they return before any HIP call, as in
tests/test_abi.py), evaluate.py's new flags and the host half of SweepTPFP."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evalmatch_ref as er  # noqa: E402

f32 = np.float32


@pytest.fixture(scope='module')
def hand():
    boxes, gl, gb, gd, gcount = er.hand_cases()
    tp, fp, n_gt = er.match_detections(boxes, gl, gb, gcount, er.COCO, gd)
    return boxes, gl, gb, gd, gcount, tp, fp, n_gt


def test_restatement_equals_the_oracle_on_the_hand_cases(hand):
    boxes, gl, gb, gd, gcount, tp, fp, n_gt = hand
    B, C, N = tp.shape
    assert (B, C, N) == (4, 3, 70) and gl.shape[1] == 130 and list(gcount) == [0, 1, 65, 130]
    for b in range(B):
        g = int(gcount[b])
        for c in range(C):
            n, a, f = er.from_oracle(1 + c, boxes[b, c], gl[b, :g], gb[b, :g], gd[b, :g], er.COCO)
            assert n == n_gt[b, c], (b, c)
            np.testing.assert_array_equal(tp[b, c], a, err_msg=str((b, c)))
            np.testing.assert_array_equal(fp[b, c], f, err_msg=str((b, c)))


def _bits(mask):
    return [t for t in range(10) if mask >> t & 1]


def test_hand_cases_say_what_they_are_meant_to(hand):
    """The per-threshold ground of the sweep, read off the masks (thresholds .50 .55 ... .95)."""
    boxes, gl, gb, gd, gcount, tp, fp, n_gt = hand
    every = (1 << 10) - 1
    # no ground truth: FP in every bit, zero-padded rows included
    assert (tp[0] == 0).all() and (fp[0] == every).all() and (n_gt[0] == 0).all()
    # ground truth 0 difficult and of another class: nothing recorded, nothing counted
    assert (tp[1] == 0).all() and (fp[1] == 0).all() and (n_gt[1] == 0).all()
    t, f = tp[2, 0], fp[2, 0]
    # A (IoU 0.6) then B (0.9) then a later 0.95 on one ground truth
    assert _bits(t[0]) == [0, 1] and _bits(t[1]) == [2, 3, 4, 5, 6, 7] and _bits(t[66]) == [8]
    assert t[0] | f[0] == every and t[1] | f[1] == every and not t[0] & f[0]
    assert _bits(f[66]) == [0, 1, 2, 3, 4, 5, 6, 7, 9]
    # IoU exactly equal to a threshold does not match: the comparison is strict
    assert er.jaccard(boxes[2, 0, 2:4], gb[2, 60:61])[:, 0].tolist() == [0.5, 0.75]
    assert t[2] == 0 and f[2] == every                     # 0.5 > 0.5 is false at bit 0, and above
    # 0.75 matches at .50 ... .70 (the 0.5 box before it never matched: the ground truth is free), not at .75
    assert _bits(t[3]) == [0, 1, 2, 3, 4] and t[3] | f[3] == every
    # twins: the first index wins, the duplicate detection is FP, the twin stays unmatched
    assert t[4] == every and f[4] == 0 and t[5] == 0 and f[5] == every
    # a zero-area ground truth has IoU 0 with everything
    assert t[6] == 0 and f[6] == every and t[7] == 0 and f[7] == every
    # class-1 detection on a class-3 box: argmax 0 is a non-difficult box -> FP
    assert t[69] == 0 and f[69] == every
    assert n_gt[2].tolist() == [5, 0, 60]
    # class 3: every grid box found once in every bit, the ten repeats are FP
    assert (tp[2, 2, :60] == every).all() and (tp[2, 2, 60:] == 0).all() and (fp[2, 2, 60:] == every).all()
    # the random image: some matched difficult boxes (neither), TPs thinning out with the threshold
    neither = (tp[3] | fp[3]) == 0
    assert neither.any() and not neither.all()
    per_t = [(tp[3] >> k & 1).sum() for k in range(10)]
    assert per_t[0] > per_t[-1] and all(a >= b for a, b in zip(per_t, per_t[1:]))


def test_abi_version_is_28_or_later():
    from rod import _abi
    assert _abi.lib().rod_abi_version() >= 28
    assert 'rod_match_detections' in _abi.parse_header()


def _call(B=1, C=2, N=8, G=4, T=1, thresholds=0x1000):
    """Every pointer but thresholds is NULL: the checks below must reject the call before the
    pointers matter (no HIP call is made)."""
    from rod import _abi
    return _abi.call('rod_match_detections', None, None, None, None, None, None, thresholds, B, C, N, G, T, 1, None,
                     None, None, None)


@pytest.mark.parametrize('kw, msg', [(dict(T=0), 'T must be'), (dict(T=17), 'T must be'), (dict(N=1025), 'N must be'),
                                     (dict(N=0), 'N must be'), (dict(G=513), 'G must be'), (dict(G=-1), 'G must be'),
                                     (dict(B=65536), 'B too large'), (dict(B=0), 'bad shape'),
                                     (dict(C=0), 'bad shape'), (dict(thresholds=None), 'thresholds')])
def test_abi_limits_are_checked_before_any_hip_call(kw, msg):
    with pytest.raises(RuntimeError, match=msg):
        _call(**kw)


def test_cli_defaults_and_sweep_flags():
    import evaluate
    F = evaluate.parse([])
    assert F.match_on == 'host' and F.ap_iou_sweep == '' and F.sweep_thresholds.size == 0
    assert F.matching_threshold == 0.5 and F.match_thresholds.tolist() == [0.5]
    F = evaluate.parse(['--match_on=device'])
    assert F.match_on == 'device' and F.sweep_thresholds.size == 0 and F.match_thresholds.tolist() == [0.5]
    F = evaluate.parse(['--ap_iou_sweep=coco'])
    assert F.match_on == 'device'                        # implied
    assert F.sweep_thresholds.dtype == np.float32
    np.testing.assert_array_equal(F.sweep_thresholds, np.linspace(0.5, 0.95, 10).astype(np.float32))
    # 0.5 is --matching_threshold already: bit 0, not repeated
    np.testing.assert_array_equal(F.match_thresholds, np.linspace(0.5, 0.95, 10).astype(np.float32))
    F = evaluate.parse(['--ap_iou_sweep=0.5,0.75,0.75', '--matching_threshold=0.75', '--match_on=device'])
    assert F.sweep_thresholds.tolist() == [0.5, 0.75] and F.match_thresholds.tolist() == [0.75, 0.5]
    F = evaluate.parse(['--ap_iou_sweep=coco', '--matching_threshold=0.4'])
    assert F.match_thresholds.size == 11 and F.match_thresholds[0] == np.float32(0.4)
    assert [evaluate.iou_key(t) for t in F.sweep_thresholds[:3]] == ['0.50', '0.55', '0.60']
    sixteen = ','.join('%.2f' % (0.21 + 0.05 * i) for i in range(16))   # 0.21 ... 0.96: no 0.5
    assert evaluate.parse(['--ap_iou_sweep=' + sixteen, '--matching_threshold=0.21']).match_thresholds.size == 16
    for bad in (['--ap_iou_sweep=' + sixteen],                      # 16 + the 0.5 default = 17
                ['--ap_iou_sweep=coco', '--match_on=host'],
                ['--ap_iou_sweep=0.5,abc'], ['--ap_iou_sweep=1.5'], ['--match_on=gpu']):
        with pytest.raises(SystemExit):
            evaluate.parse(bad)


def test_sweep_accumulator_host_half_matches_voc_ap():
    """SweepTPFP on the CPU, fed hand-written masks in two batches: per threshold and class the
    AP of oracle.post.voc_ap over the rows the reference keeps (tp or fp, score > 1e-4), 1e-12."""
    import torch

    from oracle.post import voc_ap
    from utils.tf_extended.metrics import SweepTPFP
    rng = np.random.default_rng(3)
    T, C, N, B = 3, 2, 6, 5
    thr = np.array([0.5, 0.75, 0.9], np.float32)
    scores = np.sort(rng.random((B, C, N)).astype(np.float32), -1)[..., ::-1].copy()
    scores[:, :, -1] = 0                    # zero padding
    scores[0, 0, 3] = 5e-5                  # below the 1e-4 cut
    scores[1, 1, 2] = scores[1, 1, 1]       # a tie: kept in batch order
    kind = rng.integers(0, 3, (B, C, N, T))   # 0 neither, 1 tp, 2 fp
    tpm = ((kind == 1) << np.arange(T)).sum(-1).astype(np.int32)
    fpm = ((kind == 2) << np.arange(T)).sum(-1).astype(np.int32)
    n_gt = rng.integers(0, 4, (B, C)).astype(np.int32)
    acc = SweepTPFP(thr, C, B + 1, N, 'cpu', first_label=3)
    for lo, hi in ((0, 2), (2, 5)):
        acc.update(*(torch.from_numpy(a[lo:hi]) for a in (scores, tpm, fpm, n_gt)))
    with pytest.raises(ValueError, match='capacity'):
        acc.update(*(torch.from_numpy(a[:2]) for a in (scores, tpm, fpm, n_gt)))
    ap07, ap12 = acc.average_precisions()
    assert len(ap07) == len(ap12) == T and sorted(ap07[0]) == [3, 4]
    seen = set()
    for t in range(T):
        for c in range(C):
            keep = ((kind[:, c, :, t] > 0) & (scores[:, c] > np.float32(1e-4))).reshape(-1)
            tp = (kind[:, c, :, t] == 1).reshape(-1)[keep].tolist()
            fp = (kind[:, c, :, t] == 2).reshape(-1)[keep].tolist()
            sc = [float(s) for s in scores[:, c].reshape(-1)[keep]]
            ng = int(n_gt[:, c].sum())
            assert ap07[t][3 + c] == pytest.approx(voc_ap(tp, fp, sc, ng, True), abs=1e-12)
            assert ap12[t][3 + c] == pytest.approx(voc_ap(tp, fp, sc, ng, False), abs=1e-12)
            seen.add(round(ap12[t][3 + c], 9))
    assert len(seen) > 3    # the thresholds and classes really differ
    with pytest.raises(ValueError, match='thresholds'):
        SweepTPFP(np.zeros(17, np.float32), C, 1, N, 'cpu')


def test_packed_helper_rejects_an_unknown_method():
    from utils import net_tools
    with pytest.raises(ValueError, match='nms_method'):
        net_tools.detected_bboxes_packed(None, None, nms_method='bogus')
