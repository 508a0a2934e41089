"""AP by object-size range, the parts that need no GPU: the two forms of the numpy restatement
of rod_match_detections_area (tests/areamatch_ref.py) against each other and against
evalmatch_ref on the all range, the properties of the rule (partition, the bound on the equality
edge, matched-to-ignored, no ground truth), evaluate.py's new flags, the host half of SweepTPFP
with ranges and the entry's argument checks (they return before any HIP call)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import areamatch_ref as ar  # noqa: E402
import evalmatch_ref as er  # noqa: E402

f32 = np.float32
INF = np.inf


@pytest.fixture(scope='module')
def hand():
    case = er.hand_cases()
    return case, er.match_detections(case[0], case[1], case[2], case[4], er.COCO, case[3])


@pytest.fixture(scope='module')
def clustered():
    case = er.clustered_case(B=2, C=3, N=150, G=48, seed=1)
    return case, er.match_detections(case[0], case[1], case[2], case[4], er.COCO, case[3])


def area_match(case, ranges, thr=er.COCO, **kw):
    boxes, gl, gb, gd, gcount = case
    return ar.match_detections_area(boxes, gl, gb, gcount, thr, ranges, gd, **kw)


def test_vectorised_form_equals_the_sequential_form(hand, clustered):
    for (case, (tp_all, fp_all, _)), ranges in ((hand, ar.hand_ranges(hand[0])),
                                                (clustered, ar.clustered_ranges(clustered[0], 4, er.COCO))):
        vec = area_match(case, ranges)
        seq = area_match(case, ranges, one=ar.match_one_area_sequential)
        for name, v, s in zip(('tp_mask', 'fp_mask', 'n_gt'), vec, seq):
            np.testing.assert_array_equal(v, s, err_msg=name)
        assert ar.input_conditions(ranges, *vec, tp_all, fp_all) == []


def test_the_all_range_is_evalmatch_exactly(hand, clustered):
    for case, want in (hand, clustered):
        for one in (ar.match_one_area, ar.match_one_area_sequential):
            got = area_match(case, [ar.ALL], one=one)
            for name, g, w in zip(('tp_mask', 'fp_mask', 'n_gt'), got, want):
                assert g.shape == (1,) + w.shape
                np.testing.assert_array_equal(g[0], w, err_msg=name)


def test_disjoint_ranges_that_cover_the_line_partition_the_true_positives(hand, clustered):
    for (case, (tp_all, _, n_all)), ranges in ((hand, ar.hand_ranges(hand[0])),
                                               (clustered, [[-INF, 0.01], [0.01, 0.04], [0.04, INF]])):
        tp, fp, n_gt = area_match(case, ranges)
        np.testing.assert_array_equal(n_gt.sum(0), n_all)
        np.testing.assert_array_equal(np.bitwise_or.reduce(tp, axis=0), tp_all)
        for r in range(len(tp)):
            for q in range(r):
                assert not (tp[r] & tp[q]).any(), (q, r)
        assert sum(bool(t.any()) for t in tp) >= 2       # the true positives really are split


def test_a_bound_equal_to_an_area_is_inside_from_below_and_outside_from_above(hand):
    case, _ = hand
    grid = ar.area(case[2][2, :60])
    a = ar.hand_ranges(case)[1, 0]
    on_edge = np.nonzero(grid == a)[0]
    assert on_edge.size and on_edge.size < 60 and a.dtype == f32
    inside = ar.in_range(grid, [[a, INF], [-INF, a]])
    assert inside[0, on_edge].all() and not inside[1, on_edge].any()
    # and through the matcher: class 3 of image 2 finds every grid box once (tests/evalmatch_ref.py);
    # detection i sits on grid box 59 - i
    tp, fp, n_gt = area_match(case, [[a, INF], [-INF, a]])
    assert n_gt[0, 2, 2] + n_gt[1, 2, 2] == 60 and n_gt[0, 2, 2] == (grid >= a).sum()
    every = (1 << 10) - 1
    for j in on_edge:
        assert tp[0, 2, 2, 59 - j] == every and tp[1, 2, 2, 59 - j] == 0 and fp[1, 2, 2, 59 - j] == 0


def test_matched_to_ignored_ground_truth_is_neither_until_the_match_is_lost():
    """A 0.2 x 0.2 detection (area 0.04, in range) on a 0.2 x 0.25 ground truth (area 0.05, out
    of range): IoU 0.8 -> matched at 0.5 ... 0.75, where it is neither; at 0.8 and above it no
    longer matches and is an FP of the range its own area lies in."""
    gb = np.array([[[0.1, 0.1, 0.3, 0.35]]], f32)
    boxes = np.array([[[[0.1, 0.1, 0.3, 0.3]]]], f32)
    gl, gcount, gd = np.array([[1]], np.int32), np.array([1], np.int32), np.zeros((1, 1), np.uint8)
    jac = er.jaccard(boxes[0, 0], gb[0])[0, 0]
    lost = int((er.COCO < jac).sum())          # thresholds below the IoU match (strict)
    assert 0 < lost < 10
    low, high = (1 << lost) - 1, ((1 << 10) - 1) & ~((1 << lost) - 1)
    assert ar.area(boxes)[0, 0, 0] < f32(0.045) < ar.area(gb)[0, 0]
    for one in (ar.match_one_area, ar.match_one_area_sequential):
        tp, fp, n_gt = ar.match_detections_area(boxes, gl, gb, gcount, er.COCO, [[0, 0.045], [0.045, INF], ar.ALL], gd,
                                                one=one)
        assert n_gt[:, 0, 0].tolist() == [0, 1, 1]
        assert tp[0, 0, 0, 0] == 0 and fp[0, 0, 0, 0] == high          # detection in, ground truth out
        assert tp[1, 0, 0, 0] == low and fp[1, 0, 0, 0] == 0           # ground truth in, detection out
        assert tp[2, 0, 0, 0] == low and fp[2, 0, 0, 0] == high


def test_without_ground_truth_only_in_range_detections_are_false_positives(hand):
    case, _ = hand
    tp, fp, n_gt = area_match(case, [[0.05, INF], [-INF, 0.05]])
    inside = ar.area(case[0][0]) >= f32(0.05)
    assert inside.any() and not inside.all()
    every = (1 << 10) - 1
    assert (tp[:, 0] == 0).all() and (n_gt[:, 0] == 0).all()
    np.testing.assert_array_equal(fp[0, 0], np.where(inside, every, 0))
    np.testing.assert_array_equal(fp[1, 0], np.where(inside, 0, every))


def test_cli_area_range_flags():
    import evaluate
    F = evaluate.parse([])
    assert F.ap_area_ranges == '' and F.area_names == [] and F.area_ranges.shape == (0, 2) and F.match_on == 'host'
    F = evaluate.parse(['--ap_area_ranges=coco'])
    assert F.match_on == 'device' and F.area_image_size == (720, 1280)          # implied / default
    assert F.area_names == ['all', 'small', 'medium', 'large']
    assert F.area_ranges_px.tolist() == [[0, INF], [0, 1024], [1024, 9216], [9216, INF]]
    assert F.area_ranges.dtype == np.float32
    np.testing.assert_array_equal(F.area_ranges, ar.normalised(F.area_ranges_px, (720, 1280)))
    assert F.area_ranges[1, 1] == np.float32(np.float64(1024) / (720 * 1280)) and F.area_ranges[0, 1] == INF
    F = evaluate.parse(['--ap_area_ranges=tiny:0:400, rest:400:inf', '--ap_area_image_size=300,300',
                        '--ap_iou_sweep=0.5,0.75', '--match_on=device'])
    assert F.area_names == ['tiny', 'rest'] and F.area_image_size == (300, 300)
    np.testing.assert_array_equal(F.area_ranges, ar.normalised([[0, 400], [400, INF]], (300, 300)))
    eight = ','.join('r%d:%d:%d' % (i, i, i + 1) for i in range(8))
    assert len(evaluate.parse(['--ap_area_ranges=' + eight]).area_names) == 8
    for bad in (['--ap_area_ranges=small:0'], ['--ap_area_ranges=small:0:abc'], ['--ap_area_ranges=:0:1'],
                ['--ap_area_ranges=a:0:1,a:1:2'],                   # duplicate name
                ['--ap_area_ranges=a:5:5'], ['--ap_area_ranges=a:6:5'], ['--ap_area_ranges=a:nan:5'],
                ['--ap_area_ranges=' + eight + ',r8:8:9'],          # nine
                ['--ap_area_ranges=coco', '--match_on=host'],
                ['--ap_area_ranges=coco', '--ap_area_image_size=720'],
                ['--ap_area_ranges=coco', '--ap_area_image_size=0,1280']):
        with pytest.raises(SystemExit):
            evaluate.parse(bad)


def test_sweep_accumulator_with_ranges_matches_streaming_tpfp():
    """SweepTPFP(area_ranges=...) on the CPU, fed hand-written per-range masks in two batches:
    its tuples are StreamingTPFP's after the same bits, a (range, class) without ground truth
    has AP None and mean_ap skips it; without ranges the buffer and the outputs are today's."""
    import torch

    from utils.tf_extended.metrics import (StreamingTPFP, SweepTPFP, average_precision_voc07, average_precision_voc12,
                                           mean_ap, precision_recall)
    rng = np.random.default_rng(7)
    R, T, C, N, B = 3, 2, 2, 6, 5
    thr = np.array([0.5, 0.75], np.float32)
    ranges = np.array([[-INF, INF], [0, 0.01], [0.01, INF]], np.float32)
    scores = np.sort(rng.random((B, C, N)).astype(np.float32), -1)[..., ::-1].copy()
    scores[:, :, -1] = 0
    kind = rng.integers(0, 3, (R, B, C, N, T))   # 0 neither, 1 tp, 2 fp
    tpm = ((kind == 1) << np.arange(T)).sum(-1).astype(np.int32)
    fpm = ((kind == 2) << np.arange(T)).sum(-1).astype(np.int32)
    n_gt = rng.integers(1, 4, (R, B, C)).astype(np.int32)
    n_gt[1, :, 1] = 0                            # range 1 has no ground truth of the second class
    acc = SweepTPFP(thr, C, B, N, 'cpu', first_label=3, area_ranges=ranges)
    assert tuple(acc.buf.shape) == (B, C, N + R * (2 * N + 1)) and acc.area_ranges_dev.dtype == torch.float32
    for lo, hi in ((0, 2), (2, 5)):
        acc.update(torch.from_numpy(scores[lo:hi]), *(torch.from_numpy(a[:, lo:hi].copy()) for a in (tpm, fpm, n_gt)))
    with pytest.raises(ValueError, match='masks'):
        acc.update(torch.from_numpy(scores[:1]), torch.from_numpy(tpm[0, :1]), torch.from_numpy(fpm[0, :1]),
                   torch.from_numpy(n_gt[:, :1].copy()))
    value = acc.value()
    ap07, ap12 = acc.average_precisions(value)
    assert len(value) == len(ap07) == len(ap12) == R and len(value[0]) == len(ap07[0]) == T
    for r in range(R):
        for t in range(T):
            for c in range(C):
                st = StreamingTPFP()
                for lo, hi in ((0, 2), (2, 5)):
                    st.update(n_gt[r, lo:hi, c], kind[r, lo:hi, c, :, t] == 1, kind[r, lo:hi, c, :, t] == 2,
                              scores[lo:hi, c])
                want, got = st.value(), value[r][t][3 + c]
                assert got[:2] == want[:2]
                for g, w in zip(got[2:], want[2:]):
                    np.testing.assert_array_equal(g, w)
                if (r, c) == (1, 1):
                    assert want[0] == 0 and ap07[r][t][3 + c] is None and ap12[r][t][3 + c] is None
                else:
                    pr = precision_recall(*want)
                    assert ap07[r][t][3 + c] == average_precision_voc07(*pr)
                    assert ap12[r][t][3 + c] == average_precision_voc12(*pr)
    assert mean_ap(ap12[1][0]) == ap12[1][0][3] and mean_ap(ap12[0][0]) == (ap12[0][0][3] + ap12[0][0][4]) / 2
    assert mean_ap({1: None, 2: None}) is None

    # without ranges: today's layout, today's outputs (a number, not None, for a class without ground truth)
    plain = SweepTPFP(thr, C, B, N, 'cpu', first_label=3)
    assert plain.area_ranges is None and tuple(plain.buf.shape) == (B, C, 3 * N + 1)
    plain.update(*(torch.from_numpy(a) for a in (scores, tpm[1], fpm[1], n_gt[1])))
    v = plain.value()
    assert len(v) == T and sorted(v[0]) == [3, 4]
    for t in range(T):
        for c in range(C):
            for g, w in zip(v[t][3 + c], value[1][t][3 + c]):
                np.testing.assert_array_equal(g, w)
    p07, p12 = plain.average_precisions(v)
    assert isinstance(p07[0][4], float) and p12[0][4] == 0.0 and p12[0][3] == ap12[1][0][3]


def test_abi_version_is_31_or_later():
    from rod import _abi
    assert _abi.lib().rod_abi_version() >= 31
    assert 'rod_match_detections_area' in _abi.parse_header()


def _call(B=1, C=2, N=8, G=4, T=1, R=1, thresholds=0x1000, area_ranges=0x1000):
    """Every pointer but thresholds and area_ranges is NULL: the checks below must reject the call
    before the pointers matter (no HIP call is made)."""
    from rod import _abi
    return _abi.call('rod_match_detections_area', None, None, None, None, None, None, thresholds, area_ranges, B, C, N,
                     G, T, R, 1, None, None, None, None)


@pytest.mark.parametrize('kw, msg', [(dict(R=0), 'R must be'), (dict(R=9), 'R must be'),
                                     (dict(area_ranges=None), 'area_ranges'), (dict(T=17), 'T must be'),
                                     (dict(T=0), 'T must be'), (dict(N=1025), 'N must be'), (dict(G=513), 'G must be'),
                                     (dict(B=65536), 'B too large'), (dict(C=0), 'bad shape'),
                                     (dict(thresholds=None), 'thresholds')])
def test_abi_limits_are_checked_before_any_hip_call(kw, msg):
    with pytest.raises(RuntimeError, match=msg):
        _call(**kw)


def test_op_checks_area_ranges_dtype_and_shape():
    import torch

    from rod import ops
    z = torch.zeros
    args = (z(1, 2, 8), z(1, 2, 8, 4), z(1, 4, dtype=torch.int32), z(1, 4, 4), z(1, dtype=torch.int32), z(1))
    with pytest.raises(ValueError, match='area_ranges must be a float32'):
        ops.match_detections_area(*args, z(1, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match=r'\[R, 2\]'):
        ops.match_detections_area(*args, z(2))
