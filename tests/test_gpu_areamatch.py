"""rod_match_detections_area (ABI 31) on the GPU: bit-exact against the numpy restatement
(tests/areamatch_ref.py, whose two forms tests/test_areamatch_host.py holds against each other
and against evalmatch_ref) on the hand-made edge cases with bounds on the equality edge, at the
limits, at the largest shape, against rod_match_detections on the all range and under graph
capture; then evaluate.py end to end with --ap_area_ranges.

Every multi-range case is checked on the CPU first (areamatch_ref.input_conditions): each range
has a TP bit, an FP bit and a detection ignored only because of the range, and some (range,
class) has no ground truth."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import areamatch_ref as ar  # noqa: E402
import evalmatch_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def to_dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_kernel(dev, case, thr, ranges, use_difficult=True, first_label=1):
    from rod import ops
    boxes, gl, gb, gd, gcount = case
    scores = torch.zeros(boxes.shape[:3], dtype=torch.float32, device=dev)   # no decision reads them
    thr, ranges = np.asarray(thr, np.float32), np.asarray(ranges, np.float32)
    out = ops.match_detections_area(scores, to_dev(dev, boxes), to_dev(dev, gl), to_dev(dev, gb), to_dev(dev, gcount),
                                    to_dev(dev, thr), to_dev(dev, ranges),
                                    to_dev(dev, gd) if use_difficult else None, first_label=first_label)
    assert all(o.dtype == torch.int32 for o in out)
    return out


def check(dev, case, thr, ranges, use_difficult=True):
    """The restatement's masks, after the input conditions and the bit-exact comparison."""
    boxes, gl, gb, gd, gcount = case
    gd_ = gd if use_difficult else None
    want = ar.match_detections_area(boxes, gl, gb, gcount, thr, ranges, gd_)
    if len(ranges) > 1:
        tp_all, fp_all, _ = er.match_detections(boxes, gl, gb, gcount, thr, gd_)
        assert ar.input_conditions(ranges, *want, tp_all, fp_all) == []
    got = run_kernel(dev, case, thr, ranges, use_difficult)
    R, (B, C, N) = len(ranges), boxes.shape[:3]
    assert tuple(got[0].shape) == tuple(got[1].shape) == (R, B, C, N) and tuple(got[2].shape) == (R, B, C)
    for name, g, w in zip(('tp_mask', 'fp_mask', 'n_gt'), got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)
    return want


def test_hand_made_cases_bit_exact(dev):
    """B=4, C=3, N=70, G=130, counts 0 / 1 / 65 / 130, the ten-threshold sweep and four ranges that
    cover the line; two bounds are the exact float32 area of a grid box, so those boxes sit on the
    equality edge (inside from below, outside from above); NaN boxes in the rows >= gt_count."""
    case = er.hand_cases()
    assert case[0].shape == (4, 3, 70, 4) and case[2].shape == (4, 130, 4) and np.isnan(case[2]).any()
    ranges = ar.hand_ranges(case)
    grid = ar.area(case[2][2, :60])
    assert ranges.shape == (4, 2) and (grid == ranges[1, 0]).any() and (grid == ranges[2, 0]).any()
    tp, fp, n_gt = check(dev, case, er.COCO, ranges)
    every = (1 << 10) - 1
    assert (tp[:, 0] == 0).all() and ((fp[:, 0] == every).sum(0) == 1).all()    # no ground truth: FP of one range
    assert (tp[:, 1] | fp[:, 1] == 0).all()                                      # difficult box 0
    assert n_gt[:, 2, 2].tolist() == [int((grid < ranges[1, 0]).sum()), int((grid == ranges[1, 0]).sum()),
                                      int((grid == ranges[2, 0]).sum()), 0]
    on_edge = 59 - np.nonzero(grid == ranges[1, 0])[0]          # class 3: detection i sits on grid box 59 - i
    assert (tp[1, 2, 2, on_edge] == every).all() and (tp[0, 2, 2, on_edge] == 0).all()


def limit_case(R, T):
    thr = np.linspace(0.3, 0.97, T).astype(np.float32) if T > 1 else np.array([0.5], np.float32)
    case = er.clustered_case(B=2, C=2, N=100, G=40, seed=T)
    return case, thr, ar.clustered_ranges(case, R, thr)


@pytest.mark.parametrize('R, T', [(1, 1), (8, 16)])
def test_range_and_threshold_count_limits(dev, R, T):
    case, thr, ranges = limit_case(R, T)
    assert ranges.shape == (R, 2)
    tp, fp, _ = check(dev, case, thr, ranges, use_difficult=(T > 1))
    assert tp.max() < (1 << T) and fp.max() == (1 << T) - 1 and tp.any()


def test_largest_shape_once(dev):
    """N=1024 (four detections per thread), G=512 (the whole LDS table and range bytes), R=4, T=10."""
    case = er.clustered_case(B=2, C=2, N=1024, G=512, seed=11)
    case[4][:] = [512, 301]
    tp, fp, n_gt = check(dev, case, er.COCO, ar.clustered_ranges(case, 4, er.COCO))
    assert n_gt[0].sum() > 400 and (tp[0] & 1).sum() > 100


def test_all_range_slice_equals_match_detections_on_the_device(dev):
    from rod import ops
    case = er.clustered_case(B=3, C=4, N=200, G=64, seed=2024)
    case[4][0] = 0
    ranges = ar.clustered_ranges(case, 5, er.COCO)
    assert tuple(ranges[0]) == ar.ALL
    check(dev, case, er.COCO, ranges)
    boxes, gl, gb, gd, gcount = (to_dev(dev, a) for a in case)
    scores = torch.zeros(case[0].shape[:3], dtype=torch.float32, device=dev)
    thr = to_dev(dev, er.COCO)
    area = ops.match_detections_area(scores, boxes, gl, gb, gcount, thr, to_dev(dev, ranges), gd)
    plain = ops.match_detections(scores, boxes, gl, gb, gcount, thr, gd)
    for name, a, p in zip(('tp_mask', 'fp_mask', 'n_gt'), area, plain):
        assert torch.equal(a[0], p), name
    assert not torch.equal(area[0][2], plain[0])


def test_graph_capture_replays_with_new_inputs_and_new_ranges(dev):
    from rod import ops
    cases = [er.clustered_case(B=2, C=3, N=150, G=48, seed=s) for s in (1, 2, 3)]
    ranges = [ar.clustered_ranges(c, 4, er.COCO) for c in cases]
    assert not np.array_equal(ranges[1], ranges[2])
    thr = to_dev(dev, er.COCO)
    static = [to_dev(dev, a) for a in cases[0]]            # boxes, labels, gboxes, difficult, count
    static_ranges = to_dev(dev, ranges[0])
    scores = torch.zeros(cases[0][0].shape[:3], dtype=torch.float32, device=dev)

    def op():
        return ops.match_detections_area(scores, static[0], static[1], static[2], static[4], thr, static_ranges,
                                         static[3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op()                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op()
    for case, rg in zip(cases[1:], ranges[1:]):
        for dst, src in zip(static, case):
            dst.copy_(to_dev(dev, src))
        static_ranges.copy_(to_dev(dev, rg))
        graph.replay()
        got = [o.cpu().numpy() for o in out]
        eager = [o.cpu().numpy() for o in op()]
        want = ar.match_detections_area(case[0], case[1], case[2], case[4], er.COCO, rg, case[3])
        tp_all, fp_all, _ = er.match_detections(case[0], case[1], case[2], case[4], er.COCO, case[3])
        assert ar.input_conditions(rg, *want, tp_all, fp_all) == []
        for g, e, w in zip(got, eager, want):
            np.testing.assert_array_equal(g, e)
            np.testing.assert_array_equal(g, w)


def expected_by_area(batches, classes, thresholds, ranges, names, sweep_bits):
    """The *_by_area entries from the restatement's masks over the same packed detections, through
    StreamingTPFP / precision_recall / average_precision_voc07|12 on the host."""
    from utils.tf_extended.metrics import (StreamingTPFP, average_precision_voc07, average_precision_voc12,
                                           precision_recall)
    T = len(thresholds)
    st = [[[StreamingTPFP() for _ in classes] for _ in range(T)] for _ in names]
    for scores, boxes, gl, gb, gn in batches:
        tp, fp, n_gt = ar.match_detections_area(boxes, gl, gb, gn, thresholds, ranges, first_label=classes[0])
        for r in range(len(names)):
            for t in range(T):
                for ci in range(len(classes)):
                    st[r][t][ci].update(n_gt[r, :, ci], tp[r, :, ci] >> t & 1, fp[r, :, ci] >> t & 1, scores[:, ci])

    def aps(r, t, fn):
        out = {}
        for ci, c in enumerate(classes):
            v = st[r][t][ci].value()
            out[str(c)] = fn(*precision_recall(*v)) if v[0] else None
        return out

    def mean(vals):
        vals = [v for v in vals if v is not None]
        return sum(vals) / len(vals) if vals else None
    exp = {'n_gt_by_area': {}, 'recall_by_area': {}}
    for key, fn in (('VOC07', average_precision_voc07), ('VOC12', average_precision_voc12)):
        exp['AP_%s_by_area' % key] = {n: aps(r, 0, fn) for r, n in enumerate(names)}
        exp['mAP_%s_by_area' % key] = {n: mean(exp['AP_%s_by_area' % key][n].values()) for n in names}
        if sweep_bits:
            exp['mAP_%s_sweep_by_area' % key] = {n: mean([mean(aps(r, b, fn).values()) for b in sweep_bits])
                                                 for r, n in enumerate(names)}
    for r, n in enumerate(names):
        vals = [st[r][0][ci].value() for ci in range(len(classes))]
        exp['n_gt_by_area'][n] = {str(c): v[0] for c, v in zip(classes, vals)}
        exp['recall_by_area'][n] = {str(c): float(v[2].sum()) / v[0] if v[0] else None for c, v in zip(classes, vals)}
    return exp


def same(got, want, where):
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), where
        for k in want:
            same(got[k], want[k], where + (k,))
    elif want is None or isinstance(want, int):
        assert got == want, where
    else:
        assert got == pytest.approx(want, abs=1e-12), where


def test_evaluate_by_area_end_to_end(dev, tmp_path):
    """The fixture recipe of test_evaluate_sweep_end_to_end (8 golden TFRecord images, 300x300,
    batch 4, a detector-like score distribution).  evaluate.py with the defaults, with
    --ap_area_ranges alone (three ranges cut at the terciles of the fixture's own ground-truth
    areas) and with --ap_area_ranges (eight ranges: the all-range slot makes nine, two launches) plus
    --ap_iou_sweep=0.5,0.75: the default run's keys are today's, the shared keys are == across
    the runs, every *_by_area value is the host value from the restatement's masks over the
    same detections (1e-12)."""
    import config
    import evaluate
    import predict
    from rod.checkpoint import save_variables
    from rod.data import detector_like_scores
    from rod.dataio import make_source, network_input
    from nets.catch_net import factory
    from utils import net_tools
    ds = os.path.join(GOLD, 'tfrecord')
    hw, bs, n_img = (300, 300), 4, 8
    pr = predict.Predictor(hw, dev, torch.float32, seed=61, select_threshold=0.3)
    probe = next(make_source(ds, 8, hw, dev, dtype=torch.float32, max_images=n_img))[0]
    detector_like_scores(pr, probe, rate=0.10)
    ck = str(tmp_path / 'ck' / 'mobilenet_v2.model')
    save_variables(pr.net.store, ck, 0)

    classes = list(range(1, config.total_obj_n))
    src = make_source(ds, bs, hw, dev, dtype=torch.float32, max_images=n_img)
    batches = []
    with torch.no_grad():
        for _ in range(n_img // bs):
            img, gb, gl, gn = next(src)
            refine_out, det_out, clf_out = factory(network_input(img, torch.float32), 'mobilenet_v2', False,
                                                   pr.config_dict, torch.float32, net=pr.net).get_output()
            probs = net_tools.class_probabilities(clf_out)
            boxes = net_tools.decode_all_layers(pr.anchors, refine_out, det_out, to_corner=True)
            ps, pb = net_tools.detected_bboxes_packed(probs, boxes, select_threshold=0.3, nms_threshold=0.4, top_k=400,
                                                      keep_top_k=200)
            batches.append(tuple(a.cpu().numpy() for a in (ps, pb, gl, gb, gn)))

    # bounds from the fixture's own boxes: whole pixels^2 of the 300x300 frame at the terciles / octiles
    px = np.sort(np.concatenate([ar.area(gb[b, :int(gn[b])]) for _, _, _, gb, gn in batches for b in range(bs)])
                 .astype(np.float64) * (hw[0] * hw[1]))
    assert px.size >= 16 and px[0] >= 0
    c3 = [float(np.floor(px[px.size * k // 3])) for k in (1, 2)]
    c4 = sorted(set(float(np.floor(px[px.size * k // 8])) for k in (1, 3, 5, 7)))
    assert 0 < c3[0] < c3[1] and len(c4) == 4 and c4[0] > 0
    three = [('small', 0.0, c3[0]), ('medium', c3[0], c3[1]), ('large', c3[1], np.inf)]
    eight = three + [('all', -np.inf, np.inf)] + [('o%d' % k, lo, hi) for k, (lo, hi) in
                                                  enumerate(zip(c4[:-1] + [c4[-1]], c4[1:] + [np.inf]))]
    assert len(eight) == 8
    flag = lambda rg: '--ap_area_ranges=' + ','.join('%s:%r:%r' % r for r in rg)  # noqa: E731

    common = ['--img_height=300', '--img_width=300', '--dataset_dir=' + ds, '--batch_size=%d' % bs,
              '--num_images=%d' % n_img, '--checkpoint_path=' + os.path.dirname(ck)]
    size = '--ap_area_image_size=300,300'
    evs = []
    for name, extra in (('host', []), ('area', [flag(three), size]),
                        ('both', [flag(eight), size, '--ap_iou_sweep=0.5,0.75'])):
        edir = str(tmp_path / name)
        evaluate.main(common + ['--eval_dir=' + edir] + extra)
        evs.append(json.load(open(os.path.join(edir, 'eval.json'))))
    host, area, both = evs
    today = ['AP_VOC07', 'AP_VOC12', 'checkpoint', 'mAP_VOC07', 'mAP_VOC12', 'num_batches', 'seconds', 'synthetic']
    by_area = ['AP_VOC07_by_area', 'AP_VOC12_by_area', 'area_image_size', 'area_ranges', 'mAP_VOC07_by_area',
               'mAP_VOC12_by_area', 'n_gt_by_area', 'recall_by_area']
    sweep = ['AP_VOC07_by_iou', 'AP_VOC12_by_iou', 'iou_thresholds', 'mAP_VOC07_by_iou', 'mAP_VOC07_sweep',
             'mAP_VOC12_by_iou', 'mAP_VOC12_sweep', 'mAP_VOC07_sweep_by_area', 'mAP_VOC12_sweep_by_area']
    assert sorted(host) == today
    assert sorted(area) == sorted(today + by_area) and sorted(both) == sorted(today + by_area + sweep)
    for k in ('AP_VOC07', 'AP_VOC12', 'mAP_VOC07', 'mAP_VOC12', 'checkpoint', 'num_batches', 'synthetic'):
        assert area[k] == host[k] and both[k] == host[k], k
    assert both['AP_VOC12_by_iou']['0.50'] == host['AP_VOC12'] and both['AP_VOC07_by_iou']['0.50'] == host['AP_VOC07']
    assert sum(host['AP_VOC12'].values()) > 0

    n_all = {str(c): 0 for c in classes}
    for _, _, gl, gb, gn in batches:
        for b in range(bs):
            for l in gl[b, :int(gn[b])]:
                if str(int(l)) in n_all:
                    n_all[str(int(l))] += 1
    for ev, rg, thr, bits in ((area, three, [0.5], []), (both, eight, [0.5, 0.75], [0, 1])):
        names = [r[0] for r in rg]
        assert ev['area_image_size'] == [300, 300]
        assert ev['area_ranges'] == {n: [lo, hi] for n, lo, hi in rg}
        exp = expected_by_area(batches, classes, np.array(thr, np.float32),
                               ar.normalised([[lo, hi] for _, lo, hi in rg], hw), names, bits)
        for key, want in exp.items():
            print(key, ev[key])
            same(ev[key], want, (key,))
        n = ev['n_gt_by_area']
        assert sum(sum(n[k].values()) > 0 for k in ('small', 'medium', 'large')) >= 2       # really split
        assert {c: sum(n[k][c] for k in ('small', 'medium', 'large')) for c in n_all} == n_all
        assert any(v is None for k in names for v in ev['AP_VOC12_by_area'][k].values())    # the None path
        assert any(v is not None and v > 0 for k in names for v in ev['recall_by_area'][k].values())
    assert both['n_gt_by_area']['all'] == n_all
    for k in ('n_gt_by_area', 'AP_VOC07_by_area', 'AP_VOC12_by_area', 'recall_by_area'):
        for n in ('small', 'medium', 'large'):
            assert both[k][n] == area[k][n], (k, n)
