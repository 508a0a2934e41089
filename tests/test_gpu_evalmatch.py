"""rod_match_detections (ABI 28) on the GPU: bit-exact against the numpy restatement
(tests/evalmatch_ref.py, itself checked against oracle.post.bboxes_matching in
tests/test_evalmatch_host.py) on the hand-made edge cases, at the limits, on a random clustered
case and under graph capture; then evaluate.py end to end with --ap_iou_sweep coco against
oracle.post.streaming_ap at every threshold."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evalmatch_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def run_kernel(dev, boxes, gl, gb, gd, gcount, thr, first_label=1):
    from rod import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    scores = torch.zeros(boxes.shape[:3], dtype=torch.float32, device=dev)   # no decision reads them
    tp, fp, n = ops.match_detections(scores, t(boxes), t(gl), t(gb), t(gcount), t(np.asarray(thr, np.float32)),
                                     None if gd is None else t(gd), first_label=first_label)
    assert tp.dtype == fp.dtype == n.dtype == torch.int32
    return tp.cpu().numpy(), fp.cpu().numpy(), n.cpu().numpy()


def check(dev, case, thr, use_difficult=True, first_label=1):
    boxes, gl, gb, gd, gcount = case
    gd = gd if use_difficult else None
    want = er.match_detections(boxes, gl, gb, gcount, thr, gd, first_label=first_label)
    got = run_kernel(dev, boxes, gl, gb, gd, gcount, thr, first_label=first_label)
    for name, g, w in zip(('tp_mask', 'fp_mask', 'n_gt'), got, want):
        np.testing.assert_array_equal(g, w, err_msg=name)
    return want


def test_hand_made_cases_bit_exact(dev):
    """B=4, C=3, N=70 (two waves, not a multiple of 64), G=130, counts 0 / 1 / 65 / 130, the
    ten-threshold sweep; NaN boxes and valid-looking labels in the rows >= gt_count."""
    case = er.hand_cases()
    assert case[0].shape == (4, 3, 70, 4) and case[2].shape == (4, 130, 4) and np.isnan(case[2]).any()
    tp, fp, n_gt = check(dev, case, er.COCO)
    every = (1 << 10) - 1
    assert (fp[0] == every).all() and (tp[1] | fp[1] == 0).all()     # no ground truth / difficult box 0
    assert tp[2, 0, 0] == 0b11 and tp[2, 0, 1] == 0b11111100 and tp[2, 0, 2] == 0   # A, B, the exact 0.5
    assert tp[2, 0, 4] == every and fp[2, 0, 5] == every                            # the twins


@pytest.mark.parametrize('T', [1, 16])
def test_threshold_count_limits(dev, T):
    thr = np.linspace(0.3, 0.97, T).astype(np.float32) if T > 1 else np.array([0.5], np.float32)
    case = er.clustered_case(B=2, C=2, N=100, G=40, seed=T)
    tp, fp, _ = check(dev, case, thr, use_difficult=(T > 1), first_label=1)
    assert tp.max() < (1 << T) and fp.max() == (1 << T) - 1 and tp.any()


def test_largest_shape_once(dev):
    """N=1024 (four detections per thread), G=512 (the whole LDS table), T=10."""
    case = er.clustered_case(B=2, C=2, N=1024, G=512, seed=11)
    case[4][:] = [512, 301]
    tp, fp, n_gt = check(dev, case, er.COCO)
    assert n_gt.sum() > 400 and (tp & 1).sum() > 100


def test_random_clustered_case(dev):
    """Detections jittered around the ground truth at three scales: contested boxes, TPs that
    move between detections as the threshold rises; labels offset by first_label."""
    boxes, gl, gb, gd, gcount = er.clustered_case(B=3, C=4, N=200, G=64, seed=2024)
    gcount[0] = 0
    tp, fp, _ = check(dev, (boxes, gl + 4, gb, gd, gcount), er.COCO, first_label=5)
    per_t = [int((tp >> t & 1).sum()) for t in range(10)]
    print('TPs per threshold', per_t)
    assert per_t[0] > per_t[5] > per_t[9] > 0
    moved = ((tp != 0) & (fp != 0)).sum()      # TP at some thresholds, FP at others
    assert moved > 0


def test_graph_capture_replays_with_new_inputs(dev):
    from rod import ops
    cases = [er.clustered_case(B=2, C=3, N=150, G=48, seed=s) for s in (1, 2, 3)]
    thr = torch.from_numpy(er.COCO).to(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    static = [t(a) for a in cases[0]]            # boxes, labels, gboxes, difficult, count
    scores = torch.zeros(cases[0][0].shape[:3], dtype=torch.float32, device=dev)

    def op():
        return ops.match_detections(scores, static[0], static[1], static[2], static[4], thr, static[3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op()                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op()
    for case in cases[1:]:
        for dst, src in zip(static, case):
            dst.copy_(t(src))
        graph.replay()
        got = [o.cpu().numpy() for o in out]
        eager = [o.cpu().numpy() for o in op()]
        want = er.match_detections(case[0], case[1], case[2], case[4], er.COCO, case[3])
        for g, e, w in zip(got, eager, want):
            np.testing.assert_array_equal(g, e)
            np.testing.assert_array_equal(g, w)


def test_evaluate_sweep_end_to_end(dev, tmp_path):
    """The fixture recipe of tests/test_gpu_eval.py (8 images, 300x300, batch 4, a detector-like
    score distribution).  evaluate.py with the defaults and with --ap_iou_sweep coco: the
    reference's outputs are identical (==), every *_by_iou entry is oracle.post.streaming_ap at
    that float32 threshold (1e-12) over the kernel's detections (bit-exact to the oracle's NMS:
    tests/test_gpu_eval.py), the sweep keys are the documented ones and the default run's keys
    are today's."""
    import config
    import evaluate
    import predict
    from nets.catch_net import factory
    from oracle import post as op
    from rod.checkpoint import save_variables
    from rod.data import detector_like_scores
    from rod.dataio import make_source, network_input
    from utils import net_tools
    ds = os.path.join(GOLD, 'tfrecord')
    hw, bs, n_img = (300, 300), 4, 8
    pr = predict.Predictor(hw, dev, torch.float32, seed=61, select_threshold=0.3)
    probe = next(make_source(ds, 8, hw, dev, dtype=torch.float32, max_images=n_img))[0]
    detector_like_scores(pr, probe, rate=0.10)
    ck = str(tmp_path / 'ck' / 'mobilenet_v2.model')
    save_variables(pr.net.store, ck, 0)
    common = ['--img_height=300', '--img_width=300', '--dataset_dir=' + ds, '--batch_size=%d' % bs,
              '--num_images=%d' % n_img, '--checkpoint_path=' + os.path.dirname(ck)]
    evs = []
    for name, extra in (('host', []), ('sweep', ['--ap_iou_sweep=coco'])):
        edir = str(tmp_path / name)
        evaluate.main(common + ['--eval_dir=' + edir] + extra)
        evs.append(json.load(open(os.path.join(edir, 'eval.json'))))
    host, sweep = evs
    assert sorted(host) == ['AP_VOC07', 'AP_VOC12', 'checkpoint', 'mAP_VOC07', 'mAP_VOC12', 'num_batches', 'seconds',
                            'synthetic']
    new = ['AP_VOC07_by_iou', 'AP_VOC12_by_iou', 'iou_thresholds', 'mAP_VOC07_by_iou', 'mAP_VOC07_sweep',
           'mAP_VOC12_by_iou', 'mAP_VOC12_sweep']
    assert sorted(sweep) == sorted(list(host) + new)
    for k in ('AP_VOC07', 'AP_VOC12', 'mAP_VOC07', 'mAP_VOC12'):
        assert sweep[k] == host[k], k
    thr = np.linspace(0.5, 0.95, 10).astype(np.float32)
    assert sweep['iou_thresholds'] == [float(t) for t in thr]
    keys = ['%.2f' % t for t in thr]
    assert list(sweep['AP_VOC12_by_iou']) == keys and keys[0] == '0.50' and keys[-1] == '0.95'

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
            rs, rb = net_tools.detected_bboxes(probs, boxes, select_threshold=0.3, nms_threshold=0.4, top_k=400,
                                               keep_top_k=200)
            batches.append(({c: rs[c].cpu().numpy() for c in classes}, {c: rb[c].cpu().numpy() for c in classes},
                            gl.cpu().numpy(), gb.cpu().numpy(), gn.cpu().numpy()))
    tps = []
    for k, t in zip(keys, thr):
        ap07, ap12, cnt = op.streaming_ap(batches, classes, np.float32(t), counts=True)
        print('IoU>%s (tp, fp, n_gt) per class' % k, cnt)
        tps.append([cnt[c][0] for c in classes])
        for c in classes:
            assert sweep['AP_VOC07_by_iou'][k][str(c)] == pytest.approx(ap07[c], abs=1e-12), (k, c)
            assert sweep['AP_VOC12_by_iou'][k][str(c)] == pytest.approx(ap12[c], abs=1e-12), (k, c)
        assert sweep['mAP_VOC07_by_iou'][k] == pytest.approx(sum(ap07.values()) / len(classes), abs=1e-12)
        assert sweep['mAP_VOC12_by_iou'][k] == pytest.approx(sum(ap12.values()) / len(classes), abs=1e-12)
    assert sweep['mAP_VOC12_sweep'] == pytest.approx(np.mean([sweep['mAP_VOC12_by_iou'][k] for k in keys]), abs=1e-12)
    assert sweep['mAP_VOC07_sweep'] == pytest.approx(np.mean([sweep['mAP_VOC07_by_iou'][k] for k in keys]), abs=1e-12)
    tps = np.array(tps)
    print('total TP per threshold', tps.sum(1).tolist())
    assert (np.diff(tps, axis=0) <= 0).all()       # per class, non-increasing in t
    assert tps[0].sum() > 0
