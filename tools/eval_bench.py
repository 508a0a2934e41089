"""Cost of evaluate.py's loop AFTER the network forward — per-class NMS, TP/FP matching against
the ground truth and accumulation — per batch, at B=8 images of 720x1280, bf16 network, on
synthetic BDD-shaped batches with a detector-like score distribution (rod.data):

  host      --match_on host, the default and the parent's behaviour: the NMS kernel, a device ->
            host copy of every class's scores and boxes (a sync), the Python matching loop of
            utils/tf_extended/bboxes.py at ONE threshold, StreamingTPFP on the host
  device    --match_on device: the NMS kernel, rod_match_detections, SweepTPFP.update — nothing
            leaves the GPU; measured at T=1 (one threshold) and T=10 (the 0.50:0.05:0.95 sweep)
  area      --ap_area_ranges coco --ap_iou_sweep coco: the NMS kernel, rod_match_detections_area
            over the all-range slot and COCO's four ranges (R=5, T=10), SweepTPFP.update per range

    python tools/eval_bench.py [--batches 8] [--rounds 7] [--out profiles/evalmatch_bench.json]

The class probabilities and decoded boxes of `batches` different synthetic batches are computed
once (the forward is not in the figure).  One round runs the loop body over all of them, with a
device synchronisation before the clock starts and after the last batch only; the paths
alternate within a round, after a warm-up round, and the median round is reported with the
spread, as seconds per batch.  `device_*_final_s` is the one device -> host copy plus the host AP
arithmetic at the end of a run of `batches` batches (paid once per run, not per batch).
`match_kernel_us` is rod_match_detections alone, device events around back-to-back launches;
`area_R5_T10` there is rod_match_detections_area alone, measured the same way in the same run (the
value to read it against is `T10`).  The default evaluator runs none of the area code.
No pass condition: the question this answers is whether T=10 on the device costs no more than
T=1 on the host.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'road-object-detection-for-bdd100k_amd'), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import config  # noqa: E402
import evaluate  # noqa: E402
from rod import ops  # noqa: E402
from rod.data import detector_like_scores, synthetic_batch  # noqa: E402
from utils import net_tools  # noqa: E402
import utils.tf_extended as tfe  # noqa: E402

KW = dict(select_threshold=0.3, nms_threshold=0.4, top_k=400, keep_top_k=200)   # evaluate.py's defaults


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200, help='back-to-back launches for match_kernel_us')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'evalmatch_bench.json'))
    a = ap.parse_args()
    import predict
    dev = torch.device('cuda', 0)
    B, hw = 8, (720, 1280)
    pr = predict.Predictor(hw, dev, torch.bfloat16, seed=61, select_threshold=KW['select_threshold'])
    detector_like_scores(pr, synthetic_batch(B, hw[0], hw[1], dev, seed=100)[0], rate=0.10)
    pr.keep_intermediates = True
    data = []
    for k in range(a.batches):
        img, gboxes, glabels, gn = synthetic_batch(B, hw[0], hw[1], dev, seed=200 + k)
        pr(img)
        data.append((pr.last[1].clone(), pr.last[2].clone(), gboxes, glabels, gn))
    classes = list(range(1, config.total_obj_n))
    kept = float(np.mean([(net_tools.detected_bboxes_packed(p, b, **KW)[0] > 0).float().sum().item() / B
                          for p, b, _, _, _ in data]))

    def host_run():
        state = None
        for probs, boxes, gboxes, glabels, gn in data:
            rscores, rbboxes = net_tools.detected_bboxes(probs, boxes, **KW)
            rs = {c: v.cpu().numpy() for c, v in rscores.items()}
            rb = {c: v.cpu().numpy() for c, v in rbboxes.items()}
            gl, gb, gcount = glabels.cpu().numpy(), gboxes.cpu().numpy(), gn.cpu().numpy()
            n_g, tp, fp, _ = tfe.bboxes_matching_batch(classes, rs, rb, gl, gb, np.zeros_like(gl),
                                                       matching_threshold=0.5, gt_counts=gcount)
            state = tfe.streaming_tp_fp_arrays(n_g, tp, fp, rs, state=state)
        return state

    def device_run(thr):
        acc = tfe.SweepTPFP(thr, len(classes), a.batches * B, KW['keep_top_k'], dev, first_label=classes[0])

        def run():
            acc.count = 0
            for probs, boxes, gboxes, glabels, gn in data:
                s, bx = net_tools.detected_bboxes_packed(probs, boxes, **KW)
                acc.update(s, *ops.match_detections(s, bx, glabels, gboxes, gn, acc.thresholds_dev,
                                                    first_label=classes[0]))
            return acc
        return run
    sweep = np.linspace(0.5, 0.95, 10).astype(np.float32)
    # evaluate.py --ap_area_ranges coco at the 720x1280 frame: slot 0 is (-inf, +inf), as there
    names, px = evaluate.parse_area_ranges('coco')
    slots = np.concatenate([np.array([[-np.inf, np.inf]], np.float32), evaluate.area_ranges_normalised(px, hw)])

    def area_run():
        acc = tfe.SweepTPFP(sweep, len(classes), a.batches * B, KW['keep_top_k'], dev, first_label=classes[0],
                            area_ranges=slots)

        def run():
            acc.count = 0
            for probs, boxes, gboxes, glabels, gn in data:
                s, bx = net_tools.detected_bboxes_packed(probs, boxes, **KW)
                acc.update(s, *evaluate.match_by_area(ops, s, bx, glabels, gboxes, gn, acc.thresholds_dev,
                                                      acc.area_ranges_dev, classes[0]))
            return acc
        return run
    paths = {'host': host_run, 'device_T1': device_run(sweep[:1]), 'device_T10': device_run(sweep),
             'device_area_R5_T10': area_run()}
    times = {k: [] for k in paths}
    final = {k: [] for k in paths if k != 'host'}
    for r in range(a.rounds + 1):            # round 0 is the warm-up
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.batches
            if k != 'host':
                t0 = time.perf_counter()
                ap07, ap12 = out.average_precisions()
                fin = time.perf_counter() - t0
            if r:
                times[k].append(dt)
                if k != 'host':
                    final[k].append(fin)
    # the two paths give the same AP at 0.5
    state = host_run()
    ap07, ap12 = paths['device_T10']().average_precisions()
    area_value = paths['device_area_R5_T10']().value()
    area12 = tfe.sweep_average_precisions(area_value[0])[1]
    for c in classes:
        prec, rec = tfe.precision_recall(*state[c].value())
        assert tfe.average_precision_voc12(prec, rec) == ap12[0][c], c
        assert area12[0][c] == ap12[0][c], c            # the all-range slot is rod_match_detections' answer
    n_gt_by_area = {n: int(sum(v[0] for v in area_value[1 + r][0].values())) for r, n in enumerate(names)}

    kern = {}
    probs, boxes, gboxes, glabels, gn = data[0]
    s, bx = net_tools.detected_bboxes_packed(probs, boxes, **KW)
    for name, thr in (('T1', sweep[:1]), ('T10', sweep)):
        td = torch.from_numpy(thr).to(dev)
        for _ in range(10):
            ops.match_detections(s, bx, glabels, gboxes, gn, td)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            ops.match_detections(s, bx, glabels, gboxes, gn, td)
        e1.record()
        e1.synchronize()
        kern[name] = e0.elapsed_time(e1) * 1e3 / a.launches
    td, rd = torch.from_numpy(sweep).to(dev), torch.from_numpy(slots).to(dev)
    for _ in range(10):
        ops.match_detections_area(s, bx, glabels, gboxes, gn, td, rd)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.launches):
        ops.match_detections_area(s, bx, glabels, gboxes, gn, td, rd)
    e1.record()
    e1.synchronize()
    kern['area_R5_T10'] = e0.elapsed_time(e1) * 1e3 / a.launches

    med = {k: statistics.median(v) for k, v in times.items()}
    rec = {'device': torch.cuda.get_device_name(0),
           'shape': {'B': B, 'H': hw[0], 'W': hw[1], 'dtype': 'bf16', 'anchors': int(data[0][0].shape[1]),
                     'classes': len(classes), 'keep_top_k': KW['keep_top_k'], 'G': int(data[0][2].shape[1]),
                     'detections_kept_per_image': kept},
           'batches': a.batches, 'rounds': a.rounds,
           'timing': 'wall clock around the loop over `batches` batches, device sync before and after only; '
                     'paths alternate within a round, one warm-up round, median of rounds; seconds per batch',
           'seconds_per_batch': {k: {'median': med[k], 'min': min(v), 'max': max(v)} for k, v in times.items()},
           'device_T1_final_s': statistics.median(final['device_T1']),
           'device_T10_final_s': statistics.median(final['device_T10']),
           'device_area_R5_T10_final_s': statistics.median(final['device_area_R5_T10']),
           'area_ranges_px': {n: [lo, 'inf' if np.isinf(hi) else hi] for n, (lo, hi) in zip(names, px.tolist())},
           'n_gt_by_area': n_gt_by_area,
           'device_area_over_device_T10': med['device_area_R5_T10'] / med['device_T10'],
           'match_kernel_us': {'T1': kern['T1'], 'T10': kern['T10'], 'area_R5_T10': kern['area_R5_T10'],
                               'timing': 'device events around %d back-to-back eager launches (launch-bound '
                                         'when the kernel is shorter than a launch)' % a.launches},
           'host_over_device_T10': med['host'] / med['device_T10'],
           'device_T10_over_device_T1': med['device_T10'] / med['device_T1'],
           'claim_T10_device_no_more_than_T1_host': bool(med['device_T10'] <= med['host'])}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
