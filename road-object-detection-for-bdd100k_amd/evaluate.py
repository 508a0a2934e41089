"""mAP evaluation CLI — drop-in for the reference's evaluate.py (flags 37-69, flow 86-241).

ALL-mode network in inference mode -> softmax + decode(refine_out + det_out) ->
detected_bboxes (per-class select / top-k / NMS, one kernel) -> TP/FP matching against the
ground truth -> streaming TP/FP arrays -> VOC07 / VOC12 AP per class and their mean, over
ceil(3000 / batch_size) batches (evaluate.py:219).  Matching and AP are host code, as the
reference pins them to the CPU (evaluate.py:146, 164).

Opt-in (not in the reference): --match_on device matches on the GPU (rod_match_detections) and
keeps the TP/FP masks there until the end of the run — one device -> host copy instead of one
per batch; --ap_iou_sweep evaluates AP at several matching IoU thresholds from that one launch
per batch.  At every threshold the rule is the reference's own matching rule (bboxes_matching:
first argmax of IoU over same-label boxes, strict comparison, one TP per ground truth), not
pycocotools' rule, and AP is this project's VOC12 area / VOC07 11-point value — the mean over the
sweep is a mean of those, not the COCO metric.  --ap_area_ranges also reports AP and recall by
object-size range from that same launch (rod_match_detections_area): ground truth outside a range
is ignored, a detection matched to it is neither TP nor FP, an unmatched detection is an FP only
of the ranges its own area lies in — again on the reference's argmax, not pycocotools'
re-matching.  Without the new flags the run, its printout and eval.json are today's.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import config  # noqa: E402
from utils.common_tools import logger  # noqa: E402


def str2bool(v):
    return v if isinstance(v, bool) else str(v).lower() in ('1', 'true', 't', 'yes', 'y')


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--backbone_name', default='mobilenet_v2')
    ap.add_argument('--num_readers', type=int, default=4)
    ap.add_argument('--num_preprocessing_threads', type=int, default=4)
    ap.add_argument('--checkpoint_path', default='checkpoint/')
    ap.add_argument('--eval_dir', default='evaluation/')
    ap.add_argument('--batch_size', type=int, default=1)
    ap.add_argument('--select_threshold', type=float, default=0.3)
    ap.add_argument('--select_top_k', type=int, default=400)
    ap.add_argument('--keep_top_k', type=int, default=200)
    ap.add_argument('--nms_threshold', type=float, default=0.4)
    ap.add_argument('--matching_threshold', type=float, default=0.5)
    ap.add_argument('--gpu_memory_fraction', type=float, default=0.8)
    # additions
    ap.add_argument('--nms_method', default='hard', choices=['hard', 'linear', 'gaussian'],
                    help="'hard': the reference's greedy NMS; 'linear' / 'gaussian': Soft-NMS (overlapped "
                         'detections are rescored, not dropped; AP is computed on the rescored scores)')
    ap.add_argument('--soft_nms_sigma', type=float, default=0.5, help='gaussian Soft-NMS: exp(-iou^2 / sigma)')
    ap.add_argument('--soft_nms_min_score', type=float, default=0.001,
                    help='Soft-NMS stops emitting below this rescored score')
    ap.add_argument('--num_images', type=int, default=3000, help='evaluate.py:219 hard-codes 3000')
    ap.add_argument('--img_height', type=int, default=config.img_size[0])
    ap.add_argument('--img_width', type=int, default=config.img_size[1])
    ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--dataset_dir', default='./dataset/bdd100k_TfRecord/')
    ap.add_argument('--synthetic', type=str2bool, default=False,
                    help='run on synthetic BDD-shaped batches (no dataset needed); results are not real '
                         'metrics.  Without it a missing dataset or checkpoint is an error')
    ap.add_argument('--match_on', default=None, choices=['host', 'device'],
                    help="where detections are matched with the ground truth (default host: the reference's "
                         'per-batch host loop).  device: one HIP kernel per batch, TP/FP kept on the GPU, one '
                         'copy to the host at the end of the run; same matching rule, same AP')
    ap.add_argument('--ap_iou_sweep', default='',
                    help="also report AP at these matching IoU thresholds: 'coco' = 0.50:0.05:0.95 (10 values), or "
                         "a comma list such as 0.5,0.75.  Implies --match_on device.  Each threshold applies the "
                         "reference's matching rule (not pycocotools' rule) and AP stays this project's VOC12 area "
                         '/ VOC07 11-point value; at most %d distinct thresholds with --matching_threshold'
                         % MAX_THRESHOLDS)
    ap.add_argument('--ap_area_ranges', default='',
                    help="also report AP and recall by object-size range: 'coco' = %s, or a comma list "
                         "name:lo:hi in pixels^2 of the --ap_area_image_size frame (lo inclusive, hi exclusive, hi "
                         "may be inf; unique names, at most %d).  Implies --match_on device.  Ground truth outside "
                         "a range is ignored and a detection matched to it counts as neither TP nor FP, but a "
                         "detection still competes for the reference's argmax ground truth whether that box is "
                         "ignored or not (pycocotools re-matches toward non-ignored ground truth), and AP stays "
                         "this project's VOC value, not the COCO metric" % (COCO_AREA_RANGES, MAX_AREA_RANGES))
    ap.add_argument('--ap_area_image_size', default='720,1280',
                    help='H,W of the frame the pixel bounds of --ap_area_ranges refer to (the BDD100K frame): the '
                         'boxes are normalised, so an object lands in the same range at any network resolution')
    ap.add_argument('--use_ema', type=str2bool, default=False,
                    help='evaluate the averaged weights the checkpoint holds (train.py --ema_decay) in place of '
                         'the variables; an error if it holds none')
    F = ap.parse_args(argv)
    try:
        F.sweep_thresholds = parse_iou_sweep(F.ap_iou_sweep)
    except ValueError as e:
        ap.error('--ap_iou_sweep: %s' % e)
    try:
        F.area_names, F.area_ranges_px = parse_area_ranges(F.ap_area_ranges)
        F.area_image_size = parse_image_size(F.ap_area_image_size)
    except ValueError as e:
        ap.error('--ap_area_ranges / --ap_area_image_size: %s' % e)
    F.area_ranges = area_ranges_normalised(F.area_ranges_px, F.area_image_size)
    if F.sweep_thresholds.size or F.area_names:
        if F.match_on == 'host':
            ap.error('--ap_iou_sweep and --ap_area_ranges need --match_on device (the host loop matches at one '
                     'threshold and knows no ignored ground truth)')
        F.match_on = 'device'
    elif F.match_on is None:
        F.match_on = 'host'
    # bit 0 of the device masks is --matching_threshold (today's AP outputs); the sweep values follow
    base = np.float32(F.matching_threshold)
    F.match_thresholds = np.concatenate([[base], F.sweep_thresholds[F.sweep_thresholds != base]]).astype(np.float32)
    if F.match_thresholds.size > MAX_THRESHOLDS:
        ap.error('--ap_iou_sweep: %d distinct thresholds with --matching_threshold, at most %d'
                 % (F.match_thresholds.size, MAX_THRESHOLDS))
    return F


MAX_THRESHOLDS = 16   # bits of rod_match_detections' masks (include/rod.h)


def parse_iou_sweep(text):
    """'' -> no sweep; 'coco' -> np.linspace(0.5, 0.95, 10) as float32; else a comma list of
    thresholds in [0, 1), duplicates dropped, order kept.  float32 [n]."""
    text = text.strip()
    if not text:
        return np.zeros(0, np.float32)
    if text == 'coco':
        return np.linspace(0.5, 0.95, 10).astype(np.float32)
    vals = []
    for tok in text.split(','):
        v = np.float32(float(tok))    # ValueError on a malformed number
        if not 0 <= v < 1:
            raise ValueError('threshold %r is outside [0, 1)' % tok)
        if v not in vals:
            vals.append(v)
    return np.array(vals, np.float32)


MAX_AREA_RANGES = 8   # bits of rod_match_detections_area's per-row range byte (include/rod.h)
COCO_AREA_RANGES = 'all:0:inf,small:0:1024,medium:1024:9216,large:9216:inf'   # 32^2 and 96^2 pixels


def parse_area_ranges(text):
    """'' -> no ranges; 'coco' -> COCO_AREA_RANGES; else a comma list name:lo:hi (pixels^2, lo <
    hi, hi may be inf, unique names, at most MAX_AREA_RANGES).  ([name], float64 [n, 2])."""
    text = text.strip()
    if not text:
        return [], np.zeros((0, 2), np.float64)
    names, px = [], []
    for tok in (COCO_AREA_RANGES if text == 'coco' else text).split(','):
        parts = tok.split(':')
        if len(parts) != 3 or not parts[0].strip():
            raise ValueError('range %r is not name:lo:hi' % tok)
        name, lo, hi = parts[0].strip(), float(parts[1]), float(parts[2])   # ValueError on a malformed number
        if name in names:
            raise ValueError('range name %r is given twice' % name)
        if not lo < hi:      # rejects NaN bounds too
            raise ValueError('range %r: lo must be below hi' % tok)
        names.append(name)
        px.append((lo, hi))
    if len(names) > MAX_AREA_RANGES:
        raise ValueError('%d ranges, at most %d' % (len(names), MAX_AREA_RANGES))
    return names, np.array(px, np.float64)


def parse_image_size(text):
    parts = text.split(',')
    if len(parts) != 2:
        raise ValueError('image size %r is not H,W' % text)
    h, w = int(parts[0]), int(parts[1])
    if h <= 0 or w <= 0:
        raise ValueError('image size %r is not positive' % text)
    return h, w


def area_ranges_normalised(px, image_size):
    """Pixel^2 bounds [n, 2] -> the float32 bounds in the boxes' normalised area units."""
    h, w = image_size
    return np.float32(np.float64(px) / (h * w)).reshape(-1, 2)


def iou_key(t):
    """eval.json key of a threshold: two decimals ('0.50') when that names it exactly."""
    s = '%.2f' % t
    return s if np.float32(s) == np.float32(t) else repr(float(t))


def latest_checkpoint(path, backbone):
    """A torch checkpoint (train.py writes <train_dir>/<backbone>.model) or a TF-1.x tensor
    bundle (<prefix>.index + .data-*), as a directory or a file prefix."""
    from rod.checkpoint import exists
    if os.path.isdir(path):
        cand = os.path.join(path, backbone + '.model')
        if exists(cand):
            return cand
        from rod.checkpoint import tf_latest_checkpoint
        return tf_latest_checkpoint(path)
    return path if exists(path) else None


def main(argv=None):
    F = parse(argv)
    logger.info('Asserting parameters')
    assert F.backbone_name in config.supported_backbone_name
    from nets.catch_net import CatchNet, factory
    from rod.dataio import make_source, network_input
    from utils import net_tools
    from utils.common_tools import cornerBboxes_2_centerBboxes  # noqa: F401
    import utils.tf_extended as tfe

    dev = torch.device('cuda', 0)
    config.img_size = (F.img_height, F.img_width)
    dtype = torch.bfloat16 if F.dtype == 'bf16' else torch.float32
    layer_n = len(config.extract_feat_name[F.backbone_name])
    anchors_all = net_tools.anchors_all_layer(config.img_size, config.feat_sizes(config.img_size, F.backbone_name),
                                              net_tools.init_anchor(layer_n))
    config_dict = {'process_backbone_method': config.process_backbone_method.NONE,
                   'deconv_method': config.deconv_method.LEARN_HALF,
                   'merge_method': config.merge_method.ADD, 'train_range': config.train_range.ALL}
    logger.info('Building model, using backbone---%s' % F.backbone_name)
    net = CatchNet(F.backbone_name, config_dict, dev)
    ckpt = latest_checkpoint(F.checkpoint_path, F.backbone_name)
    if ckpt is not None:
        from rod.checkpoint import load_variables
        load_variables(net.store, ckpt, use_ema=F.use_ema)
        logger.info('Evaluating %s%s' % (ckpt, ' (averaged weights)' if F.use_ema else ''))
    elif F.synthetic:
        logger.warning('--synthetic: no checkpoint at %r, evaluating randomly initialised weights',
                       F.checkpoint_path)
    else:   # tf.train.latest_checkpoint(...) -> None makes the reference's restore fail
        raise FileNotFoundError('no checkpoint under %r (evaluate.py:221-224)' % F.checkpoint_path)
    logger.info('Building data pileline, using dataset---%s' % 'bdd100k_train')
    source = make_source(F.dataset_dir, F.batch_size, config.img_size, dev, split='train', synthetic=F.synthetic,
                         dtype=dtype, num_readers=F.num_readers, max_images=F.num_images)

    num_batches = math.ceil(F.num_images / float(F.batch_size))
    state = None
    classes = list(range(1, config.total_obj_n))
    on_device = F.match_on == 'device'
    by_area = bool(F.area_names)
    if on_device:
        from rod import ops
        # by area: slot 0 is (-inf, +inf), whose masks are rod_match_detections' own and feed today's
        # outputs; the named ranges follow
        slots = np.concatenate([np.array([[-np.inf, np.inf]], np.float32), F.area_ranges]) if by_area else None
        acc = tfe.SweepTPFP(F.match_thresholds, len(classes), num_batches * F.batch_size, F.keep_top_k, dev,
                            first_label=classes[0], area_ranges=slots)
    start = time.time()
    with torch.no_grad():
        for _ in range(num_batches):
            img, gboxes, glabels, gn = next(source)
            x = network_input(img, dtype)
            refine_out, det_out, clf_out = factory(x, F.backbone_name, False, config_dict, dtype,
                                                   net=net).get_output()
            probs = net_tools.class_probabilities(clf_out)
            boxes = net_tools.decode_all_layers(anchors_all, refine_out, det_out, to_corner=True)
            if on_device:   # nothing of the batch leaves the GPU
                pscores, pboxes = net_tools.detected_bboxes_packed(
                    probs, boxes, select_threshold=F.select_threshold, nms_threshold=F.nms_threshold,
                    top_k=F.select_top_k, keep_top_k=F.keep_top_k, nms_method=F.nms_method,
                    soft_nms_sigma=F.soft_nms_sigma, soft_nms_min_score=F.soft_nms_min_score)
                if by_area:
                    acc.update(pscores, *match_by_area(ops, pscores, pboxes, glabels, gboxes, gn, acc.thresholds_dev,
                                                       acc.area_ranges_dev, classes[0]))
                    continue
                acc.update(pscores, *ops.match_detections(pscores, pboxes, glabels, gboxes, gn, acc.thresholds_dev,
                                                          first_label=classes[0]))
                continue
            rscores, rbboxes = net_tools.detected_bboxes(probs, boxes, select_threshold=F.select_threshold,
                                                         nms_threshold=F.nms_threshold, top_k=F.select_top_k,
                                                         keep_top_k=F.keep_top_k, nms_method=F.nms_method,
                                                         soft_nms_sigma=F.soft_nms_sigma,
                                                         soft_nms_min_score=F.soft_nms_min_score)
            rs = {c: v.cpu().numpy() for c, v in rscores.items()}
            rb = {c: v.cpu().numpy() for c, v in rbboxes.items()}
            gl, gb, gcount = glabels.cpu().numpy(), gboxes.cpu().numpy(), gn.cpu().numpy()
            n_g, tp, fp, _ = tfe.bboxes_matching_batch(classes, rs, rb, gl, gb, np.zeros_like(gl),
                                                       matching_threshold=F.matching_threshold, gt_counts=gcount)
            state = tfe.streaming_tp_fp_arrays(n_g, tp, fp, rs, state=state)
    aps07, aps12 = {}, {}
    if on_device:
        per_threshold = acc.value()       # the run's one device -> host copy
        if by_area:
            per_range, per_threshold = per_threshold[1:], per_threshold[0]
        by07, by12 = tfe.sweep_average_precisions(per_threshold)   # all-range: AP 0, not None, without ground truth
    for c in classes:
        prec, rec = tfe.precision_recall(*(per_threshold[0][c] if on_device else state[c].value()))
        aps07[c] = tfe.average_precision_voc07(prec, rec)
        aps12[c] = tfe.average_precision_voc12(prec, rec)
        logger.info('AP_VOC07/%d %.6f  AP_VOC12/%d %.6f' % (c, aps07[c], c, aps12[c]))
    mAP07 = sum(aps07.values()) / len(aps07)
    mAP12 = sum(aps12.values()) / len(aps12)
    if F.synthetic:
        logger.warning('--synthetic: the AP values below are over synthetic ground truth, not a BDD100K result')
    print('AP_VOC07/mAP[%s]' % mAP07)
    print('AP_VOC12/mAP[%s]' % mAP12)
    extra = {}
    if F.sweep_thresholds.size:
        bits = [int(np.nonzero(F.match_thresholds == t)[0][0]) for t in F.sweep_thresholds]
        keys = [iou_key(t) for t in F.sweep_thresholds]
        mean = lambda d: sum(d.values()) / len(d)  # noqa: E731
        extra = {'iou_thresholds': [float(t) for t in F.sweep_thresholds],
                 'AP_VOC07_by_iou': {k: by07[b] for k, b in zip(keys, bits)},
                 'AP_VOC12_by_iou': {k: by12[b] for k, b in zip(keys, bits)},
                 'mAP_VOC07_by_iou': {k: mean(by07[b]) for k, b in zip(keys, bits)},
                 'mAP_VOC12_by_iou': {k: mean(by12[b]) for k, b in zip(keys, bits)}}
        extra['mAP_VOC07_sweep'] = mean(extra['mAP_VOC07_by_iou'])
        extra['mAP_VOC12_sweep'] = mean(extra['mAP_VOC12_by_iou'])
        for k in keys:
            print('IoU>%s  AP_VOC07/mAP[%s]  AP_VOC12/mAP[%s]' % (k, extra['mAP_VOC07_by_iou'][k],
                                                                 extra['mAP_VOC12_by_iou'][k]))
        print('IoU sweep mean (reference matching rule, VOC AP)  AP_VOC07/mAP[%s]  AP_VOC12/mAP[%s]'
              % (extra['mAP_VOC07_sweep'], extra['mAP_VOC12_sweep']))
    if by_area:
        extra.update(area_outputs(F, tfe, per_range, *acc.average_precisions(per_range)))
    elapsed = time.time() - start
    print('Time spent : %.3f seconds.' % elapsed)
    print('Time spent per BATCH: %.3f seconds.' % (elapsed / num_batches))
    os.makedirs(F.eval_dir, exist_ok=True)
    with open(os.path.join(F.eval_dir, 'eval.json'), 'w') as f:
        import json
        json.dump(dict({'AP_VOC07': aps07, 'AP_VOC12': aps12, 'mAP_VOC07': mAP07, 'mAP_VOC12': mAP12,
                        'num_batches': num_batches, 'seconds': elapsed, 'synthetic': bool(F.synthetic),
                        'checkpoint': ckpt}, **extra), f)
    return mAP07, mAP12


def match_by_area(ops, scores, boxes, glabels, gboxes, gcount, thresholds, ranges, first_label):
    """ops.match_detections_area over all rows of `ranges`: one launch for up to MAX_AREA_RANGES
    rows (the all-range slot and seven named ranges); an eighth named range takes a second."""
    outs = [ops.match_detections_area(scores, boxes, glabels, gboxes, gcount, thresholds, ranges[k:k + MAX_AREA_RANGES],
                                      first_label=first_label) for k in range(0, len(ranges), MAX_AREA_RANGES)]
    return outs[0] if len(outs) == 1 else tuple(torch.cat(o) for o in zip(*outs))


def area_outputs(F, tfe, per_range, by07, by12):
    """The *_by_area entries of eval.json from SweepTPFP's per-range tuples and APs (named ranges
    only), and one printed line per range.  Bit 0 is --matching_threshold."""
    names = F.area_names
    out = {'area_ranges': {n: [float(lo), float(hi)] for n, (lo, hi) in zip(names, F.area_ranges_px)},
           'area_image_size': list(F.area_image_size),
           'n_gt_by_area': {n: {c: v[0] for c, v in per_range[r][0].items()} for r, n in enumerate(names)},
           'AP_VOC07_by_area': {n: by07[r][0] for r, n in enumerate(names)},
           'AP_VOC12_by_area': {n: by12[r][0] for r, n in enumerate(names)},
           'recall_by_area': {n: {c: float(np.sum(v[2])) / v[0] if v[0] else None for c, v in per_range[r][0].items()}
                              for r, n in enumerate(names)}}
    out['mAP_VOC07_by_area'] = {n: tfe.mean_ap(out['AP_VOC07_by_area'][n]) for n in names}
    out['mAP_VOC12_by_area'] = {n: tfe.mean_ap(out['AP_VOC12_by_area'][n]) for n in names}
    if F.sweep_thresholds.size:
        bits = [int(np.nonzero(F.match_thresholds == t)[0][0]) for t in F.sweep_thresholds]
        for key, by in (('mAP_VOC07_sweep_by_area', by07), ('mAP_VOC12_sweep_by_area', by12)):
            out[key] = {n: tfe.mean_ap({b: tfe.mean_ap(by[r][b]) for b in bits}) for r, n in enumerate(names)}
    for r, n in enumerate(names):
        line = 'area %s [%g, %g) px^2  n_gt %d  AP_VOC07/mAP[%s]  AP_VOC12/mAP[%s]' % (
            n, F.area_ranges_px[r][0], F.area_ranges_px[r][1], sum(out['n_gt_by_area'][n].values()),
            out['mAP_VOC07_by_area'][n], out['mAP_VOC12_by_area'][n])
        if F.sweep_thresholds.size:
            line += '  sweep mean AP_VOC07/mAP[%s]  AP_VOC12/mAP[%s]' % (out['mAP_VOC07_sweep_by_area'][n],
                                                                        out['mAP_VOC12_sweep_by_area'][n])
        print(line)
    return out


if __name__ == '__main__':
    main()
