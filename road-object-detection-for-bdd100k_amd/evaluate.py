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
sweep is a mean of those, not the COCO metric.  Without the new flags the run, its printout and
eval.json are today's.
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
    ap.add_argument('--use_ema', type=str2bool, default=False,
                    help='evaluate the averaged weights the checkpoint holds (train.py --ema_decay) in place of '
                         'the variables; an error if it holds none')
    F = ap.parse_args(argv)
    try:
        F.sweep_thresholds = parse_iou_sweep(F.ap_iou_sweep)
    except ValueError as e:
        ap.error('--ap_iou_sweep: %s' % e)
    if F.sweep_thresholds.size:
        if F.match_on == 'host':
            ap.error('--ap_iou_sweep needs --match_on device (the host loop matches at one threshold)')
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
    if on_device:
        from rod import ops
        acc = tfe.SweepTPFP(F.match_thresholds, len(classes), num_batches * F.batch_size, F.keep_top_k, dev,
                            first_label=classes[0])
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
        by07, by12 = acc.average_precisions(per_threshold)
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


if __name__ == '__main__':
    main()
