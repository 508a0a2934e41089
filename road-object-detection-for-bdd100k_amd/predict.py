"""Inference CLI — drop-in for the reference's predict.py (flags 27-53, flow 61-200).

ALL-mode network in inference mode -> softmax(clf_out) -> decode(refine_out + det_out)
-> corner boxes -> detected_bboxes(select 0.1, nms 0.4, top_k 400, keep 200)
(predict.py:127-137).  The reference shows each image in cv2 windows; visualisation is
out of scope here, so detections are printed / written as JSON.
--batch_size > 1 reports throughput (BASELINE config: predict b=32 at 1280x720).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import config  # noqa: E402
from utils.common_tools import logger  # noqa: E402


def str2bool(v):
    return str(v).lower() in ('1', 'true', 't', 'yes', 'y')


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--backbone_name', default='mobilenet_v2')
    ap.add_argument('--num_readers', type=int, default=4)
    ap.add_argument('--num_preprocessing_threads', type=int, default=4)
    ap.add_argument('--checkpoint_all', default='checkpoint/mobilenet_v2.model')
    ap.add_argument('--vis_height', type=int, default=720)
    ap.add_argument('--vis_width', type=int, default=1080)
    ap.add_argument('--vis_groundtruth', type=str2bool, default=True)
    # additions
    ap.add_argument('--batch_size', type=int, default=1)
    ap.add_argument('--num_batches', type=int, default=1)
    ap.add_argument('--select_threshold', type=float, default=0.1)
    ap.add_argument('--nms_threshold', type=float, default=0.4)
    ap.add_argument('--top_k', type=int, default=400)
    ap.add_argument('--keep_top_k', type=int, default=200)
    ap.add_argument('--nms_method', default='hard', choices=['hard', 'linear', 'gaussian'],
                    help="'hard': the reference's greedy NMS; 'linear' / 'gaussian': Soft-NMS (overlapped "
                         'detections are rescored, not dropped; the scores reported are the rescored ones)')
    ap.add_argument('--soft_nms_sigma', type=float, default=0.5, help='gaussian Soft-NMS: exp(-iou^2 / sigma)')
    ap.add_argument('--soft_nms_min_score', type=float, default=0.001,
                    help='Soft-NMS stops emitting below this rescored score')
    ap.add_argument('--img_height', type=int, default=config.img_size[0])
    ap.add_argument('--img_width', type=int, default=config.img_size[1])
    ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--dataset_dir', default='./dataset/bdd100k_TfRecord/')
    ap.add_argument('--synthetic', type=str2bool, default=False,
                    help='run on synthetic BDD-shaped batches (no dataset needed); results are not real '
                         'metrics.  Without it a missing dataset or checkpoint is an error')
    ap.add_argument('--vis_dir', default=None,
                    help='write the first image of every batch with its detections (and ground truth) as PNG '
                         '(the reference shows them with cv2.imshow)')
    ap.add_argument('--output', default=None, help='write detections of the last batch as JSON')
    ap.add_argument('--use_ema', type=str2bool, default=False,
                    help='predict with the averaged weights the checkpoint holds (train.py --ema_decay) in place '
                         'of the variables; an error if it holds none')
    return ap.parse_args(argv)


class Predictor(object):
    """Forward + decode + per-class NMS; reused by bench (inference FPS)."""

    def __init__(self, img_size, device, dtype=torch.float32, checkpoint=None, select_threshold=0.1,
                 nms_threshold=0.4, top_k=400, keep_top_k=200, seed=0, backbone_name='mobilenet_v2',
                 nms_method='hard', soft_nms_sigma=0.5, soft_nms_min_score=0.001, use_ema=False):
        from nets.catch_net import CatchNet
        from utils import net_tools
        if nms_method not in ('hard', 'linear', 'gaussian'):
            raise ValueError("nms_method must be 'hard', 'linear' or 'gaussian', got %r" % (nms_method,))
        config.img_size = tuple(img_size)
        self.config_dict = {'process_backbone_method': config.process_backbone_method.NONE,
                            'deconv_method': config.deconv_method.LEARN_HALF,
                            'merge_method': config.merge_method.ADD, 'train_range': config.train_range.ALL}
        self.backbone_name = backbone_name
        self.net = CatchNet(backbone_name, self.config_dict, device, seed)
        if checkpoint is not None:
            from rod.checkpoint import load_variables
            load_variables(self.net.store, checkpoint, use_ema=use_ema)
        self.anchors = net_tools.anchors_all_layer(config.img_size, config.feat_sizes(config.img_size, backbone_name),
                                                   net_tools.init_anchor(6))
        self.dtype = dtype
        self.keep_intermediates = False   # tests: keep (logits, probs, boxes) of the last call
        self.last = None
        self.kw = dict(select_threshold=select_threshold, nms_threshold=nms_threshold, top_k=top_k,
                       keep_top_k=keep_top_k, nms_method=nms_method, soft_nms_sigma=soft_nms_sigma,
                       soft_nms_min_score=soft_nms_min_score)
        # the whole forward + decode + NMS is captured once per input shape as a HIP graph and
        # replayed (no per-kernel host dispatch); re-captured when the parameters change
        self.use_graph = device.type == 'cuda' and os.environ.get('ROD_PREDICT_GRAPH', '1') != '0'
        self._graph = None

    def _forward(self, img_u8):
        from nets.catch_net import factory
        from utils import net_tools
        from rod import ops
        from rod.dataio import network_input
        x = network_input(img_u8, self.dtype)
        refine_out, det_out, clf_out = factory(x, self.backbone_name, False, self.config_dict, self.dtype,
                                               net=self.net).get_output()
        probs = net_tools.class_probabilities(clf_out)                                     # predict.py:127-128
        boxes = net_tools.decode_all_layers(self.anchors, refine_out, det_out, to_corner=True)  # 130-134
        if self.keep_intermediates:
            self.last = (ops.levels_concat(clf_out, config.total_obj_n), probs, boxes,
                         ops.levels_concat(refine_out, 4), ops.levels_concat(det_out, 4))
        kw = self.kw                                                                        # 136-137
        thr = 0.0 if kw['select_threshold'] is None else kw['select_threshold']
        if kw['nms_method'] == 'hard':
            return ops.select_topk_nms(probs, boxes, thr, kw['top_k'], kw['keep_top_k'], kw['nms_threshold'])
        return ops.select_topk_soft_nms(probs, boxes, thr, kw['top_k'], kw['keep_top_k'], kw['nms_threshold'],
                                        kw['nms_method'], kw['soft_nms_sigma'], kw['soft_nms_min_score'])

    @torch.no_grad()
    def __call__(self, img_u8):
        """detected_bboxes of the batch: ({c: scores [B, keep_top_k]}, {c: boxes [B, keep_top_k, 4]})."""
        if not self.use_graph or self.keep_intermediates:
            scores, boxes = self._forward(img_u8)
        else:
            key = (tuple(img_u8.shape), img_u8.dtype, self.net.store.version, self.kw['nms_method'],
                   self.kw['soft_nms_sigma'], self.kw['soft_nms_min_score'])
            if self._graph is None or self._graph[0] != key:
                self._graph = None
                static_in = img_u8.clone()
                self._forward(static_in)          # first run: weight layouts, anchor table, workspaces
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = self._forward(static_in)
                self._graph = (key, g, static_in, out)
            _, g, static_in, out = self._graph
            static_in.copy_(img_u8)
            g.replay()
            scores, boxes = out[0].clone(), out[1].clone()
        K = scores.shape[1] + 1
        return ({c: scores[:, c - 1] for c in range(1, K)}, {c: boxes[:, c - 1] for c in range(1, K)})


def write_vis(F, bi, img, scores, bboxes, gt_corner, gt_labels, gt_n):
    """predict.py:151-196 without a display: the first image of the batch resized to
    vis_height x vis_width with its detections (and ground truth) drawn, written as PNG."""
    from PIL import Image
    from utils import net_tools
    os.makedirs(F.vis_dir, exist_ok=True)
    a = img[0].float().cpu().numpy() if img.is_floating_point() else img[0].cpu().numpy()
    if a.dtype != np.uint8:   # the TFRecord pipeline hands over [-1, 1] images (2/255 x - 1)
        a = np.uint8(np.clip(np.rint((a + 1.0) * 127.5), 0, 255))
    im = Image.fromarray(a).resize((F.vis_width, F.vis_height), Image.BILINEAR)
    img_gt = np.asarray(im, np.uint8).copy()
    img_pred = img_gt.copy()
    for c in scores:
        s = scores[c][0].cpu().numpy()
        if s.any():
            net_tools.visualize_boxes_and_labels_on_image_array(img_pred, bboxes[c][0].cpu().numpy(),
                                                                np.full(s.shape, c, np.int32), s,
                                                                config.category_index)
    Image.fromarray(img_pred).save(os.path.join(F.vis_dir, 'pred_%04d.png' % bi))
    if F.vis_groundtruth:
        n = int(gt_n[0])
        for box, lab in zip(gt_corner[0, :n].cpu().numpy(), gt_labels[0, :n].cpu().numpy()):
            if lab > 0:
                net_tools.visualize_boxes_and_labels_on_image_array(img_gt, box[None], np.array([lab]),
                                                                    np.array([1.]), config.category_index,
                                                                    skip_scores=True, skip_labels=True)
        Image.fromarray(img_gt).save(os.path.join(F.vis_dir, 'gt_%04d.png' % bi))


def main(argv=None):
    F = parse(argv)
    logger.info('Asserting parameters')
    assert F.backbone_name in config.supported_backbone_name
    from rod.dataio import make_source
    dev = torch.device('cuda', 0)
    dtype = torch.bfloat16 if F.dtype == 'bf16' else torch.float32
    from rod.checkpoint import exists
    ckpt = F.checkpoint_all if F.checkpoint_all and exists(F.checkpoint_all) else None
    if ckpt is None:
        if not F.synthetic:   # the reference's saver.restore fails (predict.py:143-146)
            raise FileNotFoundError('checkpoint %r not found (pass --synthetic to predict with random weights)'
                                    % F.checkpoint_all)
        logger.warning('--synthetic: checkpoint %r not found, predicting with random weights', F.checkpoint_all)
    pred = Predictor((F.img_height, F.img_width), dev, dtype, ckpt, F.select_threshold, F.nms_threshold, F.top_k,
                     F.keep_top_k, backbone_name=F.backbone_name, nms_method=F.nms_method,
                     soft_nms_sigma=F.soft_nms_sigma, soft_nms_min_score=F.soft_nms_min_score, use_ema=F.use_ema)
    logger.info('Building data pileline, using dataset---%s' % 'bdd100k_train')
    source = make_source(F.dataset_dir, F.batch_size, config.img_size, dev, synthetic=F.synthetic, dtype=dtype,
                         num_readers=F.num_readers)
    t0 = time.time()
    for bi in range(F.num_batches):
        img, gt_corner, gt_labels, gt_n = next(source)
        scores, bboxes = pred(img)
        if F.vis_dir:
            write_vis(F, bi, img, scores, bboxes, gt_corner, gt_labels, gt_n)
    torch.cuda.synchronize()
    dt = time.time() - t0
    n_det = {c: int((s > 0).sum().item()) for c, s in scores.items()}
    logger.info('detections per class (batch of %d): %s' % (F.batch_size, n_det))
    logger.info('%.2f images/s' % (F.batch_size * F.num_batches / dt))
    if F.output:
        out = {str(c): {'scores': scores[c].cpu().tolist(), 'bboxes': bboxes[c].cpu().tolist()} for c in scores}
        with open(F.output, 'w') as f:
            json.dump(out, f)
    return scores, bboxes


if __name__ == '__main__':
    main()
