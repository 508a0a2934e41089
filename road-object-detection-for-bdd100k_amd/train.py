"""Training CLI — drop-in for the reference's train.py (flags train.py:26-77, loop 84-334).

    python train.py [--batch_size=20] [--learning_rate=1e-3] [--train_range=REFINE|ALL] ...
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py ...

Same flag names and defaults as the reference, plus: --train_range (the reference
hard-codes REFINE at train.py:130), --img_height/--img_width (config.img_size), --dtype
(fp32 like the reference's DTYPE, or bf16), --dataset_dir, --seed.  Data parallel when
launched with several ranks (RCCL all-reduce of the flat gradient, global-batch loss
normalisation; --batch_size is then per GPU).  Checkpoints are torch files holding the
slim-named variables and global_step (and, with --momentum, the momentum of every variable).

Optimiser: by default the reference's (plain SGD, clip by value +-5, constant rate).  Opt in to
--momentum / --nesterov, --weight_decay (conv / fc weights only), --clip_norm (global gradient
norm), --warmup_steps (linear) and --fix_learning_rate=False (the 0.97 staircase the reference
only logs becomes the applied rate); any of them selects the momentum-SGD kernel, under
--hip_graph too.  The summary record's `lr` is the rate the step applied.

Classifier loss (--train_range ALL): by default the reference's (hard-negative mining, IoU factor).
--clf_loss focal replaces both by focal loss (--focal_alpha 0.25, --focal_gamma 2.0).

Box regression loss of the ODM (--train_range ALL): by default the reference's (masked smooth-L1 on the
encoded offsets).  --loc_loss iou|giou|diou|ciou replaces it by that loss between the decoded box and
the matched box, times --loc_loss_weight (default 1.0).

Weight averaging: --ema_decay d (0 < d < 1; default 0 = off) keeps an exponential moving average of
the trainable variables (tf.train.ExponentialMovingAverage; --ema_warmup True applies its
num_updates rule min(d, (1 + step) / (10 + step))), updated inside the optimiser's launch, under
--hip_graph too.  It is saved with every checkpoint and restored on resume; evaluate.py and
predict.py read it with --use_ema True.

Mosaic augmentation (with --augment): --mosaic_prob p (default 0 = off) tiles, with probability p per
image, four images of the batch around a random centre (--mosaic_center lo,hi as fractions of the
image size, default 0.25,0.75) on the GPU; boxes under --mosaic_min_px tile pixels are dropped, and
--mosaic_stop_step N draws plain images again from step N on (0 = never).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import config  # noqa: E402
from utils.common_tools import logger  # noqa: E402


def str2bool(v):
    if isinstance(v, bool):
        return v
    return str(v).lower() in ('1', 'true', 't', 'yes', 'y')


def none_or_str(v):
    return None if v in (None, '', 'None', 'none') else v


def center_range(v):
    """'lo,hi' -> (lo, hi)"""
    try:
        lo, hi = (float(t) for t in str(v).split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('expected lo,hi, got %r' % (v,))
    return lo, hi


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--backbone_name', default='mobilenet_v2')
    ap.add_argument('--learning_rate', type=float, default=1e-3)
    ap.add_argument('--batch_size', type=int, default=20)
    ap.add_argument('--num_readers', type=int, default=4)
    ap.add_argument('--num_preprocessing_threads', type=int, default=4)
    ap.add_argument('--checkpoint_all', type=none_or_str, default=None)
    ap.add_argument('--checkpoint_refine', type=none_or_str, default='checkpoint/mbn_none53x35/refine/mobilenet_v2.model')
    ap.add_argument('--train_dir', default='checkpoint/')
    ap.add_argument('--summary_dir', default='summary/')
    ap.add_argument('--max_number_of_steps', type=int, default=None)
    ap.add_argument('--log_every_n_steps', type=int, default=20)
    ap.add_argument('--summary_every_n_steps', type=int, default=20)
    ap.add_argument('--save_every_n_steps', type=int, default=2000)
    ap.add_argument('--fix_refine', type=str2bool, default=True)
    # additions
    ap.add_argument('--sync_bn', type=str2bool, default=False,
                    help='data parallel: BatchNorm statistics over the global batch (default per rank; '
                         'the reference runs on one device)')
    ap.add_argument('--train_range', default='REFINE', choices=['REFINE', 'ALL'])
    ap.add_argument('--img_height', type=int, default=config.img_size[0])
    ap.add_argument('--img_width', type=int, default=config.img_size[1])
    ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--dataset_dir', default='./dataset/bdd100k_TfRecord/')
    ap.add_argument('--synthetic', type=str2bool, default=False,
                    help='run on synthetic BDD-shaped batches (no dataset needed); results are not real '
                         'metrics.  Without it a missing dataset or checkpoint is an error')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--save_format', default='torch', choices=['torch', 'tf'],
                    help='checkpoint format: torch file, or a TF-1.x tensor bundle the reference can restore')
    ap.add_argument('--augment', type=str2bool, default=True,
                    help='process_raw_data_train on the GPU (random crop / flip / colour); False = raw batches')
    ap.add_argument('--hip_graph', type=str2bool, default=True,
                    help='replay the training step as a HIP graph (Trainer.step_graphed, bit-identical to the '
                         'eager step; dropout steps run eager).  Data parallel over RCCL: the whole step, its '
                         'collectives included (the library\'s communicator; gradient buckets on a side stream)')
    # optimiser additions (all neutral by default: the reference's plain SGD step, bit for bit)
    ap.add_argument('--momentum', type=float, default=0.0, help='SGD momentum (0 = none)')
    ap.add_argument('--nesterov', type=str2bool, default=False, help='Nesterov momentum (needs --momentum > 0)')
    ap.add_argument('--weight_decay', type=float, default=0.0,
                    help='L2 weight decay on conv / fc weights (not depthwise filters, BatchNorm or biases), '
                         'added to the clipped gradient')
    ap.add_argument('--clip_norm', type=float, default=None,
                    help='clip the gradient to this global L2 norm (before the clip by value)')
    ap.add_argument('--warmup_steps', type=int, default=0, help='linear learning-rate warm-up over this many steps')
    ap.add_argument('--fix_learning_rate', type=str2bool, default=True,
                    help='False: apply the exponential staircase decay (0.97 every 20000 / batch_size steps) '
                         'that the reference only logs')
    # classifier-loss addition (neutral by default: the reference's hard-negative mining + IoU factor)
    ap.add_argument('--clf_loss', default='hnm', choices=['hnm', 'focal'],
                    help="ODM classifier loss (--train_range ALL): 'hnm' = softmax cross-entropy with 3:1 hard-negative "
                         "mining and the IoU factor (the reference); 'focal' = focal loss over every anchor, "
                         'normalised by the positives, in place of both')
    ap.add_argument('--focal_alpha', type=float, default=None,
                    help='focal loss: weight of the positives, 1 - alpha on the negatives; in [0, 1] (default 0.25)')
    ap.add_argument('--focal_gamma', type=float, default=None,
                    help='focal loss: focusing exponent, finite and >= 0 (default 2.0)')
    # box-regression addition (neutral by default: the reference's masked smooth-L1 on the offsets)
    ap.add_argument('--loc_loss', default='smooth_l1', choices=['smooth_l1', 'iou', 'giou', 'diou', 'ciou'],
                    help="ODM box regression loss (--train_range ALL): 'smooth_l1' = masked smooth-L1 on the encoded "
                         "offsets (the reference); 'iou' / 'giou' / 'diou' / 'ciou' = that loss between the decoded "
                         'box and the matched box, in its place')
    ap.add_argument('--loc_loss_weight', type=float, default=None,
                    help='weight of the IoU-family box loss in the training loss, finite and >= 0 (default 1.0)')
    # weight-averaging addition (neutral by default: no average is kept)
    ap.add_argument('--ema_decay', type=float, default=0.0,
                    help='keep an exponential moving average of the trainable variables with this decay, in '
                         '[0, 1) (0 = off); saved with the checkpoints, read by evaluate.py / predict.py --use_ema')
    ap.add_argument('--ema_warmup', type=str2bool, default=True,
                    help="the average's decay is min(ema_decay, (1 + step) / (10 + step)) "
                         '(tf.train.ExponentialMovingAverage with num_updates); False: ema_decay from the first step')
    # input-side addition (neutral by default: one crop per image, every draw as before)
    ap.add_argument('--mosaic_prob', type=float, default=0.0,
                    help='probability, in [0, 1], that a training image is a mosaic of four images of its batch '
                         '(0 = off); needs --augment')
    ap.add_argument('--mosaic_center', type=center_range, default=(0.25, 0.75),
                    help='lo,hi: the mosaic centre is drawn uniformly in [lo, hi] of the image height and width')
    ap.add_argument('--mosaic_min_px', type=float, default=2.0,
                    help='mosaic: drop boxes whose clipped height or width is under this many tile pixels')
    ap.add_argument('--mosaic_stop_step', type=int, default=0,
                    help='mosaic: off from this step on, for a clean final phase (0 = never)')
    F = ap.parse_args(argv)
    if not 0.0 <= F.mosaic_prob <= 1.0:       # (a NaN fails both comparisons)
        ap.error('--mosaic_prob must be in [0, 1], got %r' % F.mosaic_prob)
    if not 0.0 <= F.mosaic_center[0] <= F.mosaic_center[1] <= 1.0:
        ap.error('--mosaic_center needs 0 <= lo <= hi <= 1, got %r' % (F.mosaic_center,))
    if not (0.0 <= F.mosaic_min_px < float('inf')):
        ap.error('--mosaic_min_px must be finite and >= 0, got %r' % F.mosaic_min_px)
    if F.mosaic_stop_step < 0:
        ap.error('--mosaic_stop_step must be >= 0, got %r' % F.mosaic_stop_step)
    if F.mosaic_prob > 0 and not F.augment:
        ap.error('--mosaic_prob needs --augment True: mosaic is part of the GPU augmentation')
    if not 0.0 <= F.ema_decay < 1.0:       # (a NaN fails both comparisons)
        ap.error('--ema_decay must be in [0, 1), got %r' % F.ema_decay)
    loc_given = F.loc_loss_weight is not None
    if F.loc_loss_weight is None:
        F.loc_loss_weight = 1.0
    if not (0.0 <= F.loc_loss_weight < float('inf')):      # (a NaN fails both comparisons)
        ap.error('--loc_loss_weight must be finite and >= 0, got %r' % F.loc_loss_weight)
    if F.train_range == 'REFINE' and (F.loc_loss != 'smooth_l1' or loc_given):
        ap.error('--loc_loss / --loc_loss_weight need --train_range ALL: REFINE training has no ODM box loss to '
                 'apply them to')
    if F.loc_loss == 'smooth_l1' and loc_given:
        ap.error('--loc_loss_weight needs --loc_loss iou, giou, diou or ciou')
    given = [n for n in ('focal_alpha', 'focal_gamma') if getattr(F, n) is not None]
    if F.focal_alpha is None:
        F.focal_alpha = 0.25
    if F.focal_gamma is None:
        F.focal_gamma = 2.0
    if not 0.0 <= F.focal_alpha <= 1.0:       # (a NaN fails both comparisons)
        ap.error('--focal_alpha must be in [0, 1], got %r' % F.focal_alpha)
    if not (0.0 <= F.focal_gamma < float('inf')):
        ap.error('--focal_gamma must be finite and >= 0, got %r' % F.focal_gamma)
    if F.train_range == 'REFINE' and (F.clf_loss != 'hnm' or given):
        ap.error('--clf_loss focal / --focal_alpha / --focal_gamma need --train_range ALL: REFINE training has no '
                 'classifier loss to apply them to')
    if F.clf_loss == 'hnm' and given:
        ap.error('--%s needs --clf_loss focal' % given[0])
    return F


def load_ckpt(store, path, names_regex=None, optimizer=None):
    """saver.restore (train.py:188, 282) / restore_saver of backbone.+|refine.+ (155-158, 191-193):
    a torch checkpoint written by this CLI or a TF-1.x tensor bundle of the reference."""
    from rod.checkpoint import load_variables
    return load_variables(store, path, names_regex=names_regex, optimizer=optimizer)


def save_ckpt(store, path, step, fmt='torch', optimizer=None):
    from rod.checkpoint import save_variables
    save_variables(store, path, step, fmt, optimizer=optimizer)


def _loss_copy(losses, world):
    """The step's loss values as one small device tensor (a copy: a replayed graph overwrites
    its outputs on the next replay).  Data parallel: each rank holds its shard's sum / global
    batch, so the global loss is the all-reduced sum."""
    lv = torch.stack([l.detach().float().reshape(()) for l in losses])
    if world > 1:
        torch.distributed.all_reduce(lv)
    if lv.device.type != 'cuda':
        return lv, None
    host = torch.empty(lv.shape, dtype=lv.dtype, pin_memory=True)
    host.copy_(lv, non_blocking=True)   # queued before the next step: reading it waits for this step only
    ev = torch.cuda.Event()
    ev.record()
    return host, ev


def _loss_values(entry):
    host, ev = entry
    if ev is not None:
        ev.synchronize()
    return host.tolist()


class StepLog(object):
    """Running averages and the log / summary lines of train.py:292-320 (formats kept)."""

    def __init__(self, F, trainer, tr_range, rank, summ):
        self.F, self.trainer, self.tr_range, self.rank, self.summ = F, trainer, tr_range, rank, summ
        self.avg = [0., 0., 0.]
        self.avg_t = 0.

    def __call__(self, current_step, vals, t):
        F, avg = self.F, self.avg
        if F.log_every_n_steps is not None:
            s = current_step % F.log_every_n_steps
            if self.tr_range is config.train_range.ALL:
                tot, _, dl, cl = vals
                avg[:] = [(avg[0] * s + tot) / (s + 1.), (avg[1] * s + dl) / (s + 1.), (avg[2] * s + cl) / (s + 1.)]
            else:
                avg[0] = (avg[0] * s + vals[0]) / (s + 1.)
            self.avg_t = (self.avg_t * s + t) / (s + 1.)
            if current_step % F.log_every_n_steps == F.log_every_n_steps - 1 and self.rank == 0:
                if self.tr_range is config.train_range.ALL:
                    logger.info('Step%s total_loss:%s det_loss:%s clf_loss:%s time_each_step:%s' %
                                (str(current_step + 1), str(avg[0]), str(avg[1]), str(avg[2]), str(self.avg_t)))
                else:
                    logger.info('Step_%s refine_loss:%s time:%s' % (str(current_step + 1), str(avg[0]),
                                                                    str(self.avg_t)))
                avg[:] = [0., 0., 0.]
                self.avg_t = 0.
        if self.summ is not None and F.summary_every_n_steps is not None and \
                current_step % F.summary_every_n_steps == F.summary_every_n_steps - 1:
            rec = {'step': current_step, 'loss': vals, 'lr': self.trainer.opt.summary_lr(current_step)}
            self.summ.write(json.dumps(rec) + '\n')
            self.summ.flush()


def main(argv=None):
    F = parse(argv)
    logger.info('Asserting parameters')
    assert F.batch_size > 0
    assert F.learning_rate >= 0.
    assert F.log_every_n_steps is None or F.log_every_n_steps > 0
    assert F.summary_every_n_steps is None or F.summary_every_n_steps > 0
    assert F.save_every_n_steps is None or F.save_every_n_steps > 0
    assert F.backbone_name in config.supported_backbone_name

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:
        torch.cuda.set_device(local)
        torch.distributed.init_process_group('nccl', device_id=torch.device('cuda', local))
    dev = torch.device('cuda', local)
    from rod.dataio import make_source
    from rod.ddp import make_reducer
    from rod.trainer import Trainer

    config.img_size = (F.img_height, F.img_width)
    tr_range = getattr(config.train_range, F.train_range)
    dtype = torch.bfloat16 if F.dtype == 'bf16' else torch.float32
    logger.info('Building model, using backbone---%s' % F.backbone_name)
    trainer = Trainer(config.img_size, F.batch_size, dtype=dtype, train_range=tr_range, learning_rate=F.learning_rate,
                      device=dev, fix_refine=F.fix_refine, seed=F.seed, world_size=world,
                      reducer=make_reducer(world, rank) if world > 1 else None, backbone_name=F.backbone_name,
                      sync_bn=F.sync_bn, momentum=F.momentum, nesterov=F.nesterov, weight_decay=F.weight_decay,
                      clip_norm=F.clip_norm, warmup_steps=F.warmup_steps, fix_learning_rate=F.fix_learning_rate,
                      clf_loss=F.clf_loss, focal_alpha=F.focal_alpha, focal_gamma=F.focal_gamma,
                      loc_loss=F.loc_loss, loc_loss_weight=F.loc_loss_weight, ema_decay=F.ema_decay,
                      ema_warmup=F.ema_warmup)
    if F.ema_decay > 0:
        logger.info('Weight EMA: decay %g%s' % (F.ema_decay, ', num_updates warm-up' if F.ema_warmup else ''))
    if tr_range is config.train_range.ALL:
        logger.info('Classifier loss: %s' % ('focal loss, alpha=%g gamma=%g (no hard-negative mining, no IoU factor)'
                                              % (F.focal_alpha, F.focal_gamma) if F.clf_loss == 'focal'
                                              else 'softmax cross-entropy with 3:1 hard-negative mining'))
    if tr_range is config.train_range.ALL:
        logger.info('Box regression loss: %s' % ('%s loss on the decoded boxes, weight %g (no smooth-L1)'
                                                 % ({'iou': 'IoU', 'giou': 'GIoU', 'diou': 'DIoU', 'ciou': 'CIoU'}
                                                    [F.loc_loss], F.loc_loss_weight) if F.loc_loss != 'smooth_l1'
                                                 else 'masked smooth-L1 on the encoded offsets'))
    store = trainer.net.store
    logger.info('Total trainable parameters:%s' % str(store.trainable_count()))
    step0 = 0
    if tr_range is config.train_range.ALL:
        if F.checkpoint_all is not None:
            step0 = load_ckpt(store, F.checkpoint_all, optimizer=trainer.opt)
            logger.info('Load checkpoint for all net success...')
        if F.checkpoint_refine is not None:
            load_ckpt(store, F.checkpoint_refine, names_regex=r'backbone.+|refine.+', optimizer=trainer.opt)
            logger.info('Load checkpoint for refine net success...')
    else:
        if F.checkpoint_refine is not None:
            step0 = load_ckpt(store, F.checkpoint_refine, optimizer=trainer.opt)
            logger.info('Load checkpoint success...')
        else:
            logger.info('TF variables init success...')
    trainer.opt.global_step = step0
    logger.info('Building data pileline, using dataset---%s' % 'bdd100k_train')
    source = make_source(F.dataset_dir, F.batch_size, config.img_size, dev, seed=F.seed,
                         augment_dtype=dtype if F.augment else None, synthetic=F.synthetic, dtype=dtype,
                         num_readers=F.num_readers, rank=rank, world=world, mosaic_prob=F.mosaic_prob,
                         mosaic_center=F.mosaic_center, mosaic_min_px=F.mosaic_min_px,
                         mosaic_stop_step=F.mosaic_stop_step, start_step=step0)
    if F.mosaic_prob > 0:
        logger.info('Mosaic augmentation: probability %g, centre in [%g, %g]%s' % (
            (F.mosaic_prob,) + F.mosaic_center +
            (', off from step %d' % F.mosaic_stop_step if F.mosaic_stop_step else '',)))

    os.makedirs(F.summary_dir, exist_ok=True)
    summ = open(os.path.join(F.summary_dir, 'train_rank%d.jsonl' % rank), 'a') if rank == 0 else None
    log = StepLog(F, trainer, tr_range, rank, summ)
    # Trainer.graph_mode: the whole step as one graph (one process, or data parallel through the
    # library's RCCL communicator), forward + backward only (gloo), or eager (dropout)
    step = trainer.step_graphed if F.hip_graph else trainer.step
    # the host reads each step's losses (the reference's sess.run returns them) one step late:
    # step k+1 is queued on the GPU before step k's values are read, so the GPU does not wait
    # for the host's logging and next-batch work.  Checkpoints are written right after their
    # step (before the next is queued), so they hold exactly that step's parameters.
    pending = None
    last = time.time()
    while True:
        losses = step(*next(source))
        current_step = trainer.opt.global_step - 1
        entry = (current_step, _loss_copy(losses, world))
        if F.save_every_n_steps is not None and current_step % F.save_every_n_steps == F.save_every_n_steps - 1 \
                and rank == 0:
            logger.info('Saving model...')
            save_ckpt(store, os.path.join(F.train_dir, F.backbone_name + '.model'), current_step + 1, F.save_format,
                      optimizer=trainer.opt)
            logger.info('Save model sucess...')
        if pending is not None:
            vals = _loss_values(pending[1])   # waits for the previous step only
            now = time.time()
            log(pending[0], vals, round(now - last, 3))
            last = now
        pending = entry
        if F.max_number_of_steps is not None and current_step >= F.max_number_of_steps:
            break
    vals = _loss_values(pending[1])
    log(pending[0], vals, round(time.time() - last, 3))
    logger.info('Exit training...')
    close = getattr(source, 'close', None)
    if close is not None:
        close()
    if world > 1:
        if getattr(trainer.reducer, 'native', False):
            from rod import _abi
            _abi.call('rod_rccl_destroy')
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
