"""Cost of the mosaic augmentation entries against the plain ones they stand beside:
rod_mosaic_images + rod_mosaic_boxes against rod_augment_images + rod_augment_boxes, batch 8,
720x1280 uint8 sources -> 720x1280 normalised bf16 output (the training input of the flagship).

    python tools/mosaic_bench.py [--launches 300] [--rounds 7] [--steps 30] [--out profiles/mosaic_bench.json]

The mosaic pass writes the same output bytes and reads the same four taps per pixel as the plain
pass; what it adds is the per-pixel tile select, the tile contexts in LDS and a 4x taller sum grid
whose surplus blocks exit.  Legs, alternating within each round (median round reported, with the
spread): the plain pair; the mosaic pair with centre (360, 640), with an off-grid centre
(301, 533: cx % 4 != 0, four unequal tiles) and with centre (720, 1280) (one tile per image: the
plain image through the mosaic kernels, which isolates the kernels' own overhead from the effect of
the tiling on the reads).  Each leg is also timed with the image entry alone, and the image entry's
three launches are what a slower mosaic leg is to be explained from.

Device events around `launches` back-to-back calls after a warm-up.  The parameter tables are
uploaded once (the product path uploads a few hundred bytes per step from pinned memory; that
is the same for both forms).  Bytes are the algorithmic counts of rod.roofline.

--steps > 0 also times the training loop of `train.py --synthetic --dtype bf16 --batch_size 8`
(make_source + Trainer.step_graphed, REFINE, 720x1280) with --mosaic_prob 0 and 1: host clock
around `steps` steps ending in a device synchronise, after a warm-up.
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

from rod import _abi, ops, roofline  # noqa: E402
from rod.data import synthetic_boxes  # noqa: E402
from utils.data_pileline_tools import TrainAugmenter  # noqa: E402

B, H, W = 8, 720, 1280


def timed_rounds(runs, launches, rounds):
    """{name: [us per call, one value per round]}: the legs alternate within each round."""
    for f in runs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / launches)
    return times


def legs(dev):
    """{name: (images call, boxes call)} on device-resident tables drawn by TrainAugmenter."""
    g = torch.Generator(device='cpu').manual_seed(0)
    src = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    corner, labels, n = synthetic_boxes(B, seed=0)
    hw = np.tile(np.array([H, W], np.int32), (B, 1))
    aug = TrainAugmenter((H, W), seed=0, mosaic_prob=1.0)
    tile_src, crop, ref, mode, colour, _ = aug.sample_mosaic(hw, corner, n)
    G, gout = corner.shape[1], 256
    up = lambda a, dt: ops._device_i(a, dev, dt)
    d_off, d_hw = up(np.arange(B, dtype=np.int64) * (H * W * 3), torch.int64), up(hw, torch.int32)
    d_boxes, d_labels, d_n = up(corner, torch.float32), up(labels, torch.int32), up(n, torch.int32)
    d_tsrc, d_crop, d_ref = up(tile_src, torch.int32), up(crop, torch.int32), up(ref, torch.float32)
    d_mode, d_col = up(mode, torch.int32), up(colour, torch.float32)
    # the plain pair takes tile 0's rows: image b with the same crop, flip and colour
    p_crop, p_ref = up(crop[:, 0], torch.int32), up(ref[:, 0], torch.float32)
    p_mode, p_col = up(mode[:, 0], torch.int32), up(colour[:, 0], torch.float32)
    out = torch.empty((B, H, W, 3), dtype=torch.bfloat16, device=dev)
    ws = ops.workspace(_abi.query('rod_mosaic_workspace', B, H, W), dev)
    bo, lo, no = (torch.empty((B, gout, 4), device=dev), torch.empty((B, gout), dtype=torch.int32, device=dev),
                  torch.empty(B, dtype=torch.int32, device=dev))
    st = ops.stream()

    def plain_images():
        _abi.call('rod_augment_images', src, d_off, d_hw, p_crop, p_mode, p_col, ws, out, B, H, W, 1, 1, st)

    def plain_boxes():
        _abi.call('rod_augment_boxes', d_boxes, d_labels, d_n, p_ref, p_mode, bo, lo, no, B, G, 0.3, st)

    runs = {'plain': (plain_images, plain_boxes)}
    for name, c in (('mosaic_360_640', (360, 640)), ('mosaic_301_533', (301, 533)), ('mosaic_one_tile', (H, W))):
        d_c = up(np.tile(np.array(c, np.int32), (B, 1)), torch.int32)

        def images(d_c=d_c):
            _abi.call('rod_mosaic_images', src, d_off, d_hw, d_tsrc, d_crop, d_mode, d_col, d_c, ws, out, B, B, H, W,
                      1, 1, st)

        def boxes(d_c=d_c):
            _abi.call('rod_mosaic_boxes', d_boxes, d_labels, d_n, d_tsrc, d_ref, d_mode, d_c, bo, lo, no, B, B, G,
                      gout, H, W, 0.3, 2.0, st)
        runs[name] = (images, boxes)
    # results must not change: the one-tile leg writes what the plain leg writes
    plain_images()
    want = out.clone()
    runs['mosaic_one_tile'][0]()
    assert torch.equal(out, want), 'the one-tile mosaic differs from rod_augment_images'
    return runs


def step_rate(dev, steps, mosaic_prob):
    """Steps per second of the train.py --synthetic loop at bf16 720x1280 batch 8, REFINE."""
    from rod.dataio import make_source
    from rod.trainer import Trainer
    tr = Trainer((H, W), B, dtype=torch.bfloat16, device=dev, seed=0)
    source = make_source(None, B, (H, W), dev, seed=0, augment_dtype=torch.bfloat16, synthetic=True,
                         dtype=torch.bfloat16, mosaic_prob=mosaic_prob)
    for _ in range(16):                     # eager, the captures of the box shapes that occur, replays
        tr.step_graphed(*next(source))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step_graphed(*next(source))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {'steps': steps, 'steps_per_s': round(steps / dt, 3), 'img_per_s': round(steps * B / dt, 2),
            'graphs': len(tr._graphs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--launches', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=30, help='training-loop steps per leg (0 = skip)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mosaic_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('mosaic_bench: no GPU visible (timings are taken on the device only)')
    dev = torch.device('cuda:0')
    pairs = legs(dev)
    runs = {}
    for k, (img, box) in pairs.items():
        runs[k] = lambda img=img, box=box: (img(), box())
        runs[k + ':images'] = img
    times = timed_rounds(runs, a.launches, a.rounds)
    nbytes = roofline.cost('rod_mosaic_images', (0,) * 10 + (B, B, H, W, 1, 1, 0))[0]
    assert nbytes == roofline.cost('rod_augment_images', (0,) * 8 + (B, H, W, 1, 1, 0))[0]
    rec = {'device': torch.cuda.get_device_name(0), 'shape': 'B=8, 720x1280 uint8 -> 720x1280 bf16 normalised',
           'launches': a.launches, 'rounds': a.rounds, 'image_bytes': nbytes,
           'timing': 'device events around back-to-back calls, median of rounds', 'legs': {}}
    base = statistics.median(times['plain'])
    for k, t in times.items():
        us = statistics.median(t)
        ref = statistics.median(times['plain:images']) if k.endswith(':images') else base
        rec['legs'][k] = {'us': round(us, 2), 'us_min': round(min(t), 2), 'us_max': round(max(t), 2),
                          'ratio_to_plain': round(us / ref, 3)}
        if k.endswith(':images'):
            rec['legs'][k]['GBps'] = round(nbytes / us * 1e-3, 1)
    rec['plain_spread'] = round((max(times['plain']) - min(times['plain'])) / base, 4)
    if a.steps > 0:
        del pairs, runs
        torch.cuda.empty_cache()
        off = step_rate(dev, a.steps, 0.0)
        torch.cuda.empty_cache()
        on = step_rate(dev, a.steps, 1.0)
        rec['train_loop_720p_b8_refine_bf16'] = {'mosaic_prob_0': off, 'mosaic_prob_1': on,
                                                 'ratio_on_to_off': round(on['steps_per_s'] / off['steps_per_s'], 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
