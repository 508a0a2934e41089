"""Cost of the two ODM classifier losses at the training shape (B=8 images of 720x1280: 129,915
anchors each, K=11 classes, about 1 % positives), bf16 and fp32, forward with gradient:

  hnm    ops.softmax_ce_hnm   the default: softmax cross-entropy, global hard-negative mining and
                              the IoU factor (13 kernels: rows, count, 4 x (radix histogram +
                              scan), IoU groups, loss, finalize)
  focal  ops.softmax_focal    opt-in focal loss (3 kernels: count, loss, finalize, behind one
                              8-byte memset node)

    python tools/loss_bench.py [--replays 300] [--rounds 7] [--out profiles/loss_bench.json]

Each path is captured once as a HIP graph (so the host's launch cost is not in the figure, as in
the training step) and timed with device events around `replays` back-to-back replays, after a
warm-up; the paths alternate within each round and the median round is reported with the spread.
`focal_loss_entry` is rod_focal_loss alone (the loss and finalize kernels, counts precomputed).
The tensors are 23 MB (bf16) / 46 MB (fp32) each, so back-to-back replays find part of them in
the last-level cache: the same holds for both paths, and for the step, where the logits were
just written.  Bytes are the algorithmic counts of rod.roofline; the launch counts are read off
csrc/loss.hip, not measured.  Pass condition (exit status): focal is not slower than hnm in the
same run, for both dtypes.

The box-regression leg (--leg box, written to profiles/boxloss_bench.json) times the ODM box losses
the same way, in the same process: ops.smooth_l1_masked (the default, the yardstick) against
ops.box_iou_loss for iou / giou / diou / ciou, forward with gradient, bf16 and fp32, the same
B=8 x 129,915 rows with about 1 % positives; it reports the times, the ratio to smooth-L1 and
the fraction of 8 TB/s on the algorithmic bytes (rod.roofline.box_iou_loss_bytes with the actual
positive count).  It sets no pass condition: nothing had been measured when it was written.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'road-object-detection-for-bdd100k_amd'), ROOT]

import torch  # noqa: E402

import config  # noqa: E402
from rod import _abi, ops, roofline  # noqa: E402
from utils import net_tools  # noqa: E402

KERNELS = {'hnm': 13, 'focal': 3, 'focal_loss_entry': 2}


def level_offsets(hw, dev):
    config.img_size = hw
    name = 'mobilenet_v2'
    anchors = net_tools.anchors_all_layer(hw, config.feat_sizes(hw, name),
                                          net_tools.init_anchor(len(config.extract_feat_name[name])))
    return tuple(int(v) for v in net_tools.anchor_table(anchors, dev).lvl_off)


def time_graphs(paths, replays, rounds):
    """{name: [us per replay, one per round]} and {name: kept output}: every path captured once as a graph,
    the paths alternating within each round."""
    graphs = {}
    for k, f in paths.items():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = f()
        graphs[k] = (g, keep)
        for _ in range(20):
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, (g, _) in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                g.replay()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / replays)
    return times, {k: keep for k, (_, keep) in graphs.items()}


def box_leg(a, dev):
    """smooth-L1 against the four IoU-family losses at the training shape -> the record written to --out_box."""
    B = 8
    config.img_size = (720, 1280)
    name = 'mobilenet_v2'
    anchors = net_tools.anchors_all_layer((720, 1280), config.feat_sizes((720, 1280), name),
                                          net_tools.init_anchor(len(config.extract_feat_name[name])))
    tab = net_tools.anchor_table(anchors, dev)
    lvl_off = tuple(int(v) for v in tab.lvl_off)
    A = lvl_off[-1]
    assert A == 129915, A
    gen = torch.Generator(device=dev).manual_seed(1)
    pos = (torch.rand((B, A), device=dev, generator=gen) < 0.01).int()
    n_pos = int(pos.sum())
    t = torch.randn((B, A, 4), device=dev, generator=gen) * 0.3          # the targets' encodings
    cbox = ops.decode(tab.center, t) * pos[..., None]
    det_gt = t * pos[..., None]
    ro32 = torch.randn((B, A, 4), device=dev, generator=gen) * 0.2
    do32 = torch.randn((B, A, 4), device=dev, generator=gen) * 0.3
    rec = {'device': torch.cuda.get_device_name(0), 'shape': {'B': B, 'A': A, 'positives': n_pos},
           'replays': a.replays, 'rounds': a.rounds, 'kernels_per_call': 2,
           'kernels_per_call_source': 'csrc/targets.hip (not measured)',
           'timing': 'device events around back-to-back graph replays, median of rounds; forward with gradient',
           'dtypes': {}}
    for dname, dt in (('bf16', torch.bfloat16), ('fp32', torch.float32)):
        ro = ro32.to(dt)
        do = do32.to(dt).requires_grad_(True)
        es = do.element_size()

        def smooth_l1():
            _, tot = ops.smooth_l1_masked(do, det_gt, pos, lvl_off, float(B))
            return torch.autograd.grad(tot, do)[0]

        def box(kind):
            def f():
                _, tot = ops.box_iou_loss(tab.center, ro, do, cbox, pos, lvl_off, kind, 1.0, float(B))
                return torch.autograd.grad(tot, do)[0]
            return f
        paths = {'smooth_l1': smooth_l1}
        paths.update({k: box(k) for k in ('iou', 'giou', 'diou', 'ciou')})
        times, kept = time_graphs(paths, a.replays, a.rounds)
        assert all(torch.isfinite(k.float()).all() for k in kept.values())
        nbytes = {k: roofline.box_iou_loss_bytes(B, A, es, n_pos) for k in paths}
        nbytes['smooth_l1'] = roofline.cost('rod_smoothl1_masked', (0,) * 7 + (1, None, 0, B, A, ops.dtcode(do), 0))[0]
        r = {}
        for k, tm in times.items():
            us = statistics.median(tm)
            r[k] = {'us': round(us, 2), 'us_min': round(min(tm), 2), 'us_max': round(max(tm), 2), 'bytes': nbytes[k],
                    'GBps': round(nbytes[k] / us * 1e-3, 1),
                    'fraction_of_8TBps': round(nbytes[k] / us * 1e-3 / roofline.MI355X_HBM_PEAK_GBS, 4)}
        for k in paths:
            r[k]['over_smooth_l1'] = round(r[k]['us'] / r['smooth_l1']['us'], 4)
        rec['dtypes'][dname] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out_box)), exist_ok=True)
    with open(a.out_box, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--replays', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loss_bench.json'))
    ap.add_argument('--leg', default='all', choices=['clf', 'box', 'all'],
                    help='clf: the classifier losses (--out); box: the box-regression losses (--out_box)')
    ap.add_argument('--out_box', default=os.path.join(ROOT, 'profiles', 'boxloss_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('loss_bench: no GPU visible (timings are taken on the device only)')
    dev = torch.device('cuda:0')
    if a.leg in ('box', 'all'):
        box_leg(a, dev)
    if a.leg == 'box':
        return
    B, K = 8, config.total_obj_n
    lvl_off = level_offsets((720, 1280), dev)
    A = lvl_off[-1]
    assert (A, K) == (129915, 11), (A, K)
    gen = torch.Generator(device=dev).manual_seed(0)
    pos = (torch.rand((B, A), device=dev, generator=gen) < 0.01).int()
    lbl = torch.randint(1, K, (B, A), device=dev, generator=gen, dtype=torch.int32) * pos
    iou = torch.rand((B, A), device=dev, generator=gen) * 0.5 + 0.5
    base = torch.randn((B, A, K), device=dev, generator=gen) * 2.0
    rec = {'device': torch.cuda.get_device_name(0), 'shape': {'B': B, 'A': A, 'K': K, 'positives': int(pos.sum())},
           'replays': a.replays, 'rounds': a.rounds, 'kernels_per_call': dict(KERNELS, focal_memset_nodes=1),
           'kernels_per_call_source': 'csrc/loss.hip (not measured)',
           'timing': 'device events around back-to-back graph replays, median of rounds', 'dtypes': {}}
    ok = True
    for dname, dt in (('bf16', torch.bfloat16), ('fp32', torch.float32)):
        lg = base.to(dt).requires_grad_(True)
        counts = torch.tensor([int(pos.sum()), int(B * A - pos.sum())], dtype=torch.int32, device=dev)
        ws = ops.workspace(_abi.query('rod_softmax_focal_workspace', B, A), dev)
        out8, gbuf = torch.empty(8, device=dev), torch.empty_like(lg)

        def hnm():
            _, clf = ops.softmax_ce_hnm(lg, lbl, pos, iou, lvl_off, float(B))
            return torch.autograd.grad(clf, lg)[0]

        def focal():
            _, clf = ops.softmax_focal(lg, lbl, pos, 0.25, 2.0)
            return torch.autograd.grad(clf, lg)[0]

        def focal_loss_entry():
            _abi.call('rod_focal_loss', lg.detach(), lbl, pos, counts, 0.25, 2.0, out8, gbuf, ws, B, A, K,
                      ops.dtcode(lg), ops.stream())
            return gbuf
        paths = {'hnm': hnm, 'focal': focal, 'focal_loss_entry': focal_loss_entry}
        graphs = {}
        for k, f in paths.items():
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep = f()
            graphs[k] = (g, keep)
            for _ in range(20):
                g.replay()
        torch.cuda.synchronize()
        assert all(torch.isfinite(keep.float()).all() for _, keep in graphs.values())
        assert torch.equal(graphs['focal'][1], graphs['focal_loss_entry'][1])
        times = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k, (g, _) in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.replays):
                    g.replay()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.replays)
        es = lg.element_size()
        code = ops.dtcode(lg)
        nbytes = {'hnm': None,
                  'focal': roofline.cost('rod_softmax_focal', (0, 0, 0, 0, 0, 0, 1, 0, B, A, K, code, 0))[0],
                  'focal_loss_entry': roofline.cost('rod_focal_loss', (0, 0, 0, 0, 0, 0, 0, 1, 0, B, A, K, code, 0))[0]}
        assert nbytes['focal'] == B * A * (2 * K * es + 12)
        r = {}
        for k, t in times.items():
            us = statistics.median(t)
            r[k] = {'us': round(us, 2), 'us_min': round(min(t), 2), 'us_max': round(max(t), 2)}
            if nbytes[k]:
                r[k].update(bytes=nbytes[k], GBps=round(nbytes[k] / us * 1e-3, 1),
                            fraction_of_8TBps=round(nbytes[k] / us * 1e-3 / roofline.MI355X_HBM_PEAK_GBS, 4))
        r['focal_over_hnm'] = round(r['focal']['us'] / r['hnm']['us'], 4)
        r['pass'] = r['focal']['us'] <= r['hnm']['us']
        ok &= r['pass']
        rec['dtypes'][dname] = r
    rec['pass'] = bool(ok)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
