"""Cost of the optimiser entries on the flat parameter buffer of the 720x1280 REFINE network:
rod_sgd_clip (the default step, the yardstick), rod_sgd_momentum (momentum 0.9, weight decay,
norm clipping: 5 fp32 streams + a flag byte per 4 elements against 3 streams) and
rod_grad_sqnorm (1 stream).

    python tools/optim_bench.py [--launches 5000] [--rounds 7] [--out profiles/optim_bench.json]

Device events around `launches` back-to-back launches of one entry, after a warm-up; the three
entries alternate within each round and the median round is reported, with the spread.  The
buffers are a few tens of MB, so repeated launches find part of them in the last-level cache:
the same holds for all three entries, and for the step itself, where the gradient was just
written.  Bytes are the algorithmic counts of rod.roofline.

    python tools/optim_bench.py --ema [--step_replays 40] [--out profiles/ema_bench.json]

The weight-EMA leg, same method and buffer: rod_sgd_momentum (the baseline), rod_sgd_momentum_ema
(the average kept in the same pass: 7 fp32 streams + the flag byte) and, for context,
rod_sgd_momentum followed by a separate torch.lerp_ pass over the buffer (what keeping the average
outside the kernel costs in device time; it could not live in a captured step).  With
--step_replays > 0 it also times the whole bf16 720x1280 batch-8 REFINE step replayed as a graph,
with ema_decay off and on.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'road-object-detection-for-bdd100k_amd'), ROOT]

import torch  # noqa: E402

from rod import ops, roofline  # noqa: E402
from rod.trainer import Trainer  # noqa: E402


def timed_rounds(runs, launches, rounds):
    """{name: [us per launch, one value per round]}: the entries alternate within each round."""
    for f in runs.values():
        for _ in range(20):
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


def graphed_step_ms(dev, replays, **kw):
    """Median device time of one replay of the bf16 720x1280 batch-8 REFINE step graph."""
    from rod.data import synthetic_batch
    tr = Trainer((720, 1280), 8, dtype=torch.bfloat16, device=dev, momentum=0.9, weight_decay=1e-4, **kw)
    batch = synthetic_batch(8, 720, 1280, dev, seed=1)
    for _ in range(4):                       # eager, capture + replay, two more replays
        tr.step_graphed(*batch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.step_graphed(*batch)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    assert torch.isfinite(tr.net.store.flat).all() and len(tr._graphs) == 1
    return {'entry': tr.opt.entry, 'ms': round(statistics.median(ts), 4), 'ms_min': round(min(ts), 4),
            'ms_max': round(max(ts), 4), 'replays': replays}


def ema_leg(a, dev):
    tr = Trainer((720, 1280), 1, dtype=torch.bfloat16, device=dev, momentum=0.9, weight_decay=1e-4, clip_norm=10.0,
                 ema_decay=0.999)
    st, opt = tr.net.store, tr.opt
    n = st.numel
    st.flat_grad.normal_(generator=torch.Generator(device=dev).manual_seed(0))
    lr0 = torch.zeros(1, device=dev)      # rate 0: the parameters keep their values however many launches run
    scale = opt.hyper[1:2]
    # the average moves towards the (fixed) parameters with a real rate and stays bounded
    rate = torch.full((1,), 1e-3, device=dev)

    def momentum():
        ops.sgd_momentum_(st.flat, st.flat_grad, opt.mom, opt.flags, lr0, scale, 0.0, 1e-4, 5.0, False)

    def fused():
        ops.sgd_momentum_ema_(st.flat, st.flat_grad, opt.mom, opt.ema, opt.flags, lr0, scale, rate, 0.0, 1e-4, 5.0,
                              False)

    def separate():
        momentum()
        opt.ema.lerp_(st.flat, rate)

    runs = {'rod_sgd_momentum': momentum, 'rod_sgd_momentum_ema': fused, 'rod_sgd_momentum+torch.lerp_': separate}
    nbytes = {'rod_sgd_momentum': roofline.cost('rod_sgd_momentum', (0, 0, opt.mom, 0, n))[0],
              'rod_sgd_momentum_ema': roofline.cost('rod_sgd_momentum_ema', (0, 0, opt.mom, 0, 0, n))[0]}
    nbytes['rod_sgd_momentum+torch.lerp_'] = nbytes['rod_sgd_momentum'] + 12 * n
    times = timed_rounds(runs, a.launches, a.rounds)
    assert torch.isfinite(st.flat).all() and torch.isfinite(opt.ema).all()
    rec = {'device': torch.cuda.get_device_name(0), 'elements': n, 'launches': a.launches, 'rounds': a.rounds,
           'timing': 'device events around back-to-back launches, median of rounds', 'entries': {}}
    base = statistics.median(times['rod_sgd_momentum'])
    for k, t in times.items():
        us = statistics.median(t)
        rec['entries'][k] = {'us': round(us, 3), 'us_min': round(min(t), 3), 'us_max': round(max(t), 3),
                             'bytes': nbytes[k], 'GBps': round(nbytes[k] / us * 1e-3, 1),
                             'ratio_to_sgd_momentum': round(us / base, 3)}
    rec['bytes_ratio_fused_to_baseline'] = round(nbytes['rod_sgd_momentum_ema'] / nbytes['rod_sgd_momentum'], 3)
    if a.step_replays > 0:
        del tr, st, opt
        torch.cuda.empty_cache()
        off = graphed_step_ms(dev, a.step_replays)
        torch.cuda.empty_cache()
        on = graphed_step_ms(dev, a.step_replays, ema_decay=0.999)
        rec['graphed_step_720p_b8_refine_bf16'] = {'ema_off': off, 'ema_on': on,
                                                   'ratio_on_to_off': round(on['ms'] / off['ms'], 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--launches', type=int, default=5000)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_bench.json'))
    ap.add_argument('--ema', action='store_true', help='the weight-EMA leg (default --out profiles/ema_bench.json)')
    ap.add_argument('--step_replays', type=int, default=0,
                    help='--ema: also time this many graph replays of the 720p b8 REFINE step, EMA off and on')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('optim_bench: no GPU visible (timings are taken on the device only)')
    dev = torch.device('cuda:0')
    if a.ema:
        if a.out == ap.get_default('out'):
            a.out = os.path.join(ROOT, 'profiles', 'ema_bench.json')
        return ema_leg(a, dev)
    tr = Trainer((720, 1280), 1, dtype=torch.bfloat16, device=dev, momentum=0.9, weight_decay=1e-4, clip_norm=10.0)
    st, opt = tr.net.store, tr.opt
    n = st.numel
    st.flat_grad.normal_(generator=torch.Generator(device=dev).manual_seed(0))
    lr0 = torch.zeros(1, device=dev)      # rate 0: the buffers keep their values however many launches run
    scale = opt.hyper[1:2]
    runs = {
        'rod_sgd_clip': lambda: ops.sgd_clip_(st.flat, st.flat_grad, 0.0, 5.0),
        'rod_sgd_momentum': lambda: ops.sgd_momentum_(st.flat, st.flat_grad, opt.mom, opt.flags, lr0, scale, 0.0,
                                                      1e-4, 5.0, False),
        'rod_grad_sqnorm': lambda: ops.grad_sqnorm_(st.flat_grad, opt.flags, 10.0, scale, opt._ws),
    }
    # (momentum factor 0 in the timed update: m = 0*m + d stays bounded over thousands of launches;
    # the kernel reads and writes the same five streams whatever the factor)
    args = {
        'rod_sgd_clip': (0, 0, n),
        'rod_sgd_momentum': (0, 0, opt.mom, 0, n),
        'rod_grad_sqnorm': (0, 0, n),
    }
    times = timed_rounds(runs, a.launches, a.rounds)
    assert torch.isfinite(st.flat).all()
    rec = {'device': torch.cuda.get_device_name(0), 'elements': n, 'launches': a.launches, 'rounds': a.rounds,
           'timing': 'device events around back-to-back launches, median of rounds', 'entries': {}}
    base = statistics.median(times['rod_sgd_clip'])
    for k, t in times.items():
        us = statistics.median(t)
        nbytes = roofline.cost(k, args[k])[0]
        rec['entries'][k] = {'us': round(us, 3), 'us_min': round(min(t), 3), 'us_max': round(max(t), 3),
                             'bytes': nbytes, 'GBps': round(nbytes / us * 1e-3, 1),
                             'ratio_to_sgd_clip': round(us / base, 3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
