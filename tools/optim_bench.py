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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--launches', type=int, default=5000)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('optim_bench: no GPU visible (timings are taken on the device only)')
    dev = torch.device('cuda:0')
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
    for f in runs.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.launches)
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
