"""Run the predict.py inference path (Predictor: forward + decode + per-class NMS, HIP-graph
replay) on a synthetic batch with a detector-like score distribution, for rocprofv3 kernel
traces of configs[3] / configs[4].
Usage: python tools/predict_bench.py [--res 720|1080] [--batch 32] [--iters 10] [--no-graph]
                                     [--nms_method hard|linear|gaussian] [--probe]
--probe adds eager calls timed per entry by the call probe (rod._abi.PROBE, HIP events around
the NMS entry; a graph replay cannot be probed) and reports their median / min / max."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'road-object-detection-for-bdd100k_amd'))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=720)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--nms_method', default='hard', choices=['hard', 'linear', 'gaussian'])
    ap.add_argument('--probe', action='store_true')
    a = ap.parse_args()
    import predict
    from rod import _abi
    from rod.data import detector_like_scores, synthetic_batch
    H, W = (720, 1280) if a.res == 720 else (1080, 1920)
    dev = torch.device('cuda')
    pr = predict.Predictor((H, W), dev, torch.bfloat16, nms_method=a.nms_method)
    pr.use_graph = not a.no_graph
    img = synthetic_batch(a.batch, H, W, dev, seed=77)[0]
    frac = detector_like_scores(pr, img[:4], rate=0.02)
    for _ in range(2):
        pr(img)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        pr(img)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.iters
    out = {'img_hw': [H, W], 'batch': a.batch, 'graph': pr.use_graph, 'nms_method': a.nms_method,
           'ms_per_batch': round(dt * 1e3, 3), 'images_per_s': round(a.batch / dt, 1),
           'selected_frac': round(frac, 4)}
    if a.probe:
        entry = 'rod_select_topk_nms' if a.nms_method == 'hard' else 'rod_select_topk_softnms'
        pr.use_graph = False
        pr(img)
        _abi.PROBE.arm(entry)
        for _ in range(a.iters):
            pr(img)
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for _, e0, e1, _, _ in _abi.PROBE.records)
        _abi.PROBE.disarm()
        out['probe'] = {'entry': entry, 'calls': len(ms), 'median_ms': round(ms[len(ms) // 2], 4),
                        'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4)}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
