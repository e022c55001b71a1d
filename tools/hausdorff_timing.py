#!/usr/bin/env python3
"""Time mrirt.inr.hausdorff_distance (4 classes, unit spacing) on the large synthetic label pair of the test fixture, and —
where scipy is importable — a cKDTree formulation of the same quantity on the same host as the CPU side of the comparison.

GPU side: label volumes already on the device, `--warmup` untimed calls, then `--iters` calls each bracketed by its own
pair of events on the launch stream (the device time of the 4 x (3 passes + reduction) + 2 launches, no host read-back),
and separately the wall time of the whole Python call including the read-back of the 8 numbers.  Reported: median, min,
max.  CPU side: per class, a k-d tree over the coordinates of each mask and a nearest-neighbour query of the other mask's
points, both directions (one run; it takes tens of seconds).

    python tools/hausdorff_timing.py [--shape 240 240 155] [--iters 10] [--warmup 3] [--no-cpu] [--out FILE.json]
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def kdtree_hausdorff(pred, true, num_classes, workers=1):
    from scipy.spatial import cKDTree
    idx = np.indices(pred.shape, dtype=np.float32).reshape(3, -1).T
    out = {}
    for c in range(num_classes):
        a, b = idx[(pred == c).ravel()], idx[(true == c).ravel()]
        if len(a) == 0 or len(b) == 0:
            out[c] = float("nan")
            continue
        ab = cKDTree(b).query(a, workers=workers)[0].max()
        ba = cKDTree(a).query(b, workers=workers)[0].max()
        out[c] = float(max(ab, ba))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--workers", type=int, default=1, help="threads of the k-d tree queries (the reference uses 1)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import hausdorff_cases as hc
    from mrirt import inr
    shape = tuple(args.shape) if args.shape else hc.load_large()[0]
    pred, true = hc.large_pair(shape)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(true).cuda()
    for _ in range(args.warmup):
        inr.hausdorff_directed_sq(p, t, (1.0, 1.0, 1.0), 4)
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        inr.hausdorff_directed_sq(p, t, (1.0, 1.0, 1.0), 4)
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    for _ in range(args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = inr.hausdorff_distance(p, t, num_classes=4)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    vox = int(np.prod(shape))
    pairs = 8 * vox * sum(shape)                              # 4 classes x 2 fields, every voxel against its three lines
    res = dict(shape=list(shape), voxels=vox, classes=4, device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
               gpu_device_ms=dict(median=statistics.median(dev_ms), min=min(dev_ms), max=max(dev_ms)),
               gpu_call_wall_ms=dict(median=statistics.median(wall_ms), min=min(wall_ms), max=max(wall_ms)),
               line_pass_pairs=pairs, fp64_ops_per_pair=4,
               fp64_ops_per_second=4 * pairs / (statistics.median(dev_ms) * 1e-3),
               hausdorff={str(c): got[c] for c in got})
    if not args.no_cpu:
        try:
            import scipy  # noqa: F401
            t0 = time.perf_counter()
            cpu = kdtree_hausdorff(pred, true, 4, args.workers)
            res["cpu_kdtree_s"] = time.perf_counter() - t0
            res["cpu_kdtree_workers"] = args.workers
            res["cpu_equals_gpu"] = all((cpu[c] == got[c]) or (cpu[c] != cpu[c] and got[c] != got[c]) for c in got)
        except ImportError:
            res["cpu_kdtree_s"] = None
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
