#!/usr/bin/env python3
"""Time the class-surface extraction (mrirt_surface_count + mrirt_surface_extract, csrc/surface.hip) at 240 x 240 x 155 —
a ball of radius 40 centred at (100, 120, 80), and all three classes of the synthetic label volume (mrirt.synth.synth_labels)
— and the NumPy restatement of the definition (tests/surface_ref.py) on the same host as the CPU side of the comparison.

GPU side: the label volume already on the device, scratch and outputs allocated once, `--warmup` untimed pairs of calls,
then `--iters` pairs each bracketed by its own pair of events on the launch stream (the device time of the 12 launches, no
host read-back), and separately the wall time of mrirt.extract_surface (allocation and the read of the two counts
included).  Reported: median, min, max.  The output is compared with the restatement's (equality) before anything is timed.

    python tools/surface_timing.py [--shape 240 240 155] [--iters 20] [--warmup 3] [--no-cpu] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(240, 240, 155))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import surface_ref as sr
    import mrirt
    from mrirt import _lib, synth
    shape = tuple(args.shape)
    g = np.indices(shape).astype(np.float64)
    ball = np.where((g[0] - 100) ** 2 + (g[1] - 120) ** 2 + (g[2] - 80) ** 2 <= 40.0 ** 2, 1, 0).astype(np.int16)
    nested = synth.synth_labels(0, dims=(shape[2], shape[1], shape[0])).reshape(shape).astype(np.int16)
    lib = _lib.lib()
    hwd = (C.c_uint32 * 3)(*shape)
    sp, org = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)
    nbytes = int(lib.mrirt_surface_scratch_bytes(hwd))
    res = dict(shape=list(shape), cells=sr.num_cells(shape), scratch_bytes=nbytes, device=torch.cuda.get_device_name(0),
               iters=args.iters, warmup=args.warmup, cases={})
    for name, lab, classes in (("ball_r40", ball, (1,)), ("synth_labels_1_2_3", nested, (1, 2, 3))):
        mask = sr.class_mask(classes)
        t0 = time.perf_counter()
        want_v, want_t = sr.extract(lab, mask)
        numpy_s = time.perf_counter() - t0
        dev = torch.from_numpy(lab).cuda()
        verts, tris = mrirt.extract_surface(dev, classes)
        equal = bool(np.array_equal(verts.cpu().numpy().view(np.uint32), want_v.view(np.uint32)) and np.array_equal(tris.cpu().numpy(), want_t))
        scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
        counts = torch.empty(2, dtype=torch.int64, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def pair():
            rc = lib.mrirt_surface_count(C.c_void_p(dev.data_ptr()), hwd, mask, C.c_void_p(scratch.data_ptr()), nbytes,
                                         C.c_void_p(counts.data_ptr()), stream)
            rc = rc or lib.mrirt_surface_extract(C.c_void_p(dev.data_ptr()), hwd, mask, sp, org, C.c_void_p(verts.data_ptr()),
                                                 verts.shape[0], C.c_void_p(tris.data_ptr()), tris.shape[0],
                                                 C.c_void_p(scratch.data_ptr()), nbytes, C.c_void_p(counts.data_ptr()), stream)
            _lib.check(rc, "mrirt_surface_count / mrirt_surface_extract")

        for _ in range(args.warmup):
            pair()
        torch.cuda.synchronize()
        dev_ms, wall_ms = [], []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pair()
            e1.record()
            e1.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
        for _ in range(args.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v, t = mrirt.extract_surface(dev, classes)
            torch.cuda.synchronize()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
        res["cases"][name] = dict(classes=list(classes), vertices=len(want_v), triangles=len(want_t), equals_restatement=equal,
                                  gpu_count_plus_extract_device_ms=stats(dev_ms), extract_surface_wall_ms=stats(wall_ms),
                                  numpy_restatement_s=None if args.no_cpu else numpy_s)
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
