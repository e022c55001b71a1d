#!/usr/bin/env python3
"""Time the connected components on the GPU (csrc/components.hip) at 240 x 240 x 155 against scipy.ndimage.label on the same
box (one thread; when SciPy is installed).

Volumes: the ball-plus-noise case of tests/cc_cases.py (one large component, tens of thousands of specks) and classes 1-3 of
synth.synth_labels (three nested shells, one component).  Connectivity 1 and 3.  GPU side: the labels already on the device,
outputs and scratch allocated once, `--warmup` untimed rounds, then `--iters` rounds each bracketed by its own pair of events
on the launch stream.  Timed: mrirt_cc_label alone, and the chain label + sizes + filter (min_voxels 10) — the chain with N
read back once before it is timed, as remove_small_components reads it.  Reported: median, min, max in ms.  Every GPU result
is compared with SciPy's before anything is timed.

    python tools/cc_timing.py [--iters 20] [--warmup 3] [--no-cpu] [--out FILE.json]      (default: profiles/r20_components/cc_timing.json)
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


def timed(fn, iters, warmup, torch):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r20_components" / "cc_timing.json"))
    args = ap.parse_args()
    import torch
    import cc_cases
    from mrirt import _lib, synth
    from mrirt.mesh import class_mask
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    shape = cc_cases.BALL_SHAPE
    volumes = {"ball_plus_noise": (cc_cases.ball_with_noise(), class_mask(1)),
               "synth_labels_classes_1_3": (synth.synth_labels(0, (shape[2], shape[1], shape[0])).reshape(shape).astype(np.int16), class_mask((1, 2, 3)))}
    lib = _lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hwd = (C.c_uint32 * 3)(*shape)
    need = int(lib.mrirt_cc_scratch_bytes(hwd))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    comp = torch.empty(shape, dtype=torch.int32, device="cuda")
    count = torch.empty(1, dtype=torch.int64, device="cuda")
    out = torch.empty(shape, dtype=torch.int16, device="cuda")

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    res = dict(shape=list(shape), device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, scratch_bytes=need, runs={})
    for name, (lab, mask) in volumes.items():
        dev = torch.from_numpy(lab).cuda()
        for conn in (1, 3):
            def label():
                _lib.check(lib.mrirt_cc_label(ptr(dev), hwd, mask, conn, ptr(comp), ptr(count), ptr(scratch), need, s), "mrirt_cc_label")

            label()
            n = int(count.cpu()[0])
            sizes = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")

            def chain():
                label()
                _lib.check(lib.mrirt_cc_sizes(ptr(comp), hwd, n, ptr(sizes), s), "mrirt_cc_sizes")
                _lib.check(lib.mrirt_cc_filter(ptr(dev), ptr(comp), ptr(sizes), n, hwd, 10, 0, 0, ptr(out), s), "mrirt_cc_filter")

            run = dict(n_components=n)
            inside = (lab >= 0) & (lab < 32) & (((mask >> np.clip(lab, 0, 31).astype(np.int64)) & 1) != 0)
            if ndimage is not None:
                st = ndimage.generate_binary_structure(3, conn)
                want, wn = ndimage.label(inside, st)
                run["equals_scipy"] = bool(wn == n and np.array_equal(comp.cpu().numpy(), want))
            run["gpu_label_ms"] = timed(label, args.iters, args.warmup, torch)
            run["gpu_label_sizes_filter_ms"] = timed(chain, args.iters, args.warmup, torch)
            if ndimage is not None and not args.no_cpu:
                host = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    ndimage.label(inside, st)
                    host.append((time.perf_counter() - t0) * 1e3)
                run["scipy_label_ms"] = stats(host)
            res["runs"][f"{name}_connectivity_{conn}"] = run
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
