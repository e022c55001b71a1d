#!/usr/bin/env python3
"""Time the case preparation on the GPU (csrc/prep.hip) at 240 x 240 x 155 x 4 modalities against the host code it replaces
(volume.normalize_intensity, volume.zscore_nonzero; scipy.ndimage.gaussian_filter when SciPy is installed) on the same box.

GPU side: the raw case already on the device, scratch and outputs allocated once, `--warmup` untimed rounds, then `--iters`
rounds each bracketed by its own pair of events on the launch stream (device time of the launches, no host read-back).  One
round is all four modalities.  Reported: median, min, max in ms.  Every output is compared with the host's before anything is
timed (equality for the window, the normalisation and the Gaussian; the z-score is reported as its largest difference).

    python tools/prep_timing.py [--shape 240 240 155] [--iters 20] [--warmup 3] [--no-cpu] [--out FILE.json]
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


def host_ms(fn, repeats=3):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(240, 240, 155))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from mrirt import _lib, volume
    shape, M = tuple(args.shape), 4
    n = int(np.prod(shape))
    rng = np.random.default_rng(0)
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, k) for k in shape], indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    raw = np.stack([np.where(r > 0.9, 0.0, np.clip(1.2 - r, 0, None) * (800 + 100 * m) + rng.random(shape) * 40).astype(np.int16)
                    for m in range(M)]).astype(np.float32)                       # zero background, as skull-stripped MRI has
    lib = _lib.lib()
    dev = torch.from_numpy(raw).cuda()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dims = (C.c_uint32 * 3)(*shape)

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    # --- equality first -------------------------------------------------------------------------------------------------
    checks = {}
    lin, norm, _, _ = volume.normalize_intensity_device(dev[0])
    want_lin, want_norm, _ = volume.normalize_intensity(raw[0])
    checks["normalize_equals_host"] = bool(np.array_equal(norm.cpu().numpy(), want_norm) and np.array_equal(lin.cpu().numpy(), want_lin))
    zs, _ = volume.zscore_nonzero_device(dev)
    checks["zscore_max_abs_diff_vs_host"] = float(max(np.abs(zs[m].cpu().numpy() - volume.zscore_nonzero(raw[m])).max() for m in range(M)))
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        checks["gaussian_equals_scipy"] = bool(np.array_equal(volume.gaussian_filter_device(dev[0], args.sigma).cpu().numpy(),
                                                              ndimage.gaussian_filter(raw[0], args.sigma)))
    # --- device time ----------------------------------------------------------------------------------------------------
    need = int(lib.mrirt_prep_scratch_bytes(n))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    rec = torch.empty((M, 8), dtype=torch.float32, device="cuda")
    out_norm, out_lin = torch.empty_like(dev), torch.empty((M, n), dtype=torch.float32, device="cuda")

    def window():
        for m in range(M):
            _lib.check(lib.mrirt_prep_window(ptr(dev[m]), n, 1.0, 99.5, ptr(rec[m]), ptr(scratch), need, s), "mrirt_prep_window")

    def normalize():
        for m in range(M):
            _lib.check(lib.mrirt_prep_normalize(ptr(dev[m]), dims, ptr(rec[m]), ptr(out_norm[m]), ptr(out_lin[m]), s), "mrirt_prep_normalize")

    zneed = int(lib.mrirt_prep_zscore_scratch_bytes(n, M))
    zscratch = torch.empty(zneed, dtype=torch.uint8, device="cuda")
    zstats = torch.empty((4, M), dtype=torch.float32, device="cuda")
    zout = torch.empty_like(dev)

    def zscore():
        _lib.check(lib.mrirt_prep_zscore_stats(ptr(dev), n, M, ptr(zstats), ptr(zscratch), zneed, s), "mrirt_prep_zscore_stats")
        _lib.check(lib.mrirt_prep_zscore_apply(ptr(dev), n, M, ptr(zstats), ptr(zout), s), "mrirt_prep_zscore_apply")

    w = volume.gaussian_weights(args.sigma)
    wc = (C.c_double * len(w))(*w.tolist())
    gout, gscratch = torch.empty_like(dev), torch.empty_like(dev[0])

    def gaussian():
        for m in range(M):
            _lib.check(lib.mrirt_prep_gaussian3d(ptr(dev[m]), dims, wc, (len(w) - 1) // 2, ptr(gout[m]), ptr(gscratch), s), "mrirt_prep_gaussian3d")

    res = dict(shape=list(shape), modalities=M, device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, sigma=args.sigma,
               checks=checks, gpu_device_ms={}, host_ms={})
    for name, fn in (("window", window), ("normalize_both_layouts", normalize), ("zscore_stats_plus_apply", zscore), ("gaussian", gaussian)):
        res["gpu_device_ms"][name] = timed(fn, args.iters, args.warmup, torch)
    if not args.no_cpu:
        res["host_ms"]["normalize_intensity"] = host_ms(lambda: [volume.normalize_intensity(raw[m]) for m in range(M)])
        res["host_ms"]["zscore_nonzero"] = host_ms(lambda: [volume.zscore_nonzero(raw[m]) for m in range(M)])
        if ndimage is not None:
            res["host_ms"]["scipy_gaussian_filter"] = host_ms(lambda: [ndimage.gaussian_filter(raw[m], args.sigma) for m in range(M)])
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
