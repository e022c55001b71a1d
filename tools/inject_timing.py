#!/usr/bin/env python3
"""Time the coordinate-injection INR (csrc/inr_inject.hip) at the notebook's own shape against the same function evaluated with
torch on the same GPU in the same process.

Shape: F = 128, M = 4, widths 64 / 64 / 64, C = 4, keep = 0.7, a 240 x 240 x 155 synthetic case (normal modalities, a Glorot net,
three nested label shells for the boundary map), chunks of 50000 voxels.  Timed, each warmed, with device events around the
whole call, the library and the baseline alternating, median of `--iters` with min and max:
  predict    mrirt_inject_predict_volume (pred only)             vs  torch.sin / cos / matmul / relu / argmax, chunked alike
  uncertain  the same call with the entropy volume, S = 5        vs  the same in torch with torch.rand masks, softmax, entropy
  boundary   mrirt_boundary_weights                              vs  SciPy's distance_transform_edt loop on the host (when installed)
The torch baseline draws its own masks (its generator, not the library's Philox): it is a cost baseline, not a bit reference.
Reported with each time: the algorithmic FLOPs of the layers from the shapes (2 in out per point per layer; S + 1 passes for
the uncertainty call) and the share of the 157 TFLOP/s fp32-matrix peak they amount to over the WHOLE call -- features,
dropout words, softmax and launches included in the time, not in the FLOPs.

    python tools/inject_timing.py [--iters 20] [--warmup 3] [--no-cpu] [--out FILE.json]     (default: profiles/r22_inject/inject_timing.json)
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

HWD, F, M, WIDTHS, CL, ML, KEEP, S, CHUNK = (240, 240, 155), 128, 4, (64, 64, 64, 4), (1, 2), (2,), 0.7, 5, 50000
PEAK_FP32_MATRIX = 157e12


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def timed_pair(fns, iters, warmup, torch):
    """The functions alternate: round i times each of them once."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [stats(m) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r22_inject" / "inject_timing.json"))
    args = ap.parse_args()
    import torch
    import inject_ref as ref
    from mrirt import _lib, inr

    rng = np.random.default_rng(22)
    params = ref.glorot_net(rng, F, M, WIDTHS, CL, ML)
    n = HWD[0] * HWD[1] * HWD[2]
    mods = torch.randn((M, *HWD), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(22))
    desc = inr.inject_desc(params, CL, ML)
    w, b = ref.flat(params)
    dB, dw, db = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (params["fourier"]["B"], w, b))
    lib = _lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hwd = (C.c_uint32 * 3)(*HWD)
    need = int(lib.mrirt_inject_scratch_bytes(C.byref(desc), CHUNK))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    pred = torch.empty(HWD, dtype=torch.int16, device="cuda")
    ent = torch.empty(HWD, dtype=torch.float32, device="cuda")
    drop = inr.inject_dropout(1, KEEP, S)

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    def lib_predict():
        _lib.check(lib.mrirt_inject_predict_volume(C.byref(desc), ptr(dB), ptr(dw), ptr(db), ptr(mods), hwd, CHUNK, None, ptr(pred), None,
                                                   ptr(scratch), need, s), "mrirt_inject_predict_volume")

    def lib_uncertain():
        _lib.check(lib.mrirt_inject_predict_volume(C.byref(desc), ptr(dB), ptr(dw), ptr(db), ptr(mods), hwd, CHUNK, C.byref(drop), ptr(pred),
                                                   ptr(ent), ptr(scratch), need, s), "mrirt_inject_predict_volume")

    # ---- the torch baseline: the definition with torch.sin / cos / matmul / relu, chunked alike -----------------------------
    Ws = [torch.from_numpy(p["W"]).cuda() for p in params["mlp"]]
    bs = [torch.from_numpy(p["b"]).cuda() for p in params["mlp"]]
    shapes = ref.net_shape(F, M, WIDTHS, CL, ML)
    flat_mods = mods.reshape(M, n)
    ax = [(torch.arange(e, dtype=torch.float32, device="cuda") / float(e - 1)) * 2.0 - 1.0 for e in HWD]
    t_pred = torch.empty(n, dtype=torch.int16, device="cuda")
    t_ent = torch.empty(n, dtype=torch.float32, device="cuda")
    scale = 1.0 / KEEP

    def chunk_inputs(i0, i1):
        g = torch.arange(i0, i1, device="cuda")
        z, xy = g % HWD[2], g // HWD[2]
        c = torch.stack([ax[0][xy // HWD[1]], ax[1][xy % HWD[1]], ax[2][z]], 1)
        a = 6.2831855 * (((c + 1.0) * 0.5) @ dB.T)
        return c, flat_mods[:, i0:i1].T, torch.cat([torch.sin(a), torch.cos(a)], 1)

    def torch_layers(c, m, feat, masked):
        h = feat
        for l, (W, bb, (n_in, split, split_m, _)) in enumerate(zip(Ws, bs, shapes)):
            parts = [h] + ([c] if split_m > split else []) + ([m] if n_in > split_m else [])
            z = torch.matmul(torch.cat(parts, 1) if len(parts) > 1 else h, W) + bb
            if l == len(Ws) - 1:
                return z
            h = torch.relu(z)
            if masked:
                h = h * (torch.rand_like(h) < KEEP) * scale

    def torch_predict():
        for i0 in range(0, n, CHUNK):
            i1 = min(i0 + CHUNK, n)
            t_pred[i0:i1] = torch.argmax(torch_layers(*chunk_inputs(i0, i1), False), 1).to(torch.int16)

    def torch_uncertain():
        for i0 in range(0, n, CHUNK):
            i1 = min(i0 + CHUNK, n)
            c, m, feat = chunk_inputs(i0, i1)
            t_pred[i0:i1] = torch.argmax(torch_layers(c, m, feat, False), 1).to(torch.int16)
            acc = torch.softmax(torch_layers(c, m, feat, True), 1)
            for _ in range(S - 1):
                acc = acc + torch.softmax(torch_layers(c, m, feat, True), 1)
            mean = acc / float(S)
            t_ent[i0:i1] = -(mean * torch.log(mean + 1e-10)).sum(1)

    lib_predict()
    torch_predict()
    torch.cuda.synchronize()
    agree = float((pred.reshape(-1) == t_pred).float().mean())

    flops_pass = 2.0 * n * sum(s_[0] * s_[3] for s_ in shapes)
    res = dict(shape=list(HWD), device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, chunk=CHUNK, scratch_bytes=need,
               net=dict(F=F, M=M, widths=list(WIDTHS), keep=KEEP, samples=S), argmax_agreement_with_torch=agree, runs={})

    def record(name, pair, flops):
        lib_ms, torch_ms = pair
        res["runs"][name] = dict(library_ms=lib_ms, torch_ms=torch_ms, algorithmic_flops=flops,
                                 whole_call_share_of_fp32_matrix_peak=flops / (lib_ms["median"] * 1e-3) / PEAK_FP32_MATRIX,
                                 speedup_over_torch=torch_ms["median"] / lib_ms["median"])

    record("predict_full_volume", timed_pair([lib_predict, torch_predict], args.iters, args.warmup, torch), flops_pass)
    record("uncertainty_S5", timed_pair([lib_uncertain, torch_uncertain], args.iters, args.warmup, torch), (S + 1) * flops_pass)

    # ---- boundary weights ---------------------------------------------------------------------------------------------------
    x, y, z = np.meshgrid(*[np.arange(e) - (e - 1) / 2 for e in HWD], indexing="ij")
    r = np.sqrt((x / 90) ** 2 + (y / 80) ** 2 + (z / 60) ** 2)
    seg = (np.where(r < 0.25, 3, np.where(r < 0.4, 1, np.where(r < 0.55, 2, 0)))).astype(np.int16)
    dseg = torch.from_numpy(seg).cuda()
    bneed = int(lib.mrirt_boundary_weights_scratch_bytes(hwd))
    bscratch = torch.empty(bneed, dtype=torch.uint8, device="cuda")
    wout = torch.empty(HWD, dtype=torch.float32, device="cuda")

    def lib_boundary():
        _lib.check(lib.mrirt_boundary_weights(ptr(dseg), hwd, 4, ptr(wout), ptr(bscratch), bneed, s), "mrirt_boundary_weights")

    run = dict(library_ms=timed_pair([lib_boundary], args.iters, args.warmup, torch)[0], scratch_bytes=bneed)
    try:
        from scipy.ndimage import distance_transform_edt
    except ImportError:
        distance_transform_edt = None
    if distance_transform_edt is not None and not args.no_cpu:
        t0 = time.perf_counter()
        want = np.zeros(HWD, np.float64)
        for c in range(1, 4):
            want = np.maximum(want, 1.0 / (1.0 + distance_transform_edt(seg != c)))
        run["scipy_host_ms"] = (time.perf_counter() - t0) * 1e3
        run["equals_scipy"] = bool(np.array_equal(wout.cpu().numpy(), want.astype(np.float32)))
    res["runs"]["boundary_weights"] = run

    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
