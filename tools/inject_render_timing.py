#!/usr/bin/env python3
"""Time the fused forward of the coordinate-injection INR (csrc/inr_inject_fused.hip) and the per-sample frame it drives
(mrirt_render_brats_inject), at the notebook's shape: F = 128, M = 4, widths 64 / 64 / 64, C = 4, a Glorot net.

  classify   mrirt_inject_classify (one launch, argmax only)  vs  the chain mrirt_inject_forward (argmax only: features, one
             GEMM launch per layer, point kernel), at n = 50 000 and n = 2^22 resident random points
  frame      bench.py's C5 scene (256^3 x 4 modalities as one MOD4 grid + seg, 512 x 512 px, 256 steps) through
             mrirt_render_brats_inject, and the same frame through mrirt_render_brats_inr with the bench's 4 x 256 SIREN
Each function is warmed, the two of a pair alternate in one process, device events around the whole call, median of `--iters`
with min and max.  With each time: the algorithmic FLOPs of the layers (2 in out per point per layer) over the WHOLE call --
features, staging, plan / emit / composite included in the time, not in the FLOPs -- as a share of the 157 TFLOP/s fp32-matrix
peak; for the frames over the live (composited) samples, with the queries per frame beside them.

    python tools/inject_render_timing.py [--iters 20] [--warmup 3] [--skip-frame] [--out FILE.json]
                                                                  (default: profiles/r26_inject_render/inject_render_timing.json)
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

F, M, WIDTHS, CL, ML = 128, 4, (64, 64, 64, 4), (1, 2), (2,)
PEAK_FP32_MATRIX = 157e12
SIZES = (50000, 1 << 22)


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
    ap.add_argument("--skip-frame", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r26_inject_render" / "inject_render_timing.json"))
    args = ap.parse_args()
    import torch
    import inject_ref as ref
    import mrirt
    from mrirt import _lib, inr, synth

    rng = np.random.default_rng(26)
    params = ref.glorot_net(rng, F, M, WIDTHS, CL, ML)
    desc = inr.inject_desc(params, CL, ML)
    w, b = ref.flat(params)
    dB, dw, db = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (params["fourier"]["B"], w, b))
    lib = _lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    shapes = ref.net_shape(F, M, WIDTHS, CL, ML)
    flop_point = 2 * sum(n_in * out for n_in, _, _, out in shapes)
    result = dict(shape=dict(F=F, M=M, widths=WIDTHS, coord_layers=CL, mod_layers=ML), flop_per_point=flop_point,
                  fused_lds_bytes=int(lib.mrirt_inject_fused_lds_bytes(C.byref(desc))), iters=args.iters, warmup=args.warmup,
                  device=torch.cuda.get_device_name(0), classify={})

    # ---- (a) classify ------------------------------------------------------------------------------------------------------
    for n in SIZES:
        g = torch.Generator("cuda").manual_seed(n)
        coords = torch.rand((n, 3), device="cuda", generator=g) * 2 - 1
        mods = torch.randn((n, M), device="cuda", generator=g)
        am_f = torch.zeros(n, dtype=torch.int16, device="cuda")
        am_c = torch.zeros(n, dtype=torch.int16, device="cuda")
        need = int(lib.mrirt_inject_scratch_bytes(C.byref(desc), n))
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")

        def fused():
            _lib.check(lib.mrirt_inject_classify(C.byref(desc), ptr(dB), ptr(dw), ptr(db), ptr(coords), ptr(mods), n, None, ptr(am_f), None, s),
                       "mrirt_inject_classify")

        def chain():
            _lib.check(lib.mrirt_inject_forward(C.byref(desc), ptr(dB), ptr(dw), ptr(db), ptr(coords), ptr(mods), n, None, None, ptr(am_c),
                                                ptr(scratch), need, s), "mrirt_inject_forward")

        tf, tc = timed_pair([fused, chain], args.iters, args.warmup, torch)
        assert bool((am_f == am_c).all()), "the fused classes differ from the chain's"
        share = lambda t: flop_point * n / (t["median"] * 1e-3) / PEAK_FP32_MATRIX
        below = tf["median"] < tc["median"] and (tc["median"] - tf["median"]) > max(tf["max"] - tf["min"], tc["max"] - tc["min"])
        result["classify"][str(n)] = dict(fused_ms=tf, chain_ms=tc, fused_peak_share=share(tf), chain_peak_share=share(tc),
                                          ns_per_point_fused=tf["median"] * 1e6 / n, ns_per_point_chain=tc["median"] * 1e6 / n,
                                          chain_scratch_bytes=need, fused_below_chain_by_more_than_both_spreads=bool(below))
        print(f"classify n={n}: fused {tf['median']:.4f} [{tf['min']:.4f}, {tf['max']:.4f}] ms, chain {tc['median']:.4f} "
              f"[{tc['min']:.4f}, {tc['max']:.4f}] ms; peak share {share(tf):.3f} / {share(tc):.3f}", flush=True)
        del coords, mods, scratch

    # ---- (b) frame ---------------------------------------------------------------------------------------------------------
    if not args.skip_frame:
        import bench
        dims, sparams = bench.siren_c5(np.random.default_rng(0))
        siren = inr.pack_mlp(sparams, inr.KIND_SIREN, 0, 4)
        siren_flop = 2 * sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
        nvox, image, steps = 256, 512, 256
        vols = [synth.synth_volume(nvox, 1234 + m, phase=0.3 * m) for m in range(4)]
        lab = synth.synth_labels(nvox)
        zmu = [float(v[v != 0].mean()) for v in vols]
        zsg = [float(v[v != 0].std() + 1e-6) for v in vols]
        p5 = synth.brats_scene(nvox, image, steps, channels=4, show_seg=True, show_pred=True, intensity_alpha=0.4)
        gv = mrirt.upload_mod4(vols, (nvox, nvox, nvox))
        gl = mrirt.upload_grid(lab, (nvox, nvox, nvox), "brick")
        out = torch.empty((image, image, 4), dtype=torch.float32, device="cuda")
        _, aux_i = inr.render_brats_inject(p5, gv, params, zmu, zsg, labels=gl, out=out, return_aux=True, coord_layers=CL, mod_layers=ML)
        _, aux_s = inr.render_brats_inr(p5, gv, siren, zmu, zsg, labels=gl, out=out, return_aux=True)

        def inject_frame():
            inr.render_brats_inject(p5, gv, params, zmu, zsg, labels=gl, out=out, coord_layers=CL, mod_layers=ML)

        def siren_frame():
            inr.render_brats_inr(p5, gv, siren, zmu, zsg, labels=gl, out=out)

        ti, ts = timed_pair([inject_frame, siren_frame], args.iters, args.warmup, torch)
        result["frame"] = dict(
            scene="256^3 x 4 modalities (MOD4) + seg, 512 x 512 px, 256 steps", chunk_steps=aux_i["chunk_steps"],
            inject=dict(ms=ti, queries=aux_i["queries"], live_samples=aux_i["live_samples"],
                        peak_share_live=flop_point * aux_i["live_samples"] / (ti["median"] * 1e-3) / PEAK_FP32_MATRIX),
            siren=dict(ms=ts, queries=aux_s["queries"], live_samples=aux_s["live_samples"], flop_per_query=siren_flop))
        print(f"frame: inject {ti['median']:.3f} [{ti['min']:.3f}, {ti['max']:.3f}] ms, {aux_i['queries']} queries, {aux_i['live_samples']} live; "
              f"SIREN {ts['median']:.3f} [{ts['min']:.3f}, {ts['max']:.3f}] ms, {aux_s['queries']} queries", flush=True)

    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
