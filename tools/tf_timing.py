#!/usr/bin/env python3
"""Time the K1 march with an RGBA transfer-function table (csrc/brats_tf.hip) beside the plain march, at the two BASELINE
geometries (synth.CONFIGS):

    C2  256^3 x 4 modalities as one MOD4 grid + ground-truth overlay through label cells, 512 x 512, 256 steps, unshaded
    C3  512^3, one modality, VGA (value + gradient, axis-flat), 1024 x 1024, 512 steps, gradient-shaded

Per geometry, in one process, through the C ABI on the same grids and the same output buffer:

    ex           mrirt_render_brats_ex (no dispatch order, no skipping): the pipelined plain kernel
    ex_generic   the same with kernelVariant bit 2: the plain GENERIC kernel, which the table kernel is modelled on
    tf_ramp      mrirt_render_brats_tf with the two-entry ramp (the same bits as `ex`, hence the same samples; checked)
    tf_hot       ... with the 256-entry "hot" table (both geometries select a pipelined table kernel)
    tf_generic   ... with the "hot" table and kernelVariant bit 2: the generic table kernel (the same bits; checked)

Method: `--warmup` untimed rounds of every variant, then `--iters` rounds that ALTERNATE the variants, each launch bracketed by
its own pair of device events; reported per variant: median, min, max in ms (the spread), and live samples per frame.

    python tools/tf_timing.py [--iters 20] [--warmup 3] [--configs C2,C3] [--out FILE.json]   (default: profiles/r21_tf/tf_timing.json)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--scale", type=int, default=1, help="divide volume and image sizes (rehearsals only)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r21_tf" / "tf_timing.json"))
    args = ap.parse_args()
    import torch
    import mrirt
    from mrirt import _lib, params as mp, synth
    assert torch.cuda.is_available(), "tf_timing.py measures on the GPU: there is no fallback"
    lib = _lib.lib()
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, scale=args.scale, configs={})
    hot = torch.from_numpy(mrirt.tf_preset("hot")).cuda()
    ramp = torch.from_numpy(mrirt.tf_ramp()).cuda()
    for key in args.configs.split(","):
        cfg = synth.CONFIGS[key]
        n, image, steps = cfg["n"] // args.scale, cfg["image"] // args.scale, cfg["steps"] // args.scale
        dims = (n, n, n)
        shade = bool(cfg.get("shade"))
        p = synth.brats_scene(n, image, steps, channels=cfg["channels"], intensity_alpha=cfg["intensity_alpha"], show_seg=bool(cfg.get("show_seg")))
        ext = dict(synth.SHADE_EXT) if shade else {}
        vols = [synth.synth_volume(n, 1234 + m, phase=0.3 * m) for m in range(cfg["channels"])]
        if shade:
            grids = [mrirt.upload_grid(vols[0], dims, "vga", macro=False)] + [None] * 3
            ext["layout"], lab = "vga", None
        else:
            grids = [mrirt.upload_mod4(vols + [None] * (4 - len(vols)), dims, macro=False)] * 4
            lab = mrirt.upload_label_cells(synth.synth_labels(n), None, dims, macro=False)
            ext.update(layout="mod4", labelLayout="labcell")
        del vols
        P = mp.brats_params(p)
        vp = (C.c_void_p * 4)(*[C.c_void_p(g.data.data_ptr()) if g is not None else None for g in grids])
        lp = C.c_void_p(lab.data.data_ptr()) if lab is not None else None
        out = torch.empty((image, image, 4), dtype=torch.float32, device="cuda")
        st = torch.zeros(2, dtype=torch.int64, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def launch(table, variant, counters=False):
            E = mp.render_ext(dict(ext, kernelVariant=variant))
            sp = C.c_void_p(st.data_ptr()) if counters else None
            if table is None:
                rc = lib.mrirt_render_brats_ex(C.byref(P), C.byref(E), vp, lp, None, C.c_void_p(out.data_ptr()), image, sp, stream)
            else:
                rc = lib.mrirt_render_brats_tf(C.byref(P), C.byref(E), vp, lp, None, C.c_void_p(table.data_ptr()), int(table.shape[0]),
                                               C.c_void_p(out.data_ptr()), image, sp, stream)
            _lib.check(rc, "render")

        variants = {"ex": (None, 0), "ex_generic": (None, 4), "tf_ramp": (ramp, 0), "tf_hot": (hot, 0), "tf_generic": (hot, 4)}
        run = dict(dims=list(dims), image=image, steps=steps, layout=ext["layout"], shaded=shade, variants={})
        frames = {}
        for name, (table, variant) in variants.items():
            st.zero_()
            launch(table, variant, counters=True)
            live, shaded_n = (int(v) for v in st.cpu())
            frames[name] = out.clone()
            run["variants"][name] = dict(live_samples=live, shaded_samples=shaded_n)
        run["ramp_equals_ex"] = bool(torch.equal(frames["tf_ramp"], frames["ex"]) and torch.equal(frames["ex_generic"], frames["ex"]))
        run["generic_equals_default"] = bool(torch.equal(frames["tf_generic"], frames["tf_hot"]))
        run["hot_differs_from_ex"] = float((frames["tf_hot"] - frames["ex"]).abs().max())
        del frames
        for _ in range(args.warmup):
            for table, variant in variants.values():
                launch(table, variant)
        torch.cuda.synchronize()
        ms = {name: [] for name in variants}
        for _ in range(args.iters):
            for name, (table, variant) in variants.items():           # alternating: every round times every variant once
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(table, variant)
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        for name, xs in ms.items():
            run["variants"][name].update(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs))
        res["configs"][key] = run
        del grids, lab, out
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
