#!/usr/bin/env python3
"""Time Muon on the notebook's SIREN shapes (7 -> 3 x 256 -> 4 and 7 -> 4 x 256 -> 4, micro-batch 4096 and 65536):

  optimiser step   one step of mrirt_inr_train_run_muon (sampler, forward, loss, backward, Muon update; accum 1) beside one step
                   of mrirt_siren_train_run (the same with the AdamW update), and beside the Python composition of the separate
                   library calls with the Muon update written in torch (momentum, Newton-Schulz with torch.matmul in fp32, apply)
  orthogonalize    mrirt_muon_orthogonalize of the network's matrices alone beside the same Newton-Schulz with torch.matmul

Everything already on the device, `--warmup` untimed calls, then `--iters` calls each bracketed by its own pair of events on
the launch stream; medians.  The one-call runs are timed as `--run-steps` steps divided by the count.

    python tools/muon_timing.py [--iters 20] [--warmup 5] [--out profiles/r12_muon/timing.json]
"""
import argparse
import json
import math
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SHAPES = [dict(hidden=256, hidden_layers=hl, classes=4, n=n) for hl in (3, 4) for n in (4096, 65536)]
CW, DW, W0, M = [0.5, 1.0, 2.0, 1.5], 0.5, 30.0, 4
LR = 2e-4


def timed(fn, iters, warmup, per=1):
    import torch
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
        ms.append(e0.elapsed_time(e1) / per)
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def torch_ns(mats, coeffs, steps, eps):
    """The Newton-Schulz of include/mrirt.h on a list of (in, out) fp32 matrices, with torch.matmul."""
    import torch
    c0, c1, c2 = coeffs
    out = []
    for m in mats:
        X = m / (torch.linalg.matrix_norm(m) + eps)
        t = m.shape[0] > m.shape[1]
        if t:
            X = X.T
        for _ in range(steps):
            A = torch.matmul(X, X.T)
            B = c1 * A + c2 * torch.matmul(A, A)
            X = c0 * X + torch.matmul(B, X)
        out.append(X.T if t else X)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--run-steps", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import inr_ref
    from mrirt import inr, synth
    torch.set_float32_matmul_precision("highest")
    dev = torch.device("cuda:0")
    size = 32
    mods = np.stack([synth.synth_volume(size, 1234 + m, phase=0.3 * m).reshape(size, size, size).transpose(2, 1, 0) for m in range(M)])
    mods = ((mods - mods.mean((1, 2, 3), keepdims=True)) / mods.std((1, 2, 3), keepdims=True)).astype(np.float32)
    seg = synth.synth_labels(size).reshape(size, size, size).transpose(2, 1, 0).astype(np.int16)
    cache = inr.VoxelCache([{"mods": np.ascontiguousarray(mods), "seg": np.ascontiguousarray(seg)}])
    hp = inr.muon_hp()
    rows = []
    for s in SHAPES:
        rng = np.random.default_rng(1)
        dims = [3 + M] + [s["hidden"]] * s["hidden_layers"] + [s["classes"]]
        n = s["n"]
        layers = inr_ref.siren_params(rng, dims)
        desc = inr.siren_train_desc(dims, M, W0)
        sizes = [a * b for a, b in zip(dims[:-1], dims[1:])]
        scales = [math.sqrt(max(1.0, b / a)) for a, b in zip(dims[:-1], dims[1:])]

        def views(flat):
            return [v.view(a, b) for v, a, b in zip(torch.split(flat, sizes), dims[:-1], dims[1:])]

        def state():
            return inr.AdamWState.from_params(layers)
        cfg_adamw = inr.train_cfg(n, 1, 3, CW, DW, LR, LR, 0, 1000, 0.0)
        cfg_muon = inr.train_cfg(n, 1, 3, CW, DW, LR, LR, 0, 1000, 0.0, b1=inr.MUON_BIAS_B1, b2=inr.MUON_BIAS_B2, eps=inr.MUON_BIAS_EPS,
                                 weight_decay=inr.MUON_BIAS_WEIGHT_DECAY)
        st_a, st_m, st_c = state(), state(), state()
        scratch_a = torch.empty(int(inr._run_entry(desc, None)[1](inr.C.byref(desc), inr.C.byref(cache.desc), inr.C.byref(cfg_adamw))),
                                dtype=torch.uint8, device=dev)
        scratch_m = torch.empty(int(inr._run_entry(desc, hp)[1](inr.C.byref(desc), inr.C.byref(cache.desc), inr.C.byref(cfg_muon))),
                                dtype=torch.uint8, device=dev)

        def run_adamw():
            return inr.train_run(desc, cache, cfg_adamw, st_a, args.run_steps, scratch_a)

        def run_muon():
            return inr.train_run(desc, cache, cfg_muon, st_m, args.run_steps, scratch_m, muon=hp)
        step_scratch = inr.siren_train_scratch(desc, n, dev)
        gw, gb = torch.empty_like(st_c.w), torch.empty_like(st_c.b)
        beta = inr.MUON_BETA

        def composition():
            t = st_c.step
            coords, feats, labels = cache.sample(3, t, n)
            logits = inr.siren_forward_f32(desc, st_c.w, st_c.b, coords, feats, n, step_scratch)
            _, _, dl = inr.loss_and_dlogits(logits, labels, CW, DW, step_scratch)
            inr.siren_backward_f32(desc, st_c.w, n, dl, step_scratch, gw, gb)
            st_c.mu_w.mul_(beta).add_(gw, alpha=1.0 - beta)
            mhat = beta * (st_c.mu_w / (1.0 - beta ** (t + 2))) + (1.0 - beta) * (gw / (1.0 - beta ** (t + 1)))
            for W, O, sc in zip(views(st_c.w), torch_ns(views(mhat), inr.MUON_NS_COEFFS, inr.MUON_NS_STEPS, inr.MUON_EPS), scales):
                W.sub_(O, alpha=LR * sc)
            st_c.mu_b.mul_(0.9).add_(gb, alpha=0.1)
            st_c.nu_b.mul_(0.999).addcmul_(gb, gb, value=0.001)
            st_c.b.sub_(LR * (st_c.mu_b / (1.0 - 0.9 ** (t + 1))) / ((st_c.nu_b / (1.0 - 0.999 ** (t + 1))).sqrt() + 1e-8))
            st_c.step += 1
        m_flat = torch.from_numpy(rng.standard_normal(sum(sizes)).astype(np.float32)).to(dev)
        ns_scratch = inr._muon_scratch(inr.train_desc(dims), dev)

        def ns_library():
            return inr.muon_orthogonalize(dims, m_flat, hp, ns_scratch)

        def ns_torch():
            return torch_ns(views(m_flat), inr.MUON_NS_COEFFS, inr.MUON_NS_STEPS, inr.MUON_EPS)
        got, want = ns_library(), torch.cat([o.reshape(-1) for o in ns_torch()])
        row = dict(shape=s, dims=dims, ns_max_abs_difference_library_vs_torch=float((got - want).abs().max()),
                   adamw_step_ms=timed(run_adamw, args.iters, max(1, args.warmup // 2), per=args.run_steps),
                   muon_step_ms=timed(run_muon, args.iters, max(1, args.warmup // 2), per=args.run_steps),
                   composition_step_ms=timed(composition, args.iters, args.warmup),
                   orthogonalize_ms=timed(ns_library, args.iters, args.warmup), torch_matmul_ns_ms=timed(ns_torch, args.iters, args.warmup))
        row["ratio_muon_over_adamw_step"] = row["muon_step_ms"]["median"] / row["adamw_step_ms"]["median"]
        row["ratio_muon_over_composition"] = row["muon_step_ms"]["median"] / row["composition_step_ms"]["median"]
        row["ratio_orthogonalize_over_torch"] = row["orthogonalize_ms"]["median"] / row["torch_matmul_ns_ms"]["median"]
        flop = inr.MUON_NS_STEPS * 2 * sum(2 * min(a, b) ** 2 * max(a, b) + min(a, b) ** 3 for a, b in zip(dims[:-1], dims[1:]))
        row["orthogonalize_tflops"] = flop / (row["orthogonalize_ms"]["median"] * 1e-3) / 1e12
        rows.append(row)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, run_steps=args.run_steps, lr=LR, rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
