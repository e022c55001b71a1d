#!/usr/bin/env python3
"""Time the pieces of the hybrid, uncertainty-guided sampler (csrc/inr_hybrid.hip):

  class index    mrirt_inr_class_count + the host's prefix sums + mrirt_inr_class_index for two 240 x 240 x 155 cases, C = 4 (load
                 time: once per cache), beside the tumour index of the same cache
  selection      mrirt_select_largest at n = 10 000, k = 2000 and 3000 (the notebook's stage 1 and 2), with torch.topk beside it
                 for scale (topk returns its picks in value order and has no tie rule)
  micro-batch    VoxelCache.sample_hybrid (U = 2000, P = 300, sigma > 0, with the boundary field: one launch) against
                 VoxelCache.sample + VoxelCache.sample_field (two launches), n = 4000
  step           a whole train_inject step with the notebook's keys at micro-batch 4000 against the same step without them, and
                 the pieces of the uncertainty pass (candidates, five MC-dropout passes over 10 000 candidates, selection) on
                 their own, which gives their share of the step

Inputs are on the device; after `--warmup` untimed rounds the paths alternate for `--iters` rounds in one process, each call
bracketed by its own pair of events on the launch stream.  Reported: median [min, max] in ms.

    python tools/hybrid_timing.py [--iters 20] [--warmup 5] [--out profiles/r25_hybrid/timing.json]
"""
import argparse
import json
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

NC, CW = 4, [0.1, 1.5, 1.0, 2.0]
F, M, HIDDEN = 128, 4, (64, 64, 64)


def alternate(fns, iters, warmup):
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ms.items()}


def blob_labels(rng, hwd):
    """Three nested tumour classes around a centre, about 1 % of the voxels."""
    g = np.meshgrid(*[np.arange(e, dtype=np.float32) for e in hwd], indexing="ij")
    c = [e * (0.35 + 0.3 * rng.random()) for e in hwd]
    r = np.sqrt(sum((a - b) ** 2 for a, b in zip(g, c)))
    return ((r < 30).astype(np.int16) + (r < 20) + (r < 10)).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from mrirt import inr, synth
    if not torch.cuda.is_available():
        raise SystemExit("hybrid_timing.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup)

    # ---- class index: two BraTS-sized label volumes (no modalities: the index reads the labels alone)
    rng = np.random.default_rng(0)
    hwd = (240, 240, 155)
    big = [{"mods": np.zeros((0, *hwd), np.float32), "seg": blob_labels(rng, hwd)} for _ in range(2)]

    def class_index():
        inr.VoxelCache.class_index(big_cache, NC)
        big_cache._classes.clear()

    def tumour_index():
        inr.VoxelCache.tumour_index(big_cache)
        big_cache._tumour = None
    big_cache = inr.VoxelCache(big)
    t = alternate({"class_index": class_index, "tumour_index": tumour_index}, args.iters, args.warmup)
    big_cache.class_index(NC)
    res["class_index"] = dict(hwd=hwd, ncases=2, C=NC, voxels_per_class=[int(sum((c["seg"] == k).sum() for c in big)) for k in range(NC)], ms=t,
                              note="count + the host's read of the counts + three launches + the synchronisation that frees the scratch")
    del big_cache, big

    # ---- selection
    rows = []
    for n, k in ((10000, 2000), (10000, 3000), (65536, 3000)):
        v = torch.from_numpy(np.random.default_rng(n + k).random(n).astype(np.float32) * np.float32(1.386)).to(dev)
        t = alternate({"mrirt_select_largest": lambda: inr.select_largest(v, k), "torch_topk": lambda: torch.topk(v, k)}, args.iters, args.warmup)
        same = sorted(inr.select_largest(v, k).cpu().tolist()) == sorted(torch.topk(v, k).indices.cpu().tolist())
        rows.append(dict(n=n, k=k, ms=t, same_set_as_topk=same))
    res["select_largest"] = rows

    # ---- micro-batch and step: the notebook's shape on a 48^3 synthetic case
    size = 48
    mods = np.stack([synth.synth_volume(size, 1234 + m, phase=0.3 * m).reshape(size, size, size).transpose(2, 1, 0) for m in range(M)])
    mods = ((mods - mods.mean((1, 2, 3), keepdims=True)) / mods.std((1, 2, 3), keepdims=True)).astype(np.float32)
    seg = np.clip(synth.synth_labels(size).reshape(size, size, size).transpose(2, 1, 0), 0, NC - 1).astype(np.int16)
    cache = inr.VoxelCache([{"mods": np.ascontiguousarray(mods), "seg": np.ascontiguousarray(seg)}])
    cache.set_boundary()
    cache.class_index(NC)
    n, U, P, n_cand = 4000, 2000, 300, 10000
    picks = inr.select_largest(torch.rand(n_cand, device=dev), U)
    t = alternate({"sample_hybrid": lambda: cache.sample_hybrid(3, 1, n, U, picks, P, NC, 0.01, with_field=True),
                   "sample_hybrid_uniform_no_noise": lambda: cache.sample_hybrid(3, 1, n, with_field=True),
                   "sample_plus_sample_field": lambda: (cache.sample(3, 1, n), cache.sample_field(3, 1, n))}, args.iters, args.warmup)
    res["micro_batch"] = dict(n=n, U=U, P=P, C=NC, ms=t)

    params = inr.inject_init(1, F, M, HIDDEN, NC)
    desc = inr.inject_desc(params)
    B, w, b = inr._inject_flat(params, dev)
    scratch = inr._inject_scratch(desc, n_cand, dev)
    drop = inr.inject_dropout(4, 0.7, 5, 0, 0)
    cc, cm, _ = cache.sample_candidates(3, 1, n_cand)
    ent = inr.inject_uncertainty(desc, B, w, b, cc, cm, n_cand, drop, scratch)
    t = alternate({"sample_candidates": lambda: cache.sample_candidates(3, 1, n_cand),
                   "inject_uncertainty_5_passes": lambda: inr.inject_uncertainty(desc, B, w, b, cc, cm, n_cand, drop, scratch),
                   "select_largest": lambda: inr.select_largest(ent, U)}, args.iters, args.warmup)
    res["uncertainty_pass"] = dict(n_cand=n_cand, samples=5, k=U, ms=t)

    steps = 10
    base = dict(NUM_CLASSES=NC, RNG_SEED=3, FOURIER_DIM=F, HIDDEN_DIMS=list(HIDDEN), COORD_INJECTION_LAYERS=[1, 2, 3], MODALITY_INJECTION_LAYERS=[2],
                DROPOUT_RATE=0.3, MICRO_BATCH_SIZE=n, ACCUM_STEPS=1, STAGE1_STEPS=steps + 1, STAGE2_STEPS=0, LR_STAGE1=2e-3, LR_STAGE2=5e-4,
                MIN_LR=1e-5, WARMUP_STEPS=0, WEIGHT_DECAY=1e-4, CLIP_NORM=1.0, CLASS_WEIGHTS=CW, UNIFIED_FOCAL_GAMMA=0.5, UNIFIED_FOCAL_LAMBDA=0.5,
                TV_WEIGHT_STAGE1=0.02, TV_WEIGHT_STAGE2=0.05, BOUNDARY_WEIGHT=0.1)
    hybrid = dict(base, UNCERTAINTY_RATIO=0.5, BALANCED_RATIO=0.3, UNIFORM_RATIO=0.2, COORD_NOISE_SIGMA_INIT=0.01, COORD_NOISE_SIGMA_FINAL=0.001)
    # step 0 runs without uncertainty (t > WARMUP_STEPS gates it), the ten after it with: eleven steps, divided by eleven
    t = alternate({"train_inject_plain": lambda: inr.train_inject(base, cache, params), "train_inject_hybrid": lambda: inr.train_inject(hybrid, cache, params)},
                  max(3, args.iters // 4), 1)
    per = {k: {s: v / (steps + 1) for s, v in d.items()} for k, d in t.items()}
    unc = res["uncertainty_pass"]["ms"]
    res["step"] = dict(micro_batch=n, steps=steps + 1, steps_with_uncertainty=steps, ms_per_step=per,
                       uncertainty_share_of_hybrid_step=(unc["inject_uncertainty_5_passes"]["median"] * steps / (steps + 1)) / per["train_inject_hybrid"]["median"],
                       candidates_and_selection_share=((unc["sample_candidates"]["median"] + unc["select_largest"]["median"]) * steps / (steps + 1))
                       / per["train_inject_hybrid"]["median"])
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
