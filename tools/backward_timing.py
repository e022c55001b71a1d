#!/usr/bin/env python3
"""K1 forward and backward on BASELINE config 2's geometry (256^3 x 4 modalities + seg overlay, 512^2, 256 steps, STRICT) on
LINEAR grids — the layout the backward pass takes: device events around 20 runs of each after 3 warm-ups.
    python3 tools/backward_timing.py [n] [image] [steps]
Prints one line with the two times and their ratio (profiles/r08_backward/README.md)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, mrirt
from mrirt import synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
image = int(sys.argv[2]) if len(sys.argv) > 2 else 512
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 256
WARMUP, RUNS = 3, 20
vols = [torch.from_numpy(synth.synth_volume(n, 1234 + m, phase=0.3 * m)).cuda().reshape(-1) for m in range(4)]
lab = torch.from_numpy(synth.synth_labels(n).astype(np.int32)).cuda().reshape(-1)
p = synth.brats_scene(n, image, steps, channels=4, show_seg=True, intensity_alpha=0.4)
out = torch.empty((image, image, 4), device="cuda")
G = torch.randn((image, image, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
acc = ([torch.zeros(n ** 3, device="cuda") for _ in range(4)], torch.zeros(4, dtype=torch.float64, device="cuda"))


def timed(fn):
    for _ in range(WARMUP):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(RUNS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / RUNS


fwd = timed(lambda: mrirt.render_brats(p, vols, labels=lab, out=out))
bwd = timed(lambda: mrirt.render_brats_backward(p, vols, G, labels=lab, accumulate_into=acc))
print(f"K1 LINEAR {n}^3 x 4 + seg, {image}^2, {steps} steps: forward {fwd:.3f} ms, backward {bwd:.3f} ms, backward / forward {bwd / fwd:.1f}")
