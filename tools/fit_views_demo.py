#!/usr/bin/env python3
"""The differentiability proof: gradients flow rendered pixels -> ray marcher -> MLP weights, and an optimisation converges.
A teacher SIREN 7 -> 2 x 32 -> 4 is rendered from three cameras through the soft prediction overlay; a perturbed copy of it is then
fitted to those frames with mrirt.inr.fit_views (MSE, AdamW) and the loss history is printed.
    python3 tools/fit_views_demo.py [steps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, mrirt
from mrirt import synth

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
n, image, w0 = 16, 32, 30.0
vols = [torch.from_numpy(synth.synth_volume(n, 1234 + m, phase=0.3 * m)).cuda().reshape(-1) for m in range(4)]
gparams = synth.brats_scene(n, image, 32, channels=4, intensity_alpha=1.5)
cams = []
for seed in (1, 2, 3):                                      # three cameras on the scene's orbit
    p = synth.brats_scene(n, image, 32, channels=4, intensity_alpha=1.5)
    rot = np.random.default_rng(seed).normal(size=3)
    eye = np.asarray(p["eye"], np.float64)
    eye = np.linalg.norm(eye) * (eye / np.linalg.norm(eye) + 0.6 * rot / np.linalg.norm(rot))
    W = -eye / np.linalg.norm(eye)
    U = np.cross(W, [0.0, 1.0, 0.0]); U /= np.linalg.norm(U)
    V = np.cross(U, W)
    cams.append(dict(eye=eye.astype(np.float32), U=U.astype(np.float32), V=V.astype(np.float32), W=W.astype(np.float32)))
teacher = mrirt.inr.siren_init(7, 7, [32, 32], 4, w0)
other = mrirt.inr.siren_init(8, 7, [32, 32], 4, w0)
start = {k: {q: (teacher[k][q] + np.float32(0.35) * other[k][q]).astype(np.float32) for q in ("w", "b")} for k in teacher}
zmu, zsigma = (0.5,) * 4, (0.25,) * 4
with torch.no_grad():
    tW = [torch.from_numpy(teacher[f"l{i}"]["w"]).cuda() for i in range(3)]
    tb = [torch.from_numpy(teacher[f"l{i}"]["b"]).cuda() for i in range(3)]
    targets = [mrirt.inr.render_brats_inr_autograd({**gparams, **c}, vols, tW, tb, zmu, zsigma, w0=w0) for c in cams]
losses, _ = mrirt.inr.fit_views(dict(STEPS=steps, LR=2e-3, W0=w0), cams, targets, vols, start, gparams, zmu, zsigma,
                                log=lambda s, l: print(f"step {s:3d}  loss {l:.6e}"))
print(f"loss {losses[0]:.3e} -> {losses[-1]:.3e} ({losses[-1] / losses[0]:.3f} x) over {steps} steps")
