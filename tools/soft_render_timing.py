#!/usr/bin/env python3
"""The soft prediction overlay on a training-sized frame: 128^3 x 4 modalities, 256^2, 128 steps per diagonal (about 3 M march
samples), LINEAR grids, STRICT — device events around every run, median of 20 after 3 warm-ups.
    python3 tools/soft_render_timing.py [n] [image] [steps] [--out profiles/r15_soft/timing.json]
Measures  the soft forward against mrirt_render_brats_stream on the same frame (classes = argmax of the same logits),
          the soft backward (and its ratio to the forward),
          the whole step of a 7 -> 3 x 256 -> 4 SIREN: emit + fp32 forward + soft render + soft backward + weight backward
          (mrirt.inr.render_brats_inr_autograd + backward; it contains the one host read of the sample total),
and writes them as JSON."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, mrirt
from mrirt import _lib, params, synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "r15_soft", "timing.json")
if "--out" in sys.argv:
    args.remove(out_path)
n = int(args[0]) if len(args) > 0 else 128
image = int(args[1]) if len(args) > 1 else 256
steps = int(args[2]) if len(args) > 2 else 128
WARMUP, RUNS, CLASSES = 3, 20, 4
vols = [torch.from_numpy(synth.synth_volume(n, 1234 + m, phase=0.3 * m)).cuda().reshape(-1) for m in range(4)]
lab = torch.from_numpy(synth.synth_labels(n).astype(np.int32)).cuda().reshape(-1)
p = synth.brats_scene(n, image, steps, channels=4, show_seg=True, intensity_alpha=0.4)
p = dict(p, showPred=1)
P, E = params.brats_params(p), params.render_ext(None)
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
counts = torch.empty(image * image, dtype=torch.int32, device="cuda")
_lib.check(_lib.lib().mrirt_brats_sample_counts(C.byref(P), C.byref(E), ptr(counts), None), "mrirt_brats_sample_counts")
ends = torch.cumsum(counts.to(torch.int64), 0)
offsets = (ends - counts).contiguous()
total = int(ends[-1])
gen = torch.Generator(device="cuda").manual_seed(1)
logits = 2.0 * torch.randn((max(total, 1), CLASSES), device="cuda", generator=gen)
classes = logits.argmax(1).to(torch.int16)
G = torch.randn((image, image, 4), device="cuda", generator=gen)
frame = torch.empty((image, image, 4), device="cuda")
dl = torch.zeros_like(logits)
vp = (C.c_void_p * 4)(*[ptr(v) for v in vols])


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def hard():
    _lib.check(_lib.lib().mrirt_render_brats_stream(C.byref(P), C.byref(E), vp, ptr(lab), ptr(classes), ptr(offsets), ptr(frame), image, None, None),
               "mrirt_render_brats_stream")


rng = np.random.default_rng(3)
dims = [7, 256, 256, 256, 4]
Ws = [torch.from_numpy(rng.uniform(-1, 1, (a, b)).astype(np.float32) * np.float32(np.sqrt(6.0 / a) / (30.0 if i == 0 else 1.0))).cuda().requires_grad_(True)
      for i, (a, b) in enumerate(zip(dims[:-1], dims[1:]))]
bs = [torch.zeros(b, device="cuda", requires_grad=True) for b in dims[1:]]


def step():
    for t in Ws + bs:
        t.grad = None
    fr = mrirt.inr.render_brats_inr_autograd(p, vols, Ws, bs, (0.5,) * 4, (0.25,) * 4, w0=30.0, labels=lab)
    (fr * G).sum().backward()


res = dict(volume=n, image=image, steps=steps, samples=total, classes=CLASSES, runs=RUNS, statistic="median of device-event times, ms")
res["hard_stream_forward_ms"] = timed(hard)
res["soft_forward_ms"] = timed(lambda: mrirt.render_brats_soft(p, vols, logits, offsets, lab, out=frame))
res["soft_backward_ms"] = timed(lambda: mrirt.render_brats_soft_backward(p, vols, logits, offsets, G, lab, out=dl))
res["soft_over_hard"] = res["soft_forward_ms"] / res["hard_stream_forward_ms"]
res["backward_over_forward"] = res["soft_backward_ms"] / res["soft_forward_ms"]
res["siren_7_3x256_4_whole_step_ms"] = timed(step)
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
