#!/usr/bin/env python3
"""Host time per call of the torch operators, through both doors (torch.ops.mrirt and torch.ops.mrirt_native).

The operators are meant to be thin.  This times the valid tiny calls of tests/test_gpu_torch_ops_refusals.py (8^3 voxels, 8 x 8
pixels, 64 points: the kernels are a few microseconds, so what is measured is the operator layer and the dispatcher): per
operator and door CALLS calls enqueued back to back with one synchronisation at the end, wall time over CALLS.  One JSON line.

    python tools/torch_ops_host_cost.py [calls] [package root]

``package root``: the directory holding mrirt.py and the package to measure (default: this checkout) — how a parent
checkout's operator layer is timed by the same script, alternating with this one's."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else HERE
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mrirt  # noqa: E402,F401
from test_gpu_torch_ops_refusals import build_calls  # noqa: E402

OPERATORS = ("render_brats[linear]", "render_brats_soft_backward", "inr_loss", "inr_sample_batch_mix")

env = build_calls()
result = {"root": ROOT, "calls": CALLS, "us_per_call": {}}
for name in OPERATORS:
    op, args = env["calls"][name]
    for door, ops in env["doors"]:
        fn = getattr(ops, op)
        for _ in range(200):                             # warm-up: code objects, the allocator's blocks, the dispatcher's caches
            fn(*args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn(*args)
        torch.cuda.synchronize()
        result["us_per_call"][f"{op}/{door}"] = round((time.perf_counter() - t0) / CALLS * 1e6, 3)
print(json.dumps(result))
