"""A plain ``bench.py`` run measures the headline only, and ``--dump-outputs`` writes the frame its last timed step rendered:
on the one GPU (the frame loop) and through the N > 1 exchange path rehearsed at world size 1 (``--force-exchange``)."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
SIDE_KEYS = ("pipelined", "k1_reference_path", "inr_path", "scaling_model", "cpu_baseline", "parity")


@pytest.mark.parametrize("extra", [[], ["--force-exchange"]], ids=["one_gpu", "force_exchange"])
def test_plain_run_dumps_the_last_timed_frame(tmp_path, extra):
    from mrirt import synth
    from oracle import oracle_c
    n, image, steps = 64, 128, 64
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "1", "--volume", str(n), "--image", str(image),
                        "--march-steps", str(steps), "--dump-outputs", str(tmp_path), *extra],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "Msamples/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert not [k for k in SIDE_KEYS if k in out], "side measurements belong to --full"
    frame = np.load(tmp_path / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (image, image, 4)
    # the bench scene (STRICT math: bit-identical to the oracle)
    p = synth.brats_scene(n, image, steps, channels=1, intensity_alpha=16.0)
    ref = oracle_c.brats_main(p, [synth.synth_volume(n)], None, None, synth.SHADE_EXT)
    assert np.array_equal(frame, ref), f"max-abs {float(np.abs(frame - ref).max()):.3e}"
