"""The transfer-function table on the CPU: the NumPy restatement (tf_ref.py) tied to the oracle through the two-entry ramp, the
cases' coverage, the table builders, the C ABI's declaration and its refusals (which launch nothing), the FAST tolerance.  No GPU."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import tf_cases as TC
import tf_ref
from mrirt import _lib, params, transfer
from oracle import oracle_np as onp

ROOT = pathlib.Path(__file__).resolve().parent.parent
OK, ERR_NULL, ERR_LAYOUT, ERR_ARG = 0, -1, -3, -5


def _plain(name):
    c, d = TC.BY_NAME[name], TC.data(name)
    return onp.brats_main(c["params"], d["vols"], d["labels"], d["preds"], c["ext"], return_aux=True)


@pytest.mark.parametrize("name", TC.NAMES)
def test_ramp_is_the_oracle(name):
    """tf_ref with the two-entry ramp == oracle_np.brats_main on EVERY scene: frame bits, live and shaded counts, per-pixel T."""
    frame, aux = _plain(name)
    r = TC.reference(name, "ramp")
    assert tf_ref.compare(frame, aux["live_samples"], aux["shaded_samples"], r) == []
    assert np.array_equal(aux["T"], r["T"]) and np.array_equal(aux["nsteps"], r["nsteps"])


@pytest.mark.parametrize("name", TC.GENERAL_NAMES)
def test_a_table_changes_the_frame(name):
    """No test can pass by ignoring the table: every non-ramp case differs from the plain frame by >= 1e-2 somewhere."""
    frame, _ = _plain(name)
    r = TC.reference(name)
    diff = float(np.abs(r["frame"].astype(np.float64) - frame).max())
    print(f"{name}: max |table frame - plain frame| = {diff:.3f}")
    assert diff >= 1e-2


def test_cases_cover_the_table_events():
    seen = {}
    for name in TC.NAMES:
        c, r = TC.BY_NAME[name], TC.reference(name)
        for k, v in r["seen"].items():
            seen[k] = seen.get(k, False) or v
        if c["dense"]:
            ert = np.float32(c["ext"].get("ertThreshold", 0.01))
            n = int((r["T"] <= ert).sum())
            print(f"{name}: {n} rays ended by early termination")
            assert n > 0, name
    assert seen == dict(i_first=True, i_last=True, u_top=True, sigma_nonpos=True, sigma_above_one=True), seen
    assert {TC.TABLES[TC.BY_NAME[n]["table"]].shape[0] for n in TC.NAMES} >= {2, 3, 17, 256, 1024}
    assert (TC.TABLES["negative"][:, 3] < 0).any() and not TC.TABLES["zero"].any()
    for n in (2, 3, 17, 256, 1024):
        s = TC.TABLES[f"n{n}"][:, 3]
        assert s[0] == 0 and s.max() > 1
    assert {TC.BY_NAME[n]["hw"] for n in TC.NAMES} >= {(20, 24), (8, 8), (1, 1)}
    assert all(int(TC.reference(n)["nsteps"].max()) <= 48 for n in TC.NAMES)
    assert TC.reference("ramp_all_miss")["live"] == 0
    for name in TC.FAST_CASES + TC.RAMP_FAST_CASES:          # the FAST comparisons: no ray decides on the early-termination threshold
        assert float(TC.reference(name)["T"].min()) > 0.05, name
    assert any(TC.BY_NAME[n]["shade"] for n in TC.RAMP_FAST_CASES) and not all(TC.BY_NAME[n]["shade"] for n in TC.RAMP_FAST_CASES)


def test_table_builders_match_their_fp64_definition():
    for n in (2, 3, 17, 256, 1024):
        x = np.arange(n, dtype=np.float64) / (n - 1)
        ramp = transfer.tf_ramp(n)
        assert ramp.shape == (n, 4) and ramp.dtype == np.float32
        assert all(np.array_equal(ramp[:, k], x.astype(np.float32)) for k in range(4))
        assert np.array_equal(transfer.tf_preset("gray", n), ramp)
    assert np.array_equal(transfer.tf_ramp(), TC.TABLES["ramp"])
    # control points: held ends, a repeated x (a step), fp64 evaluation rounded once
    pts = [(0.25, 0.1, 0.9, 0.3, -0.5), (0.5, 0.7, 0.2, 0.3, 2.0), (0.5, 0.2, 0.2, 0.8, 0.0), (0.875, 1.0, 0.0, 0.1, 3.0)]
    for n in (2, 17, 256):
        got = transfer.tf_from_points(pts, n)
        assert got.shape == (n, 4) and got.dtype == np.float32
        want = np.empty((n, 4), np.float64)
        for i in range(n):
            x = i / (n - 1)
            if x <= 0.25:
                row = pts[0][1:]
            elif x >= 0.875:
                row = pts[3][1:]
            else:
                a, b = (pts[0], pts[1]) if x < 0.5 else (pts[2], pts[3])
                w = (x - a[0]) / (b[0] - a[0])
                row = [a[k] + w * (b[k] - a[k]) for k in range(1, 5)]
            want[i] = row
        assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -24 * 3.0       # half an ulp of the largest value (3.0 < 4)
    hot = transfer.tf_preset("hot")
    assert hot.shape == (256, 4)
    x = np.arange(256, dtype=np.float64) / 255
    want = np.stack([np.clip(3 * x, 0, 1), np.clip(3 * x - 1, 0, 1), np.clip(3 * x - 2, 0, 1), x], axis=1)
    assert np.abs(hot.astype(np.float64) - want).max() <= 1e-7
    assert np.array_equal(hot[0], [0, 0, 0, 0]) and np.array_equal(hot[-1], [1, 1, 1, 1])
    for bad in (lambda: transfer.tf_ramp(1), lambda: transfer.tf_ramp(1025), lambda: transfer.tf_preset("viridis"),
                lambda: transfer.tf_from_points([(0.5, 0, 0, 0, 0), (0.25, 1, 1, 1, 1)]), lambda: transfer.tf_from_points([(0.0, 0, 0, 0)])):
        with pytest.raises(ValueError):
            bad()


def test_symbol_is_declared_listed_and_exported():
    header = (ROOT / "include" / "mrirt.h").read_text()
    assert re.search(r"\bint\s+mrirt_render_brats_tf\s*\(", header)
    assert "mrirt_render_brats_tf" in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), "mrirt_render_brats_tf")
    assert "brats_tf.hip" in _lib.HIP_SOURCES and (_lib.CSRC / "brats_tf.h").exists()
    assert _lib.lib().mrirt_abi_version() == 4                       # functions are only added


def test_pipelined_table_kernels_keep_gathers_untouched_until_their_wait():
    """The pipelined table kernels issue their gathers as inline asm, like brats_march_pipe_kernel; the build gate's in-flight
    scan goes by that kernel's name, so the same scan (tools/check_async_loads.py: check) runs here on brats_tf_pipe_kernel:
    nothing reads or writes a gather's destination between the gather and the wait that retires it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_async_loads", ROOT / "tools" / "check_async_loads.py")
    gate = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gate)
    text = gate.device_disassembly(_lib.SO_PATH)
    funcs, cur = {}, None
    for no, line in enumerate(text.splitlines()):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur is not None:
            funcs[cur].append((no, line))
    names = sorted(n for n in funcs if "brats_tf_pipe_kernel" in n and not n.startswith("__"))
    assert len(names) == 6, names                     # {STRICT, FAST} x {MOD4, MOD4 + label cells, VGA shaded}
    for name in names:
        lines = funcs[name]
        loads = sum(1 for _, t in lines if gate.LOAD.match(t.split("//")[0].strip()))
        cells = "ELi6ELb1E" in name
        assert loads >= 2 * (9 if cells else 8), (name, loads)          # one static issue site per stage (+ the table's fill)
        waits = [t for _, t in lines if re.search(r"s_waitcnt vmcnt\((8|9)\)", t)]
        assert len(waits) == 2, (name, waits)                            # one counted wait per stage
        assert gate.check(name, lines) == [], name
        assert gate.hazard_scan(name, lines) == [], name


def _call(tf=0x10000, entries=17, variant=0, p="default", ext_kw=None, out=0x20000):
    """mrirt_render_brats_tf with placeholder addresses: only calls that are refused before anything is launched."""
    c = TC.BY_NAME["n17_four_dense_overlays"]
    P = params.brats_params(c["params"]) if p == "default" else p
    E = params.render_ext(dict(c["ext"], kernelVariant=variant, **(ext_kw or {})))
    fake = C.c_void_p(0x1000)
    vp = (C.c_void_p * 4)(fake, fake, fake, fake)
    return int(_lib.lib().mrirt_render_brats_tf(C.byref(P) if P is not None else None, C.byref(E), vp, fake, fake, C.c_void_p(tf), entries,
                                                C.c_void_p(out), 24, None, None))


def test_refusals_launch_nothing():
    assert _call(tf=None) == ERR_NULL
    for n in (0, 1, 1025, 4096, 0xFFFFFFFF):
        assert _call(entries=n) == ERR_ARG, n
    for off in (4, 8, 12, 1):
        assert _call(tf=0x10000 + off) == ERR_ARG, off
    for bit in [0] + list(range(3, 32)):
        assert _call(variant=1 << bit) == ERR_ARG, bit
    assert _call(variant=2 | 4 | 64) == ERR_ARG
    # ... and the checks it shares with mrirt_render_brats_ex through prepare()
    assert _call(p=None) == ERR_NULL
    assert _call(ext_kw=dict(layout="quad", shadeMode=1)) == ERR_LAYOUT
    assert _call(ext_kw=dict(layout="mod4", shadeMode=1)) == ERR_LAYOUT
    assert _call(ext_kw=dict(layout="vg", labelLayout="labcell")) == ERR_LAYOUT
    assert _call(out=None) == ERR_NULL
    bad = params.brats_params(dict(TC.BY_NAME["n17_four_dense_overlays"]["params"], stepSize=0.0))
    assert _call(p=bad) == ERR_ARG
    # a rank that owns no tile: nothing to launch, nothing to refuse (24 x 20 at tile 16 has 4 tiles)
    assert _call(ext_kw=dict(tileSize=16, tileRank=5, tileWorld=7), out=None) == OK


def test_comparison_reports_one_ulp_in_one_table_entry():
    """The helper the GPU tests compare with sees a reference whose table differs by one ulp in one entry."""
    name = "n17_four_dense_overlays"
    c, d = TC.BY_NAME[name], TC.data(name)
    good = TC.reference(name)
    assert tf_ref.compare(good["frame"].copy(), good["live"], good["shaded"], good) == []
    table = TC.TABLES["n17"].copy()
    table[9, 1] = np.nextafter(table[9, 1], np.float32(2.0))
    other = tf_ref.march(c["params"], d["vols"], d["labels"], d["preds"], c["ext"], table)
    msgs = tf_ref.compare(good["frame"], good["live"], good["shaded"], other)
    assert len(msgs) == 1 and msgs[0].startswith("frame differs"), msgs
    assert tf_ref.compare(good["frame"], good["live"] + 1, good["shaded"], good) == [f"live samples {good['live'] + 1} != {good['live']}"]
    assert tf_ref.compare(good["frame"], good["live"], good["shaded"] - 1, good)[0].startswith("shaded samples")


def test_fp32_reference_error():
    """The yardstick of the FAST tolerance: tf_ref in float32 against the same loop in float64 on the FAST cases."""
    worst = 0.0
    for name in TC.FAST_CASES:
        c, d = TC.BY_NAME[name], TC.data(name)
        assert c["params"]["intensityAlpha"] < 1.0 and not c["dense"]
        r64 = tf_ref.march(c["params"], d["vols"], d["labels"], d["preds"], c["ext"], TC.TABLES[c["table"]], dtype=np.float64)
        r32 = TC.reference(name)
        assert r64["live"] == r32["live"] and r64["shaded"] == r32["shaded"]          # the same samples
        dev = float(np.abs(r32["frame"].astype(np.float64) - r64["frame"]).max())
        print(f"{name}: max |fp32 - fp64| = {dev:.3e}")
        worst = max(worst, dev)
    print(f"FP32_REF_ERROR measured {worst:.3e}; tf_cases.py records {TC.FP32_REF_ERROR:.3e}; FAST tolerance {TC.TOL_FAST:.3e}")
    assert worst <= TC.FP32_REF_ERROR <= 1.25 * worst
    assert TC.TOL_FAST == min(8.0 * TC.FP32_REF_ERROR, 1e-4)
