"""Hausdorff distance and the exact distance transform on the GPU (csrc/edt.hip).  The contract is bit-identical to the
reference's hausdorff_distance (inr/inr/model.py:164-195; tests/golden/inr_hausdorff.npz holds what it returned): every
comparison below is ``==`` (NaN matching NaN) or ``array_equal``, never a tolerance."""
import ctypes as C

import numpy as np
import pytest

import hausdorff_cases as hc
import hausdorff_ref as href

pytestmark = pytest.mark.gpu

CASES = hc.load_cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def env():
    import torch
    import mrirt
    from mrirt import torch_ops
    assert torch.cuda.is_available()
    return dict(torch=torch, mrirt=mrirt, inr=mrirt.inr, native=torch_ops.load_native())


def _assert_same(name, got, want, nc, how):
    print(name, how, [float(got[c]) for c in range(nc)], [float(w) for w in want])
    for c in range(nc):
        assert hc.same(got[c], want[c]), f"{name} via {how}, class {c}: got {float(got[c])!r}, reference {float(want[c])!r}"


def _from_directed(d, nc):
    d = d.cpu().numpy()
    assert d.shape == (nc, 2) and d.dtype == np.float64
    return [float(np.sqrt(np.float64(max(d[c, 0], d[c, 1])))) if d[c, 0] == d[c, 0] and d[c, 1] == d[c, 1] else float("nan")
            for c in range(nc)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hausdorff_distance_numpy_and_tensor_input(env, case):
    torch, inr = env["torch"], env["inr"]
    name, pred, true, sp, nc, want = case
    got = inr.hausdorff_distance(pred, true, spacing=sp, num_classes=nc)
    assert sorted(got) == list(range(nc)) and all(type(v) is float for v in got.values())
    _assert_same(name, got, want, nc, "numpy int16")
    _assert_same(name, inr.hausdorff_distance(pred.astype(np.int64), true.astype(np.int32), sp, nc), want, nc, "numpy int64 / int32")
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(true).cuda()
    _assert_same(name, inr.hausdorff_distance(p, t, sp, nc), want, nc, "device int16")
    _assert_same(name, inr.hausdorff_distance(p.to(torch.int64), t.to(torch.int32), sp, nc), want, nc, "device int64 / int32")
    _assert_same(name, inr.hausdorff_distance(p, true, sp, nc), want, nc, "device + numpy")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hausdorff_raw_abi_and_torch_operators(env, case):
    torch, mrirt = env["torch"], env["mrirt"]
    name, pred, true, sp, nc, want = case
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(true).cuda()
    lib = mrirt._lib.lib()
    hwd, spc = (C.c_uint32 * 3)(*pred.shape), (C.c_float * 3)(*sp)
    nbytes = int(lib.mrirt_edt_scratch_bytes(hwd, nc))
    assert nbytes >= 16 * pred.size
    # the scratch is exactly as long as the ABI asks for, between two guard blocks that must come back untouched
    guard = 4096
    buf = torch.full((guard + nbytes + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((nc + 1, 2), -7.0, dtype=torch.float64, device="cuda")
    rc = lib.mrirt_hausdorff(C.c_void_p(p.data_ptr()), C.c_void_p(t.data_ptr()), hwd, spc, nc, C.c_void_p(out.data_ptr()),
                             C.c_void_p(buf.data_ptr() + guard), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 0x5A).all()) and bool((buf[guard + nbytes:] == 0x5A).all()), "scratch guard overwritten"
    assert bool((out[nc] == -7.0).all()), "directed_sq written past 2 * num_classes"
    _assert_same(name, _from_directed(out[:nc], nc), want, nc, "mrirt_hausdorff")
    _assert_same(name, _from_directed(torch.ops.mrirt.hausdorff(p, t, list(sp), nc), nc), want, nc, "torch.ops.mrirt.hausdorff")
    _assert_same(name, _from_directed(env["native"].hausdorff(p, t, list(sp), nc), nc), want, nc, "torch.ops.mrirt_native.hausdorff")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_distance_transform_field_equals_the_restatement(env, case):
    torch, inr = env["torch"], env["inr"]
    name, pred, true, sp, nc, _ = case
    p = torch.from_numpy(pred).cuda()
    classes = range(nc + 1) if pred.size <= 70000 else (1, 3)          # nc itself: absent or out of range -> +inf or not
    for c in classes:
        want = href.edt_squared(pred == c, sp)
        got = inr.distance_transform(pred, cls=c, spacing=sp)
        assert got.dtype == torch.float64 and tuple(got.shape) == pred.shape and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), f"{name} class {c}: field differs from the restatement"
        assert np.array_equal(torch.ops.mrirt.edt_squared(p, c, list(sp)).cpu().numpy(), want), f"{name} class {c}: torch.ops.mrirt.edt_squared"
        assert np.array_equal(env["native"].edt_squared(p, c, list(sp)).cpu().numpy(), want), f"{name} class {c}: mrirt_native.edt_squared"
    # a mask instead of labels (bool NumPy, and a device tensor of non-zero values)
    want = href.edt_squared(true > 1, sp)
    assert np.array_equal(inr.distance_transform(true > 1, spacing=sp).cpu().numpy(), want)
    assert np.array_equal(inr.distance_transform(torch.from_numpy((true > 1) * 9).cuda(), spacing=sp).cpu().numpy(), want)


def test_empty_mask_is_all_inf_and_wide_labels_do_not_wrap(env):
    torch, inr = env["torch"], env["inr"]
    lab = np.zeros((5, 6, 7), np.int32)
    assert bool(torch.isinf(inr.distance_transform(lab, cls=2)).all())
    lab[1, 2, 3] = 65536 + 2                                           # int16 would read it as class 2
    assert bool(torch.isinf(inr.distance_transform(lab, cls=2)).all())
    got = inr.hausdorff_distance(lab, lab, num_classes=4)
    assert got[0] == 0.0 and all(np.isnan(got[c]) for c in (1, 2, 3))


@pytest.mark.parametrize("shape,sp", [((4096, 1, 2), (0.7, 1.0, 1.0)), ((3, 4096, 1), (1.0, 0.9375, 1.0)), ((2, 2, 4096), (1.0, 1.0, 1.3)),
                                      ((5, 700, 3), (1.0, 1.1, 1.0))])
def test_longest_supported_line(env, shape, sp):
    """4096 voxels along each axis in turn (one line per tile), and a length that takes 8-line tiles."""
    torch, inr = env["torch"], env["inr"]
    rng = np.random.default_rng(shape[1])
    a, b = (np.where(rng.random(shape) < 0.98, 0, rng.integers(1, 3, shape)).astype(np.int16) for _ in range(2))
    want = href.hausdorff(a, b, sp, 3)
    _assert_same(f"line{shape}", inr.hausdorff_distance(a, b, sp, 3), want, 3, "hausdorff_distance")
    assert np.array_equal(inr.distance_transform(a, cls=1, spacing=sp).cpu().numpy(), href.edt_squared(a == 1, sp))


def test_large_case_equals_the_recorded_reference_values(env):
    torch, inr = env["torch"], env["inr"]
    shape, sp, nc, crc_p, crc_t, want = hc.load_large()
    pred, true = hc.large_pair(shape)
    assert (hc.crc(pred), hc.crc(true)) == (crc_p, crc_t), "the synthetic volumes differ on this platform"
    got = inr.hausdorff_distance(torch.from_numpy(pred).cuda(), torch.from_numpy(true).cuda(), spacing=sp, num_classes=nc)
    _assert_same(f"large{shape}", got, want, nc, "hausdorff_distance")


def test_non_default_stream_gives_the_same_result(env):
    torch, inr = env["torch"], env["inr"]
    name, pred, true, sp, nc, want = next(c for c in CASES if c[0] == "medium_blob")
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(true).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = inr.hausdorff_directed_sq(p, t, sp, nc)
        f = inr.distance_transform(p, cls=2, spacing=sp)
        got = inr.hausdorff_distance(p, t, sp, nc)
    s.synchronize()
    _assert_same(name, got, want, nc, "side stream")
    _assert_same(name, _from_directed(d, nc), want, nc, "side stream, device result")
    assert np.array_equal(f.cpu().numpy(), inr.distance_transform(p, cls=2, spacing=sp).cpu().numpy())


def test_evaluate_single_case_is_the_composition_of_its_parts(env, golden_dir):
    torch, inr = env["torch"], env["inr"]
    g = np.load(golden_dir / "inr_fourier.npz")
    K = int(g["k4h64_K"])
    params = [{"W": g[f"k4h64_W{i}"], "b": g[f"k4h64_b{i}"]} for i in range(5)]
    rng = np.random.default_rng(5)
    mods = rng.standard_normal((4, 22, 20, 18)).astype(np.float32)
    seg = hc.blob_labels((22, 20, 18), 3).astype(np.int16)
    case = {"mods": mods, "seg": seg}
    res = inr.evaluate_single_case(7, case, params, 4, K)
    assert list(res) == ["case_idx", "pred_vol", "true_vol", "case_data", "class_scores", "coverage_dice", "mean_dice", "hausdorff_scores"]
    pred, true = inr.predict_volume(params, case, K)
    assert res["case_idx"] == 7 and res["case_data"] is case and res["true_vol"] is seg
    assert torch.equal(res["pred_vol"], pred) and tuple(res["pred_vol"].shape) == seg.shape
    dice = inr.dice_score(pred, true, 4)
    hd = inr.hausdorff_distance(pred, true, num_classes=4)
    assert sorted(res["class_scores"]) == sorted(res["hausdorff_scores"]) == [0, 1, 2, 3]
    for c in range(4):
        assert hc.same(res["class_scores"][c], dice[c]) and hc.same(res["hausdorff_scores"][c], hd[c])
    assert res["coverage_dice"] == inr.coverage_dice(pred, true)
    valid = [v for v in dice.values() if not np.isnan(v)]
    assert type(res["mean_dice"]) is float and res["mean_dice"] == (float(np.mean(valid)) if valid else 0.0)
    # and the Hausdorff part is the definition's value on that very prediction
    ref = href.hausdorff(pred.cpu().numpy(), seg, (1.0, 1.0, 1.0), 4)
    for c in range(4):
        assert hc.same(res["hausdorff_scores"][c], ref[c])
