"""Case preparation on the GPU where the library uses it: inr.prepare_case feeding VoxelCache,
inr.predict_volume(prefilter_sigma=...) and the viewer's prep="device", each against the same path fed by the NumPy
restatements of tests/prep_ref.py (or by the host preparation).  Every comparison is equality."""
import numpy as np
import pytest

import prep_ref as pr

pytestmark = pytest.mark.gpu

DIMS = (30, 26, 20)
MODS = ("T1n", "T1c", "T2w", "FLAIR")


@pytest.fixture(scope="module")
def case():
    """A BraTS-shaped synthetic case: integer-valued intensities with a zero background, labels 0, 1, 2 and 4."""
    rng = np.random.default_rng(8)
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, n) for n in DIMS], indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    mods = []
    for i in range(4):
        v = np.clip(1.2 - r, 0, None) * (800 + 100 * i) * (1 + 0.2 * np.sin((4 + i) * x)) + rng.random(DIMS) * 40
        v[r > 1.1] = 0.0
        mods.append(v.astype(np.int16).astype(np.float32))
    seg = np.zeros(DIMS, np.uint8)
    seg[r < 0.5], seg[r < 0.35], seg[r < 0.2] = 2, 1, 4
    mods = np.stack(mods)
    mods.setflags(write=False)
    return mods, seg


def _restated_zscore(mods):
    return np.stack([pr.zscore_apply(m, *pr.zscore_stats(m)) for m in mods])


def _params(rng, K, M, hidden=32, layers=3):
    sizes = [3 + 6 * K + M] + [hidden] * (layers - 1) + [4]
    return [{"W": (rng.uniform(-1, 1, (sizes[i], sizes[i + 1])) * np.sqrt(6 / (sizes[i] + sizes[i + 1]))).astype(np.float32),
             "b": rng.uniform(-0.3, 0.3, sizes[i + 1]).astype(np.float32)} for i in range(layers)]


def test_prepare_case_feeds_the_voxel_cache_like_the_restated_case(case):
    import torch
    from mrirt import inr, volume
    mods, seg = case
    got = inr.prepare_case(mods, seg)
    assert got["mods"].is_cuda and tuple(got["mods"].shape) == mods.shape and got["mods"].dtype == torch.float32
    assert got["seg"].is_cuda and got["seg"].dtype == torch.int16 and tuple(got["zstats"].shape) == (4, 4)
    want_seg = np.where(seg == 4, 3, seg).astype(np.int16)
    assert np.array_equal(got["seg"].cpu().numpy(), want_seg) and 3 in want_seg and 4 not in want_seg
    want_mods = _restated_zscore(mods)
    zmu, zsig, cnt = volume.zscore_constants(got["zstats"])
    for m in range(4):
        mu, sg, count = pr.zscore_stats(mods[m])
        assert (zmu[m], zsig[m], cnt[m]) == (mu, np.float32(sg + np.float32(1e-6)), count)
    assert np.array_equal(got["mods"].cpu().numpy(), want_mods)
    a = inr.VoxelCache([got]).sample(seed=5, batch_index=3, n=4099)
    b = inr.VoxelCache([{"mods": want_mods, "seg": want_seg}]).sample(seed=5, batch_index=3, n=4099)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # labels kept as they are on request; no segmentation at all; a device tensor in
    assert np.array_equal(inr.prepare_case(mods, seg, remap_label4=False)["seg"].cpu().numpy(), seg.astype(np.int16))
    again = inr.prepare_case(torch.from_numpy(mods.copy()).cuda())
    assert again["seg"] is None and torch.equal(again["mods"], got["mods"]) and torch.equal(again["zstats"], got["zstats"])


@pytest.mark.parametrize("sigma", [0.5, 1.0])
def test_predict_volume_prefilter_equals_predicting_the_prefiltered_case(case, sigma):
    import torch
    from mrirt import inr
    mods, _ = case
    z = _restated_zscore(mods)
    K = 4
    params = _params(np.random.default_rng(3), K, 4)
    filtered = np.stack([pr.gaussian_filter(z[m], sigma) for m in range(4)])
    want, _ = inr.predict_volume(params, {"mods": filtered, "seg": None}, K)
    got, seg = inr.predict_volume(params, {"mods": z, "seg": None}, K, prefilter_sigma=sigma)
    plain, _ = inr.predict_volume(params, {"mods": z, "seg": None}, K)
    assert seg is None and got.dtype == torch.int16 and tuple(got.shape) == DIMS
    assert torch.equal(got, want)
    assert not torch.equal(got, plain), "the filter must matter on this case, or the comparison shows nothing"
    assert torch.equal(plain, inr.predict_volume(params, {"mods": z, "seg": None}, K, prefilter_sigma=None)[0])


def test_viewer_with_device_preparation_renders_the_host_frame(case):
    import torch
    from mrirt.viewer import BraTSViewer
    mods, seg = case
    arrays = {k: mods[i] for i, k in enumerate(MODS)}
    frames = {}
    for prep in ("host", "device"):
        v = BraTSViewer(up="Z")
        v.load_arrays(arrays, (1.0, 1.0, 1.0), seg.astype(np.float32), prep=prep)
        assert tuple(v.vol_dims) == DIMS and v.seg_buffer is not None
        is_dev = [isinstance(v.raw_volumes[k], torch.Tensor) and v.raw_volumes[k].is_cuda for k in MODS]
        assert all(is_dev) if prep == "device" else not any(is_dev)
        v.camera.orbit(0.4, -0.3)
        v.step_size = 0.02
        frames[prep] = v.render(96, 64).to_numpy().copy()
        if prep == "device":
            host = BraTSViewer(up="Z")
            host.load_arrays(arrays, (1.0, 1.0, 1.0), seg.astype(np.float32))
            for k in MODS:
                assert np.array_equal(v.raw_volumes[k].cpu().numpy(), host.raw_volumes[k])
                assert np.array_equal(v.buffers[k].to_numpy(), host.buffers[k].to_numpy())
    assert frames["host"][..., :3].max() > 0.05, "the case must actually be visible"
    assert np.array_equal(frames["host"], frames["device"])
    with pytest.raises(ValueError):
        BraTSViewer(up="Z").load_arrays(arrays, prep="gpu")


def test_viewer_inr_prepass_from_device_volumes(case, tmp_path):
    """load_inr after prep="device" z-scores on the device: the prediction is predict_volume's on zscore_nonzero_device of the
    viewer's own normalised volumes (which the other tests hold to the restatement)."""
    import json
    import torch
    from mrirt import inr, volume
    from mrirt.viewer import BraTSViewer
    mods, seg = case
    K = 4
    params = _params(np.random.default_rng(3), K, 4, hidden=64, layers=5)
    flat = {}
    for i, p in enumerate(params):
        flat[f"W_{i}"], flat[f"b_{i}"] = p["W"], p["b"]
    np.savez(tmp_path / "inr.npz", **flat)
    (tmp_path / "inr_info.json").write_text(json.dumps({"config": {"FOURIER_FREQS": K}}))
    v = BraTSViewer(up="Y")
    v.load_arrays({k: mods[i] for i, k in enumerate(MODS)}, prep="device")
    v.load_inr(tmp_path / "inr.npz")
    assert v.show_pred and v.pred_buffer is not None
    z, _ = volume.zscore_nonzero_device(torch.stack([v.raw_volumes[k] for k in MODS]))
    want, _ = inr.predict_volume(params, {"mods": z, "seg": None}, K)
    assert torch.equal(v.pred_buffer.tensor, inr.labels_for_viewer(want))
