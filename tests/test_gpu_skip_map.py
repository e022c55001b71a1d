"""The per-launch "contributes nothing" mask of exact empty-space skipping (csrc/brats_skip.hip) against its fp32 formula
and against an fp64 brute force that never forms a bound (tests/grid_ref.py) — and frames built so that a wrong mask or a
wrong macro-cell bound changes them: spikes ON the macro-cell boundaries, where only the overlap plane 8m + 8 of a cell's
range keeps the neighbouring cell alive.  The mask is read through the inspection hook ``render._last_skip_mask``."""
import numpy as np
import pytest

import grid_cases as gc
import grid_ref as gr

pytestmark = pytest.mark.gpu

F = np.float32
ORACLE_KEYS = ("cameraMode", "orthoHalfHeight", "shadeMode", "ka", "kd", "ks", "specPow2", "gradEps", "ertThreshold")


def _scene(dims, channels, weights, wl, ww, image=32, show_seg=False, show_pred=False):
    from mrirt import synth
    p = synth.brats_scene(0, image, 64, dims=dims, channels=channels, intensity_alpha=6.0, show_seg=show_seg, show_pred=show_pred)
    p["volWeight"] = tuple(F(w) for w in weights)
    p["wl"], p["ww"] = F(wl), F(ww)
    return p


def _render_and_read_mask(p, grids, ext, labels=None, preds=None, stats=False):
    """One skip=True frame; returns (frame or (frame, stats), the mask as booleans, True = empty).  A configuration that does
    not march with a map fails here instead of passing vacuously."""
    import mrirt
    from mrirt import render
    assert render.kernel_family(p, ext, skip=True)["skipping"], "this configuration does not march with a map"
    render._SKIP_MAPS.clear()
    render._last_skip_mask = None
    out = mrirt.render_brats(p, grids, labels=labels, preds=preds, ext=ext, stats=stats, skip=True)
    assert render._last_skip_mask is not None, "the launch built no map"
    dims = tuple(int(v) for v in p["dims"])
    cells = int(np.prod(gr.macro_dims(dims)))
    return out, gr.unpack_mask(render._last_skip_mask.cpu().numpy(), cells)


def _reference_masks(vols, p, dims, seg=None, pred=None):
    en, w = [int(v) for v in p["volEnabled"]], [F(v) for v in p["volWeight"]]
    ch = [m for m in range(4) if en[m]]
    ubs = [gr.macro_max_ref(vols[m], dims) for m in ch]
    ws = [w[m] for m in ch]
    tf_lo, wsum = gr.window_floor(p["wl"], p["ww"]), gr.weight_sum(en, w)
    seg = seg if int(p["showSeg"]) else None
    pred = pred if int(p["showPred"]) else None
    empty = gr.skip_mask_ref(ubs, ws, wsum, tf_lo, None if seg is None else gr.macro_labels_ref(seg, dims),
                             None if pred is None else gr.macro_labels_ref(pred, dims))
    return empty, gr.needed_ref([vols[m] for m in ch], ws, dims, tf_lo, seg, pred), gr.skip_value_ref(ubs, ws, wsum), tf_lo


@pytest.mark.parametrize("weights", sorted(gc.WEIGHTS))
@pytest.mark.parametrize("channels", [1, 2, 4])
def test_strict_mask_is_the_fp32_formula(channels, weights):
    """(65,41,17): 162 macro cells, so the last ballot is ragged.  Random fields, the window put at the median of the cells'
    values so that about half are empty; seg / pred shown or not, with a label blob in otherwise empty air."""
    import mrirt
    dims = gc.SKIP_DIMS
    vols = gc.textured_volumes(dims, channels, seed=10 + channels)
    w = gc.WEIGHTS[weights]
    seg, pred = gc.air_labels(dims, 2), gc.air_labels(dims, 3, at=(2, 30, 60))
    grids = [mrirt.upload_grid(v, dims, "quad") for v in vols]
    gseg, gpred = mrirt.upload_grid(seg, dims, "linear"), mrirt.upload_grid(pred, dims, "linear")
    # the window: floor halfway between the two middle cell values of this configuration
    probe = _scene(dims, channels, w, 0.5, 0.5)
    v = np.sort(_reference_masks(vols, probe, dims)[2])
    ww = F(0.5)
    wl = F(0.5 * (float(v[v.size // 2 - 1]) + float(v[v.size // 2])) + 0.25)
    seen = set()
    for show_seg, show_pred in ((0, 0), (1, 0), (0, 1), (1, 1)):
        p = _scene(dims, channels, w, wl, ww, show_seg=bool(show_seg), show_pred=bool(show_pred))
        want, needed, val, tf_lo = _reference_masks(vols, p, dims, seg, pred)
        assert np.all(val != tf_lo), "a cell value tied with the window floor"
        assert 0.3 < want.mean() < 0.7
        _, got = _render_and_read_mask(p, grids, dict(layout="quad", math="strict"), labels=gseg if show_seg else None,
                                       preds=gpred if show_pred else None)
        assert np.array_equal(got, want), (show_seg, show_pred, np.flatnonzero(got != want))
        assert not (got & needed).any()                  # soundness: empty => not needed
        seen.add(want.tobytes())
    assert len(seen) == 4, "the label blobs must change the mask: they float in cells that are empty without them"


@pytest.mark.parametrize("weights", sorted(gc.WEIGHTS))
@pytest.mark.parametrize("channels", [1, 2, 4])
def test_fast_mask_equals_strict_mask_equals_brute_force_on_gap_volumes(channels, weights):
    """Voxels 0 or in [0.3, 0.9], window floor 0.1: no cell value lies within 0.1 of the floor, so FAST's fused multiply-adds
    and reciprocal cannot move a cell across it: FAST mask == STRICT mask == not needed."""
    import mrirt
    dims = gc.SKIP_DIMS
    vols = gc.gap_volumes(dims, channels, seed=channels)
    seg = gc.air_labels(dims)
    grids = [mrirt.upload_grid(v, dims, "quad") for v in vols]
    gseg = mrirt.upload_grid(seg, dims, "linear")
    for show_seg in (False, True):
        p = _scene(dims, channels, gc.WEIGHTS[weights], gc.GAP_WL, gc.GAP_WW, show_seg=show_seg)
        want, needed, val, tf_lo = _reference_masks(vols, p, dims, seg)
        assert np.all((val == 0) | (val.astype(np.float64) - float(tf_lo) >= 0.1))
        assert np.array_equal(want, ~needed) and 0.2 < want.mean() < 0.9
        masks = {}
        for math in ("strict", "fast"):
            _, masks[math] = _render_and_read_mask(p, grids, dict(layout="quad", math=math), labels=gseg if show_seg else None)
        assert np.array_equal(masks["strict"], want)
        assert np.array_equal(masks["fast"], masks["strict"])
        assert np.array_equal(masks["fast"], ~needed)


def _cameras(dims):
    """One orthographic view along each axis (from outside the box) and one perspective view from inside it."""
    from mrirt import synth
    e = np.eye(3, dtype=F)
    views = []
    for axis in range(3):
        u, v = e[(axis + 1) % 3], e[(axis + 2) % 3]
        views.append((f"ortho{'xyz'[axis]}", dict(eye=(3 * e[axis]).astype(F), U=u, V=v, W=(-e[axis]).astype(F)),
                      dict(cameraMode=1, orthoHalfHeight=1.0)))
    eye, U, V, W = synth.bench_camera(radius=0.2).get_basis()
    views.append(("inside", dict(eye=eye, U=U, V=V, W=W), {}))
    return views


def _spike_scene(dims, cam, show_seg=False):
    p = _scene(dims, 1, gc.WEIGHTS["equal"], gc.GAP_WL, gc.GAP_WW, image=64, show_seg=show_seg)
    p.update(cam)
    p["stepSize"] = 0.03                                 # a voxel is 1.8 / 33 = 0.0545 wide
    assert p["stepSize"] < float(np.min(p["voxelSize"]))
    return p


@pytest.mark.parametrize("layout,shade", [("vg", True), ("vga", True), ("quad", False), ("mod4", False)])
def test_spikes_on_macro_cell_boundaries_survive_skipping(layout, shade):
    """Zeros plus unit spikes at coordinates from {0, 7, 8, 9, D - 1}: the only non-empty voxel near a ray lies ON a macro-cell
    boundary, and a sample with base 8m + 7 lands next to it.  The skipped frame and counters are the plain ones, the plain
    frame is the oracle's, and the mask keeps exactly the cells whose inclusive range holds a spike."""
    import torch
    import mrirt
    from mrirt import synth
    from oracle import oracle_c
    dims = gc.SPIKE_DIMS
    vol = gc.frame_spike_volume(dims)
    grid = mrirt.upload_mod4([vol, None, None, None], dims) if layout == "mod4" else mrirt.upload_grid(vol, dims, layout)
    need = gc.frame_spike_cells(dims)
    assert need.sum() == 8 + 8 + 2 + 4 + 2 - 1           # (0,0,0)'s cell and one of (7,16,16)'s four are among (8,8,8)'s eight
    for name, cam, cam_ext in _cameras(dims):
        p = _spike_scene(dims, cam)
        base = dict(synth.SHADE_EXT, **cam_ext) if shade else dict(cam_ext)
        ref, aux = oracle_c.brats_main(p, [vol], None, None, {k: v for k, v in base.items() if k in ORACLE_KEYS}, return_aux=True)
        for math in ("strict", "fast"):
            ext = dict(base, layout=layout, math=math)
            plain, st0 = mrirt.render_brats(p, [grid], ext=ext, stats=True)
            (skipped, st1), empty = _render_and_read_mask(p, [grid], ext, stats=True)
            assert torch.equal(plain, skipped), (name, math)
            assert st0 == st1 and st0["live_samples"] > 0, (name, math)
            assert np.array_equal(~empty, need), (name, math)
            if math == "strict":
                assert np.array_equal(plain.cpu().numpy(), ref), name
                assert st0["live_samples"] == aux["live_samples"], name
                assert (ref[..., :3] != 0).any(), "no ray saw a spike: the view is not doing its job"


@pytest.mark.parametrize("layout,shade", [("vg", True), ("vga", True), ("quad", False), ("mod4", False)])
def test_label_spikes_on_macro_cell_boundaries_survive_skipping(layout, shade):
    """The same frames with the spikes as the only non-zero labels of a shown overlay, on zero intensities: only the label
    summary keeps those cells alive."""
    import torch
    import mrirt
    from mrirt import synth
    from oracle import oracle_c
    dims = gc.SPIKE_DIMS
    vol = np.zeros(gc.nvox(dims), F)
    lab = gc.frame_spike_volume(dims, np.uint32, 3)
    grid = mrirt.upload_mod4([vol, None, None, None], dims) if layout == "mod4" else mrirt.upload_grid(vol, dims, layout)
    glab = mrirt.upload_grid(lab, dims, "linear")
    need = gc.frame_spike_cells(dims)
    for name, cam, cam_ext in _cameras(dims):
        p = _spike_scene(dims, cam, show_seg=True)
        base = dict(synth.SHADE_EXT, **cam_ext) if shade else dict(cam_ext)
        ref, aux = oracle_c.brats_main(p, [vol], lab, None, {k: v for k, v in base.items() if k in ORACLE_KEYS}, return_aux=True)
        assert (ref[..., :3] != 0).any(), "no ray saw a label spike: the view is not doing its job"
        for math in ("strict", "fast"):
            ext = dict(base, layout=layout, math=math)
            plain, st0 = mrirt.render_brats(p, [grid], labels=glab, ext=ext, stats=True)
            (skipped, st1), empty = _render_and_read_mask(p, [grid], ext, labels=glab, stats=True)
            assert torch.equal(plain, skipped), (name, math)
            assert st0 == st1 and st0["live_samples"] > 0, (name, math)
            assert np.array_equal(~empty, need), (name, math)
            off = mrirt.render_brats(dict(p, showSeg=0), [grid], ext=ext)
            assert not torch.equal(off, plain), (name, math)
            if math == "strict":
                assert np.array_equal(plain.cpu().numpy(), ref), name
                assert st0["live_samples"] == aux["live_samples"], name
