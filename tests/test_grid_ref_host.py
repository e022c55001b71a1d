"""The NumPy layout references of tests/grid_ref.py, pinned without a GPU: the GPU tests compare the builders with them
bit for bit, which proves nothing unless the references themselves are checked: element counts against the library's
host-only size queries, the maps for being one-to-one and self-consistent, values against hand-written expectations, the
macro bound against the oracle's trilinear fetch and the mask against a brute force that never forms a bound.  (The
library exposes no voxel-to-element map to the host: what ties the maps to the library's own formula is the size
comparison here plus the bit-exact comparison of whole buffers in tests/test_gpu_grid_builders.py.)"""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import grid_ref as gr
from mrirt import _lib
from oracle import oracle_np as onp

F = np.float32


def _d(dims):
    return (C.c_uint32 * 3)(*dims)


@pytest.mark.parametrize("dims", gc.BUILDER_DIMS, ids=str)
def test_every_voxel_has_one_element_of_its_own(dims):
    lib = _lib.lib()                                     # host-only calls: nothing is launched
    e, total = gr.vec4_elem(dims)
    assert total == lib.mrirt_vec4_elems(_d(dims))
    assert e.min() >= 0 and e.max() < total and np.unique(e).size == gc.nvox(dims)
    geo = gr.vga_geometry_ref(dims)
    assert sum(g["elems"] for g in geo) == lib.mrirt_vga_elems(_d(dims))
    assert [g["base"] for g in geo] == [0, geo[0]["elems"], geo[0]["elems"] + geo[1]["elems"]]
    for a in range(3):
        ea = gr.vga_elem(dims, a)
        assert ea.min() >= 0 and ea.max() < geo[a]["elems"] and np.unique(ea).size == gc.nvox(dims)
    # the references fill exactly those elements: distinct non-zero voxels in, the same multiset out, zeros elsewhere
    v = gc.distinct_field(dims)
    for buf in (gr.vec4_ref(v, dims, "vg"), gr.vec4_ref(v, dims, "quad"), gr.vec4_ref([v, v, v, v], dims, "mod4")):
        assert np.array_equal(np.sort(buf[:, 0][buf[:, 0] != 0]), np.sort(v))
        assert np.count_nonzero(buf.view(np.uint32).any(axis=1)) == gc.nvox(dims)
    vga = gr.vga_ref(v, dims)
    for a in range(3):
        part = vga[geo[a]["base"]:geo[a]["base"] + geo[a]["elems"], 0]
        assert np.array_equal(np.sort(part[part != 0]), np.sort(v))


@pytest.mark.parametrize("dims", sorted(gc.VGA_PITCHES), ids=str)
def test_the_padded_cases_are_padded(dims):
    geo = gr.vga_geometry_ref(dims)
    assert [(g["rowLines"], g["sliceLines"]) for g in geo] == gc.VGA_PITCHES[dims]
    assert [tuple(g["nb"]) for g in geo] == gc.VGA_BRICKS[dims]
    row_padded = [g["rowLines"] != g["nb"][0] for g in geo]
    slice_padded = [g["sliceLines"] != g["rowLines"] * g["nb"][1] for g in geo]
    want = {(16, 8, 8): ([False] * 3, [False] * 3), (67, 9, 5): ([True, False, False], [True] * 3),
            (13, 70, 3): ([False] * 3, [True] * 3), (261, 5, 4): ([True] * 3, [True] * 3)}[dims]
    assert (row_padded, slice_padded) == want
    for g in geo:                                        # padded pitches sit on their residues modulo 64
        assert g["rowLines"] < 64 or g["rowLines"] % 64 == 8
        assert g["sliceLines"] < 64 or g["sliceLines"] % 64 == 36


@pytest.mark.parametrize("dims", gc.BUILDER_DIMS, ids=str)
def test_vga_map_agrees_with_the_march_s_neighbour_deltas(dims):
    """flat_cell (csrc/mrirt_device.h): the cell origin is sum (i >> sh) mul + (i & mask) inner, and the +1 neighbour of an
    axis is `inner` away inside a brick and `wrap = mul - mask inner` away from a brick's last slot.  Walked in NumPy over
    every cell: the eight corners must land on the elements of the eight neighbour voxels.  The terms come from
    vga_geometry_ref itself, so this checks that the restated map and the restated walk are consistent with each other (a
    wrong `inner`, mask or shift in the reference breaks it; a wrong pitch cannot) — it does not pin them to the library."""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    for a, g in enumerate(gr.vga_geometry_ref(dims)):
        e = gr.vga_elem(dims, a)
        wrap = [g["mul"][k] - g["mask"][k] * g["inner"][k] for k in range(3)]
        d = [np.where((i & g["mask"][k]) == g["mask"][k], wrap[k], g["inner"][k]) for k, i in enumerate((x, y, z))]
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    ok = (x + cx < X) & (y + cy < Y) & (z + cz < Z)
                    walked = e + cx * d[0] + cy * d[1] + cz * d[2]
                    there = e[np.minimum(z + cz, Z - 1), np.minimum(y + cy, Y - 1), np.minimum(x + cx, X - 1)]
                    assert np.array_equal(walked[ok], there[ok]), (a, cx, cy, cz)


def test_vec4_ref_values_on_a_hand_checked_volume():
    """(3,2,1): small enough to write the expected float4s down."""
    v = np.array([1, 2, 4, 8, 16, 32], F)               # row y=0: 1 2 4; row y=1: 8 16 32
    vg = gr.vec4_ref(v, (3, 2, 1), "vg")
    quad = gr.vec4_ref(v, (3, 2, 1), "quad")
    assert vg.shape == quad.shape == (16, 4)
    # element = 8 * brick + (x & 1) + 2 (y & 1); bricks x-fastest: voxel (2, 1, 0) is brick 1, slot 2
    assert vg[0].tolist() == [1, 2 - 1, 8 - 1, 0] and vg[1].tolist() == [2, 4 - 1, 16 - 2, 0]
    assert vg[8 + 2].tolist() == [32, 32 - 16, 32 - 4, 0] and vg[3].tolist() == [16, 32 - 8, 16 - 2, 0]
    assert quad[0].tolist() == [1, 8, 2, 16] and quad[8 + 2].tolist() == [32, 32, 32, 32] and quad[8].tolist() == [4, 32, 4, 32]
    for buf in (vg, quad):                               # slots 4..7 (z = 1) and brick 1's x = 3 column are pads: +0.0 bits
        pads = [4, 5, 6, 7, 9, 11, 12, 13, 14, 15]
        assert not buf.view(np.uint32)[pads].any()
    c8 = gr.cell8_ref(np.array([1, 2, 4, 8, 16, 32], np.uint8), (3, 2, 1))
    assert c8[0].tolist() == [1, 2, 8, 16, 1, 2, 8, 16] and c8[5].tolist() == [32] * 8 and c8[2].tolist() == [4, 4, 32, 32, 4, 4, 32, 32]


def _bound_volumes(dims):
    rng = np.random.default_rng(5)
    n = gc.nvox(dims)
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    big = F(3e38)
    yield "random", rng.standard_normal(n).astype(F)
    yield "negative", (-1 - 100 * rng.random(n)).astype(F)
    yield "denormal", (rng.integers(-5000, 5000, n) * np.float64(1.4e-45)).astype(F)
    yield "checker 3e38", np.where((x + y + z) % 2 == 0, big, -big).astype(F).reshape(-1)
    for name, axis in (("x", x), ("y", y), ("z", z)):
        yield f"slabs 3e38 along {name}", np.where(axis % 2 == 0, big, -big).astype(F).reshape(-1)
    # the edges of the overflow rule: extremes +-h with everything else in between, so the inner lerps can leave [-h, h] by
    # ulps.  Range FLT_MAX exactly (finite, but one ulp more is not): bounded by +inf.  Range just under FLT_MAX / 2: the
    # bound stays finite, and so must every fetch
    fmax = np.finfo(F).max
    for name, h in (("range FLT_MAX 3e38", F(0.5) * fmax), ("range just under FLT_MAX / 2", F(0.25) * fmax * F(1 - 2.0 ** -20))):
        v = (rng.uniform(-1, 1, n) * np.float64(h)).astype(F)
        ends = rng.random(n) < 0.5
        v[ends] = np.where(rng.random(int(ends.sum())) < 0.5, h, -h)
        assert F(v.max() - v.min()) == F(2) * h and np.isfinite(F(2) * h)
        yield name, v


@pytest.mark.parametrize("dims", [(9, 9, 9), (17, 8, 3), (21, 13, 10)], ids=str)
def test_macro_bound_is_never_exceeded_by_the_trilinear_fetch(dims):
    """Brute force over samples: the oracle's sampleLinear at a few thousand random points never exceeds the bound of the
    macro cell that holds the sample's base voxel.  The +-3e38 volumes are the ones where `max + 2e-6 max|v|` alone is NOT a
    bound: lerp's b - a overflows and -3e38 + t inf is +inf between two finite voxels (slabs along z: about half of the
    samples), which is why a cell whose value range reaches FLT_MAX / 2 is bounded by +inf."""
    X, Y, Z = dims
    mx, my, _ = gr.macro_dims(dims)
    rng = np.random.default_rng(11)
    q = [rng.uniform(-0.5, d - 0.5, 4000).astype(F) for d in dims]
    for k in range(3):                                   # and points on the lattice planes themselves
        q[k][:400] = np.rint(q[k][:400])
    overflowed = 0
    for name, v in _bound_volumes(dims):
        ub = gr.macro_max_ref(v, dims)
        with np.errstate(invalid="ignore", over="ignore"):
            s, (ix, iy, iz, _, _, _) = onp._sample_linear(v, q[0], q[1], q[2], X, Y, Z)
        cell = ix // 8 + mx * (iy // 8 + my * (iz // 8))
        assert not (s > ub[cell]).any(), name
        overflowed += int(np.isposinf(s).sum())
        if "3e38" not in name:
            assert np.isfinite(ub).all() and np.isfinite(s).all(), name
        if name == "range FLT_MAX 3e38":
            assert np.isposinf(ub[0]) and np.isposinf(ub).mean() >= 0.5, name     # (cells of a voxel or two may hold one end only)
    assert overflowed > 0, "the +-3e38 volumes no longer overflow the lerps: they are not doing their job"


def test_macro_refs_on_spikes_and_a_nan():
    for dims in gc.MACRO_DIMS:
        v, spikes = gc.spike_field(dims)
        want = np.zeros(int(np.prod(gr.macro_dims(dims))), F)
        for x, y, z, h in spikes:                        # ascending heights: the last one a cell sees is its maximum
            want[gc.cells_seeing(x, y, z, dims)] = F(h + F(F(2e-6) * h))
        assert np.array_equal(gr.macro_max_ref(v, dims).view(np.uint32), want.view(np.uint32)), dims
        lab = (v != 0).astype(np.uint32) * 4
        assert np.array_equal(gr.macro_labels_ref(lab, dims) != 0, want != 0)
    # a spike at 8 is seen by cells 0 and 1 of that axis; 7 and 9 by one cell each; the last voxel by every cell that reaches it
    assert gr.axis_cells(8, 17) == [0, 1] and gr.axis_cells(7, 17) == [0] and gr.axis_cells(9, 17) == [1]
    assert gr.axis_cells(16, 17) == [1, 2] and gr.axis_cells(8, 9) == [0, 1] and gr.axis_cells(7, 8) == [0] and gr.axis_cells(0, 1) == [0]
    v = np.zeros(gc.nvox((17, 9, 9)), F)
    v[8 + 17 * (8 + 9 * 3)] = np.nan
    ub = gr.macro_max_ref(v, (17, 9, 9))
    assert np.array_equal(np.isposinf(ub), np.isin(np.arange(ub.size), gc.cells_seeing(8, 8, 3, (17, 9, 9)))) and np.isposinf(ub).sum() == 4
    assert not ub[~np.isposinf(ub)].view(np.uint32).any()


def _masks_of(vols, weights, enabled, dims, wl, ww, seg=None, pred=None):
    ch = [m for m in range(4) if enabled[m]]
    ubs = [gr.macro_max_ref(vols[m], dims) for m in ch]
    w = [weights[m] for m in ch]
    tf_lo = gr.window_floor(wl, ww)
    wsum = gr.weight_sum(enabled, weights)
    seg_any = None if seg is None else gr.macro_labels_ref(seg, dims)
    pred_any = None if pred is None else gr.macro_labels_ref(pred, dims)
    empty = gr.skip_mask_ref(ubs, w, wsum, tf_lo, seg_any, pred_any)
    needed = gr.needed_ref([vols[m] for m in ch], w, dims, tf_lo, seg, pred)
    return empty, needed, gr.skip_value_ref(ubs, w, wsum), tf_lo


@pytest.mark.parametrize("channels", [1, 2, 4])
@pytest.mark.parametrize("weights", sorted(gc.WEIGHTS))
def test_gap_construction_makes_the_mask_the_complement_of_needed(channels, weights):
    """Voxels 0 or in [0.3, 0.9], window floor 0.1: every cell's value is 0 or at least 0.1 above the floor, so whatever
    rounding a kernel applies, `empty` must be exactly `not needed` — with and without a label blob in the air."""
    dims = gc.SKIP_DIMS
    vols = gc.gap_volumes(dims, channels, seed=channels)
    w, en = gc.WEIGHTS[weights], gc.enabled_of(channels)
    lab = gc.air_labels(dims)
    for seg, pred in ((None, None), (lab, None), (None, lab), (lab, lab)):
        empty, needed, v, tf_lo = _masks_of(vols, w, en, dims, gc.GAP_WL, gc.GAP_WW, seg, pred)
        assert abs(float(tf_lo) - 0.1) < 1e-7
        assert np.all((v == 0) | (v.astype(np.float64) - float(tf_lo) >= 0.1))
        assert np.array_equal(empty, ~needed)
        assert 0.2 < empty.mean() < 0.9
    e0 = _masks_of(vols, w, en, dims, gc.GAP_WL, gc.GAP_WW)[0]
    e1 = _masks_of(vols, w, en, dims, gc.GAP_WL, gc.GAP_WW, lab)[0]
    assert (e0 & ~e1).sum() >= 2, "the label blob must keep cells alive that are empty without it"


def test_a_bound_without_the_overlap_plane_would_flag_needed_cells():
    """The mutation `8 c + 8 -> 8 c + 7` of the macro kernels, on the CPU: on the spike volume of the frame tests the mask it
    would give differs from the brute force, the real one does not."""
    dims = gc.SPIKE_DIMS
    X, Y, Z = dims
    v = gc.frame_spike_volume(dims)
    tf_lo = gr.window_floor(gc.GAP_WL, gc.GAP_WW)
    needed = gr.needed_ref([v], [1.0], dims, tf_lo)
    assert np.array_equal(needed, gc.frame_spike_cells(dims))
    good = gr.skip_mask_ref([gr.macro_max_ref(v, dims)], [1.0], F(1.0), tf_lo, None, None)
    assert np.array_equal(good, ~needed)
    mx, my, mz = gr.macro_dims(dims)
    vol = v.reshape(Z, Y, X)
    short = np.array([vol[8 * cz:min(8 * cz + 7, Z - 1) + 1, 8 * cy:min(8 * cy + 7, Y - 1) + 1, 8 * cx:min(8 * cx + 7, X - 1) + 1].max()
                      for cz in range(mz) for cy in range(my) for cx in range(mx)], F)
    bad = gr.skip_mask_ref([short], [1.0], F(1.0), tf_lo, None, None)
    assert (bad & needed).sum() >= 10, "the +7 bound must flag cells the brute force needs"
