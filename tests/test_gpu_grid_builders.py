"""The load-time builders of csrc/grid_ops.hip and csrc/volume_march.hip, element by element: every buffer they write —
pad voxels, pad lines and pad rows included — must be the same BITS as the NumPy restatement of the layout's documented
definition (tests/grid_ref.py), at dims chosen to reach every branch of the builders.  Frames cannot see most of this:
no ray reads a pad element, and a perspective view of a centred blob hardly weights the outermost voxel layer."""
import numpy as np
import pytest

import grid_cases as gc
import grid_ref as gr

pytestmark = pytest.mark.gpu

F = np.float32


def _bits(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32).reshape(-1)


def _fields(dims):
    yield "distinct", gc.distinct_field(dims)
    yield "wild", gc.wild_field(dims, seed=sum(dims))


@pytest.mark.parametrize("dims", gc.BUILDER_DIMS, ids=str)
def test_vg_quad_and_vga_grids_are_the_reference_bit_for_bit(dims):
    import mrirt
    if dims in gc.VGA_PITCHES:       # the case still reaches the padding branch it is here for
        assert [(g["rowLines"], g["sliceLines"]) for g in gr.vga_geometry_ref(dims)] == gc.VGA_PITCHES[dims]
    for name, v in _fields(dims):
        for layout, want in (("vg", gr.vec4_ref(v, dims, "vg")), ("quad", gr.vec4_ref(v, dims, "quad")), ("vga", gr.vga_ref(v, dims))):
            g = mrirt.upload_grid(v, dims, layout, macro=False)
            got = g.data.cpu().numpy()
            assert got.size == want.size, (layout, name)
            if name == "distinct":   # no NaN anywhere: raw bytes, so a -0.0 in a pad slot counts
                assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32)), (layout, name)
            else:                    # inf - inf: bit patterns of the non-NaN elements, NaN-ness of the rest
                assert gc.same_floats(got, want), (layout, name)


@pytest.mark.parametrize("dims", gc.BUILDER_DIMS[1:], ids=str)
def test_mod4_grid_is_the_reference_bit_for_bit(dims):
    import mrirt
    if min(dims) < 2:
        with pytest.raises(mrirt._lib.MrirtError):       # MOD4 refuses a degenerate axis
            mrirt.upload_mod4([gc.distinct_field(dims)] * 4, dims, macro=False)
        return
    n = gc.nvox(dims)
    mods = [gc.distinct_field(dims, scale=1.0, offset=1.0 + m * n) for m in range(3)] + [gc.wild_field(dims, seed=7)]
    for bound in (mods, [mods[0], None, mods[3], None], [None, None, None, mods[1]]):
        g = mrirt.upload_mod4(bound, dims, macro=False)
        want = gr.vec4_ref(bound, dims, "mod4")          # a None slot is stored as zeros
        got = g.data.cpu().numpy()
        assert got.size == want.size and gc.same_floats(got, want)


@pytest.mark.parametrize("dims", [(37, 29, 23), (1, 3, 2)], ids=str)
def test_cell8_is_the_reference_from_both_source_modes(dims):
    from mrirt import render, volume
    n = gc.nvox(dims)
    rng = np.random.default_rng(n)
    u8 = rng.integers(0, 256, n).astype(np.uint8)
    if n >= 256:                                         # (1,3,2) has six voxels: it is here for the clamps, not for the byte values
        u8[rng.choice(n, 256, replace=False)] = np.arange(256, dtype=np.uint8)
        assert np.unique(u8).size == 256                 # every byte value present
    want = gr.cell8_ref(u8, dims)
    for mode, src in (("u8", u8), ("u32x4", volume.pack_u8_as_u32x4(u8))):
        got = render.build_cell8(src, dims, mode).cpu().numpy()
        assert got.dtype == np.int64 and got.size == n
        assert np.array_equal(got.view(np.uint8).reshape(n, 8), want), mode


def _macro_ub(v, dims):
    import mrirt
    return mrirt.upload_grid(v, dims, "linear").macro


@pytest.mark.parametrize("dims", gc.MACRO_DIMS, ids=str)
def test_macro_bounds_are_the_reference_bit_for_bit(dims):
    cells = int(np.prod(gr.macro_dims(dims)))
    n = gc.nvox(dims)
    rng = np.random.default_rng(n)
    fields = {"wild": gc.wild_field(dims, seed=n), "random": rng.standard_normal(n).astype(F),
              "negative": (-1 - rng.random(n)).astype(F), "denormal": (rng.integers(-5000, 5000, n) * np.float64(1.4e-45)).astype(F)}
    for name, v in fields.items():
        got = _macro_ub(v, dims).cpu().numpy()
        want = gr.macro_max_ref(v, dims)
        assert got.shape == (cells,) and not np.isnan(want).any()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    # single spikes on and next to the macro-cell boundaries, said outright: the k-th spike has height k + 1, and a cell's
    # bound is the bound of the highest spike whose voxel lies in [8m, min(8m + 8, D - 1)] on every axis
    v, spikes = gc.spike_field(dims)
    want = np.zeros(cells, F)
    for x, y, z, h in spikes:
        want[gc.cells_seeing(x, y, z, dims)] = F(h + F(F(2e-6) * h))
    got = _macro_ub(v, dims).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), gr.macro_max_ref(v, dims).view(np.uint32))
    if dims[0] >= 9:                                     # a spike at 8 is seen by cells 0 and 1 of that axis
        one = np.zeros(n, F)
        one[8] = 1
        got = _macro_ub(one, dims).cpu().numpy()
        assert np.flatnonzero(got).tolist() == [0, 1] and got[0] == got[1] == F(F(1) + F(2e-6))
    # one NaN voxel: +inf in exactly the cells whose inclusive range holds it, +0.0 elsewhere
    x, y, z = min(8, dims[0] - 1), min(8, dims[1] - 1), min(8, dims[2] - 1)
    v = np.zeros(n, F)
    v[x + dims[0] * (y + dims[1] * z)] = np.nan
    got = _macro_ub(v, dims).cpu().numpy()
    hit = np.isin(np.arange(cells), gc.cells_seeing(x, y, z, dims))
    assert np.array_equal(np.isposinf(got), hit) and not got[~hit].view(np.uint32).any()
    # a value range beyond FLT_MAX: the lerps overflow between two finite voxels, the bound is +inf
    v = np.where(np.arange(n) // (dims[0] * dims[1]) % 2 == 0, F(3e38), F(-3e38)).astype(F)
    got = _macro_ub(v, dims).cpu().numpy()
    want = gr.macro_max_ref(v, dims)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (np.isposinf(got).any() or dims[2] == 1)


@pytest.mark.parametrize("dims", gc.MACRO_DIMS, ids=str)
def test_macro_label_summaries_are_the_reference(dims):
    import mrirt
    cells = int(np.prod(gr.macro_dims(dims)))
    lab = gc.sparse_labels(dims, seed=3)
    assert (lab >= 8).any() and lab[-1] != 0
    got = mrirt.upload_grid(lab, dims, "linear").macro.cpu().numpy().view(np.uint32)
    assert got.shape == (cells,) and np.array_equal(got, gr.macro_labels_ref(lab, dims))
    assert got[-1] & 5 == 5                              # the label of the last voxel reaches the last cell
    # both summaries of a label-cell grid and the four of a MOD4 grid come from the same kernels
    if min(dims) >= 2:
        prd = gc.sparse_labels(dims, seed=4)
        g = mrirt.upload_label_cells(lab, prd, dims)
        assert np.array_equal(g.macro.cpu().numpy().view(np.uint32), gr.macro_labels_ref(lab, dims))
        assert np.array_equal(g.macro2.cpu().numpy().view(np.uint32), gr.macro_labels_ref(prd, dims))
        v = gc.wild_field(dims, seed=9)
        g4 = mrirt.upload_mod4([v, None, gc.distinct_field(dims), None], dims)
        assert g4.macros[1] is None and g4.macros[3] is None
        assert np.array_equal(_bits(g4.macros[0]), gr.macro_max_ref(v, dims).view(np.uint32))
        assert np.array_equal(_bits(g4.macros[2]), gr.macro_max_ref(gc.distinct_field(dims), dims).view(np.uint32))


def test_bc4_decodes_every_endpoint_pair():
    """One 1024 x 1024 slice = 256 x 256 blocks: block (r0, r1) holds that endpoint pair, and its sixteen codes cycle
    through 0..7 from a start that moves with the block, so every code occurs in every block and at varying texels."""
    from mrirt import volume
    r1, r0 = np.meshgrid(np.arange(256, dtype=np.uint64), np.arange(256, dtype=np.uint64), indexing="ij")     # block (by, bx) = (r1, r0)
    codes = (np.arange(16, dtype=np.uint64)[None, None, :] + (r0 + 3 * r1)[:, :, None]) % np.uint64(8)
    bits = np.zeros((256, 256), np.uint64)
    for t in range(16):
        bits |= codes[:, :, t] << np.uint64(3 * t)
    blk = np.empty((256, 256, 8), np.uint8)
    blk[..., 0], blk[..., 1] = r0, r1
    for k in range(6):
        blk[..., 2 + k] = (bits >> np.uint64(8 * k)) & np.uint64(0xff)
    pairs = blk[..., 0].astype(int) * 256 + blk[..., 1]
    assert np.unique(pairs).size == 65536 and all(np.unique(c).size == 8 for c in codes.reshape(-1, 16)[::997])
    want = volume.bc4_decode(blk.tobytes(), 1024, 1024, 1)
    got = volume.bc4_decode_device(blk.reshape(-1), 1024, 1024, 1).cpu().numpy()
    assert got.dtype == np.uint8 and got.size == 1 << 20 and np.array_equal(got, want)
