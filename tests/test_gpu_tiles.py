"""Tile-sharded frames on one GPU: every K1 march kernel, K2 and the de-tiling kernel on a ragged image, held bit for bit to the
oracle through tests/tiles_ref.py (the deal restated from include/mrirt.h).

The scene is tests/k1_plan_ref.py's (40 x 34 x 27 voxels, 40 x 28 pixels, 60 steps) with a background colour that is not zero.  At
tile 16 the image is a 3 x 2 tile grid with compact-buffer slots outside the image along the right edge (x 40..47), the bottom
edge (y 28..31) and both in the corner tile: map_pixel's kind 2, which a kernel must not march and must fill with the background.
Every output buffer is NaN before the launch, so an unwritten slot shows; the ranks' counters must add up to the whole frame's, so
a marched kind-2 lane shows.

  a  every kernel identity of K.cases_by_kernel() plus the tagged twin, one pytest id each: the first configuration that maps to
     it, both workgroup shapes, (tile, world, skew) = (16, 3, 2) and (16, 7, 0) — rank 6 of 7 owns nothing.  STRICT against
     oracle_c, FAST against the same kernel's whole-frame launch; skipping plans also with the map, which must be used.
  b  one representative per family (generic, pipelined, rolling, skipping pipelined, skipping rolling, slab, ring) over eight
     setups, the XCD band bits and row-major lanes on the 16- and 48-pixel tiles, rgba16f, tileSkew passed unreduced.
  c  K2 (four voxel modes, both cameras, both maths, both formats) in tiles, and its whole-frame rgba16f output.
  d  mrirt_detile alone on buffers that name their own slots, padded tiles NaN: sizes, tiles, worlds, every skew, both formats,
     a pitched output with guard columns, the host branch of tiles.assemble_frame, tiles.FrameExchange, the refusals.
  e  the rank that owns no tile: an empty buffer, zero counters, nothing launched, through every door; a NULL output with
     work to do stays MRIRT_ERR_NULL.

MEASURED: 249 ids (174 of them a: one per kernel identity, the tagged twin and the count) in 6.6 s of wall time on an MI355X; the
slowest id takes 1.5 s (the empty rank, which loads the operator library), every other one under 0.2 s — so (a) keeps both setups.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import k1_plan_ref as K
import tiles_ref as R
from test_gpu_k1_kernels import _Bound, _ext

pytestmark = pytest.mark.gpu

W, H = K.IMAGE_WH
BG = (0.125, 0.5, 0.75)
EXP_RANGE = "large"
CASES = K.cases_by_kernel()
TAG_KERNEL = K.plan(K.TAG_CONFIG).kernel
KERNEL_CONFIGS = {k: v[0] for k, v in CASES.items()}
KERNEL_CONFIGS[TAG_KERNEL] = K.TAG_CONFIG
KERNELS = sorted(KERNEL_CONFIGS, key=K.kernel_id)
SETUPS_A = [(16, 3, 2), (16, 7, 0)]
SETUPS_B = [(16, 1, 0), (16, 2, 1), (16, 4, 5), (16, 6, 1), (16, 32, 0), (32, 2, 1), (32, 3, 0), (48, 1, 0)]
# kernelVariant: bit 3 (contiguous runs per XCD), bits 4-5 = 1, 2, 3 (16, 32, 64 px bands), bit 0 (row-major lanes)
MAP_VARIANTS = [8, 16, 32, 48, 1]
SLAB, RING = 64, 2048


@pytest.fixture(scope="module")
def bound():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _Bound()


def _params(c):
    p = K.params(c, EXP_RANGE)
    p["bgColor"] = np.array(BG, np.float32)
    return p


_REFS = {}


def _oracle(c):
    """(frame, aux) of oracle_c for a configuration with the background colour, once per K.reference_key."""
    key = K.reference_key(c, EXP_RANGE)
    if key not in _REFS:
        from oracle import oracle_c
        s = K.shared_scene()
        ref, aux = oracle_c.brats_main(_params(c), s["vols"], s["lab"], s["prd"], K.shade_ext(c), return_aux=True)
        ref.setflags(write=False)
        _REFS[key] = (ref, aux)
    return _REFS[key]


def _nan(shape, half=False):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float16 if half else torch.float32, device="cuda")


def _whole(bound, c, p, ext, skip):
    gl, gp = bound.labels(c)
    out = _nan((H, W, 4))
    img, st = bound.mrirt.render_brats(p, bound.vols(c.layout), gl, gp, out=out, ext=ext, stats=True, skip=skip)
    return img.cpu().numpy(), st


def _tiles(bound, c, p, ext, setup, skip, half=False):
    """Every rank's compact buffer (rendered into NaN) and counters."""
    ts, world, skew = setup
    gl, gp = bound.labels(c)
    bufs, stats = [], []
    for r in range(world):
        n = R.tiles_for_rank(W, H, ts, r, world)
        out = _nan((n, ts, ts, 4), half)
        e = dict(ext, tileSize=ts, tileRank=r, tileWorld=world, tileSkew=skew)
        if half:
            e["outFormat"] = "rgba16f"
        img, st = bound.mrirt.render_brats(p, bound.vols(c.layout), gl, gp, out=out, ext=e, stats=True, skip=skip)
        assert img.shape == (n, ts, ts, 4) and img.data_ptr() == out.data_ptr()
        bufs.append(img.cpu().numpy())
        stats.append(st)
    return bufs, stats


def _hold(bufs, frame, setup, what, dtype=np.float32):
    """Every rank's buffer is expected_compact of the frame, bit for bit; alpha is 1 in every slot."""
    ts, world, skew = setup
    for r, got in enumerate(bufs):
        want = R.expected_compact(frame, BG, W, H, ts, r, world, skew, dtype=dtype)
        assert got.shape == want.shape and got.dtype == want.dtype, (what, r, got.shape, got.dtype)
        if not np.array_equal(got, want):
            bad = (got != want).any(axis=-1)
            off = (R.expected_compact(np.full((H, W, 4), 2.0, np.float32), (3.0, 3.0, 3.0), W, H, ts, r, world, skew)[..., 0] == 3.0)
            raise AssertionError(f"{what}: rank {r} of {world} (tile {ts}, skew {skew}) differs in {int(bad.sum())} slots, "
                                 f"{int((bad & off).sum())} of them outside the image, {int(np.isnan(got).any(axis=-1).sum())} with a NaN")
        assert np.all(got[..., 3] == 1), (what, r)


def _sum(stats):
    return {k: sum(s[k] for s in stats) for k in ("live_samples", "shaded_samples")}


def _counters(aux):
    return {k: aux[k] for k in ("live_samples", "shaded_samples")}


def _check_tiled(bound, c, flip, setup, extra=0, frame_and_counters=None):
    """One configuration, one workgroup shape, one setup.  STRICT: oracle_c; FAST: the whole-frame launch of the same kernel."""
    from mrirt import render
    pl = K.plan(c)
    p = _params(c)
    ext = _ext(c, flip, extra)
    what = f"{c} {'16x16' if flip else '8x8'} variant {ext['kernelVariant']} setup {setup}"
    skips = (False, True) if pl.skipping else (c.skip,)
    first = None
    for skip in skips:
        if c.math == "strict":
            frame, aux = _oracle(c)
            want = _counters(aux)
        else:
            frame, want = frame_and_counters[skip]
        bufs, stats = _tiles(bound, c, p, ext, setup, skip)
        _hold(bufs, frame, setup, f"{what} skip={skip}")
        assert _sum(stats) == want, f"{what} skip={skip}: the ranks' counters {_sum(stats)} do not add up to the whole frame's {want}"
        for r, st in enumerate(stats):
            if R.tiles_for_rank(W, H, setup[0], r, setup[1]) == 0:
                assert st == {"live_samples": 0, "shaded_samples": 0}, (what, r, st)
        if first is None:
            first = (bufs, stats)
        else:
            assert all(np.array_equal(a, b) for a, b in zip(bufs, first[0])) and stats == first[1], f"{what}: the skipping march differs from the plain one"
    if pl.skipping:
        # the tiled launch really took the skipping kernel: kernelVariant bit 7 counts the samples it did not fetch
        bufs7, stats7 = _tiles(bound, c, p, _ext(c, flip, extra | K.VARIANT_COUNT_UNFETCHED), setup, True)
        assert all(np.array_equal(a, b) for a, b in zip(bufs7, first[0])), what
        grew = [s7["shaded_samples"] - s["shaded_samples"] for s7, s in zip(stats7, first[1])]
        assert [s7["live_samples"] for s7 in stats7] == [s["live_samples"] for s in first[1]] and min(grew) >= 0, (what, grew)
        assert max(grew) > 0, f"{what}: the skipping march fetched every sample on every rank"
        (entry,) = render._SKIP_MAPS.values()
        assert entry.built, what


# ----------------------------------------------------------------------------------------------------------------------
# a. every kernel
# ----------------------------------------------------------------------------------------------------------------------
def test_one_id_per_kernel_identity():
    assert len(KERNELS) == len(set(K.kernel_id(k) for k in KERNELS)) == len(K.cases_by_kernel()) + 1
    assert TAG_KERNEL not in CASES and TAG_KERNEL[-1] is True


@pytest.mark.parametrize("kernel", KERNELS, ids=K.kernel_id)
def test_kernel_in_tiles(bound, kernel):
    from mrirt import render
    c = KERNEL_CONFIGS[kernel]
    pl = K.plan(c)
    assert pl.kernel == kernel
    for flip in (False, True):
        if pl.skipping:
            render._SKIP_MAPS.clear()
        whole = None
        if c.math == "fast":
            whole = {skip: _whole(bound, c, _params(c), _ext(c, flip), skip) for skip in ((False, True) if pl.skipping else (c.skip,))}
            for frame, _ in whole.values():
                assert not np.isnan(frame).any()
        for setup in SETUPS_A:
            _check_tiled(bound, c, flip, setup, frame_and_counters=whole)


# ----------------------------------------------------------------------------------------------------------------------
# b. the setup grid on one representative per family
# ----------------------------------------------------------------------------------------------------------------------
_ONE = K.Config("strict", "vga", True, (2,), 1.0, "none", False, False, False)
FAMILIES = {
    "generic": (K.Config("strict", "brick", True, (2,), 1.0, "seg", False, False, False), 0, "generic"),
    "pipelined": (_ONE, 0, "pipelined"),
    "rolling": (K.Config("strict", "vg", True, (0, 3), 1.0, "none", False, False, False), 0, "rolling"),
    "skipping-pipelined": (_ONE._replace(skip=True), 0, "pipelined"),
    "skipping-rolling": (K.Config("strict", "vg", True, (0, 3), 1.0, "none", False, True, False), 0, "rolling"),
    "slab": (_ONE, SLAB, "slab"),
    "ring": (_ONE, RING, "ring"),
}


def _family_of(c, ext, setup, rank):
    from mrirt import render
    ts, world, skew = setup
    return render.kernel_family(_params(c), dict(ext, tileSize=ts, tileRank=rank, tileWorld=world, tileSkew=skew), skip=K.plan(c).skipping)


@pytest.mark.parametrize("setup", SETUPS_B, ids=lambda s: "t%d-w%d-s%d" % s)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_over_the_setups(bound, family, setup):
    from mrirt import render
    c, lds, want_family = FAMILIES[family]
    pl = K.plan(c)
    assert pl.family == ("pipelined" if lds else want_family) and pl.skipping == family.startswith("skipping")
    ts, world, skew = setup
    tiles_x, _ = R.tile_grid(W, H, ts)
    render._SKIP_MAPS.clear()
    flips = (False,) if lds else (False, True)           # (the LDS kernels are written for one packet per workgroup)
    for flip in flips:
        variants = [0] + (MAP_VARIANTS if ts in (16, 48) else [])
        for v in variants:
            ext = _ext(c, flip, lds | v)
            for r in range(world):
                fam = _family_of(c, ext, setup, r)
                owns = R.tiles_for_rank(W, H, ts, r, world) > 0
                assert fam["family"] == (want_family if owns else "none") and fam["skipping"] == (pl.skipping and owns), (family, setup, v, r, fam)
            _check_tiled(bound, c, flip, setup, extra=lds | v)
        # rgba16f: the same frame, rounded
        ext = _ext(c, flip, lds)
        frame, aux = _oracle(c)
        bufs, stats = _tiles(bound, c, _params(c), ext, setup, pl.skipping, half=True)
        _hold(bufs, frame, setup, f"{family} rgba16f {setup}", dtype=np.float16)
        assert _sum(stats) == _counters(aux)
        # tileSkew is reduced modulo tilesX by the library
        for raw in (5, tiles_x + 1):
            a, sa = _tiles(bound, c, _params(c), ext, (ts, world, raw), pl.skipping)
            b, sb = _tiles(bound, c, _params(c), ext, (ts, world, raw % tiles_x), pl.skipping)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and sa == sb, (family, setup, raw)
            _hold(a, frame, (ts, world, raw), f"{family} unreduced skew {raw}")


# ----------------------------------------------------------------------------------------------------------------------
# c. K2
# ----------------------------------------------------------------------------------------------------------------------
K2_DIMS = (20, 17, 13)
K2_SETUPS = [(16, 3, 2), (16, 7, 0), (32, 2, 1), (48, 1, 0)]
K2_BG = (0.0, 0.0, 0.0)
K2_CAMERAS = {"perspective": {}, "ortho": dict(cameraMode=1, orthoHalfHeight=1.1)}


@pytest.fixture(scope="module")
def k2():
    import mrirt
    from mrirt import synth
    from oracle import oracle_np
    f = synth.synth_volume(0, 1234, dims=K2_DIMS)
    u8 = np.rint(f * 255).astype(np.uint8)
    p = synth.volume_scene(0, 0, 24, 1.5, 4.5, dims=K2_DIMS)
    p["imageSize"] = (np.uint32(W), np.uint32(H))
    host = {"u8": u8, "cell8": u8, "u32x4": oracle_np.pack_u8_volume(u8), "f32": f}
    dev = dict(host, cell8=mrirt.render.build_cell8(u8.reshape(-1), K2_DIMS, "u8"))
    return dict(p=p, host=host, dev=dev)


def _k2_tiles(k2, mode, ext, setup, half):
    import mrirt
    ts, world, skew = setup
    bufs, live = [], 0
    for r in range(world):
        n = R.tiles_for_rank(W, H, ts, r, world)
        e = dict(ext, tileSize=ts, tileRank=r, tileWorld=world, tileSkew=skew, outFormat="rgba16f" if half else "rgba32f")
        img, st = mrirt.render_volume_u8(k2["p"], k2["dev"][mode], mode=mode, out=_nan((n, ts, ts, 4), half), ext=e, stats=True)
        assert img.shape == (n, ts, ts, 4)
        if n == 0:
            assert st["live_samples"] == 0
        bufs.append(img.cpu().numpy())
        live += st["live_samples"]
    return bufs, live


def _k2_hold(bufs, frame, setup, what, dtype):
    ts, world, skew = setup
    for r, got in enumerate(bufs):
        want = R.expected_compact(frame, K2_BG, W, H, ts, r, world, skew, dtype=dtype)
        assert got.dtype == want.dtype and np.array_equal(got, want), f"{what}: rank {r} of {world} (tile {ts}, skew {skew}) differs in " \
            f"{int((got != want).any(axis=-1).sum())} slots, {int(np.isnan(got).any(axis=-1).sum())} with a NaN"
        assert np.all(got[..., 3] == 1)


@pytest.mark.parametrize("camera", sorted(K2_CAMERAS))
@pytest.mark.parametrize("mode", ["u8", "cell8", "u32x4", "f32"])
def test_k2_in_tiles(k2, mode, camera):
    import torch
    import mrirt
    from oracle import oracle_c
    cam = K2_CAMERAS[camera]
    ref, aux = oracle_c.volume_cs(k2["p"], k2["host"][mode], mode="u8" if mode == "cell8" else mode, ext=cam, return_aux=True)
    assert ref.max() > 0.05 and aux["live_samples"] > 0
    for math in ("strict", "fast"):
        ext = dict(cam, math=math)
        whole, st = mrirt.render_volume_u8(k2["p"], k2["dev"][mode], mode=mode, out=_nan((H, W, 4)), ext=ext, stats=True)
        frame, live = whole.cpu().numpy(), st["live_samples"]
        if math == "strict":
            assert np.array_equal(frame, ref) and live == aux["live_samples"]
            # the whole-frame rgba16f output: the oracle's frame, rounded
            half = mrirt.render_volume_u8(k2["p"], k2["dev"][mode], mode=mode, out=_nan((H, W, 4), True), ext=dict(ext, outFormat="rgba16f"))
            assert half.dtype == torch.float16 and np.array_equal(half.cpu().numpy(), ref.astype(np.float16)), (mode, camera)
            frame = ref
        else:
            assert not np.isnan(frame).any()
            half = mrirt.render_volume_u8(k2["p"], k2["dev"][mode], mode=mode, out=_nan((H, W, 4), True), ext=dict(ext, outFormat="rgba16f"))
            assert np.array_equal(half.cpu().numpy(), frame.astype(np.float16)), (mode, camera)
        for setup in K2_SETUPS:
            for half_out in (False, True):
                bufs, tiled_live = _k2_tiles(k2, mode, ext, setup, half_out)
                _k2_hold(bufs, frame, setup, f"K2 {mode} {camera} {math} {'rgba16f' if half_out else 'rgba32f'}", np.float16 if half_out else np.float32)
                assert tiled_live == live, (mode, camera, math, setup, tiled_live, live)


# ----------------------------------------------------------------------------------------------------------------------
# d. mrirt_detile alone
# ----------------------------------------------------------------------------------------------------------------------
DETILE_SIZES = [(40, 28), (16, 16), (1, 1), (49, 33), (130, 70)]
DETILE_TILES = [16, 32, 48]
DETILE_WORLDS = [1, 2, 3, 5, 8, 13]


@pytest.mark.parametrize("size", DETILE_SIZES, ids=lambda s: "%dx%d" % s)
def test_detile_synthetic_buffers(size):
    import torch
    import mrirt
    from mrirt import tiles
    w, h = size
    for ts, world in itertools.product(DETILE_TILES, DETILE_WORLDS):
        tiles_x, _ = R.tile_grid(w, h, ts)
        for dtype in (np.float32, np.float16):
            g = R.synthetic_gathered(w, h, ts, world, dtype)
            assert np.nanmax(g.astype(np.float32)) < 2048
            dev = torch.from_numpy(g).cuda()
            for skew in range(tiles_x + 1):
                want = R.expected_frame(g, w, h, ts, world, skew)
                assert not np.isnan(want).any()
                got = mrirt.detile(dev, w, h, ts, world, skew=skew).cpu().numpy()
                assert got.dtype == dtype and got.shape == (h, w, 4)
                assert not np.isnan(got).any(), f"a padded slot reached the frame: {size} tile {ts} world {world} skew {skew}"
                assert np.array_equal(got, want), (size, ts, world, skew, dtype.__name__, int((got != want).any(axis=-1).sum()))
                # the device branch of assemble_frame is that kernel; the host branch is plain indexing
                assert torch.equal(tiles.assemble_frame(dev, w, h, ts, world, skew), torch.from_numpy(want).cuda())
                if dtype is np.float32:
                    assert np.array_equal(tiles.assemble_frame(torch.from_numpy(g), w, h, ts, world, skew).numpy(), want)
            # a pitch wider than the image: the guard columns stay as they were
            skew = 1 % tiles_x
            wide = torch.full((h, w + 5, 4), -1.0, dtype=dev.dtype, device="cuda")
            out = mrirt.detile(dev, w, h, ts, world, out=wide[:, :w], skew=skew)
            assert out.data_ptr() == wide.data_ptr() and out.stride(0) == 4 * (w + 5)
            full = wide.cpu().numpy()
            assert np.array_equal(full[:, :w], R.expected_frame(g, w, h, ts, world, skew)) and np.all(full[:, w:] == -1), (size, ts, world)


@pytest.mark.parametrize("half", [False, True], ids=["rgba32f", "rgba16f"])
def test_frame_exchange_without_a_process_group(half):
    import torch
    import torch.distributed as dist
    from mrirt import tiles
    assert not dist.is_initialized()
    dtype = np.float16 if half else np.float32
    for (w, h), ts in itertools.product([(40, 28), (49, 33)], [16, 32]):
        tiles_x, _ = R.tile_grid(w, h, ts)
        g = R.synthetic_gathered(w, h, ts, 1, dtype)
        for skew in (0, 1, tiles_x + 1):
            ex = tiles.FrameExchange(w, h, ts, torch.float16 if half else torch.float32, "cuda", depth=2, skew=skew)
            assert ex.world == 1 and ex.n_local == ex.max_local == g.shape[1]
            for i in (0, 1):
                ex.local(i).copy_(torch.from_numpy(g[0] + dtype(i)).cuda())
            for i in (0, 1):
                ex.submit(i)
            for i in (1, 0):
                got = ex.finish(i).cpu().numpy()
                assert np.array_equal(got, R.expected_frame(g + dtype(i), w, h, ts, 1, skew)), (w, h, ts, skew, i)


def test_detile_refusals_leave_the_frame_untouched():
    import torch
    import mrirt
    lib = mrirt._lib.lib()
    w, h, ts, world = 40, 28, 16, 3
    g = torch.from_numpy(R.synthetic_gathered(w, h, ts, world)).cuda()
    frame = torch.full((h, w, 4), -1.0, device="cuda")
    G, F = C.c_void_p(g.data_ptr()), C.c_void_p(frame.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    NULL_, DIMS_, LAYOUT_, ARG_ = -1, -2, -3, -5
    calls = {
        "tileSize 0": (ARG_, (G, F, w, h, w, 0, world, 0, 0, s)),
        "tileSize 8": (DIMS_, (G, F, w, h, w, 8, world, 0, 0, s)),
        "world 0": (ARG_, (G, F, w, h, w, ts, 0, 0, 0, s)),
        "pitch < width": (ARG_, (G, F, w, h, w - 1, ts, world, 0, 0, s)),
        "outFormat 2": (LAYOUT_, (G, F, w, h, w, ts, world, 0, 2, s)),
        "NULL gathered": (NULL_, (None, F, w, h, w, ts, world, 0, 0, s)),
        "NULL frame": (NULL_, (G, None, w, h, w, ts, world, 0, 0, s)),
    }
    for what, (code, args) in calls.items():
        assert lib.mrirt_detile(*args) == code, what
        torch.cuda.synchronize()
        assert bool((frame == -1).all()), what
    assert lib.mrirt_detile(G, F, w, h, w, ts, world, 0, 0, s) == 0
    assert np.array_equal(frame.cpu().numpy(), R.expected_frame(g.cpu().numpy(), w, h, ts, world, 0))


# ----------------------------------------------------------------------------------------------------------------------
# e. the rank that owns no tile
# ----------------------------------------------------------------------------------------------------------------------
EMPTY = [(16, 6, 7), (16, 31, 32), (48, 1, 2)]            # (tile, rank, world) with mrirt_tiles_for_rank == 0


def _k1_blocks(bound, c, ext):
    """(MrirtBratsParams, MrirtRenderExt, the four grid pointers) of a raw C-ABI call."""
    from mrirt import params
    P, E = params.brats_params(_params(c)), params.render_ext(ext)
    grids = bound.vols(c.layout)
    vp = (C.c_void_p * 4)(*[C.c_void_p(g.data.data_ptr()) if P.volEnabled[m] != 0 else None for m, g in enumerate(grids)])
    return P, E, vp, grids


def test_empty_rank_renders_nothing_and_raises_nothing(bound, k2):
    import torch
    import mrirt
    from mrirt import render, torch_ops
    native = torch_ops.load_native()
    lib = mrirt._lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for c in (_ONE, _ONE._replace(skip=True), FAMILIES["generic"][0], FAMILIES["rolling"][0]._replace(skip=True)):
        gl, gp = bound.labels(c)
        for (ts, rank, world), half in itertools.product(EMPTY, (False, True)):
            assert render.tiles_for_rank(W, H, ts, rank, world) == 0 == R.tiles_for_rank(W, H, ts, rank, world)
            dt = torch.float16 if half else torch.float32
            ext = dict(_ext(c, False), tileSize=ts, tileRank=rank, tileWorld=world, outFormat="rgba16f" if half else "rgba32f")
            assert render.kernel_family(_params(c), ext, skip=c.skip)["family"] == "none"
            for skip in (False, True):
                img, st = mrirt.render_brats(_params(c), bound.vols(c.layout), gl, gp, ext=ext, stats=True, skip=skip)
                assert img.shape == (0, ts, ts, 4) and img.dtype == dt and img.is_cuda, (c, ts, rank, world, skip)
                assert st == {"live_samples": 0, "shaded_samples": 0}
            # the operators, both registrations
            P, E, vp, grids = _k1_blocks(bound, c, ext)
            args = (torch_ops.pack_brats_params(_params(c)), torch_ops.pack_render_ext(ext),
                    *[g.data if P.volEnabled[m] != 0 else None for m, g in enumerate(grids)], gl.data.view(torch.int32) if gl is not None else None, gp.data.view(torch.int32) if gp is not None else None)
            for door in (torch.ops.mrirt, native):
                img = door.render_brats(*args)
                assert img.shape == (0, ts, ts, 4) and img.dtype == dt and img.is_cuda
            # the raw ABI: a NULL output is fine where there is nothing to write
            st = torch.zeros(2, dtype=torch.int64, device="cuda")
            rc = lib.mrirt_render_brats_ex(C.byref(P), C.byref(E), vp, C.c_void_p(gl.data.data_ptr()) if gl is not None else None,
                                           C.c_void_p(gp.data.data_ptr()) if gp is not None else None, None, W, C.c_void_p(st.data_ptr()), s)
            assert rc == 0 and st.cpu().tolist() == [0, 0]
    # K2
    p = k2["p"]
    for (ts, rank, world), half, mode in itertools.product(EMPTY, (False, True), ("u8", "cell8", "u32x4", "f32")):
        dt = torch.float16 if half else torch.float32
        ext = dict(tileSize=ts, tileRank=rank, tileWorld=world, outFormat="rgba16f" if half else "rgba32f")
        img, st = mrirt.render_volume_u8(p, k2["dev"][mode], mode=mode, ext=ext, stats=True)
        assert img.shape == (0, ts, ts, 4) and img.dtype == dt and st == {"live_samples": 0}
    u8 = torch.from_numpy(k2["host"]["u8"].reshape(-1)).cuda()
    for (ts, rank, world), half in itertools.product(EMPTY, (False, True)):
        ext = dict(tileSize=ts, tileRank=rank, tileWorld=world, outFormat="rgba16f" if half else "rgba32f")
        for door in (torch.ops.mrirt, native):
            img = door.render_volume(torch_ops.pack_volume_params(p), torch_ops.pack_render_ext(ext), u8, 1)
            assert img.shape == (0, ts, ts, 4) and img.dtype == (torch.float16 if half else torch.float32)
        from mrirt import params
        rc = lib.mrirt_render_volume(C.byref(params.volume_params(p)), C.byref(params.render_ext(ext)), C.c_void_p(u8.data_ptr()), 1, None, W, None, s)
        assert rc == 0


def test_null_output_with_work_to_do_is_still_refused(bound, k2):
    import torch
    import mrirt
    from mrirt import params
    lib = mrirt._lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    c = _ONE
    u8 = torch.from_numpy(k2["host"]["u8"].reshape(-1)).cuda()
    for tile in ({}, dict(tileSize=16, tileRank=0, tileWorld=7), dict(tileSize=16, tileRank=5, tileWorld=7), dict(tileSize=48, tileRank=0, tileWorld=1)):
        P, E, vp, grids = _k1_blocks(bound, c, dict(_ext(c, False), **tile))
        st = torch.zeros(2, dtype=torch.int64, device="cuda")
        assert lib.mrirt_render_brats_ex(C.byref(P), C.byref(E), vp, None, None, None, W, C.c_void_p(st.data_ptr()), s) == -1, tile
        assert lib.mrirt_render_volume(C.byref(params.volume_params(k2["p"])), C.byref(params.render_ext(tile)), C.c_void_p(u8.data_ptr()), 1,
                                       None, W, C.c_void_p(st.data_ptr()), s) == -1, tile
        assert st.cpu().tolist() == [0, 0]


class _FakeGroup:
    """torch.distributed as tiles.py uses it, for `world` ranks that run one after the other in this process: the ranks other
    than `dst` leave what they send, `dst` (run last) receives it."""

    def __init__(self, world):
        self.world, self.rank, self.sent = world, 0, {}

    def is_initialized(self):
        return True

    def get_world_size(self, group=None):
        return self.world

    def get_rank(self, group=None):
        return self.rank

    def gather(self, send, parts, dst=0, group=None, async_op=False):
        self.sent[self.rank] = send
        if parts is not None:
            for r, part in enumerate(parts):
                part.copy_(self.sent[r])


def test_sharded_render_pads_the_empty_ranks(bound, monkeypatch):
    """tiles.render_brats_sharded over seven ranks of a six-tile image, the collective emulated in-process: rank 6 sends rank 0's
    tile count of padding, and rank 0 assembles the oracle's frame."""
    import torch
    from mrirt import tiles
    c = _ONE
    frame, _ = _oracle(c)
    world, ts = 7, 16
    fake = _FakeGroup(world)
    monkeypatch.setattr(tiles, "dist", fake)
    got = None
    for rank in (1, 2, 3, 4, 5, 6, 0):
        fake.rank = rank
        got = tiles.render_brats_sharded(_params(c), bound.vols(c.layout), ext=_ext(c, False), tile=ts)
        assert (got is None) == (rank != 0)
        assert fake.sent[rank].shape == (R.max_local(W, H, ts, world), ts, ts, 4), rank
    assert torch.equal(got, torch.from_numpy(frame.copy()).cuda())
    assert not bool(fake.sent[6].isnan().any())
