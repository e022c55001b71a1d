"""Dispatch order of the K1 march (mrirt_render_brats_ordered): whatever table the launch is given — identity, reversed,
random, learned from the last frame, learned from another camera — the frame and the counters are the SAME BITS as the
plain launch's; the step record the march leaves is the per-workgroup maximum of the oracle's per-pixel step counts; tiled
and skipping launches ignore the scratch.  A 64^3 volume at 136 x 120 px (ragged edge workgroups) and 128 x 128 px, the
shaded VGA and the unshaded QUAD kernels (STRICT), both workgroup sizes (kernelVariant bit 1)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS = (64, 64, 64)
XCDS = 8
SHAPES = {"ragged": (120, 136), "square": (128, 128)}              # (H, W)
KINDS = {"vga-shaded": ("vga", True), "quad": ("quad", False)}


@functools.lru_cache(maxsize=None)
def volume():
    from mrirt import synth
    return synth.synth_volume(0, 4321, phase=0.2, dims=DIMS)


@functools.lru_cache(maxsize=None)
def grid(layout):
    import mrirt
    return mrirt.upload_grid(volume(), DIMS, layout)


def scene(shape, other_camera=False):
    from mrirt import synth
    cam = synth.bench_camera(radius=2.6, phi_deg=20.0, theta_deg=-35.0) if other_camera else None
    return synth.brats_scene(0, 0, 96, dims=DIMS, image_hw=SHAPES[shape], channels=1, intensity_alpha=16.0, camera=cam)


def ext_of(kind, big):
    from mrirt import synth
    layout, shade = KINDS[kind]
    e = dict(synth.SHADE_EXT) if shade else {}
    return dict(e, layout=layout, kernelVariant=2 if big else 0)


@functools.lru_cache(maxsize=None)
def oracle_steps(shape):
    """per-pixel march steps of the frame (H, W): early termination depends on the opacities alone, so shaded or not"""
    from oracle import oracle_np
    _, aux = oracle_np.brats_main(scene(shape), [volume(), None, None, None], None, None, None, return_aux=True)
    return aux["nsteps"]


class Launch:
    """One configuration's bound arguments and a scratch [order | steps] of exactly mrirt_order_words words each."""

    def __init__(self, shape, kind, big, other_camera=False, ext_extra=None):
        import torch
        from mrirt import _lib, render
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.ext = dict(ext_of(kind, big), **(ext_extra or {}))
        self.params, self.grid = scene(shape, other_camera), grid(KINDS[kind][0])
        self.P, self.E, self.vols, lab, prd, _ = render._bind_brats(self.params, [self.grid], None, None, self.ext, self.dev)
        self.vp = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) if t is not None else None for t in self.vols])
        size = (C.c_uint32 * 2)(int(self.P.imageSize[0]), int(self.P.imageSize[1]))
        self.words = int(_lib.lib().mrirt_order_words(size, C.byref(self.E)))
        self.H, self.W = SHAPES[shape]

    def applicable(self):
        from mrirt import _lib
        return int(_lib.lib().mrirt_brats_order_applicable(C.byref(self.P), C.byref(self.E), self.vp, None, None, None))

    def plain(self):
        import mrirt
        o, st = mrirt.render_brats(self.params, [self.grid], ext=dict(self.ext, order=False), stats=True)
        return o.cpu().numpy(), (st["live_samples"], st["shaded_samples"])

    def ordered(self, scratch, classes):
        """mrirt_render_brats_ordered with scratch = int32 tensor [order | steps]; returns (frame, stats)"""
        import torch
        from mrirt import _lib, render
        words = scratch.numel() // 2
        O = _lib.Order()
        O.order, O.steps, O.words, O.classes = scratch.data_ptr(), scratch.data_ptr() + 4 * words, words, classes
        out = torch.full((self.H, self.W, 4), -7.0, dtype=torch.float32, device=self.dev)
        st = torch.zeros(2, dtype=torch.int64, device=self.dev)
        rc = _lib.lib().mrirt_render_brats_ordered(C.byref(self.P), C.byref(self.E), self.vp, None, None, None, C.byref(O),
                                                   render._ptr(out), self.W, render._ptr(st), render._stream_ptr(None))
        _lib.check(rc, "mrirt_render_brats_ordered")
        s = st.cpu()
        return out.cpu().numpy(), (int(s[0]), int(s[1]))


launch = Launch


def scratch_with(l, table):
    import torch
    t = np.concatenate([np.asarray(table, dtype=np.uint32), np.zeros(l.words, dtype=np.uint32)]).view(np.int32)
    return torch.from_numpy(t.copy()).to(l.dev)


def per_xcd(words, fn):
    """a table that permutes each XCD's slots by fn(n) -> permutation of range(n)"""
    table = np.zeros(words, dtype=np.uint32)
    for x in range(XCDS):
        pos = np.arange(x, words, XCDS, dtype=np.uint32)
        table[pos] = pos[fn(pos.size)]
    return table


CASES = [(s, k, b) for s in SHAPES for k in KINDS for b in (False, True)]


@pytest.mark.parametrize("shape,kind,big", CASES, ids=[f"{s}-{k}-{'16px' if b else '8px'}" for s, k, b in CASES])
def test_any_order_renders_the_same_bits(shape, kind, big):
    l = launch(shape, kind, big)
    assert l.applicable() == 1 and l.words > 0
    block = 16 if big else 8
    assert l.words >= -(-l.W // block) * -(-l.H // block)
    want, want_st = l.plain()
    rng = np.random.default_rng(99)
    tables = {
        "identity": np.arange(l.words, dtype=np.uint32),
        "reversed": per_xcd(l.words, lambda n: np.arange(n)[::-1]),
        "random": per_xcd(l.words, lambda n: rng.permutation(n)),
    }
    for name, table in tables.items():
        got, st = l.ordered(scratch_with(l, table), 0)                # classes 0: the caller's table, no builder
        assert np.array_equal(got, want), name
        assert st == want_st, (name, st, want_st)
    # learned: frame 1 builds from a zero record (identity) and records; frame 2 marches in the learned order
    sc = scratch_with(l, np.full(l.words, 0xFFFFFFFF, dtype=np.uint32))      # the table needs no initial value
    for frame in (1, 2):
        got, st = l.ordered(sc, 4)
        table = sc.cpu().numpy().view(np.uint32)[: l.words]
        assert np.array_equal(np.sort(table), np.arange(l.words, dtype=np.uint32)), frame
        assert np.array_equal(table % XCDS, np.arange(l.words, dtype=np.uint32) % XCDS), frame
        if frame == 1:
            assert np.array_equal(table, np.arange(l.words, dtype=np.uint32))
        else:
            assert not np.array_equal(table, np.arange(l.words, dtype=np.uint32))       # long and short workgroups exist
        assert np.array_equal(got, want) and st == want_st, frame
    # stale: frame 3 is another camera's, dispatched by this camera's record
    other = launch(shape, kind, big, other_camera=True)
    want_o, want_o_st = other.plain()
    assert not np.array_equal(want_o, want)
    got, st = other.ordered(sc, 4)
    assert np.array_equal(got, want_o) and st == want_o_st


def logical_of(b, blocks_x, band_shift):
    """map_logical (csrc/mrirt_device.h) for bands one workgroup row high"""
    xcd, k = b % XCDS, b // XCDS
    j, p = k // blocks_x, k % blocks_x
    return (j * XCDS + xcd) * blocks_x + (p + j * band_shift) % blocks_x


@pytest.mark.parametrize("shape,kind,big", CASES, ids=[f"{s}-{k}-{'16px' if b else '8px'}" for s, k, b in CASES])
def test_step_record_is_the_workgroups_longest_ray(shape, kind, big):
    from mrirt import _lib
    l = launch(shape, kind, big)
    sc = scratch_with(l, np.arange(l.words, dtype=np.uint32))
    l.ordered(sc, 0)
    rec = sc.cpu().numpy().view(np.uint32)[l.words:]
    block = 16 if big else 8
    bx, by = -(-l.W // block), -(-l.H // block)
    steps = oracle_steps(shape)
    padded = np.zeros((by * block, bx * block), dtype=np.int64)
    padded[: l.H, : l.W] = steps
    longest = padded.reshape(by, block, bx, block).max(axis=(1, 3)).reshape(-1)
    shift = 0 if big or bx < 8 else (3 * bx) // 8                   # 8-px workgroups start each band 3/8 of a row along
    want = np.zeros(l.words, dtype=np.uint32)
    for b in range(l.words):
        lg = logical_of(b, bx, shift)
        if lg < bx * by:
            want[b] = longest[lg]
    assert len(np.unique(longest)) > 4                                # the frame has long and short workgroups
    assert np.array_equal(rec, want)
    # ... and the builder kernel's table for this record is the host's (the same header, counted with ballots)
    l.ordered(sc, 4)
    table = sc.cpu().numpy().view(np.uint32)[: l.words]
    host = np.zeros(l.words, dtype=np.uint32)
    assert _lib.lib().mrirt_order_build_host(want.ctypes.data, l.words, 4, host.ctypes.data) == 0
    assert np.array_equal(table, host)
    for classes in (2, 16):
        l.ordered(sc, classes)                                        # (the record is the same frame's again)
        table = sc.cpu().numpy().view(np.uint32)[: l.words]
        assert _lib.lib().mrirt_order_build_host(want.ctypes.data, l.words, classes, host.ctypes.data) == 0
        assert np.array_equal(table, host), classes


def test_tiled_and_skipping_launches_ignore_the_scratch():
    import mrirt
    from mrirt import render, synth
    # tiled: ordering reports off, the table size is 0, and the call renders the plain compact buffer
    l = launch("square", "vga-shaded", False, ext_extra=dict(tileSize=64, tileRank=0, tileWorld=2))
    assert l.applicable() == 0 and l.words == 0
    p, ext = scene("square"), dict(ext_of("vga-shaded", False), tileSize=64, tileRank=0, tileWorld=2)
    before = render.order_binds
    a = mrirt.render_brats(p, [grid("vga")], ext=dict(ext, order=True)).cpu().numpy()
    b = mrirt.render_brats(p, [grid("vga")], ext=dict(ext, order=False)).cpu().numpy()
    assert render.order_binds == before and np.array_equal(a, b)
    # skipping: a launch that marches with an empty-radius map takes no order
    ext = ext_of("vga-shaded", False)
    g = grid("vga")
    builds = render.skip_map_builds
    a, sa = mrirt.render_brats(p, [g], ext=dict(ext, order=True), skip=True, stats=True)
    assert render.skip_map_builds == builds + 1 and render.order_binds == before
    b, sb = mrirt.render_brats(p, [g], ext=dict(ext, order=False), stats=True)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and sa == sb
    # ... while the plain launch of the same frame does, through render_brats's own cache: same bits frame after frame
    for _ in range(3):
        c, sc = mrirt.render_brats(p, [g], ext=dict(ext, order=True), stats=True)
        assert np.array_equal(c.cpu().numpy(), b.cpu().numpy()) and sc == sb
    assert render.order_binds == before + 3
    # an undersized scratch is refused before anything is launched
    l = launch("square", "vga-shaded", False)
    import torch
    from mrirt import _lib
    small = torch.zeros(2 * (l.words - 8), dtype=torch.int32, device=l.dev)
    with pytest.raises(_lib.MrirtError):
        l.ordered(small, 4)
