"""mrirt_render_brats_tf on the GPU (csrc/brats_tf.hip), through the C ABI unless noted.

  a  the two-entry ramp, STRICT: every layout x shading the matrix allows x label layouts (LABCELL with QUAD and MOD4) x both
     workgroup shapes; frame and counters == mrirt_render_brats_ex == the oracle.
  b  the ramp, FAST: every layout within the project's 2e-6 bar against the oracle (scenes without early termination).
  c  general tables, STRICT: every case on every layout it allows: frame, live and shaded counts == tf_ref; the table between NaN
     guard blocks; the output pre-filled with 0x00 and with 0xFF; guard rows behind the frame; rgba16f == the fp32 frame rounded;
     kernelVariant bits 1 and 2.
  d  general tables, FAST: the two low-opacity cases within tf_cases.TOL_FAST of tf_ref.
  p  pipelined vs generic: every launch that selects a pipelined table kernel == the same call with kernelVariant bit 2.
  e  tile mode: 56 x 40, tile 16, worlds 3 and 16 (ranks 12..15 own nothing) with balanced_skew; detile == the whole frame.
  f  bindings: render_brats(tf=...), the shim with gTransfer, BraTSViewer.set_transfer("hot") == the ABI frame; tf=None and a shim
     without gTransfer == today's frames.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import tf_cases as TC
import tf_ref

pytestmark = pytest.mark.gpu

OK = 0
LAYOUTS = ("linear", "brick", "vg", "vga", "quad", "mod4")
UNSHADED_ONLY = ("quad", "mod4")
GUARD = 64                       # floats on either side of the table (256 B: the table stays 16-byte aligned)
FLIP, GENERIC = 2, 4             # kernelVariant bit 1 (workgroup shape), bit 2 (the generic table kernel)


def _layouts(c):
    return [l for l in LAYOUTS if not (c["shade"] and l in UNSHADED_ONLY)]


def _pairs(names):
    """(case, layout) for every layout the case's shading allows."""
    return [(n, l) for n in names for l in _layouts(TC.BY_NAME[n])]


def _label_layouts(c, layout):
    if c["overlays"] == "off":
        return ["linear"]
    return ["linear", "brick"] + (["labcell"] if layout in UNSHADED_ONLY else [])


@functools.lru_cache(maxsize=None)
def _grids(name, layout):
    """The case's intensity grids in one layout: four bound slots (Grid | None)."""
    import mrirt
    c, d = TC.BY_NAME[name], TC.data(name)
    if layout == "mod4":
        return [mrirt.upload_mod4(d["vols"], c["dims"], macro=False)] * 4
    return [None if v is None else mrirt.upload_grid(v, c["dims"], layout, macro=False) for v in d["vols"]]


@functools.lru_cache(maxsize=None)
def _labels(name, lab_layout):
    import mrirt
    c, d = TC.BY_NAME[name], TC.data(name)
    if lab_layout == "labcell":
        return mrirt.upload_label_cells(d["labels"], d["preds"], c["dims"], macro=False), None
    return tuple(None if a is None else mrirt.upload_grid(a.astype(np.int64), c["dims"], lab_layout, macro=False) for a in (d["labels"], d["preds"]))


@functools.lru_cache(maxsize=None)
def _table(key):
    """(device buffer [NaN guard | table | NaN guard], the table's device pointer, N)."""
    import torch
    t = TC.TABLES[key]
    buf = torch.full((2 * GUARD + t.size,), float("nan"), dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + t.size] = torch.from_numpy(t.reshape(-1).copy()).cuda()
    assert (buf.data_ptr() + 4 * GUARD) % 16 == 0
    return buf, buf.data_ptr() + 4 * GUARD, t.shape[0]


def _render(c, layout, lab_layout, *, table=None, variant=0, math="strict", half=False, fill=None, params=None, extra_ext=None):
    """One call of mrirt_render_brats_tf (table = a key of TC.TABLES) or mrirt_render_brats_ex (table None) on the case's grids.
    -> (frame as numpy, live, shaded).  The output has two guard rows behind the frame, checked here."""
    import torch
    from mrirt import _lib, params as mp
    name = c["name"]
    p = params or c["params"]
    P = mp.brats_params(p)
    e = dict(c["ext"], layout=layout, labelLayout=lab_layout, kernelVariant=variant, math=math, outFormat="rgba16f" if half else "rgba32f")
    e.update(extra_ext or {})
    E = mp.render_ext(e)
    vols = _grids(name, layout)
    lab, prd = _labels(name, lab_layout)
    vp = (C.c_void_p * 4)(*[C.c_void_p(g.data.data_ptr()) if g is not None else None for g in vols])
    lp = C.c_void_p(lab.data.data_ptr()) if lab is not None else None
    pp = C.c_void_p(prd.data.data_ptr()) if prd is not None else None
    Wd, Hd = int(p["imageSize"][0]), int(p["imageSize"][1])
    dt = torch.float16 if half else torch.float32
    out = torch.empty((Hd + 2, Wd, 4), dtype=dt, device="cuda")
    out.view(torch.uint8).fill_(0xFF if fill is None else fill)
    before = out[Hd:].clone()
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if table is None:
        rc = lib.mrirt_render_brats_ex(C.byref(P), C.byref(E), vp, lp, pp, C.c_void_p(out.data_ptr()), Wd, C.c_void_p(st.data_ptr()), stream)
    else:
        buf, ptr, n = _table(table)
        rc = lib.mrirt_render_brats_tf(C.byref(P), C.byref(E), vp, lp, pp, C.c_void_p(ptr), n, C.c_void_p(out.data_ptr()), Wd,
                                       C.c_void_p(st.data_ptr()), stream)
    assert rc == OK, (name, layout, lab_layout, table, rc)
    s = st.cpu()
    assert torch.equal(out[Hd:].view(torch.uint8), before.view(torch.uint8)), "the rows behind the frame were written"
    if table is not None:
        g = _table(table)[0]
        assert bool(torch.isnan(g[:GUARD]).all()) and bool(torch.isnan(g[-GUARD:]).all())
    return out[:Hd].cpu().numpy(), int(s[0]), int(s[1])


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import oracle_np as onp
    c, d = TC.BY_NAME[name], TC.data(name)
    frame, aux = onp.brats_main(c["params"], d["vols"], d["labels"], d["preds"], c["ext"], return_aux=True)
    frame.setflags(write=False)
    return dict(frame=frame, live=aux["live_samples"], shaded=aux["shaded_samples"])


# ----------------------------------------------------------------------------------------------------------------------
# a, b: the ramp
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout", _pairs(TC.RAMP_NAMES))
def test_ramp_strict_is_the_plain_render_and_the_oracle(name, layout):
    c = TC.BY_NAME[name]
    want = _oracle(name)
    for lab_layout in _label_layouts(c, layout):
        for variant in (0, FLIP):
            what = f"{name} {layout} labels {lab_layout} variant {variant}"
            plain = _render(c, layout, lab_layout, variant=variant)
            got = _render(c, layout, lab_layout, table="ramp", variant=variant)
            assert tf_ref.compare(plain[0], plain[1], plain[2], want) == [], what + " (mrirt_render_brats_ex)"
            assert tf_ref.compare(got[0], got[1], got[2], want) == [], what
            assert np.all(got[0][..., 3] == 1)


@pytest.mark.parametrize("name,layout", _pairs(TC.RAMP_FAST_CASES))
def test_ramp_fast_within_the_projects_bar(name, layout):
    c = TC.BY_NAME[name]
    want = _oracle(name)
    for lab_layout in _label_layouts(c, layout):
        frame, live, shaded = _render(c, layout, lab_layout, table="ramp", math="fast")
        err = float(np.abs(frame.astype(np.float64) - want["frame"]).max())
        print(f"{name} {layout} labels {lab_layout}: FAST max |frame - oracle| = {err:.3e} (bar {TC.RAMP_FAST_BAR:.1e})")
        assert err <= TC.RAMP_FAST_BAR and live == want["live"]


# ----------------------------------------------------------------------------------------------------------------------
# c, d: general tables
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout", _pairs(TC.GENERAL_NAMES))
def test_general_table_strict(name, layout):
    c = TC.BY_NAME[name]
    want = TC.reference(name)
    half = want["frame"].astype(np.float16)
    for lab_layout in _label_layouts(c, layout):
        what = f"{name} {layout} labels {lab_layout}"
        zero = _render(c, layout, lab_layout, table=c["table"], fill=0x00)
        ones = _render(c, layout, lab_layout, table=c["table"], fill=0xFF, variant=FLIP)
        generic = _render(c, layout, lab_layout, table=c["table"], fill=0xFF, variant=GENERIC)
        for got, how in ((zero, "output 0x00"), (ones, "output 0xFF, 256-thread workgroups"), (generic, "kernelVariant bit 2")):
            assert tf_ref.compare(got[0], got[1], got[2], want) == [], f"{what} ({how})"
            assert np.all(got[0][..., 3] == 1)
        f16, live, shaded = _render(c, layout, lab_layout, table=c["table"], half=True)
        assert f16.dtype == np.float16 and np.array_equal(f16.view(np.uint16), half.view(np.uint16)), what + " (rgba16f)"
        assert (live, shaded) == (want["live"], want["shaded"])


@pytest.mark.parametrize("name,layout", _pairs(TC.FAST_CASES))
def test_general_table_fast(name, layout):
    c = TC.BY_NAME[name]
    want = TC.reference(name)
    frame, live, shaded = _render(c, layout, _label_layouts(c, layout)[-1], table=c["table"], math="fast")
    err = float(np.abs(frame.astype(np.float64) - want["frame"]).max())
    print(f"{name} {layout}: FAST max |frame - tf_ref| = {err:.3e} (tolerance {TC.TOL_FAST:.3e})")
    assert err <= TC.TOL_FAST
    assert (live, shaded) == (want["live"], want["shaded"])


def _selects_pipelined(c, layout, lab_layout, math):
    """The launches brats_tf.hip gives to a pipelined table kernel (restated from its selection): MOD4 unshaded with overlays off
    or through label cells; VGA shaded, one modality, no overlays; STRICT only for gamma == 1."""
    p = c["params"]
    if math == "strict" and float(p["gamma"]) != 1.0:
        return False
    if layout == "mod4":
        return not c["shade"] and (c["overlays"] == "off" or lab_layout == "labcell")
    return layout == "vga" and c["shade"] and sum(int(v) != 0 for v in p["volEnabled"]) == 1 and c["overlays"] == "off"


PIPELINED = [(n, l, ll, m) for n in TC.NAMES for l in ("mod4", "vga") if l in _layouts(TC.BY_NAME[n])
             for ll in _label_layouts(TC.BY_NAME[n], l) for m in ("strict", "fast") if _selects_pipelined(TC.BY_NAME[n], l, ll, m)]


def test_pipelined_selection_is_covered():
    strict = [(n, l, ll) for n, l, ll, m in PIPELINED if m == "strict"]
    assert {l for _, l, _ in strict} == {"mod4", "vga"} and any(ll == "labcell" for _, _, ll in strict)
    assert any(TC.BY_NAME[n]["dense"] for n, _, _ in strict) and any(TC.BY_NAME[n]["table"] == "n1024" for n, _, _ in strict)
    assert len(strict) >= 10, strict


@pytest.mark.parametrize("name,layout,lab_layout,math", PIPELINED)
def test_pipelined_equals_generic(name, layout, lab_layout, math):
    """Every launch that selects a pipelined table kernel: the default call == the same call with kernelVariant bit 2 (the
    generic table kernel), frame bits and counters, in both workgroup shapes."""
    c = TC.BY_NAME[name]
    for flip in (0, FLIP):
        default = _render(c, layout, lab_layout, table=c["table"], math=math, variant=flip)
        generic = _render(c, layout, lab_layout, table=c["table"], math=math, variant=flip | GENERIC)
        assert np.array_equal(default[0].view(np.uint32), generic[0].view(np.uint32)) and default[1:] == generic[1:], (name, layout, lab_layout, math, flip)
        if math == "strict":
            want = TC.reference(name)
            assert tf_ref.compare(default[0], default[1], default[2], want) == []


def test_refusals_on_the_device():
    """With real grids bound: shading on QUAD / MOD4 grids is MRIRT_ERR_LAYOUT and the output stays untouched."""
    import torch
    from mrirt import _lib, params as mp
    c = TC.BY_NAME["n256_shaded"]
    for layout in UNSHADED_ONLY:
        vols = _grids(c["name"], layout)
        P, E = mp.brats_params(c["params"]), mp.render_ext(dict(c["ext"], layout=layout))
        vp = (C.c_void_p * 4)(*[C.c_void_p(g.data.data_ptr()) if g is not None else None for g in vols])
        out = torch.full((20, 24, 4), float("nan"), device="cuda")
        _, ptr, n = _table("n256")
        rc = _lib.lib().mrirt_render_brats_tf(C.byref(P), C.byref(E), vp, None, None, C.c_void_p(ptr), n, C.c_void_p(out.data_ptr()), 24, None, None)
        torch.cuda.synchronize()
        assert rc == -3 and bool(torch.isnan(out).all()), layout


# ----------------------------------------------------------------------------------------------------------------------
# e: tile mode
# ----------------------------------------------------------------------------------------------------------------------
TILE_W, TILE_H, TILE = 56, 40, 16


@functools.lru_cache(maxsize=None)
def _tile_scene(gamma):
    c = TC.BY_NAME["n17_four_dense_overlays"]
    d = TC.data(c["name"])
    p = dict(c["params"], imageSize=[TILE_W, TILE_H], gamma=gamma)
    ref = tf_ref.march(p, d["vols"], d["labels"], d["preds"], c["ext"], TC.TABLES["n17"])
    return c, p, ref


@pytest.mark.parametrize("world", [3, 16])
@pytest.mark.parametrize("layout,lab_layout,gamma", [("vga", "brick", 2.2), ("mod4", "labcell", 2.2), ("mod4", "labcell", 1.0)])
def test_tiles_detile_to_the_whole_frame(layout, lab_layout, gamma, world):
    """(gamma 2.2: the generic table kernel; gamma 1 on MOD4 + label cells: the pipelined one)"""
    import torch
    import mrirt
    from mrirt import tiles
    c, p, ref = _tile_scene(gamma)
    whole = _render(c, layout, lab_layout, table="n17", params=p)
    assert tf_ref.compare(whole[0], whole[1], whole[2], ref) == []
    skew = tiles.balanced_skew(TILE_W, TILE, world)
    n_tiles = tiles.num_tiles(TILE_W, TILE_H, TILE)
    max_local = tiles.local_tile_count(TILE_W, TILE_H, TILE, 0, world)
    gathered = torch.full((world, max_local, TILE, TILE, 4), float("nan"), device="cuda")
    live = shaded = 0
    vols, (lab, prd) = _grids(c["name"], layout), _labels(c["name"], lab_layout)
    for rank in range(world):
        n = tiles.local_tile_count(TILE_W, TILE_H, TILE, rank, world)
        ext = tiles.shard_ext(dict(c["ext"]), rank, world, TILE, skew)
        local, st = mrirt.render_brats(p, vols, lab, prd, ext=ext, stats=True, tf=TC.TABLES["n17"])
        assert tuple(local.shape) == (n, TILE, TILE, 4)
        if rank >= n_tiles:
            assert n == 0 and st == {"live_samples": 0, "shaded_samples": 0}
        gathered[rank, :n] = local
        live, shaded = live + st["live_samples"], shaded + st["shaded_samples"]
    frame = mrirt.detile(gathered, TILE_W, TILE_H, TILE, world, skew=skew).cpu().numpy()
    assert tf_ref.compare(frame, live, shaded, ref) == [], f"{layout} world {world} skew {skew}"


# ----------------------------------------------------------------------------------------------------------------------
# f: bindings
# ----------------------------------------------------------------------------------------------------------------------
def test_render_brats_binding():
    import torch
    import mrirt
    name = "n17_four_dense_overlays"
    c, d = TC.BY_NAME[name], TC.data(name)
    abi = _render(c, "linear", "linear", table="n17")
    lin = [None if v is None else torch.from_numpy(v.copy()).cuda() for v in d["vols"]]
    lab, prd = (torch.from_numpy(a.astype(np.int32)).cuda() for a in (d["labels"], d["preds"]))
    for table in (TC.TABLES["n17"], torch.from_numpy(TC.TABLES["n17"].copy()).cuda(), TC.TABLES["n17"].astype(np.float64)):
        frame, st = mrirt.render_brats(c["params"], lin, lab, prd, ext=c["ext"], stats=True, tf=table)
        assert np.array_equal(frame.cpu().numpy(), abi[0]) and (st["live_samples"], st["shaded_samples"]) == abi[1:]
    # Grid objects in another layout, an `order` entry in ext (not used with a table)
    frame = mrirt.render_brats(c["params"], _grids(name, "mod4"), *_labels(name, "labcell"), ext=dict(c["ext"], order=True), tf=mrirt.tf_from_points(
        [(i / 16, *row) for i, row in enumerate(TC.TABLES["n17"].astype(np.float64))], 17))
    assert np.array_equal(frame.cpu().numpy(), abi[0])
    # tf=None is today's path: the plain frame
    plain = _render(c, "linear", "linear")
    frame, st = mrirt.render_brats(c["params"], lin, lab, prd, ext=c["ext"], stats=True, tf=None)
    assert np.array_equal(frame.cpu().numpy(), plain[0]) and (st["live_samples"], st["shaded_samples"]) == plain[1:]
    assert not np.array_equal(plain[0], abi[0])
    with pytest.raises(ValueError, match="skip"):
        mrirt.render_brats(c["params"], _grids(name, "mod4"), *_labels(name, "labcell"), ext=c["ext"], skip=True, tf=TC.TABLES["n17"])
    for bad in (np.zeros((1, 4), np.float32), np.zeros((1025, 4), np.float32), np.zeros((4, 3), np.float32), np.zeros(8, np.float32)):
        with pytest.raises(ValueError):
            mrirt.render_brats(c["params"], lin, lab, prd, ext=c["ext"], tf=bad)


def test_shim_binding():
    from mrirt import shim
    name = "n17_four_dense_overlays"
    c, d = TC.BY_NAME[name], TC.data(name)
    with_table = _render(c, "linear", "linear", table="n17")[0]
    plain = _render(c, "linear", "linear")[0]
    Wd, Hd = c["params"]["imageSize"]
    for layout in ("auto", "linear"):
        ks = shim.KernelShim("brats_main", layout=layout)
        dev = ks.device
        bufs = {f"gIntensity{m}": shim.Buffer.from_numpy(dev, v) for m, v in enumerate(d["vols"])}
        bufs["gLabels"], bufs["gPreds"] = shim.Buffer.from_numpy(dev, d["labels"]), shim.Buffer.from_numpy(dev, d["preds"])
        tex = dev.create_texture(shim.Format.rgba32_float, Wd, Hd)
        bound = dict(bufs, gOutput=tex, gParams=c["params"])
        ks.dispatch([Wd, Hd, 1], dict(bound, gTransfer=shim.Buffer.from_numpy(dev, TC.TABLES["n17"])), ext=c["ext"])
        assert np.array_equal(tex.to_numpy(), with_table), layout
        ks.dispatch([Wd, Hd, 1], dict(bound, gTransfer=TC.TABLES["n17"].reshape(-1).copy()), ext=c["ext"])
        assert np.array_equal(tex.to_numpy(), with_table), layout
        ks.dispatch([Wd, Hd, 1], bound, ext=c["ext"])                         # no gTransfer: unchanged
        assert np.array_equal(tex.to_numpy(), plain), layout
        with pytest.raises(KeyError):
            ks.dispatch([Wd, Hd, 1], dict(bound, gTable=TC.TABLES["n17"]), ext=c["ext"])


def test_viewer_set_transfer():
    import torch
    import mrirt
    from mrirt.viewer import BraTSViewer, MOD_ORDER
    rng = np.random.default_rng(7)
    dims = (16, 12, 10)
    mods = {k: rng.uniform(0.0, 1000.0, dims).astype(np.float32) for k in MOD_ORDER}
    seg = rng.integers(0, 5, dims).astype(np.float32)
    v = BraTSViewer(up="Z")
    v.load_arrays(mods, (1.0, 1.0, 1.0), seg)
    v.camera.orbit(0.4, -0.3)
    v.intensity_alpha = 6.0
    today = v.render(48, 40).to_numpy().copy()

    def direct(table):
        lin = [v.buffers[k].tensor for k in MOD_ORDER]
        return mrirt.render_brats(v.params(48, 40), lin, v.seg_buffer.tensor, None, ext={"outFormat": "rgba16f"}, tf=table).cpu().numpy()

    assert np.array_equal(today, direct(None))
    v.set_transfer("hot")
    hot = v.render(48, 40).to_numpy().copy()
    assert hot.dtype == np.float16 and np.array_equal(hot, direct(mrirt.tf_preset("hot")))
    assert float(np.abs(hot.astype(np.float32) - today.astype(np.float32)).max()) >= 1e-2
    v.set_transfer(TC.TABLES["n17"])
    assert np.array_equal(v.render(48, 40).to_numpy(), direct(TC.TABLES["n17"]))
    v.set_transfer(None)
    assert np.array_equal(v.render(48, 40).to_numpy(), today)
    assert np.array_equal(BraTSViewer(up="Z", tf="gray").transfer_buffer.to_numpy().reshape(-1, 4), mrirt.tf_ramp(256))
    with pytest.raises(ValueError):
        v.set_transfer(np.zeros((3, 3), np.float32))
    assert isinstance(v.buffers[MOD_ORDER[0]].tensor, torch.Tensor)
