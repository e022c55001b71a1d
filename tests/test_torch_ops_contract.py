"""The contract of the operator layer, checked without a GPU: ``torch.ops.mrirt.*`` (mrirt/torch_ops.py) and
``torch.ops.mrirt_native.*`` (csrc/torch_binding.cpp) register the same 19 operators with the same schemas, every fake kernel
of the Python door gives the shapes, dtypes and devices written out below, and the refusals that need no device raise the
pinned exception class through each door.

A new operator is added HERE first: its name in NAMES, a meta call with literal output shapes in test_every_fake_kernel, and
its host-side refusals (tests/test_gpu_torch_ops_refusals.py holds the ones that need device tensors).  The expected shapes
are literals on purpose: nothing below is computed with a helper of torch_ops."""
import ctypes as C

import pytest
import torch

import mrirt
from mrirt import _lib, synth, torch_ops

NAMES = ["edt_squared", "hausdorff", "inr_adamw_step", "inr_backward", "inr_forward", "inr_forward_f32", "inr_loss", "inr_loss_ext",
         "inr_sample_batch", "inr_sample_batch_mix", "render_brats", "render_brats_backward", "render_brats_soft",
         "render_brats_soft_backward", "render_mesh", "render_sdf", "render_volume", "surface_count", "surface_extract"]

F16, F32, F64, I32, I64, U8 = torch.float16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
W, H = 8, 6                        # the image
DIMS = (4, 5, 6)                   # the volume: 120 voxels
N = 10                             # points
NET = (0, 3, 16, 4, 32, 2, 1)      # kind 0 (Fourier/ReLU), 3 layers, in 3 + 3 * 2 * 2 + 1, out 4, hidden 32, 2 frequencies, 1 modality


@pytest.fixture(scope="module")
def native():
    _lib.build_torch_binding()
    return torch_ops.load_native()


def meta(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


def _brats(**kw):
    return torch_ops.pack_brats_params(synth.brats_scene(0, 0, 8, dims=DIMS, image_hw=(H, W), **kw))


def _mesh_blob():
    eye, U, V, Wv = synth.bench_camera().get_basis()
    return torch_ops.pack_mesh_params({"imageSize": (W, H), "fovY": 0.8, "eye": eye, "U": U, "V": V, "W": Wv})


def _volume_blob():
    p = synth.volume_scene(0, W, 8, dims=DIMS)
    p["imageSize"] = (W, H)
    return torch_ops.pack_volume_params(p)


def _registered(namespace):
    names = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith(namespace + "::")}
    return sorted(n.split("::")[1] for n in names)


def test_both_doors_register_the_same_operators_with_the_same_schemas(native):
    assert _registered("mrirt") == NAMES
    assert _registered("mrirt_native") == NAMES
    for name in NAMES:
        a = getattr(torch.ops.mrirt, name).default._schema
        b = getattr(native, name).default._schema
        assert [x.name for x in a.arguments] == [x.name for x in b.arguments], name
        assert [str(x.type) for x in a.arguments] == [str(x.type) for x in b.arguments], name
        assert [str(x.type) for x in a.returns] == [str(x.type) for x in b.returns], name


def _is(out, *want):
    """Every output against its literal (shape, dtype); all of them on the meta device."""
    outs = [out] if isinstance(out, torch.Tensor) else list(out)
    assert len(outs) == len(want)
    for o, (shape, dtype) in zip(outs, want):
        assert tuple(o.shape) == shape and o.dtype == dtype and o.device.type == "meta", (tuple(o.shape), o.dtype, o.device, shape, dtype)


def test_every_fake_kernel():
    ops = torch.ops.mrirt
    ext = torch_ops.pack_render_ext
    plain, half = ext(None), ext({"outFormat": "rgba16f"})
    tiled1, tiled0 = ext({"tileSize": 16, "tileRank": 1, "tileWorld": 3}), ext({"tileSize": 4, "tileRank": 0, "tileWorld": 3})
    assert mrirt.tiles.local_tile_count(W, H, 16, 1, 3) == 0 and mrirt.tiles.local_tile_count(W, H, 4, 0, 3) == 2
    vol, lab = meta(120), meta(120, dtype=I32)
    none4 = (None, None, None, None)
    # K1
    one = _brats(channels=1)
    _is(ops.render_brats(one, plain, vol, *none4, None), ((6, 8, 4), F32))
    _is(ops.render_brats(one, half, vol, *none4, None), ((6, 8, 4), F16))
    _is(ops.render_brats(one, tiled1, vol, *none4, None), ((0, 16, 16, 4), F32))
    _is(ops.render_brats(one, tiled0, vol, *none4, None), ((2, 4, 4, 4), F32))
    _is(ops.render_brats(one, ext({"outFormat": "rgba16f", "tileSize": 4, "tileRank": 2, "tileWorld": 3}), vol, *none4, None), ((1, 4, 4, 4), F16))
    # K1 backward: modalities 0..2 enabled; 0 bound, 1 empty, 2 None, 3 bound but disabled
    three = _brats(channels=3, show_seg=True)
    g = meta(6, 8, 4)
    _is(ops.render_brats_backward(three, plain, g, vol, meta(0), None, vol, lab, None),
        ((120,), F32), ((0,), F32), ((0,), F32), ((0,), F32), ((4,), F64))
    _is(ops.render_brats_backward(_brats(channels=4), plain, g, vol, vol, vol, vol, None, None),
        ((120,), F32), ((120,), F32), ((120,), F32), ((120,), F32), ((4,), F64))
    # K1 soft overlay
    z, off = meta(37, 4), meta(48, dtype=I64)
    _is(ops.render_brats_soft(one, plain, z, off, vol, None, None, None, None), ((6, 8, 4), F32))
    _is(ops.render_brats_soft_backward(one, plain, g, z, off, vol, None, None, None, None), ((37, 4), F32))
    # K2, K3, K4
    vb = _volume_blob()
    _is(ops.render_volume(vb, plain, meta(120, dtype=U8), 1), ((6, 8, 4), F32))
    _is(ops.render_volume(vb, half, meta(120, dtype=U8), 1), ((6, 8, 4), F16))
    _is(ops.render_volume(vb, tiled1, meta(120, dtype=I32), 0), ((0, 16, 16, 4), F32))
    _is(ops.render_volume(vb, tiled0, meta(120), 2), ((2, 4, 4, 4), F32))
    sp, eye, U, V, Wv = synth.sdf_scene()
    _is(ops.render_sdf(torch_ops.pack_sdf_params(sp, eye, U, V, Wv), W, H, vol), ((6, 8, 4), F32))
    mesh = (meta(24), meta(8, dtype=I32), meta(16))
    _is(ops.render_mesh(_mesh_blob(), plain, *mesh, 2), ((6, 8, 4), F32))
    _is(ops.render_mesh(_mesh_blob(), half, *mesh, 2), ((6, 8, 4), F16))
    # INR forward (packed bf16 image) and the fp32 training step
    kind, layers, in_dim, out_dim, hidden, freqs, mods = NET
    co, fe = meta(N, 3), meta(N, 1)
    _is(ops.inr_forward(meta(1, dtype=U8), meta(1), kind, layers, in_dim, out_dim, hidden, freqs, mods, 30.0, co, fe, N), ((10, 4), F32))
    d = _lib.InrDesc()
    d.kind, d.numLayers, d.inDim, d.outDim, d.hidden, d.fourierFreqs, d.numMods = NET
    scratch_bytes = int(_lib.lib().mrirt_inr_train_scratch_bytes(C.byref(d), N))
    assert scratch_bytes > 0
    w, b = meta(1664), meta(68)                                  # 16 * 32 + 32 * 32 + 32 * 4 weights, 32 + 32 + 4 biases
    _is(ops.inr_forward_f32(w, b, *NET, co, fe, N), ((10, 4), F32), ((scratch_bytes,), U8))
    _is(ops.inr_backward(w, meta(N, 4), meta(scratch_bytes, dtype=U8), *NET, N), ((1664,), F32), ((68,), F32))
    logits, labels = meta(N, 4), meta(N, dtype=I32)
    _is(ops.inr_loss(logits, labels, [1.0, 2.0, 3.0, 4.0], 0.5), ((1,), F32), ((2, 4), F32), ((10, 4), F32))
    _is(ops.inr_loss_ext(logits, labels, [1.0, 2.0, 3.0, 4.0], [], 0.5, True, 2.0, 0.1, 0.2, 0.3, 0.7, 0.4, 0.01, 2),
        ((1,), F32), ((2, 4), F32), ((5,), F32), ((10, 4), F32))
    # the samplers, with and without modalities
    table = meta(2, dtype=I64)
    for mods_table, m in ((table, 3), (None, 0)):
        want = (((10, 3), F32), ((10, m), F32), ((10,), I32))
        _is(ops.inr_sample_batch(mods_table, table, m, 4, 5, 6, 7, 0, N), *want)
        _is(ops.inr_sample_batch_mix(mods_table, table, meta(9, dtype=I32), meta(3, dtype=I64), m, 4, 5, 6, 7, 0, N, 4), *want)
        _is(ops.inr_sample_batch_mix(mods_table, table, None, None, m, 4, 5, 6, 7, 0, N, 0), *want)
    # AdamW
    out = ops.inr_adamw_step(w, b, w, b, w, b, w, b, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 0, 1.0)
    assert isinstance(out, (list, tuple))
    _is(out, ((1664,), F32), ((68,), F32), ((1664,), F32), ((68,), F32), ((1664,), F32), ((68,), F32), ((2,), F64))
    # label volumes
    lv = meta(4, 5, 6, dtype=torch.int16)
    _is(ops.edt_squared(lv, 1, [1.0, 1.0, 1.0]), ((4, 5, 6), F64))
    _is(ops.hausdorff(lv, lv, [1.0, 1.0, 1.0], 4), ((4, 2), F64))
    _is(ops.surface_count(lv, 2), ((2,), I64))
    _is(ops.surface_extract(lv, 2, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], 11, 22), ((11, 3), F32), ((22, 3), I32))


def test_refusals_that_need_no_gpu_through_both_doors(native):
    """Each door's exception class is a literal.  Nothing here can reach a device: there is none."""
    plain = torch_ops.pack_render_ext(None)
    one = _brats(channels=1)
    host, host_i32 = torch.zeros(120), torch.zeros(120, dtype=I32)
    sp, eye, U, V, Wv = synth.sdf_scene()
    none4 = (None, None, None, None)
    for door, ops, short_blob, host_tensor, unbound in (("mrirt", torch.ops.mrirt, TypeError, TypeError, ValueError),
                                                        ("mrirt_native", native, TypeError, TypeError, ValueError)):
        # a parameter blob (or the ext blob) one byte short
        for call in (lambda: ops.render_brats(one[:-1], plain, host, *none4, None),
                     lambda: ops.render_brats(one, plain[:-1], host, *none4, None),
                     lambda: ops.render_brats_backward(one[:-1], plain, host, host, *none4, None),
                     lambda: ops.render_brats_soft(one[:-1], plain, host, host, host, *none4),
                     lambda: ops.render_brats_soft_backward(one[:-1], plain, host, host, host, host, *none4),
                     lambda: ops.render_volume(_volume_blob()[:-1], plain, host, 2),
                     lambda: ops.render_sdf(torch_ops.pack_sdf_params(sp, eye, U, V, Wv)[:-1], W, H, host),
                     lambda: ops.render_mesh(_mesh_blob()[:-1], plain, host, host_i32, host, 2)):
            with pytest.raises(short_blob):
                call()
        # a host tensor where a device tensor is required
        for call in (lambda: ops.render_brats(one, plain, host, *none4, None),
                     lambda: ops.render_brats_backward(one, plain, torch.zeros(H, W, 4), host, *none4, None),
                     lambda: ops.render_brats_soft(one, plain, torch.zeros(37, 4), torch.zeros(48, dtype=I64), host, *none4),
                     lambda: ops.render_volume(_volume_blob(), plain, host, 2),
                     lambda: ops.render_sdf(torch_ops.pack_sdf_params(sp, eye, U, V, Wv), W, H, host),
                     lambda: ops.render_mesh(_mesh_blob(), plain, host, host_i32, host, 2),
                     lambda: ops.inr_loss(torch.zeros(N, 4), torch.zeros(N, dtype=I32), [1.0] * 4, 0.5),
                     lambda: ops.inr_sample_batch(None, torch.zeros(2, dtype=I64), 0, 4, 5, 6, 7, 0, N),
                     lambda: ops.edt_squared(torch.zeros(DIMS, dtype=torch.int16), 1, [1.0, 1.0, 1.0]),
                     lambda: ops.surface_count(torch.zeros(DIMS, dtype=torch.int16), 2)):
            with pytest.raises(host_tensor):
                call()
        # an enabled modality bound as None
        with pytest.raises(unbound):
            ops.render_brats(one, plain, None, *none4, None)


def test_operands_on_different_devices_are_refused():
    """Through the operators this needs two GPUs (the device-tensor check comes first; tests/test_gpu_torch_ops_refusals.py does it
    where there are two); the Python door's check itself runs on any two torch devices."""
    a, b = torch.empty(1, device="meta"), torch.empty(1)
    assert torch_ops._one_device([("x", a), ("y", None), ("z", a)]) == a.device
    with pytest.raises(ValueError, match="same GPU"):
        torch_ops._one_device([("x", a), ("y", b)])
    with pytest.raises(ValueError):
        torch_ops._one_device([("x", None)])
