"""Both operator doors on the device: ``torch.ops.mrirt.*`` (mrirt/torch_ops.py) and ``torch.ops.mrirt_native.*``
(csrc/torch_binding.cpp).  One valid tiny call per operator succeeds through both and gives ``torch.equal`` results; then one
operand at a time is spoiled in a way the operator layer itself refuses on the host before any launch, and each door raises
its pinned exception class.

Only sizes, shapes and scalar arguments are spoiled — things the layer checks.  Nothing the layer cannot see (the contents of
``offsets``, of the address tables, of a BVH) is ever wrong here: a case of this file must not be able to reach the device
with bad arguments.  tests/test_torch_ops_contract.py holds the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

from mesh_cases import params as mesh_params

pytestmark = pytest.mark.gpu

N = 64                              # points
NET = (0, 3, 16, 4, 32, 2, 1)       # kind 0 (Fourier/ReLU), 3 layers, in 3 + 3 * 2 * 2 + 1, out 4, hidden 32, 2 frequencies, 1 modality
NW, NB = 16 * 32 + 32 * 32 + 32 * 4, 32 + 32 + 4
HWD = (6, 5, 4)                     # label volumes and the sampler's cases


def build_calls():
    """name -> (operator, arguments) of the valid tiny calls, and both doors (tools/torch_ops_host_cost.py times some of them)."""
    import mrirt
    from mrirt import _lib, inr, params, synth, torch_ops
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    calls = {}
    # K1: 8^3 voxels, 8 x 8 pixels, step 0.05
    n, dims = 8, (8, 8, 8)
    lib = _lib.lib()
    cdims = (C.c_uint32 * 3)(*dims)
    vols = [synth.synth_volume(n, 1234 + m, phase=0.3 * m) for m in range(4)]
    lab_np, pred_np = synth.synth_labels(n), np.roll(synth.synth_labels(n), 3)
    lab = torch.from_numpy(lab_np.astype(np.int32)).to(dev)
    prd = torch.from_numpy(pred_np.astype(np.int32)).to(dev)
    p1 = dict(synth.brats_scene(n, 8, 64, channels=1, show_seg=True, intensity_alpha=8.0), stepSize=0.05)
    p4 = dict(synth.brats_scene(n, 8, 64, channels=4, show_seg=True, show_pred=True, intensity_alpha=4.0), stepSize=0.05)
    blob1, blob4 = torch_ops.pack_brats_params(p1), torch_ops.pack_brats_params(p4)
    ext = torch_ops.pack_render_ext
    lin = mrirt.upload_grid(vols[0], dims, "linear").data
    vga = mrirt.upload_grid(vols[0], dims, "vga").data
    quad = mrirt.upload_grid(vols[0], dims, "quad").data
    mod4 = mrirt.upload_mod4(vols, dims).data
    cells = mrirt.upload_label_cells(lab_np, pred_np, dims).data
    # "one element short" below means short of exactly what the layout needs
    assert lin.numel() == 512 and vga.numel() == 4 * lib.mrirt_vga_elems(cdims) and mod4.numel() == 4 * lib.mrirt_vec4_elems(cdims)
    assert cells.numel() == 2 * lib.mrirt_vec4_elems(cdims) and cells.dtype == torch.int32
    none3 = (None, None, None)
    calls["render_brats[linear]"] = ("render_brats", (blob1, ext(None), lin, *none3, lab, None))
    calls["render_brats[vga]"] = ("render_brats", (blob1, ext(dict(synth.SHADE_EXT, layout="vga")), vga, *none3, lab, None))
    calls["render_brats[mod4]"] = ("render_brats", (blob4, ext(dict(layout="mod4", labelLayout="labcell")), mod4, *none3, cells, None))
    calls["render_brats[labcell]"] = ("render_brats", (torch_ops.pack_brats_params(dict(p1, showPred=1)),
                                                      ext(dict(layout="quad", labelLayout="labcell")), quad, *none3, cells, None))
    G = torch.from_numpy(rng.standard_normal((8, 8, 4)).astype(np.float32)).to(dev)
    p2 = dict(synth.brats_scene(n, 8, 64, channels=2, show_seg=True, show_pred=True, intensity_alpha=8.0), stepSize=0.05)
    lin1 = torch.from_numpy(vols[1]).reshape(-1).to(dev)
    calls["render_brats_backward"] = ("render_brats_backward", (torch_ops.pack_brats_params(p2), ext(None), G, lin, lin1, None, None, lab, prd))
    # the soft overlay: the rows are the library's own sample counts for this very frame
    P, E = params.brats_params(p1), params.render_ext(None)
    counts = torch.empty(64, dtype=torch.int32, device=dev)
    _lib.check(lib.mrirt_brats_sample_counts(C.byref(P), C.byref(E), C.c_void_p(counts.data_ptr()), None), "mrirt_brats_sample_counts")
    ends = torch.cumsum(counts.to(torch.int64), 0)
    offsets = (ends - counts).contiguous()
    rows = max(int(ends[-1]), 1)
    z = torch.from_numpy(rng.standard_normal((rows, 4)).astype(np.float32)).to(dev)
    calls["render_brats_soft"] = ("render_brats_soft", (blob1, ext(None), z, offsets, lin, *none3, lab))
    calls["render_brats_soft_backward"] = ("render_brats_soft_backward", (blob1, ext(None), G, z, offsets, lin, *none3, lab))
    # K2, K3, K4
    u8 = torch.from_numpy(synth.synth_u8_volume(n).reshape(-1).copy()).to(dev)
    calls["render_volume"] = ("render_volume", (torch_ops.pack_volume_params(synth.volume_scene(n, 8, 8)), ext(None), u8, 1))
    sp, eye, U, V, W = synth.sdf_scene()
    calls["render_sdf"] = ("render_sdf", (torch_ops.pack_sdf_params(sp, eye, U, V, W), 8, 8, u8))
    quad_v = np.array([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.5, 0.5, 0.0], [-0.5, 0.5, 0.0]], np.float32)
    dm = mrirt.upload_mesh(mrirt.build_bvh(quad_v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)))
    calls["render_mesh"] = ("render_mesh", (torch_ops.pack_mesh_params(mesh_params("outside", 8, 8)), ext(None), dm.nodes, dm.tris, dm.verts, dm.depth))
    # INR: Fourier/ReLU, 3 layers, hidden 32, 4 classes
    widths = [16, 32, 32, 4]
    layers = [{"W": (rng.standard_normal((widths[i], widths[i + 1])) * 0.3).astype(np.float32),
               "b": (rng.standard_normal(widths[i + 1]) * 0.1).astype(np.float32)} for i in range(3)]
    net = inr.pack_mlp(layers, inr.KIND_FOURIER_RELU, 2, 1)
    co = (torch.rand((N, 3), device=dev) * 2 - 1).contiguous()
    fe = torch.rand((N, 1), device=dev).contiguous()
    calls["inr_forward"] = ("inr_forward", (net.weights, net.biases, *NET, 30.0, co, fe, N))
    w = torch.from_numpy(np.concatenate([l["W"].reshape(-1) for l in layers])).to(dev)
    b = torch.from_numpy(np.concatenate([l["b"] for l in layers])).to(dev)
    assert w.numel() == NW and b.numel() == NB
    calls["inr_forward_f32"] = ("inr_forward_f32", (w, b, *NET, co, fe, N))
    logits, scratch = torch.ops.mrirt.inr_forward_f32(w, b, *NET, co, fe, N)
    labels = torch.from_numpy(rng.integers(0, 4, N).astype(np.int32)).to(dev)
    cw = [1.0, 2.0, 3.0, 4.0]
    calls["inr_loss"] = ("inr_loss", (logits, labels, cw, 0.5))
    calls["inr_loss_ext"] = ("inr_loss_ext", (logits, labels, cw, [0.25, 0.5, 0.75, 1.0], 0.5, True, 2.0, 0.1, 0.2, 0.3, 0.7, 0.4, 0.01, 2))
    dl = torch.ops.mrirt.inr_loss(logits, labels, cw, 0.5)[2]
    calls["inr_backward"] = ("inr_backward", (w, dl, scratch, *NET, N))
    # the samplers: 2 cases
    cs = [{"mods": rng.random((1, *HWD)).astype(np.float32), "seg": rng.integers(0, 4, HWD).astype(np.int16)} for _ in range(2)]
    cache = inr.VoxelCache(cs)
    cache.tumour_index()
    assert cache.tumour_offsets.numel() == 3
    calls["inr_sample_batch"] = ("inr_sample_batch", (cache.mods_table, cache.seg_table, 1, *HWD, 7, 3, N))
    calls["inr_sample_batch_mix"] = ("inr_sample_batch_mix", (cache.mods_table, cache.seg_table, cache.tumour_voxels, cache.tumour_offsets, 1, *HWD,
                                                              7, 3, N, 16))
    # AdamW
    gw, gb = (torch.from_numpy(rng.standard_normal(k).astype(np.float32)).to(dev) for k in (NW, NB))
    zw, zb = torch.zeros(NW, device=dev), torch.zeros(NB, device=dev)
    calls["inr_adamw_step"] = ("inr_adamw_step", (w, b, gw, gb, zw, zb, zw, zb, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 0, 1.0))
    # label volumes 6 x 5 x 4, every class present in both (no NaN rows)
    k = np.arange(120)
    pred = torch.from_numpy((k % 4).astype(np.int16).reshape(HWD)).to(dev)
    truth = torch.from_numpy(((k // 2) % 4).astype(np.int16).reshape(HWD)).to(dev)
    calls["edt_squared"] = ("edt_squared", (pred, 1, [1.0, 1.5, 2.0]))
    calls["hausdorff"] = ("hausdorff", (pred, truth, [1.0, 1.5, 2.0], 4))
    block = torch.zeros(HWD, dtype=torch.int16, device=dev)
    block[1:4, 1:4, 1:3] = 2                                   # one small box: its surface fits the static sizes below
    calls["surface_count"] = ("surface_count", (block, 0b0100))
    calls["surface_extract"] = ("surface_extract", (block, 0b0100, [1.0, 1.5, 2.0], [0.0, 0.0, 0.0], 256, 512))
    return dict(calls=calls, doors=(("mrirt", torch.ops.mrirt), ("mrirt_native", torch_ops.load_native())), keep=(cache, dm, net))


@pytest.fixture(scope="module")
def env():
    return build_calls()                # once; the tensors are shared and never written


VALID = ["render_brats[linear]", "render_brats[vga]", "render_brats[mod4]", "render_brats[labcell]", "render_brats_backward", "render_brats_soft",
         "render_brats_soft_backward", "render_volume", "render_sdf", "render_mesh", "inr_forward", "inr_forward_f32", "inr_loss", "inr_loss_ext",
         "inr_backward", "inr_sample_batch", "inr_sample_batch_mix", "inr_adamw_step", "edt_squared", "hausdorff", "surface_count",
         "surface_extract"]


def _outputs(out):
    return [out] if isinstance(out, torch.Tensor) else list(out)


@pytest.mark.parametrize("name", VALID)
def test_the_valid_call_gives_equal_results_through_both_doors(env, name):
    op, args = env["calls"][name]
    (_, py), (_, native) = env["doors"]
    a, b = _outputs(getattr(py, op)(*args)), _outputs(getattr(native, op)(*args))
    assert len(a) == len(b)
    if op == "inr_forward_f32":             # [1] is the activations' scratch: its padding is never written (inr_backward reads what is)
        a, b = a[:1], b[:1]
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device and torch.equal(x, y), name
    if op == "surface_extract":             # the static sizes hold the surface (nothing is written otherwise)
        counts = py.surface_count(*args[:2]).cpu()
        assert 0 < int(counts[0]) <= args[4] and 0 < int(counts[1]) <= args[5]


def test_all_19_operators_have_a_valid_call(env):
    assert len({op for op, _ in env["calls"].values()}) == 19 and sorted(env["calls"]) == sorted(VALID)


def _put(i, f):
    """Spoil argument i: f maps the valid operand to the bad one."""
    return lambda a: a[:i] + (f(a[i]),) + a[i + 1:]


short = lambda t: t[:-1]                                    # noqa: E731   one element short (a 1-D tensor stays contiguous)
wide17 = lambda t: torch.zeros((t.shape[0], 17), dtype=t.dtype, device=t.device)        # noqa: E731

# (id, valid call, spoil, the Python door's class, the C++ door's class).  The two doors agree on every case of this list today;
# where a later case finds them apart, write each door's present class here under a comment that says so — aligning them is
# a change of its own.
CASES = [
    ("brats_linear_grid_short", "render_brats[linear]", _put(2, short), ValueError, ValueError),
    ("brats_vga_grid_short", "render_brats[vga]", _put(2, short), ValueError, ValueError),
    ("brats_mod4_grid_short", "render_brats[mod4]", _put(2, short), ValueError, ValueError),
    ("brats_labcell_grid_short", "render_brats[labcell]", _put(6, short), ValueError, ValueError),
    ("brats_labels_unbound", "render_brats[linear]", _put(6, lambda t: None), ValueError, ValueError),
    ("backward_grad_out_shape", "render_brats_backward", _put(2, lambda t: t[:, :7].contiguous()), ValueError, ValueError),
    ("backward_grid_short", "render_brats_backward", _put(4, short), ValueError, ValueError),
    ("backward_enabled_modality_empty", "render_brats_backward", _put(3, lambda t: t[:0]), ValueError, ValueError),
    ("backward_preds_short", "render_brats_backward", _put(8, short), ValueError, ValueError),
    ("soft_logits_17_classes", "render_brats_soft", _put(2, wide17), ValueError, ValueError),
    ("soft_offsets_short", "render_brats_soft", _put(3, short), ValueError, ValueError),
    ("soft_grid_short", "render_brats_soft", _put(4, short), ValueError, ValueError),
    ("soft_labels_unbound", "render_brats_soft", _put(8, lambda t: None), ValueError, ValueError),
    ("soft_backward_grad_out_shape", "render_brats_soft_backward", _put(2, lambda t: t[:7].contiguous()), ValueError, ValueError),
    ("soft_backward_logits_17_classes", "render_brats_soft_backward", _put(3, wide17), ValueError, ValueError),
    ("soft_backward_offsets_short", "render_brats_soft_backward", _put(4, short), ValueError, ValueError),
    ("forward_biases_short", "inr_forward", _put(1, short), ValueError, ValueError),
    ("forward_coords_short", "inr_forward", _put(10, lambda t: t[:-1]), ValueError, ValueError),
    ("forward_feats_short", "inr_forward", _put(11, lambda t: t[:-1]), ValueError, ValueError),
    ("forward_f32_biases_short", "inr_forward_f32", _put(1, short), ValueError, ValueError),
    ("forward_f32_coords_short", "inr_forward_f32", _put(9, lambda t: t[:-1]), ValueError, ValueError),
    ("forward_f32_coords_unbound", "inr_forward_f32", _put(9, lambda t: None), ValueError, ValueError),
    ("backward_scratch_short", "inr_backward", _put(2, short), TypeError, TypeError),
    ("backward_dlogits_short", "inr_backward", _put(1, lambda t: t[:-1]), ValueError, ValueError),
    ("loss_logits_17_classes", "inr_loss", lambda a: (wide17(a[0]), a[1], [1.0] * 17, a[3]), ValueError, ValueError),
    ("loss_class_weights_length", "inr_loss", _put(2, lambda v: v[:3]), ValueError, ValueError),
    ("loss_labels_short", "inr_loss", _put(1, short), ValueError, ValueError),
    ("loss_ext_class_weights_length", "inr_loss_ext", _put(2, lambda v: v + [1.0]), ValueError, ValueError),
    ("loss_ext_focal_alpha_length", "inr_loss_ext", _put(3, lambda v: v[:3]), ValueError, ValueError),
    ("sampler_mods_table_short", "inr_sample_batch", _put(0, short), ValueError, ValueError),
    ("mix_tumour_offsets_length", "inr_sample_batch_mix", _put(3, short), ValueError, ValueError),
    ("mix_tumour_index_unbound", "inr_sample_batch_mix", _put(2, lambda t: None), ValueError, ValueError),
    ("adamw_moment_size", "inr_adamw_step", _put(4, short), ValueError, ValueError),
    ("adamw_bias_moment_size", "inr_adamw_step", _put(7, short), ValueError, ValueError),
    ("edt_labels_not_3d", "edt_squared", _put(0, lambda t: t.reshape(30, 4)), ValueError, ValueError),
    ("edt_spacing_of_two", "edt_squared", _put(2, lambda v: v[:2]), ValueError, ValueError),
    ("hausdorff_labels_not_3d", "hausdorff", lambda a: (a[0].reshape(30, 4), a[1].reshape(30, 4)) + a[2:], ValueError, ValueError),
    ("hausdorff_shapes_differ", "hausdorff", _put(1, lambda t: t[:5].contiguous()), ValueError, ValueError),
    ("hausdorff_spacing_of_two", "hausdorff", _put(2, lambda v: v[:2]), ValueError, ValueError),
    ("surface_count_labels_not_3d", "surface_count", _put(0, lambda t: t.reshape(-1)), ValueError, ValueError),
    ("surface_count_negative_mask", "surface_count", _put(1, lambda m: -1), ValueError, ValueError),
    ("surface_extract_negative_mask", "surface_extract", _put(1, lambda m: -1), ValueError, ValueError),
    ("surface_extract_spacing_of_two", "surface_extract", _put(2, lambda v: v[:2]), ValueError, ValueError),
    ("surface_extract_labels_not_3d", "surface_extract", _put(0, lambda t: t.reshape(30, 4)), ValueError, ValueError),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_one_spoiled_operand_is_refused_on_the_host_through_both_doors(env, case):
    _, name, spoil, py_class, native_class = case
    op, args = env["calls"][name]
    bad = spoil(args)
    for (_, ops), want in zip(env["doors"], (py_class, native_class)):
        with pytest.raises(want):
            getattr(ops, op)(*bad)


def test_operands_on_two_gpus_are_refused(env):
    """Every device tensor of one call lives on one GPU; checked where a second GPU exists (one GPU: nothing to mix)."""
    if torch.cuda.device_count() >= 2:
        for name, i in (("render_mesh", 4), ("inr_loss", 1), ("hausdorff", 1), ("render_brats[linear]", 6)):
            op, args = env["calls"][name]
            bad = _put(i, lambda t: t.to("cuda:1"))(args)
            for _, ops in env["doors"]:
                with pytest.raises(ValueError):
                    getattr(ops, op)(*bad)
