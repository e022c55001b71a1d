"""The soft prediction overlay on the GPU (mrirt_render_brats_soft / _backward, csrc/brats_soft.hip) against the fp64 reference of
brats_soft_ref.py, through every door: ctypes (mrirt.render_brats_soft, render_brats_soft_backward), torch.ops.mrirt, mrirt_native
(C++) and the autograd function; then the end-to-end composition with the fp32 training step (grad_w / grad_b of a SIREN and a
Fourier/ReLU network) and the fitting loop.

Frame: |C - C_ref| <= TOL_F.  Gradients: |d - d_ref| <= TOL_G * A, A being the closed form with every term replaced by its
absolute value.  The tolerances are the constants of brats_soft_cases.py, 8 x the reference's own fp32 deviation measured on
the CPU — never derived from a kernel's output.  What the contract makes exact is compared with ==."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import brats_soft_cases as sc
import brats_soft_ref as ref

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="The given NumPy array is not writable")


@functools.lru_cache(maxsize=None)
def solved(name):
    return ref.closed_form(sc.BY_NAME[name], sc.data(name), geo=sc.geo(name))     # once per case, shared, read-only


def _gpu_counts(p, ext):
    import torch
    from mrirt import _lib, params
    P, E = params.brats_params(p), params.render_ext(ext)
    counts = torch.empty(int(P.imageSize[0]) * int(P.imageSize[1]), dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().mrirt_brats_sample_counts(C.byref(P), C.byref(E), C.c_void_p(counts.data_ptr()), None), "mrirt_brats_sample_counts")
    return counts.cpu().numpy().astype(np.int64)


def _device(name, logits=None):
    """The case on the device.  The rows the kernels touch are the GPU's own sample counts from `offsets` on: they are checked
    against the reference's before anything is launched on them."""
    import torch
    c, d = sc.BY_NAME[name], sc.data(name)
    assert np.array_equal(_gpu_counts(c["params"], c["ext"]), d["counts"]), name
    vols = [None if v is None else torch.from_numpy(v.copy()).cuda() for v in d["vols"]]
    lab = None if d["labels"] is None else torch.from_numpy(d["labels"].astype(np.int32)).cuda()
    z = torch.from_numpy(np.array(d["logits"] if logits is None else logits, dtype=np.float32)).cuda()
    assert z.shape[0] >= d["rows"]
    return vols, lab, z, torch.from_numpy(d["offsets"].copy()).cuda(), torch.from_numpy(d["G"].copy()).cuda()


def _check_frame(name, how, frame, want, tol):
    H, W = frame.shape[:2]
    got = frame.detach().cpu().numpy().astype(np.float64)
    err = float(np.abs(got[..., :3] - want.reshape(H, W, 3)).max())
    print(f"{name} {how} frame: max |C - C_ref| = {err:.3e} (TOL_F {tol:.1e})")
    assert np.all(got[..., 3] == 1.0), (name, how)
    assert err <= tol, (name, how, err)


def _check_grad(name, how, got, want, A, tol):
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    worst = float((err / np.maximum(A, 1e-300))[A > 0].max()) if (A > 0).any() else 0.0
    print(f"{name} {how}: worst |d - d_ref| / A = {worst:.3e} (TOL {tol:.1e})")
    assert np.all(err <= tol * A), (name, how, worst)


@pytest.mark.parametrize("name", sc.NAMES)
def test_frame_and_dlogits_match_the_reference_through_every_door(name):
    import torch
    import mrirt
    from mrirt import torch_ops
    c, d, cf = sc.BY_NAME[name], sc.data(name), solved(name)
    p, ext = c["params"], c["ext"]
    vols, lab, z, off, G = _device(name)
    own = sc.owned_rows(name)
    # ctypes: the frame, the counter, the gradient into a NaN-filled buffer
    frame, st = mrirt.render_brats_soft(p, vols, z, off, lab, ext=ext, return_stats=True)
    _check_frame(name, "ctypes", frame, cf.frame, sc.TOL_F)
    assert st["live_samples"] == cf.rec.composited, name
    dl = torch.full_like(z, float("nan"))
    out = mrirt.render_brats_soft_backward(p, vols, z, off, G, lab, ext=ext, out=dl)
    assert out is dl
    got = dl.cpu().numpy()
    assert np.all(np.isnan(got[~own])) and np.all(np.isfinite(got[own])), name      # gap rows and guards untouched, every owned row written
    got = np.where(own[:, None], got, 0.0)
    _check_grad(name, "ctypes dlogits", got, cf.dlogits, cf.A, sc.TOL_G)
    dead = own[:, None] & (cf.A == 0)
    assert np.all(got[dead] == 0) and not np.signbit(got[dead]).any(), name         # not taken / sigma <= 0 / G == 0: exact +0
    # the same bits again, and through the operator libraries and the autograd function
    assert torch.equal(mrirt.render_brats_soft(p, vols, z, off, lab, ext=ext), frame)
    again = mrirt.render_brats_soft_backward(p, vols, z, off, G, lab, ext=ext)
    want_bits = torch.where(torch.from_numpy(own).cuda()[:, None], dl, torch.zeros_like(dl))
    assert torch.equal(again.view(torch.int32), want_bits.view(torch.int32)), name
    blobs = (torch_ops.pack_brats_params(p), torch_ops.pack_render_ext(ext))
    native = torch_ops.load_native()
    for how, ops in (("torch.ops.mrirt", torch.ops.mrirt), ("mrirt_native", native)):
        assert torch.equal(ops.render_brats_soft(*blobs, z, off, *vols, lab), frame), (name, how)
        assert torch.equal(ops.render_brats_soft_backward(*blobs, G, z, off, *vols, lab).view(torch.int32), want_bits.view(torch.int32)), (name, how)
    leaf = z.clone().requires_grad_(True)
    fr = mrirt.render_brats_soft_autograd(p, vols, leaf, off, lab, ext=ext)
    assert torch.equal(fr, frame)
    (fr * G).sum().backward()
    assert torch.equal(leaf.grad.view(torch.int32), want_bits.view(torch.int32)), name


def test_dead_rows_are_not_vacuous():
    """Rows after a ray's termination and rows of G == 0 rays exist in the cases that claim them (their zeros are asserted above)."""
    for name in ("c16_dense_ert", "reversed_gaps"):
        d, cf = sc.data(name), solved(name)
        taken = np.zeros(d["counts"].size, np.int64)
        for s in cf.rec.steps:
            if not s.empty:
                taken[s.idx] += 1
        assert (taken < d["counts"]).sum() > 20, name
    d = sc.data("reversed_gaps")
    W = sc.BY_NAME["reversed_gaps"]["hw"][1]
    dark = (np.arange(d["counts"].size) % W >= W // 2) & (d["counts"] > 0)
    assert dark.sum() > 20


@pytest.mark.parametrize("name", ["c4_random", "c2_seg_ones"])                      # without and with the ground-truth overlay
@pytest.mark.parametrize("how", ["zero_lut", "one_class", "class_zero"])
def test_without_events_the_frame_is_render_brats_and_dlogits_is_zero(name, how):
    import torch
    import mrirt
    c, d = sc.BY_NAME[name], sc.data(name)
    p, ext = dict(c["params"]), c["ext"]
    logits = d["logits"]
    if how == "zero_lut":
        lut = np.array(sc.LUT)
        lut[:, 3] = 0.0
        p["lutColorAlpha"] = lut
    elif how == "one_class":
        logits = d["logits"][:, :1]
    else:
        logits = np.full(d["logits"].shape, -1e4, np.float32)
        logits[:, 0] = 1e4
    vols, lab, z, off, G = _device(name, logits)
    frame = mrirt.render_brats_soft(p, vols, z, off, lab, ext=ext)
    assert torch.equal(frame, mrirt.render_brats(dict(p, showPred=0), vols, lab, None, ext=ext)), (name, how)
    dl = mrirt.render_brats_soft_backward(p, vols, z, off, G, lab, ext=ext, out=torch.full_like(z, float("nan")))
    own = torch.from_numpy(sc.owned_rows(name)).cuda()
    assert torch.all(dl[own].view(torch.int32) == 0), (name, how)                    # +0, bit for bit
    assert torch.all(torch.isnan(dl[~own]))


@pytest.mark.parametrize("name", ["c4_random", "one_packet", "reversed_gaps", "c9_half_zero"])
def test_one_hot_logits_give_the_class_stream_frame_and_no_gradient(name):
    import torch
    import mrirt
    from mrirt import _lib, params
    c, d = sc.BY_NAME[name], sc.data(name)
    p, ext = c["params"], c["ext"]
    rng = np.random.default_rng(7)
    cls = rng.integers(1, c["classes"], d["logits"].shape[0])
    logits = np.full(d["logits"].shape, -1e4, np.float32)
    logits[np.arange(cls.size), cls] = 1e4
    vols, lab, z, off, G = _device(name, logits)
    frame = mrirt.render_brats_soft(p, vols, z, off, lab, ext=ext)
    H, W = c["hw"]
    want = ref.forward(c, d, torch.from_numpy(logits), geo=sc.geo(name)).numpy()
    _check_frame(name, "one-hot vs reference", frame, want, sc.TOL_F)
    # the hard compositor on the same classes
    P, E = params.brats_params(dict(p, showPred=1)), params.render_ext(ext)
    vp = (C.c_void_p * 4)(*[C.c_void_p(v.data_ptr()) if v is not None else None for v in vols])
    classes = torch.from_numpy(cls.astype(np.int16)).cuda()
    hard = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _lib.check(_lib.lib().mrirt_render_brats_stream(C.byref(P), C.byref(E), vp, ptr(lab), ptr(classes), ptr(off), ptr(hard), W, None, None),
               "mrirt_render_brats_stream")
    err = float((frame - hard).abs().max())
    print(f"{name}: soft one-hot vs mrirt_render_brats_stream: max |dC| = {err:.3e} (TOL_F {sc.TOL_F:.1e})")
    assert err <= sc.TOL_F
    dl = mrirt.render_brats_soft_backward(p, vols, z, off, G, lab, ext=ext)
    assert torch.count_nonzero(dl) == 0, name                                        # saturated softmax


@pytest.mark.parametrize("which", list(sc.E2E_NETS))
def test_end_to_end_weight_gradients(which):
    """MLP + render: the frame and grad_w / grad_b of render_brats_inr_autograd against fp64 autograd of the composition."""
    import torch
    import mrirt
    c, d = sc.E2E_CASE, sc.e2e_data()
    g = ref.geometry(c)
    kind, par, _ = sc.E2E_NETS[which]
    layers = sc.e2e_layers(which)
    assert np.array_equal(_gpu_counts(c["params"], c["ext"]), d["counts"])
    coords, feats = ref.mlp_inputs(c, d, g)
    gw, gb, fr64, lg = ref.end_to_end(c, d, (kind, par), layers, torch.float64, g, coords, feats)
    cf = ref.closed_form(c, dict(d, logits=lg.numpy()), geo=g)
    Ws64 = [torch.from_numpy(p["W"].astype(np.float64)) for p in layers]
    bs64 = [torch.from_numpy(p["b"].astype(np.float64)) for p in layers]
    Aw, Ab = ref.weight_abs_scale((kind, par), Ws64, bs64, torch.from_numpy(coords), torch.from_numpy(feats), cf.A)
    vols = [torch.from_numpy(v.copy()).cuda() for v in d["vols"]]
    lab = torch.from_numpy(d["labels"].astype(np.int32)).cuda()
    Ws = [torch.from_numpy(p["W"].copy()).cuda().requires_grad_(True) for p in layers]
    bs = [torch.from_numpy(p["b"].copy()).cuda().requires_grad_(True) for p in layers]
    kw = dict(w0=par) if kind == "siren" else dict(fourier_freqs=par)
    frame = mrirt.inr.render_brats_inr_autograd(c["params"], vols, Ws, bs, d["zmu"], d["zsigma"], labels=lab, ext=c["ext"], **kw)
    _check_frame("e2e", which, frame, fr64, sc.TOL_E2E_F)
    (frame * torch.from_numpy(d["G"].copy()).cuda()).sum().backward()
    for i in range(len(layers)):
        _check_grad("e2e", f"{which} grad_w[{i}]", Ws[i].grad.cpu().numpy(), gw[i], Aw[i], sc.TOL_E2E_G)
        _check_grad("e2e", f"{which} grad_b[{i}]", bs[i].grad.cpu().numpy(), gb[i], Ab[i], sc.TOL_E2E_G)


def test_fit_views_follows_the_fp64_history():
    """3 cameras, an 8 x 8 x 8 volume, 16 x 16 frames, SIREN 7 -> 2 x 32 -> 4, targets rendered from the teacher, 24 steps: the loss
    history follows the recorded fp64 CPU history within 8 x the fp32 CPU loop's own deviation (relative to the largest loss),
    and the last loss is below the first."""
    import torch
    import mrirt
    import inr_loop_ref as loop
    views, teacher, start = sc.fit_data()
    vols = [torch.from_numpy(v.copy()).cuda() for v in views[0]["vols"]]
    gparams = sc.FIT_CASES[0]["params"]
    cams = [{k: c["params"][k] for k in ("eye", "U", "V", "W")} for c in sc.FIT_CASES]
    for c, d in zip(sc.FIT_CASES, views):
        assert np.array_equal(_gpu_counts(c["params"], c["ext"]), d["counts"])
    as_dict = lambda layers: {f"l{i}": {"w": p["W"], "b": p["b"]} for i, p in enumerate(layers)}
    with torch.no_grad():
        tW = [torch.from_numpy(p["W"].copy()).cuda() for p in teacher]
        tb = [torch.from_numpy(p["b"].copy()).cuda() for p in teacher]
        targets = [mrirt.inr.render_brats_inr_autograd({**gparams, **cam}, vols, tW, tb, sc.ZMU, sc.ZSIGMA, w0=sc.FIT_CONFIG["W0"]) for cam in cams]
    losses, st = mrirt.inr.fit_views(sc.FIT_CONFIG, cams, targets, vols, as_dict(start), gparams, sc.ZMU, sc.ZSIGMA)
    dev = loop.loss_deviation(losses, np.asarray(sc.FIT_HISTORY_FP64))
    print("GPU history:", ", ".join(f"{x:.6e}" for x in losses))
    print(f"deviation from the fp64 history {dev:.3e} (tolerance {sc.FIT_TOL:.3e})")
    assert st.step == sc.FIT_STEPS and len(losses) == sc.FIT_STEPS
    assert losses[-1] < losses[0]
    assert dev <= sc.FIT_TOL


def test_refusals_reach_python():
    import torch
    import mrirt
    name = "c4_random"
    c = sc.BY_NAME[name]
    vols, lab, z, off, G = _device(name)
    with pytest.raises(mrirt._lib.MrirtError):
        mrirt.render_brats_soft(c["params"], vols, z, off, ext=dict(shadeMode=1))
    lut = np.array(sc.LUT)
    lut[3, 3] = -1.0
    with pytest.raises(mrirt._lib.MrirtError):
        mrirt.render_brats_soft_backward(dict(c["params"], lutColorAlpha=lut), vols, z, off, G)
    with pytest.raises(ValueError):
        mrirt.render_brats_soft_autograd(c["params"], vols, z, off, ext=dict(math="fast"))
    with pytest.raises(TypeError):
        mrirt.render_brats_soft(c["params"], vols, z, off[:-1])
    with pytest.raises(ValueError):
        mrirt.render_brats_soft(c["params"], vols, torch.zeros((4, 17), device="cuda"), off)
    with pytest.raises(TypeError):
        mrirt.render_brats_soft_backward(c["params"], vols, z, off, G[:, :5])
