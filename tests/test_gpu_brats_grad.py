"""K1 backward on the GPU (mrirt_render_brats_backward, csrc/brats_backward.hip) against the fp64 reference of brats_grad_ref.py,
through all four doors: ctypes (mrirt.render_brats_backward), torch.ops.mrirt, mrirt_native (C++) and the autograd function.

Everything is measured as |g - g_ref| <= TOL * A + 1e-30, A being the reference's sum of absolute per-sample contributions (per
voxel for the grids, per scalar for the transfer function) and TOL the constant of brats_grad_cases.py, which comes from the
reference's own fp32 error — never from the kernel's output."""
import functools

import numpy as np
import pytest

import brats_grad_cases as bc
import brats_grad_ref as ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def solved(name):
    return ref.closed_form(bc.BY_NAME[name], bc.data(name))          # once per case, shared, read-only


def _device(name):
    import torch
    d = bc.data(name)
    vols = [None if v is None else torch.from_numpy(v.copy()).cuda() for v in d["vols"]]
    lab = None if d["labels"] is None else torch.from_numpy(d["labels"].astype(np.int32)).cuda()
    prd = None if d["preds"] is None else torch.from_numpy(d["preds"].astype(np.int32)).cuda()
    return vols, lab, prd, torch.from_numpy(d["G"].copy()).cuda()


def _assert_close(name, how, gv, gtf, scale=1.0):
    cf = solved(name)
    for m in range(4):
        want = cf.grad_vols[m]
        if want is None:
            assert gv[m] is None or gv[m].numel() == 0, (name, how, m)
            continue
        got = gv[m].detach().cpu().numpy().astype(np.float64).reshape(-1)
        A = cf.A_vols[m] * scale
        err = np.abs(got - scale * want)
        worst = float((err / np.maximum(A, 1e-300)).max())
        print(f"{name} {how} vol{m}: worst |g - g_ref| / A = {worst:.3e} (TOL {bc.TOL:.1e})")
        assert np.all(err <= bc.TOL * A + 1e-30), (name, how, m, worst)
        assert np.all(got[cf.A_vols[m] == 0] == 0), (name, how, m)          # voxels no contributing sample touches: exact zeros
    got = gtf.detach().cpu().numpy().astype(np.float64).reshape(-1)
    err = np.abs(got - scale * cf.grad_tf)
    print(f"{name} {how} tf: |g - g_ref| / A = {err / np.maximum(cf.A_tf * scale, 1e-300)}")
    assert np.all(err <= bc.TOL * cf.A_tf * scale + 1e-30), (name, how, got, cf.grad_tf)


@pytest.mark.parametrize("name", bc.NAMES)
def test_backward_matches_the_reference_through_every_door(name):
    import torch
    import mrirt
    from mrirt import torch_ops
    c = bc.BY_NAME[name]
    p, ext = c["params"], c["ext"]
    vols, lab, prd, G = _device(name)
    # ctypes
    gv, gtf = mrirt.render_brats_backward(p, vols, G, lab, prd, ext=ext)
    _assert_close(name, "ctypes", gv, gtf)
    # the two operator libraries
    blobs = (torch_ops.pack_brats_params(p), torch_ops.pack_render_ext(ext))
    empty = torch.empty(0, dtype=torch.float32, device="cuda")
    out = torch.ops.mrirt.render_brats_backward(*blobs, G, *[empty if v is None else v for v in vols], lab, prd)
    _assert_close(name, "torch.ops.mrirt", out[:4], out[4])
    out = torch_ops.load_native().render_brats_backward(*blobs, G, *vols, lab, prd)
    _assert_close(name, "mrirt_native", out[:4], out[4])
    # autograd: the frame is render_brats's, bit for bit; backward delivers the same gradients
    leaves = [None if v is None else v.clone().requires_grad_(True) for v in vols]
    tf = torch.tensor([float(np.float32(p[k])) for k in mrirt.grad.TF_FIELDS], dtype=torch.float32, device="cuda", requires_grad=True)
    frame = mrirt.render_brats_autograd(p, leaves, tf, lab, prd, ext=ext)
    assert torch.equal(frame, mrirt.render_brats(p, vols, lab, prd, ext=ext))
    (frame * G).sum().backward()
    _assert_close(name, "autograd", [None if v is None else v.grad for v in leaves], tf.grad)


def test_all_miss_frame_gives_exact_zeros():
    import torch
    import mrirt
    c = bc.BY_NAME["all_miss"]
    vols, lab, prd, G = _device("all_miss")
    gv, gtf = mrirt.render_brats_backward(c["params"], vols, G, ext=c["ext"])
    assert torch.count_nonzero(gv[0]) == 0 and torch.count_nonzero(gtf) == 0


def test_rays_with_zero_upstream_touch_nothing():
    """G is zero on the right half of the image: a voxel that only those rays sample keeps an exact zero, and rendering the left
    half's G alone gives the same gradient as the full call (same rays march, so also the same A)."""
    import torch
    import mrirt
    name = "four_modalities_half_zero"
    c = bc.BY_NAME[name]
    cf = solved(name)
    vols, lab, prd, G = _device(name)
    gv, _ = mrirt.render_brats_backward(c["params"], vols, G, ext=c["ext"])
    full = ref.closed_form(c, dict(bc.data(name), G=np.ones_like(bc.data(name)["G"])))
    only_dark = [(full.A_vols[m] > 0) & (cf.A_vols[m] == 0) for m in range(4)]
    assert sum(int(x.sum()) for x in only_dark) > 0                           # the property is not vacuous
    for m in range(4):
        assert torch.count_nonzero(gv[m][torch.from_numpy(only_dark[m]).cuda()]) == 0


def test_disabled_modality_is_untouched_and_calls_accumulate():
    import torch
    import mrirt
    name = "middle_disabled"
    c = bc.BY_NAME[name]
    nvox = int(np.prod(c["dims"]))
    vols, lab, prd, G = _device(name)
    sentinel = torch.full((nvox,), 12345.0, dtype=torch.float32, device="cuda")
    acc = [torch.zeros(nvox, dtype=torch.float32, device="cuda") for _ in range(4)]
    acc[1] = sentinel
    tf = torch.zeros(4, dtype=torch.float64, device="cuda")
    bound = list(vols)
    bound[1] = torch.zeros(nvox, dtype=torch.float32, device="cuda")            # bound, but volEnabled[1] == 0
    for _ in range(2):
        gv, gtf = mrirt.render_brats_backward(c["params"], bound, G, ext=c["ext"], accumulate_into=(acc, tf))
    assert gv[1] is sentinel and torch.all(sentinel == 12345.0)
    _assert_close(name, "two accumulating calls", [gv[0], None, gv[2], gv[3]], gtf, scale=2.0)


def test_refusals_reach_python():
    import torch
    import mrirt
    c = bc.BY_NAME["one_modality"]
    vols, lab, prd, G = _device("one_modality")
    with pytest.raises(mrirt._lib.MrirtError):
        mrirt.render_brats_backward(c["params"], vols, G, ext=dict(shadeMode=1))
    with pytest.raises(ValueError):
        mrirt.render_brats_autograd(c["params"], vols, ext=dict(math="fast"))
    with pytest.raises(TypeError):
        mrirt.render_brats_backward(c["params"], vols, G[:, :5])


def test_fitting_a_volume_decreases_the_loss():
    """Ten Adam steps on an 8 x 8 x 8 volume towards a frame rendered from a different volume: the loss falls monotonically over the
    first five."""
    import torch
    import mrirt
    c = bc.BY_NAME["one_packet"]
    p = dict(c["params"], imageSize=[24, 20])
    rng = np.random.default_rng(5)
    target_vol = torch.from_numpy(rng.uniform(0.2, 0.8, 512).astype(np.float32)).cuda()
    target = mrirt.render_brats(p, [target_vol])
    vol = torch.full((8, 8, 8), 0.5, dtype=torch.float32, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([vol], lr=0.02)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        frame = mrirt.render_brats_autograd(p, [vol])
        loss = ((frame[..., :3] - target[..., :3]) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", losses)
    assert all(b < a for a, b in zip(losses[:5], losses[1:6])), losses
    assert losses[-1] < losses[0]
