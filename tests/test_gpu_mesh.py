"""K4 on the MI355X: STRICT frames of mrirt_render_mesh bit-identical to the NumPy restatement of compute_main
(tests/mesh_ref.py) on the reference's own BVHs, with the pop / triangle-test counters equal to the restatement's totals;
a 1.3 M-triangle mesh on a pixel sample; rgba16f; the torch operator; the slangpy-shaped shim running app.py's call
sequence; argument checks."""
import numpy as np
import pytest
import torch

import mesh_ref
from mesh_cases import MESHES, fixture, params

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (33, 17), (1, 1), (200, 40))
CAMERAS = ("outside", "inside", "axis", "grazing")


def _mrirt():
    import mrirt
    return mrirt


_UPLOADED = {}


def _mesh(name):
    if name not in _UPLOADED:
        m = _mrirt()
        f = fixture(name)
        b = m.mesh.BVH(f["nodes"], f["bvh_tris"], f["bvh_verts"], 0)
        _UPLOADED[name] = (m.upload_mesh(b), f)
    return _UPLOADED[name]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", MESHES)
def test_strict_frames_bit_identical_to_restatement(name):
    m = _mrirt()
    dm, f = _mesh(name)
    tris, verts = m.mesh.pack_tris(f["bvh_tris"]), m.mesh.pack_verts(f["bvh_verts"])
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    bad = []
    for cam in CAMERAS:
        for (w, h) in SIZES:
            for mode in (0, 1):
                p = params(cam, w, h)
                ext = {"cameraMode": mode}
                got, st = m.render_mesh(p, dm, ext=ext, stats=True, status=status)
                ref, pops, tests = mesh_ref.render(p, f["nodes"], tris, verts, camera_mode=mode)
                g = got.cpu().numpy()
                same = np.array_equal(_u32(g), _u32(ref))
                counts = (st["pops"], st["tests"]) == (int(pops.sum()), int(tests.sum()))
                if not (same and counts):
                    nd = int((_u32(g) != _u32(ref)).any(axis=-1).sum())
                    bad.append(f"{cam} {w}x{h} mode {mode}: {nd} pixels differ; stats {st} vs "
                               f"({int(pops.sum())}, {int(tests.sum())})")
    assert int(status.item()) == 0, "status bit set on a valid tree"
    assert not bad, "\n".join(bad)


def test_large_mesh_pixel_sample():
    """A noise-displaced icosphere of 1 310 720 triangles at 1024^2, compared on a seeded sample of 16 384 pixels."""
    m = _mrirt()
    v, t = m.mesh.icosphere(8, noise=0.12, seed=7)
    b = m.build_bvh(m.normalize_mesh(v).astype(np.float32), t)
    dm = m.upload_mesh(b)
    tris, verts = m.mesh.pack_tris(b.tris), m.mesh.pack_verts(b.vert_pos)
    rng = np.random.default_rng(1234)
    for cam in ("outside", "inside"):
        p = params(cam, 1024, 1024)
        got = m.render_mesh(p, dm).cpu().numpy()
        idx = rng.choice(1024 * 1024, size=16384, replace=False)
        px, py = idx % 1024, idx // 1024
        ref, _, _ = mesh_ref.render(p, b.nodes, tris, verts, pixels=(px, py))
        sel = got[py, px]
        nd = int((_u32(sel) != _u32(ref)).any(axis=-1).sum())
        assert nd == 0, f"{cam}: {nd} of 16384 sampled pixels differ"


def test_rgba16f_is_the_fp32_frame_rounded():
    m = _mrirt()
    dm, _ = _mesh("ico4")
    for cam in ("outside", "grazing"):
        p = params(cam, 64, 48)
        full = m.render_mesh(p, dm).cpu().numpy()
        half = m.render_mesh(p, dm, ext={"outFormat": "rgba16f"})
        assert half.dtype == torch.float16
        assert np.array_equal(half.cpu().numpy().view(np.uint16), full.astype(np.float16).view(np.uint16))


def test_out_with_pitch_and_stream():
    m = _mrirt()
    dm, _ = _mesh("torus")
    p = params("outside", 33, 17)
    ref = m.render_mesh(p, dm)
    big = torch.full((17, 40, 4), -1.0, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        m.render_mesh(p, dm, out=big[:, :33], stream=s)
    s.synchronize()
    assert torch.equal(big[:, :33], ref)
    assert bool((big[:, 33:] == -1.0).all())


def test_shim_runs_the_app_sequence():
    """scripts/mesh_rt/app.py: load_program, create_compute_kernel, create_buffer(element_size=16) + copy_from_numpy of the
    float4 nodes / uint4 triangles / float4 vertices, an rgba16_float texture, dispatch with its vars, blit, finish, submit."""
    m = _mrirt()
    from mrirt import shim as spy
    _, f = _mesh("ico3")
    device = spy.Device(enable_debug_layers=True, compiler_options={"include_paths": []})
    kernel = device.create_compute_kernel(device.load_program("mesh_rt.slang", ["compute_main"]))
    nodes4 = f["nodes"].astype(np.float32).reshape((-1, 4))
    tris_u32 = np.concatenate([f["bvh_tris"].astype(np.uint32), np.zeros((len(f["bvh_tris"]), 1), np.uint32)], axis=1)
    v = np.concatenate([f["bvh_verts"], np.ones((len(f["bvh_verts"]), 1), np.float32)], axis=1)
    bufs = []
    for arr in (nodes4, tris_u32, v):
        b = device.create_buffer(element_count=arr.shape[0], element_size=16, usage=spy.BufferUsage.shader_resource)
        b.copy_from_numpy(arr)
        bufs.append(b)
    W, H = 80, 48
    out = device.create_texture(format=spy.Format.rgba16_float, width=W, height=H,
                                usage=spy.TextureUsage.shader_resource | spy.TextureUsage.unordered_access, label="mesh_rt_output")
    surface = device.create_texture(format=spy.Format.rgba16_float, width=W, height=H)
    p = params("outside", W, H)
    gparams = {"imageSize": (np.uint32(W), np.uint32(H)), "fovY": np.float32(p["fovY"]), "maxBounces": np.uint32(1),
               "eye": p["eye"], "U": p["U"], "V": p["V"], "W": p["W"]}
    for _ in range(2):                                   # the second frame reuses the validated buffers
        ce = device.create_command_encoder()
        kernel.dispatch(thread_count=[W, H, 1], vars={"gOutput": out, "gBVHNodes": bufs[0], "gTris": bufs[1], "gVerts": bufs[2],
                                                      "gParams": gparams}, command_encoder=ce)
        ce.blit(surface, out)
        device.submit_command_buffer(ce.finish())
    device.wait()
    dm, _ = _mesh("ico3")
    ref = m.render_mesh(gparams, dm, ext={"outFormat": "rgba16f"})
    assert torch.equal(out.tensor, ref) and torch.equal(surface.tensor, ref)
    assert len(device._mesh) == 1


def test_load_program_compute_main():
    from mrirt import shim as spy
    device = spy.Device()
    prog = device.load_program("mesh_rt.slang", ["compute_main"])
    assert device.create_compute_kernel(prog).kind == "K4"


def test_invalid_arguments_launch_nothing():
    m = _mrirt()
    dm, _ = _mesh("cube")
    p = params("outside", 16, 16)
    out = torch.full((16, 16, 4), 7.0, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for ext in ({"math": "fast"}, {"tileSize": 16, "tileWorld": 1}, {"kernelVariant": 2}):
        with pytest.raises(m._lib.MrirtError) as e:
            m.render_mesh(p, dm, out=out, ext=ext, status=status)
        assert e.value.status == -5
    for field, val in (("node_count", 1 << 23), ("tri_count", 1 << 23)):
        bad = m.mesh.Mesh(**{**dm.__dict__, field: val})
        with pytest.raises(m._lib.MrirtError) as e:
            m.render_mesh(p, bad, out=out, status=status)
        assert e.value.status == -5
    wide = torch.full((16, 16, 4), 7.0, device="cuda")
    import ctypes as C
    from mrirt.params import mesh_params, render_ext
    P, E = mesh_params(p), render_ext(None)
    rc = m._lib.lib().mrirt_render_mesh(C.byref(P), C.byref(E), dm.nodes.data_ptr(), dm.node_count, dm.tris.data_ptr(),
                                        dm.tri_count, dm.verts.data_ptr(), dm.vert_count, dm.depth, wide.data_ptr(), 15,
                                        None, None, None)
    assert rc == -5
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((wide == 7.0).all()) and int(status.item()) == 0


def test_torch_operator_equals_render_mesh():
    m = _mrirt()
    from mrirt import torch_ops
    dm, _ = _mesh("torus")
    for ext in (None, {"outFormat": "rgba16f"}, {"cameraMode": 1}):
        p = params("outside", 64, 48)
        ref = m.render_mesh(p, dm, ext=ext)
        blob, eb = torch_ops.pack_mesh_params(p), torch_ops.pack_render_ext(ext)
        got = torch.ops.mrirt.render_mesh(blob, eb, dm.nodes, dm.tris, dm.verts, dm.depth)
        assert torch.equal(got, ref)
        native = torch_ops.load_native().render_mesh(blob, eb, dm.nodes, dm.tris, dm.verts, dm.depth)
        assert torch.equal(native, ref)
        meta = [x.to("meta") for x in (dm.nodes, dm.tris, dm.verts)]
        fake = torch_ops.render_mesh_fake(blob, eb, *meta, dm.depth)
        assert tuple(fake.shape) == (48, 64, 4) and fake.dtype == ref.dtype and fake.device.type == "meta"
