"""Class surfaces of label volumes on the GPU (csrc/surface.hip).  The contract is equality with the NumPy restatement of the
definition (tests/surface_ref.py, pinned by the literals of surface_cases.py): vertex bits, triangles and counts, every
comparison ``array_equal`` / ``torch.equal``, never a tolerance."""
import ctypes as C

import numpy as np
import pytest

import mesh_cases
import surface_cases as sc
import surface_ref as sr

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()
IDS = [c[0] for c in CASES]
_REF = {}


def _ref(case):
    """The restatement's arrays of a case, computed once per session and never modified."""
    if case[0] not in _REF:
        v, t = sr.extract(case[1], case[2], case[3], case[4])
        v.setflags(write=False)
        t.setflags(write=False)
        _REF[case[0]] = (v, t)
    return _REF[case[0]]


def _by_name(name):
    return next(c for c in CASES if c[0] == name)


@pytest.fixture(scope="module")
def env():
    import torch
    import mrirt
    from mrirt import torch_ops
    assert torch.cuda.is_available()
    return dict(torch=torch, mrirt=mrirt, native=torch_ops.load_native())


def _assert_equal(name, how, verts, tris, want_v, want_t):
    v, t = verts.cpu().numpy(), tris.cpu().numpy()
    print(name, how, v.shape, t.shape, want_v.shape, want_t.shape)
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape == want_v.shape and t.shape == want_t.shape, (name, how)
    assert np.array_equal(v.view(np.uint32), want_v.view(np.uint32)), f"{name} via {how}: vertex bits differ from the restatement"
    assert np.array_equal(t, want_t), f"{name} via {how}: triangles differ from the restatement"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_extract_surface_equals_the_restatement(env, case):
    torch, mrirt = env["torch"], env["mrirt"]
    name, lab, mask, sp, org, counts = case
    want_v, want_t = _ref(case)
    if counts is not None:
        assert (len(want_v), len(want_t)) == counts
    classes = [b for b in range(32) if (mask >> b) & 1]
    verts, tris = mrirt.extract_surface(lab, classes, sp, org)
    assert verts.is_cuda and tris.is_cuda
    _assert_equal(name, "numpy int16", verts, tris, want_v, want_t)
    dev = torch.from_numpy(lab).cuda()
    _assert_equal(name, "device int64", *mrirt.extract_surface(dev.to(torch.int64), classes, sp, org), want_v, want_t)
    if len(classes) == 1:
        _assert_equal(name, "int class", *mrirt.extract_surface(dev, classes[0], sp, org), want_v, want_t)


def test_wide_labels_do_not_wrap_into_a_class(env):
    mrirt = env["mrirt"]
    lab = np.zeros((4, 5, 6), np.int32)
    lab[1, 2, 3] = 65536 + 1                                          # int16 would read it as class 1
    v, t = mrirt.extract_surface(lab, 1)
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3)


@pytest.mark.parametrize("name", ["random_0b1110", "ball_24x22x20_spaced", "empty_class", "ball_127x97x95"])
def test_torch_operators_equal_the_ctypes_path(env, name):
    torch, mrirt, native = env["torch"], env["mrirt"], env["native"]
    _, lab, mask, sp, org, _ = case = _by_name(name)
    want_v, want_t = _ref(case)
    dev = torch.from_numpy(lab).cuda()
    verts, tris = mrirt.extract_surface(dev, [b for b in range(32) if (mask >> b) & 1], sp, org)
    for how, ops in (("torch.ops.mrirt", torch.ops.mrirt), ("torch.ops.mrirt_native", native)):
        counts = ops.surface_count(dev, mask)
        assert counts.is_cuda and counts.dtype == torch.int64 and counts.tolist() == [len(want_v), len(want_t)], how
        v, t = ops.surface_extract(dev, mask, list(sp), list(org), len(want_v), len(want_t))
        assert torch.equal(v, verts) and torch.equal(t, tris), f"{name}: {how}.surface_extract differs from extract_surface"
        assert v.dtype == torch.float32 and t.dtype == torch.int32
    _assert_equal(name, "ctypes", verts, tris, want_v, want_t)


@pytest.mark.parametrize("short", ["verts", "tris"])
def test_too_small_capacity_reports_the_counts_and_writes_nothing(env, short):
    torch, mrirt = env["torch"], env["mrirt"]
    _, lab, mask, sp, org, (nv, nt) = _by_name("ball_24x22x20_spaced")
    lib = mrirt._lib.lib()
    dev = torch.from_numpy(lab).cuda()
    hwd = (C.c_uint32 * 3)(*lab.shape)
    nbytes = int(lib.mrirt_surface_scratch_bytes(hwd))
    # the scratch is exactly as long as the ABI asks for, between two guard blocks that must come back untouched
    guard = 4096
    buf = torch.full((guard + nbytes + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    vcap, tcap = (nv - 1, nt) if short == "verts" else (nv, nt - 1)
    verts = torch.full((nv + 8, 3), -7.0, dtype=torch.float32, device="cuda")
    tris = torch.full((nt + 8, 3), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((3,), -7, dtype=torch.int64, device="cuda")

    def run(vc, tc):
        rc = lib.mrirt_surface_extract(C.c_void_p(dev.data_ptr()), hwd, mask, (C.c_float * 3)(*sp), (C.c_float * 3)(*org),
                                       C.c_void_p(verts.data_ptr()), vc, C.c_void_p(tris.data_ptr()), tc,
                                       C.c_void_p(buf.data_ptr() + guard), nbytes, C.c_void_p(counts.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((buf[:guard] == 0x5A).all()) and bool((buf[guard + nbytes:] == 0x5A).all()), "scratch guard overwritten"
        assert counts.tolist() == [nv, nt, -7]

    run(vcap, tcap)                                       # one capacity one short: the true counts, no geometry at all
    assert bool((verts == -7.0).all()) and bool((tris == -7).all())
    run(nv, nt)                                           # both fit: the geometry, and the canaries past it untouched
    want_v, want_t = _ref(_by_name("ball_24x22x20_spaced"))
    _assert_equal("ball_24x22x20_spaced", "mrirt_surface_extract", verts[:nv], tris[:nt], want_v, want_t)
    assert bool((verts[nv:] == -7.0).all()) and bool((tris[nt:] == -7).all())


def test_surface_mesh_renders_like_the_restatements_mesh(env):
    torch, mrirt = env["torch"], env["mrirt"]
    _, lab, mask, _, _, _ = _by_name("ball_24x22x20")
    voxel_size, vol_min, target, radius = mrirt.volume.world_frame(lab.shape, (1.0, 1.0, 1.0))
    mesh = mrirt.surface_mesh(lab, 1, voxel_size, vol_min)
    want_v, want_t = sr.extract(lab, mask, voxel_size, vol_min)
    ref = mrirt.upload_mesh(mrirt.build_bvh(want_v, want_t, 4))
    assert (mesh.vert_count, mesh.tri_count, mesh.node_count, mesh.depth) == (986, 1968, ref.node_count, ref.depth)
    assert torch.equal(mesh.nodes, ref.nodes) and torch.equal(mesh.tris, ref.tris) and torch.equal(mesh.verts, ref.verts)
    params = mesh_cases.params("axis", 64, 48)                       # from (0, 0, 2.5) down the z axis onto the volume
    got = mrirt.render_mesh(params, mesh).cpu().numpy()
    want = mrirt.render_mesh(params, ref).cpu().numpy()
    assert got.shape == (48, 64, 4) and np.array_equal(got, want)
    corner = got[0, 0]
    assert (got != corner).any(axis=2).sum() > 100, "the frame is all background"
    with pytest.raises(ValueError):
        mrirt.surface_mesh(lab, 9, voxel_size, vol_min)                # an empty surface


def test_non_default_stream_gives_the_same_arrays(env):
    torch, mrirt = env["torch"], env["mrirt"]
    case = sc.large_case()
    name, lab, mask, sp, org, _ = case
    want_v, want_t = _ref(case)
    dev = torch.from_numpy(lab).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    verts, tris = mrirt.extract_surface(dev, 1, sp, org, stream=s)
    with torch.cuda.stream(s):
        v2, t2 = mrirt.extract_surface(dev, 1, sp, org)
    s.synchronize()
    _assert_equal(name, "stream argument", verts, tris, want_v, want_t)
    _assert_equal(name, "side stream current", v2, t2, want_v, want_t)
