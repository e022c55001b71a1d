"""K4 on the host: the PLY loader and the BVH builder against the reference's own output (tests/golden/mesh_*), the
MrirtMeshParams layout, validation of malformed buffers (refused before any launch), and the NumPy restatement of the shader
against a brute-force closest hit that uses no BVH at all."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref
from mesh_cases import GOLDEN, MESHES, fixture, params
from mrirt import _lib, mesh


@pytest.mark.parametrize("name", MESHES)
def test_build_bvh_equals_reference(name):
    f = fixture(name)
    b = mesh.build_bvh(f["verts"], f["tris"], max_leaf_tris=4)
    assert np.array_equal(b.nodes, f["nodes"])
    assert np.array_equal(b.tris, f["bvh_tris"])
    assert np.array_equal(b.vert_pos, f["bvh_verts"])
    assert b.depth == mesh.validate_bvh(f["nodes"], f["bvh_tris"], len(f["bvh_verts"]))


def test_load_ply_equals_reference_loader():
    g = np.load(GOLDEN / "mesh_ply.npz")
    for key, mf in (("all", None), ("max2", 2), ("max3", 3)):
        v, t = mesh.load_ply(GOLDEN / "mesh_ascii.ply", max_faces=mf)
        assert np.array_equal(v, g[f"verts_{key}"]) and v.dtype == np.float32
        assert np.array_equal(t, g[f"tris_{key}"]) and t.dtype == np.uint32
    v, t = mesh.load_ply(GOLDEN / "mesh_cube.ply")
    assert np.array_equal(v, g["verts_cube"]) and np.array_equal(t, g["tris_cube"])


def test_binary_ply_round_trip(tmp_path):
    for src in ("mesh_ascii.ply", "mesh_cube.ply"):
        v, t = mesh.load_ply(GOLDEN / src)
        p = tmp_path / ("bin_" + src)
        mesh.save_ply_binary(p, v, t)
        v2, t2 = mesh.load_ply(p)
        assert np.array_equal(v, v2) and np.array_equal(t, t2) and t2.dtype == np.uint32
        assert np.array_equal(mesh.load_ply(p, max_faces=2)[1], t[:2])


def test_binary_ply_mixed_faces_and_extra_properties(tmp_path):
    # uint counts and uint indices, an extra vertex property, and a quad that is skipped as the ASCII loader skips it
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    hdr = ("ply\nformat binary_little_endian 1.0\ncomment mixed\nelement vertex 4\nproperty float x\nproperty float y\n"
           "property float z\nproperty uchar flag\nelement face 3\nproperty list uint uint vertex_indices\nend_header\n")
    body = b"".join(x.tobytes() + b"\x07" for x in v)
    for face in ([0, 1, 2], [0, 1, 2, 3], [0, 2, 3]):
        body += np.array([len(face)] + face, "<u4").tobytes()
    p = tmp_path / "mixed.ply"
    p.write_bytes(hdr.encode() + body)
    v2, t2 = mesh.load_ply(p)
    assert np.array_equal(v2, v)
    assert np.array_equal(t2, np.array([[0, 1, 2], [0, 2, 3]], np.uint32))


def test_mesh_params_layout():
    P = _lib.MeshParams
    assert C.sizeof(P) == 80
    assert (P.eye.offset, P.U.offset, P.V.offset, P.W.offset) == (16, 32, 48, 64)
    assert (P.imageSize.offset, P.fovY.offset, P.maxBounces.offset, P.padEye.offset) == (0, 8, 12, 28)
    assert _lib.lib().mrirt_sizeof(6) == C.sizeof(P)
    assert "mrirt_render_mesh" in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), "mrirt_render_mesh")


def _valid():
    f = fixture("ico3")
    return f["nodes"].copy(), f["bvh_tris"].copy(), f["bvh_verts"].copy()


def _malformed():
    """(kind, nodes, tris, verts) — one fault each."""
    out = []
    nodes, tris, verts = _valid()
    inner = int(np.nonzero(nodes[:, 7] < 0)[0][1])
    leaf = int(np.nonzero(nodes[:, 7] > 0)[0][0])
    n = nodes.copy(); n[inner, 6] = len(nodes); out.append(("left child out of range", n, tris, verts))
    n = nodes.copy(); n[inner, 7] = -(len(nodes) + 5); out.append(("right child out of range", n, tris, verts))
    n = nodes.copy(); n[inner, 7] = 0; out.append(("inner node with count 0", n, tris, verts))
    n = nodes.copy(); n[leaf, 7] = len(tris) + 1; out.append(("huge leaf count", n, tris, verts))
    n = nodes.copy(); n[leaf, 6] = -7; out.append(("negative leaf start", n, tris, verts))
    n = nodes.copy(); n[inner, 6] = 0; out.append(("cycle to the root", n, tris, verts))
    n = nodes.copy(); n[inner, 6] = np.nan; out.append(("NaN index", n, tris, verts))
    n = nodes.copy(); n[inner, 7] = -(n[inner, 6] + 1); out.append(("shared child", n, tris, verts))
    t = tris.copy(); t[5, 1] = len(verts); out.append(("vertex index out of range", nodes, t, verts))
    # a chain 66 levels deep: inner node k has children k+1 (inner) and a leaf
    depth = 66
    ch = np.zeros((2 * depth - 1, 8), np.float32)
    ch[:, 0:3], ch[:, 3:6] = -1, 1
    for k in range(depth - 1):
        i, lf = 2 * k, 2 * k + 1
        ch[i, 6], ch[i, 7] = i + 2, -(lf + 1)
        ch[lf, 6], ch[lf, 7] = 0, 1
    ch[2 * depth - 2, 6], ch[2 * depth - 2, 7] = 0, 1
    out.append(("deeper than the stack", ch, tris[:1], verts))
    return out


@pytest.mark.parametrize("kind", [k for k, *_ in _malformed()])
def test_validation_refuses_malformed_buffers(kind, monkeypatch):
    launched = []
    monkeypatch.setattr(mesh._lib, "lib", lambda: launched.append(1))
    _, nodes, tris, verts = next(c for c in _malformed() if c[0] == kind)
    with pytest.raises(ValueError, match="mesh:"):
        mesh.validate_bvh(nodes, mesh.pack_tris(tris), len(verts))
    with pytest.raises(ValueError, match="mesh:"):
        mesh.upload_mesh(nodes, tris, verts)
    assert not launched


def test_validation_refuses_counts_at_2_pow_23():
    nodes, tris, verts = _valid()
    big_nodes = np.broadcast_to(nodes[:1], (1 << 23, 8))
    with pytest.raises(ValueError, match="node count"):
        mesh.validate_bvh(big_nodes, tris, len(verts))
    big_tris = np.broadcast_to(mesh.pack_tris(tris[:1]), (1 << 23, 4))
    with pytest.raises(ValueError, match="triangle count"):
        mesh.validate_bvh(nodes, big_tris, len(verts))
    assert mesh.validate_bvh(nodes, tris, len(verts)) >= 1


def test_abi_refuses_bad_arguments_before_any_launch():
    """The C entry point's argument checks run on the host before anything is enqueued: the pointers here are never read."""
    l = _lib.lib()
    P = _lib.MeshParams()
    P.imageSize[0], P.imageSize[1], P.fovY = 8, 8, 0.8
    P.W[2] = 1.0
    fake = C.c_void_p(4096)

    def call(ext=None, nodes=7, tris=4, verts=8, depth=3, pitch=8):
        return l.mrirt_render_mesh(C.byref(P), C.byref(ext) if ext is not None else None, fake, nodes, fake, tris, fake,
                                   verts, depth, fake, pitch, None, None, None)
    from mrirt.params import render_ext
    assert call(render_ext({"math": "fast"})) == -5
    assert call(render_ext({"tileSize": 16, "tileWorld": 1})) == -5
    assert call(render_ext({"kernelVariant": 1})) == -5
    assert call(nodes=1 << 23) == -5
    assert call(tris=1 << 23) == -5
    assert call(pitch=7) == -5
    assert call(depth=0) == -5 and call(depth=65) == -5


CAMS = (("outside", 0), ("inside", 0), ("axis", 1))


@pytest.mark.parametrize("name", MESHES)
def test_restatement_agrees_with_brute_force(name):
    """Closest hit through the BVH (the shader's box cull and near-first order) vs closest hit over every triangle: the
    same hit / miss and the same t on at least 99.9 % of the rays, for three cameras (one inside the mesh)."""
    f = fixture(name)
    tris, verts = mesh.pack_tris(f["bvh_tris"]), mesh.pack_verts(f["bvh_verts"])
    for cam, mode in CAMS:
        p = params(cam, 48, 40)
        o, d = mesh_ref.primary_rays(p, *np.meshgrid(np.arange(48), np.arange(40), indexing="xy"), camera_mode=mode)
        o = [x.reshape(-1) for x in o]
        d = [x.reshape(-1) for x in d]
        t_bvh, tri_bvh, _, _ = mesh_ref.trace(o, d, f["nodes"], tris, verts)
        hit_bf, t_bf = mesh_ref.brute_force(p, tris, verts, camera_mode=mode)
        hit_bvh = t_bvh < np.float32(1e29)
        agree = (hit_bvh == hit_bf) & (~hit_bf | (t_bvh == t_bf))
        frac = agree.mean()
        print(f"{name} {cam}: {int((~agree).sum())} of {agree.size} rays differ, {int(hit_bf.sum())} hits")
        assert frac >= 0.999, f"{name} / {cam}: {frac:.5f}"
