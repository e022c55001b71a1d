"""K4 — the triangle-mesh BVH ray tracer of scripts/mesh_rt (app.py, bvh.py, ply_loader.py, mesh_rt.slang).

  load_ply        ASCII PLY as the reference loader reads it (its quirks included), and binary little-endian PLY
  normalize_mesh  the centre-and-scale of app.py:84-88
  build_bvh       the reference's median-split BVH, element for element, built level by level
  upload_mesh     host-side validation (once) + the device buffers app.py uploads (float4 nodes, uint4 tris, float4 verts)
  render_mesh     compute_main on the current stream (mrirt_render_mesh), no synchronisation
  extract_surface the surface of a set of classes of a label volume as a triangle mesh (naive surface nets, csrc/surface.hip)
  surface_mesh    extract_surface + build_bvh + upload_mesh: a label volume to a mesh render_mesh draws
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, Iterable, Mapping, Optional, Tuple, Union

import numpy as np

from . import _lib

MAX_INDEX = 1 << 23          # the shader decodes indices stored as floats with int(x + 0.5): exact below 2^23
MAX_DEPTH = 64               # the shader's uint stack[64]


# ------------------------------------------------------------------------------------------------------------------
# PLY
# ------------------------------------------------------------------------------------------------------------------
def _load_ply_ascii(path: Path, max_faces: Optional[int]) -> Tuple[np.ndarray, np.ndarray]:
    # line for line what ply_loader.load_ply_ascii does: x, y, z are the first three columns of a vertex line; a face
    # line that is empty, not a triangle or short is skipped but uses up one of the header's faces; max_faces counts
    # the triangles kept
    with open(path, "r", encoding="utf-8") as f:
        if not f.readline().startswith("ply"):
            raise ValueError("Not a PLY file")
        vertex_count = face_count = 0
        while True:
            line = f.readline()
            if not line:
                raise ValueError("Unexpected EOF while reading header")
            line = line.strip()
            if line == "end_header":
                break
            if line.startswith("element vertex"):
                vertex_count = int(line.split()[-1])
            elif line.startswith("element face"):
                face_count = int(line.split()[-1])
        verts = np.zeros((vertex_count, 3), dtype=np.float32)
        for i in range(vertex_count):
            parts = f.readline().strip().split()
            if len(parts) < 3:
                raise ValueError("Malformed vertex line")
            verts[i, 0], verts[i, 1], verts[i, 2] = float(parts[0]), float(parts[1]), float(parts[2])
        tris = []
        limit = max_faces if max_faces is not None else face_count
        for _ in range(face_count):
            if len(tris) >= limit:
                f.readline()
                continue
            parts = f.readline().strip().split()
            if not parts or int(parts[0]) != 3 or len(parts) < 4:
                continue
            tris.append((int(parts[1]), int(parts[2]), int(parts[3])))
        if not tris:
            raise ValueError("No triangular faces found in PLY")
        return verts, np.array(tris, dtype=np.uint32)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2",
              "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4",
              "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}


def _load_ply_binary(data: bytes, header_end: int, header: list, max_faces: Optional[int]) -> Tuple[np.ndarray, np.ndarray]:
    elements = []                                       # [name, count, [(prop, type) | (prop, ('list', ct, it))]]
    for line in header:
        w = line.split()
        if not w:
            continue
        if w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property" and elements:
            if w[1] == "list":
                elements[-1][2].append((w[4], ("list", _PLY_TYPES[w[2]], _PLY_TYPES[w[3]])))
            else:
                elements[-1][2].append((w[2], _PLY_TYPES[w[1]]))
    pos = header_end
    verts = tris = None
    for name, count, props in elements:
        lists = [p for p in props if isinstance(p[1], tuple)]
        if not lists:
            dt = np.dtype([(p, t) for p, t in props])
            rec = np.frombuffer(data, dtype=dt, count=count, offset=pos)
            pos += dt.itemsize * count
            if name == "vertex":
                verts = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32)
            continue
        if name != "face" or len(props) != 1:
            raise ValueError(f"binary PLY: element '{name}' with list properties is not supported")
        _, ct, it = props[0][1]
        ct, it = np.dtype(ct), np.dtype(it)
        # all triangles: one fixed-size record per face
        dt = np.dtype([("n", ct), ("i", it, (3,))])
        if pos + dt.itemsize * count <= len(data):
            rec = np.frombuffer(data, dtype=dt, count=count, offset=pos)
            if np.all(rec["n"] == 3):
                tris = rec["i"].astype(np.int64)
                pos += dt.itemsize * count
                continue
        out = []
        for _ in range(count):
            n = int(np.frombuffer(data, dtype=ct, count=1, offset=pos)[0])
            pos += ct.itemsize
            idx = np.frombuffer(data, dtype=it, count=n, offset=pos)
            pos += it.itemsize * n
            if n == 3:
                out.append(idx.astype(np.int64))
        tris = np.array(out, dtype=np.int64).reshape(-1, 3)
    if verts is None or tris is None:
        raise ValueError("binary PLY: no vertex or face element")
    if max_faces is not None:
        tris = tris[:max(0, int(max_faces))]
    if len(tris) == 0:
        raise ValueError("No triangular faces found in PLY")
    return verts, tris.astype(np.uint32)


def load_ply(path: Union[str, Path], max_faces: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(verts f32[N,3], tris u32[M,3]) of an ASCII or binary little-endian PLY.  Faces that are not triangles are skipped;
    ``max_faces`` caps the triangles kept."""
    path = Path(path)
    with open(path, "rb") as f:
        head = f.read(1 << 16)
    end = head.find(b"end_header")
    fmt = None
    if head.startswith(b"ply") and end >= 0:
        lines = head[:end].decode("ascii", "replace").splitlines()
        fmt = next((ln.split()[1] for ln in lines if ln.startswith("format")), None)
    if fmt in (None, "ascii"):
        return _load_ply_ascii(path, max_faces)
    if fmt != "binary_little_endian":
        raise ValueError(f"PLY format '{fmt}' is not supported (ascii, binary_little_endian)")
    data = path.read_bytes()
    nl = data.index(b"\n", end)
    return _load_ply_binary(data, nl + 1, lines, max_faces)


def save_ply_binary(path: Union[str, Path], verts: np.ndarray, tris: np.ndarray) -> None:
    """Binary little-endian PLY: float32 x y z, uchar count + int indices."""
    v = np.ascontiguousarray(verts, dtype="<f4").reshape(-1, 3)
    t = np.asarray(tris).reshape(-1, 3)
    rec = np.zeros(len(t), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    rec["n"], rec["i"] = 3, t
    hdr = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\n"
           f"property float z\nelement face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(hdr.encode("ascii"))
        f.write(v.tobytes())
        f.write(rec.tobytes())


def normalize_mesh(verts: np.ndarray) -> np.ndarray:
    """Centre on the bounding box and scale its longest side to 1.8 (app.py:84-88)."""
    vmin = verts.min(axis=0)
    vmax = verts.max(axis=0)
    center = 0.5 * (vmin + vmax)
    scale = 1.0 / float(np.max(vmax - vmin) + 1e-8)
    return (verts - center) * scale * 1.8


# ------------------------------------------------------------------------------------------------------------------
# BVH
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class BVH:
    nodes: np.ndarray      # float32 [N, 8]: min.xyz, max.xyz, leftFirst, triCountOrRight (bvh.py's packing)
    tris: np.ndarray       # [M, 3] triangles in leaf order (the input's dtype, as bvh.py)
    vert_pos: np.ndarray   # float32 [V, 3]
    depth: int             # nodes on the longest root-to-leaf path


def build_bvh(vert_pos: np.ndarray, tris: np.ndarray, max_leaf_tris: int = 4) -> BVH:
    """The reference's build_bvh (bvh.py:15-83), element for element.

    The reference recurses: a node of more than max_leaf_tris triangles is split at the median of np.argsort of its
    triangles' centroids along the longest axis of their bounds, nodes are numbered in pre-order and leaves take their
    triangles in that order.  Here the tree is built one level at a time.  The shape of the tree is a function of the
    triangle count alone (n -> n // 2, n - n // 2), so every node's pre-order number is known up front.  A node whose keys
    are all distinct has one sorted order, which one stable sort over all of a level's nodes gives at once; a node with
    equal keys (or NaN) calls np.argsort on exactly the sub-array the reference passes it, in the same element order,
    so the (unstable) order of its ties is numpy's, as there."""
    V = vert_pos.astype(np.float32, copy=False)
    T = tris.astype(np.uint32, copy=False)
    M = len(T)
    if M == 0:
        raise ValueError("build_bvh: no triangles")
    L = int(max_leaf_tris)
    VT = V[T]
    cent = VT.mean(axis=1)
    tbmin = VT.min(axis=1)
    tbmax = VT.max(axis=1)

    sizes: Dict[int, int] = {}

    def subtree(n: int) -> int:                          # nodes of the subtree over n triangles
        stack = [n]
        while stack:
            k = stack[-1]
            if k in sizes:
                stack.pop()
                continue
            if k <= L:
                sizes[k] = 1
                stack.pop()
                continue
            a, b = k // 2, k - k // 2
            if a in sizes and b in sizes:
                sizes[k] = 1 + sizes[a] + sizes[b]
                stack.pop()
            else:
                stack.extend([x for x in (a, b) if x not in sizes])
        return sizes[n]

    N = subtree(M)
    nodes = np.zeros((N, 8), dtype=np.float32)
    left_first = np.zeros(N, dtype=np.int64)
    tri_count = np.zeros(N, dtype=np.int64)
    final = np.empty(M, dtype=np.int64)

    cur = np.arange(M, dtype=np.int64)                  # the active nodes' triangles, node after node, in the reference's order
    seg_len = np.array([M], dtype=np.int64)
    seg_gstart = np.array([0], dtype=np.int64)          # offset of the node's triangles in the leaf order
    seg_node = np.array([0], dtype=np.int64)
    depth = 0
    while len(seg_len):
        depth += 1
        starts = np.concatenate([[0], np.cumsum(seg_len)[:-1]])
        seg_of = np.repeat(np.arange(len(seg_len)), seg_len)
        bmin = np.minimum.reduceat(tbmin[cur], starts, axis=0)
        bmax = np.maximum.reduceat(tbmax[cur], starts, axis=0)
        nodes[seg_node, 0:3] = bmin
        nodes[seg_node, 3:6] = bmax
        leaf = seg_len <= L
        if leaf.any():
            el = leaf[seg_of]
            pos = seg_gstart[seg_of] + (np.arange(len(cur)) - starts[seg_of])
            final[pos[el]] = cur[el]
            left_first[seg_node[leaf]] = seg_gstart[leaf]
            tri_count[seg_node[leaf]] = seg_len[leaf]
        inner = ~leaf
        if not inner.any():
            break
        ei = inner[seg_of]
        cur_i, seg_of_i = cur[ei], seg_of[ei]
        ln, gs, nd = seg_len[inner], seg_gstart[inner], seg_node[inner]
        remap = np.cumsum(inner) - 1                      # old segment -> inner segment number
        seg_of_i = remap[seg_of_i]
        st_i = np.concatenate([[0], np.cumsum(ln)[:-1]])
        cmin = np.minimum.reduceat(cent[cur_i], st_i, axis=0)
        cmax = np.maximum.reduceat(cent[cur_i], st_i, axis=0)
        axis = np.argmax(cmax - cmin, axis=1)
        keys = cent[cur_i, axis[seg_of_i]]
        order = np.lexsort((keys, seg_of_i))
        perm = cur_i[order]
        sk = keys[order]
        same = (sk[1:] == sk[:-1]) & (seg_of_i[order][1:] == seg_of_i[order][:-1])
        tie_segs = np.unique(np.concatenate([seg_of_i[order][1:][same], seg_of_i[np.isnan(keys)]]))
        for s in tie_segs.tolist():
            a, b = int(st_i[s]), int(st_i[s] + ln[s])
            sub = cur_i[a:b]
            perm[a:b] = sub[np.argsort(cent[sub, axis[s]])]
        half = ln // 2
        lnode = nd + 1
        rnode = nd + 1 + np.array([subtree(int(h)) for h in half], dtype=np.int64)
        left_first[nd] = lnode
        tri_count[nd] = -(rnode + 1)
        cur = perm
        seg_len = np.stack([half, ln - half], axis=1).reshape(-1)
        seg_gstart = np.stack([gs, gs + half], axis=1).reshape(-1)
        seg_node = np.stack([lnode, rnode], axis=1).reshape(-1)
    nodes[:, 6] = left_first.astype(np.float32)
    nodes[:, 7] = tri_count.astype(np.float32)
    return BVH(nodes=nodes, tris=tris[final.astype(np.int32)], vert_pos=V, depth=depth)


# ------------------------------------------------------------------------------------------------------------------
# validation (host, once per upload)
# ------------------------------------------------------------------------------------------------------------------
def _decode(nodes: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """int(b.z + 0.5), int(b.w +- 0.5) in fp32 as the shader (:96-97); ok = False where there is no int value."""
    z, w = nodes[:, 6].astype(np.float32), nodes[:, 7].astype(np.float32)
    with np.errstate(invalid="ignore"):
        x = z + np.float32(0.5)
        y = w + np.where(w >= 0, np.float32(0.5), np.float32(-0.5)).astype(np.float32)
        ok = (x > -1.0) & (x < 2147483648.0) & (y > -2147483648.0) & (y < 2147483648.0)
        lf = np.where(ok, np.trunc(np.where(ok, x, 0)), 0).astype(np.int64)
        cr = np.where(ok, np.trunc(np.where(ok, y, 0)), 0).astype(np.int64)
    return lf, cr, ok


def validate_bvh(nodes: np.ndarray, tris: np.ndarray, vert_count: int) -> int:
    """Check a node / triangle buffer pair the way the kernel relies on it; returns the tree's depth (nodes on the longest
    root-to-leaf path).  Raises ValueError naming the first fault: counts outside [1, 2^23), an index that does not decode,
    a child or leaf range out of range, a vertex index >= vert_count, a node reached twice or never from root 0, depth > 64."""
    nodes = np.asarray(nodes, dtype=np.float32).reshape(-1, 8)
    tris = np.asarray(tris).reshape(len(tris), -1)
    N, M = len(nodes), len(tris)
    if not (1 <= N < MAX_INDEX):
        raise ValueError(f"mesh: node count {N} outside [1, 2^23)")
    if not (1 <= M < MAX_INDEX):
        raise ValueError(f"mesh: triangle count {M} outside [1, 2^23)")
    if vert_count < 1:
        raise ValueError("mesh: no vertices")
    idx = tris[:, :3].astype(np.int64)
    bad = np.nonzero((idx < 0).any(axis=1) | (idx >= vert_count).any(axis=1))[0]
    if len(bad):
        raise ValueError(f"mesh: triangle {int(bad[0])} has a vertex index outside [0, {vert_count})")
    lf, cr, ok = _decode(nodes)
    if not ok.all():
        raise ValueError(f"mesh: node {int(np.nonzero(~ok)[0][0])} holds an index that does not decode")
    leaf = cr > 0
    badl = np.nonzero(leaf & ((lf < 0) | (lf + cr > M)))[0]
    if len(badl):
        raise ValueError(f"mesh: leaf node {int(badl[0])} has a triangle range outside [0, {M})")
    right = -cr - 1
    badi = np.nonzero(~leaf & ((lf < 0) | (lf >= N) | (right < 0) | (right >= N)))[0]
    if len(badi):
        raise ValueError(f"mesh: inner node {int(badi[0])} has a child index outside [0, {N})")
    seen = np.zeros(N, dtype=bool)
    seen[0] = True
    level = np.array([0], dtype=np.int64)
    depth = 0
    while len(level):
        depth += 1
        if depth > MAX_DEPTH:
            raise ValueError(f"mesh: tree deeper than the {MAX_DEPTH}-entry traversal stack")
        inner = level[~leaf[level]]
        kids = np.concatenate([lf[inner], right[inner]])
        if len(kids) and (seen[kids].any() or len(np.unique(kids)) != len(kids)):
            k = kids[seen[kids]] if seen[kids].any() else kids
            raise ValueError(f"mesh: node {int(k[0])} is reached more than once from the root (a cycle or a shared child)")
        seen[kids] = True
        level = kids
    if not seen.all():
        raise ValueError(f"mesh: node {int(np.nonzero(~seen)[0][0])} is not reached from the root")
    return depth


# ------------------------------------------------------------------------------------------------------------------
# device
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class Mesh:
    """A validated mesh on the device, in the buffers app.py uploads (app.py:94-111)."""
    nodes: Any                 # torch float32 [N * 8]  (float4 x 2 per node)
    tris: Any                  # torch int32 [M * 4]    (uint4, xyz used)
    verts: Any                 # torch float32 [V * 4]  (float4, xyz used)
    node_count: int
    tri_count: int
    vert_count: int
    depth: int                 # nodes on the longest root-to-leaf path = stack entries a ray needs


def pack_tris(tris: np.ndarray) -> np.ndarray:
    t = np.asarray(tris).astype(np.uint32)
    return np.concatenate([t[:, :3], np.zeros((len(t), 1), np.uint32)], axis=1) if t.shape[1] == 3 else t


def pack_verts(verts: np.ndarray) -> np.ndarray:
    v = np.asarray(verts, dtype=np.float32)
    return np.concatenate([v[:, :3], np.ones((len(v), 1), np.float32)], axis=1) if v.shape[1] == 3 else v


def upload_mesh(mesh: Union[BVH, np.ndarray], tris: Optional[np.ndarray] = None, verts: Optional[np.ndarray] = None,
                stream=None) -> Mesh:
    """``upload_mesh(bvh)`` or ``upload_mesh(nodes, tris, verts)`` (nodes [N, 8] or [2N, 4] float32, tris [M, 3|4],
    verts [V, 3|4]).  Validates on the host first (:func:`validate_bvh`, ValueError before anything reaches the device)."""
    import torch
    from .render import _on_stream, _require_gpu
    if isinstance(mesh, BVH):
        nodes, tris, verts = mesh.nodes, mesh.tris, mesh.vert_pos
    else:
        nodes = mesh
        if tris is None or verts is None:
            raise TypeError("upload_mesh(nodes, tris, verts): tris and verts are required")
    nodes = np.ascontiguousarray(np.asarray(nodes, dtype=np.float32).reshape(-1, 8))
    tris, verts = np.asarray(tris), np.asarray(verts)
    if tris.ndim != 2 or tris.shape[1] not in (3, 4) or verts.ndim != 2 or verts.shape[1] not in (3, 4):
        raise ValueError("mesh: tris must be [M, 3 or 4] and verts [V, 3 or 4]")
    t4, v4 = pack_tris(tris), pack_verts(verts)
    depth = validate_bvh(nodes, t4, len(v4))
    dev = _require_gpu()
    with _on_stream(stream):
        n_t = torch.from_numpy(nodes.reshape(-1)).to(dev)
        t_t = torch.from_numpy(np.ascontiguousarray(t4).view(np.int32).reshape(-1)).to(dev)
        v_t = torch.from_numpy(np.ascontiguousarray(v4).reshape(-1)).to(dev)
    return Mesh(n_t, t_t, v_t, len(nodes), len(t4), len(v4), depth)


def render_mesh(params: Mapping[str, Any], mesh: Mesh, out=None, ext: Optional[Mapping[str, Any]] = None, stream=None,
                stats: bool = False, status=None):
    """K4 — drop-in for ``kernel.dispatch`` of ``compute_main`` (app.py:224-243).  ``params`` is the gParams dict
    (imageSize, fovY, maxBounces, eye, U, V, W).  Enqueued on the current stream (or ``stream``), not synchronised.
    ``stats=True`` also returns {'pops', 'tests'} (this synchronises); ``status``: an int32 device tensor of one element
    whose bit 0 the kernel sets for a ray that met a malformed buffer."""
    import torch
    from .params import mesh_params, render_ext
    from .render import _alloc_out, _on_stream, _ptr, _require_gpu, _stream_ptr
    dev = _require_gpu()
    P = mesh_params(params)
    E = render_ext(ext)
    with _on_stream(stream):
        whole = _lib.RenderExt.from_buffer_copy(E)
        whole.tileSize = 0                                  # a frame, always: the library refuses tiles (MRIRT_ERR_ARG)
        o, pitch = _alloc_out(int(P.imageSize[0]), int(P.imageSize[1]), whole, dev, out)
        st = torch.zeros(2, dtype=torch.int64, device=dev) if stats else None
        rc = _lib.lib().mrirt_render_mesh(C.byref(P), C.byref(E), _ptr(mesh.nodes), mesh.node_count, _ptr(mesh.tris),
                                          mesh.tri_count, _ptr(mesh.verts), mesh.vert_count, mesh.depth, _ptr(o), pitch,
                                          _ptr(st), _ptr(status), _stream_ptr(stream))
        _lib.check(rc, "mrirt_render_mesh")
        if stats:
            s = st.cpu()
            return o, {"pops": int(s[0]), "tests": int(s[1])}
    return o


# ------------------------------------------------------------------------------------------------------------------
# class surfaces of label volumes
# ------------------------------------------------------------------------------------------------------------------
def class_mask(classes: Union[int, Iterable[int]]) -> int:
    """The uint32 class set of mrirt_surface_*: bit l is set when label l is inside.  ``classes``: a label or an iterable
    of labels, each in 0..31."""
    try:
        labels = [int(c) for c in classes]              # type: ignore[union-attr]
    except TypeError:
        labels = [int(classes)]                         # type: ignore[arg-type]
    mask = 0
    for c in labels:
        if not 0 <= c < 32:
            raise ValueError(f"classes: label {c} outside 0..31")
        mask |= 1 << c
    return mask


def _frame3(values, what: str):
    v = [float(np.float32(x)) for x in values]
    if len(v) != 3:
        raise ValueError(f"{what}: expected three values (one per axis)")
    return (C.c_float * 3)(*v)


def extract_surface(labels, classes, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), stream=None):
    """The surface of the voxels whose label is in ``classes`` (an int or an iterable of labels in 0..31; ``(1, 2, 3)`` is the
    whole tumour) as a closed, outward-oriented triangle mesh — naive surface nets on the GPU (csrc/surface.hip), element
    for element the definition of DESIGN.md section 12.  ``labels``: an (H, W, D) integer volume, a NumPy array or a device
    tensor (what ``predict_volume`` returns); axis k is world axis k, voxel i at ``origin + i * spacing``.
    Returns device tensors ``(verts float32 [V, 3], tris int32 [T, 3])``; an empty class gives two empty tensors.
    One host read (the two counts) between ``mrirt_surface_count`` and ``mrirt_surface_extract``."""
    import torch
    from .inr import _label_volume
    from .render import _on_stream, _ptr, _require_gpu, _stream_ptr
    mask = class_mask(classes)
    sp, org = _frame3(spacing, "spacing"), _frame3(origin, "origin")
    dev = labels.device if isinstance(labels, torch.Tensor) and labels.is_cuda else _require_gpu()
    lib = _lib.lib()
    with torch.cuda.device(dev), _on_stream(stream):
        lab = _label_volume(labels, dev, "labels")
        hwd = (C.c_uint32 * 3)(*lab.shape)
        nbytes = int(lib.mrirt_surface_scratch_bytes(hwd))
        if nbytes <= 0:
            raise ValueError(f"extract_surface: a volume of shape {tuple(lab.shape)} is outside the supported sizes")
        scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.mrirt_surface_count(_ptr(lab), hwd, mask, _ptr(scratch), nbytes, _ptr(counts), _stream_ptr(stream)),
                   "mrirt_surface_count")
        nv, nt = (int(x) for x in counts.cpu())
        verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        _lib.check(lib.mrirt_surface_extract(_ptr(lab), hwd, mask, sp, org, _ptr(verts) if nv else None, nv,
                                             _ptr(tris) if nt else None, nt, _ptr(scratch), nbytes, _ptr(counts),
                                             _stream_ptr(stream)), "mrirt_surface_extract")
    return verts, tris


def surface_mesh(labels, classes, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), max_leaf_tris: int = 4) -> Mesh:
    """A label volume to a mesh :func:`render_mesh` draws: :func:`extract_surface`, the reference's BVH on the host
    (:func:`build_bvh`), :func:`upload_mesh`.  With ``origin = volMin`` and ``spacing = voxelSize`` of
    ``volume.world_frame`` the surface lies on the K1 volume.  ValueError for an empty surface and for one beyond K4's
    2^23 triangle limit."""
    verts, tris = extract_surface(labels, classes, spacing, origin)
    if tris.shape[0] == 0:
        raise ValueError("surface_mesh: the surface is empty (no voxel of the volume has a label in `classes`)")
    if tris.shape[0] >= MAX_INDEX or verts.shape[0] >= MAX_INDEX:
        raise ValueError(f"surface_mesh: {tris.shape[0]} triangles / {verts.shape[0]} vertices are beyond K4's limit of 2^23")
    return upload_mesh(build_bvh(verts.cpu().numpy(), tris.cpu().numpy(), max_leaf_tris))


# ------------------------------------------------------------------------------------------------------------------
# procedural meshes (tests, tools/mesh_bench.py)
# ------------------------------------------------------------------------------------------------------------------
def icosphere(subdiv: int, noise: float = 0.0, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Unit icosphere as a triangle soup (three vertices per triangle): 20 * 4^subdiv triangles.  ``noise`` > 0 displaces
    every vertex radially by a seeded sum of sines of its position (a vertex shared by triangles moves the same way)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                  [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                  [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    tri = v[f] / np.linalg.norm(v[f], axis=2, keepdims=True)         # [T, 3, 3]
    for _ in range(int(subdiv)):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = a + b, b + c, c + a
        ab /= np.linalg.norm(ab, axis=1, keepdims=True)
        bc /= np.linalg.norm(bc, axis=1, keepdims=True)
        ca /= np.linalg.norm(ca, axis=1, keepdims=True)
        tri = np.stack([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1),
                        np.stack([ab, bc, ca], 1)], axis=1).reshape(-1, 3, 3)
    p = tri.reshape(-1, 3)
    if noise > 0.0:
        rng = np.random.default_rng(seed)
        r = np.ones(len(p))
        for _ in range(6):
            k = rng.normal(size=3) * 4.0
            r += noise / 6.0 * np.sin(p @ k + rng.uniform(0, 2 * np.pi))
        p = p * r[:, None]
    verts = p.astype(np.float32)
    return verts, np.arange(len(verts), dtype=np.uint32).reshape(-1, 3)


def torus(n_major: int = 48, n_minor: int = 24, R: float = 0.7, r: float = 0.25) -> Tuple[np.ndarray, np.ndarray]:
    """Torus around the y axis with shared vertices: 2 * n_major * n_minor triangles."""
    u = np.arange(n_major) * (2 * np.pi / n_major)
    w = np.arange(n_minor) * (2 * np.pi / n_minor)
    U, W = np.meshgrid(u, w, indexing="ij")
    verts = np.stack([(R + r * np.cos(W)) * np.cos(U), r * np.sin(W), (R + r * np.cos(W)) * np.sin(U)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n_major), np.arange(n_minor), indexing="ij")
    a = i * n_minor + j
    b = ((i + 1) % n_major) * n_minor + j
    c = ((i + 1) % n_major) * n_minor + (j + 1) % n_minor
    d = i * n_minor + (j + 1) % n_minor
    tris = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return verts.astype(np.float32), tris.astype(np.uint32)
