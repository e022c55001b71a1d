"""The reference of the C5 case grid (tests/c5_cases.py) and the comparisons the GPU tests make with it.  TEST INFRASTRUCTURE ONLY.

reference(case) is the oracle march (oracle_np.brats_main) with the case's rule as its class source — no MLP, no GPU:
  frame              the frame with the case's early-termination threshold
  L                  per ray, the composited steps of that march (aux["nsteps"])
  n                  per ray, the steps in [t0, t1): the same march with ertThreshold = -1
  live, shaded       aux["live_samples"], aux["shaded_samples"]
  offsets, coords, feats, classes
                     the MLP inputs (oracle_np.inr_sample_inputs) and the rule's class of ALL n samples of every ray, ray by ray
                     in pixel order: what the whole-ray form emits

The plan logic of the chunked form classifies, for a pass length c,
    queries(c) = sum over rays of min(n, ceil(L / c) * c)
samples: a ray is planned for a pass iff t < t1 and T > ert after the previous one (the first pass: iff it hits), i.e. for the
ceil(L / c) passes that hold one of its L composited steps — a ray that runs to t1 has L == n — and a planned pass holds its next
min(c, steps left) samples.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import c5_cases as cc
from oracle import oracle_np as onp


def _march(case, ert_off, source):
    vols, lab, _, _ = cc.volumes(case.dims, case.vol_seed)
    ext = cc.oracle_ext(case)
    if ert_off:
        ext = dict(ext, ertThreshold=-1.0)
    return onp.brats_main(cc.params_of(case), list(vols), lab if case.labels is not None else None, source, ext, return_aux=True)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    case = cc.CASES[name]
    vols, _, zmu, zsg = cc.volumes(case.dims, case.vol_seed)
    rec = []

    def recording(idx, k, qx, qy, qz):
        c, f = onp.inr_sample_inputs(vols, case.dims, zmu, zsg, qx, qy, qz)
        cls = cc.rule(case.net, c, f)
        rec.append((idx.copy(), np.asarray(k).copy(), c, f, cls))
        return cls

    frame_all, aux_all = _march(case, True, recording)
    n = aux_all["nsteps"].astype(np.int64)
    ends = np.cumsum(n.reshape(-1))
    offsets = ends - n.reshape(-1)
    total = int(ends[-1]) if ends.size else 0
    coords, feats = np.zeros((total, 3), np.float32), np.zeros((total, 4), np.float32)
    classes = np.full(total, -1, np.int64)
    for idx, k, c, f, cls in rec:
        rows = offsets[idx] + k
        coords[rows], feats[rows], classes[rows] = c, f, cls
    assert (classes >= 0).all()

    if case.ert is not None and case.ert < 0:
        frame, aux = frame_all, aux_all
    else:
        frame, aux = _march(case, False, lambda idx, k, qx, qy, qz: classes[offsets[idx] + k])
    out = dict(frame=frame, L=aux["nsteps"].astype(np.int64), n=n, live=int(aux["live_samples"]), shaded=int(aux["shaded_samples"]),
               offsets=offsets, coords=coords, feats=feats, classes=classes)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def frame_with_classes(case, classes, offsets):
    """The oracle's frame (the case's own termination) with another class stream: what the sensitivity tests perturb."""
    return _march(case, False, lambda idx, k, qx, qy, qz: classes[offsets[idx] + k])[0]


def live_rows(ref):
    """Rows of the composited samples (k < L of every ray) in the whole-ray numbering."""
    L, off = ref["L"].reshape(-1), ref["offsets"]
    return np.concatenate([off[r] + np.arange(L[r]) for r in range(L.size)] or [np.zeros(0, np.int64)]).astype(np.int64)


def queries(n, L, c, floor=False):
    n, L = np.asarray(n, np.int64), np.asarray(L, np.int64)
    passes = L // c if floor else (L + c - 1) // c
    return int(np.minimum(n, passes * c).sum())


# ---- the host side of mrirt_render_brats_inr, restated ------------------------------------------------------------------------------
MAX_PASSES = 1024


def default_chunk(case) -> int:
    """render_brats_inr's choice with chunk_steps=None: 96 where the intensity channel alone cannot terminate a ray, else 32."""
    p = cc.params_of(case)
    diag = math.sqrt(sum((float(np.float32(p["voxelSize"][k])) * case.dims[k]) ** 2 for k in range(3)))
    ert = 0.01 if case.ert is None else float(np.float32(case.ert))
    return 96 if ert > 0.0 and float(np.float32(case.alpha)) * diag <= -math.log(ert) else 32


def max_steps(case, with_drift=True) -> int:
    """The bound on a ray's step count that sizes the number of passes: the box diagonal over stepSize, stretched by the drift
    of the fp32 running sum t += stepSize at the far end of the box (brats_c5.hip, mrirt_render_brats_inr)."""
    p = cc.params_of(case)
    diag2 = dist2 = 0.0
    for k in range(3):
        e = float(np.float32(p["voxelSize"][k])) * float(case.dims[k])
        c = float(np.float32(p["volMin"][k])) + 0.5 * e - float(np.float32(p["eye"][k]))
        diag2 += e * e
        dist2 += c * c
    t_far = math.sqrt(dist2) + math.sqrt(diag2)
    if case.cam.ortho is not None:
        t_far += abs(float(np.float32(case.cam.ortho))) * (1.0 + case.frame[0] / max(1.0, float(case.frame[1])))
    ulp = float(np.spacing(np.float32(t_far)))
    step = float(np.float32(p["stepSize"]))
    drift = 1.0 + ulp / step if with_drift else 1.0
    return int(math.sqrt(diag2) / step * drift) + 3


def passes(case, c, with_drift=True) -> int:
    return (max_steps(case, with_drift) + c - 1) // c


def chunks_of(case, ref):
    """The pass lengths a case is rendered with: 1, 2, one equal to some ray's n, one on which an early termination falls,
    32, the wrapper's choice (None) and 4096 — or the case's own list."""
    if case.chunks is not None:
        return list(case.chunks)
    out = [1, 2]
    c_n, c_e = chunk_of_a_ray(ref), chunk_of_a_death(ref)
    for c in (c_n, c_e):
        if c is not None and c not in out:
            out.append(c)
    return out + [32, None, 4096]


def _commonest(values, avoid=(1, 2)):
    values = np.asarray(values, np.int64)
    values = values[values > 0]
    if values.size == 0:
        return None
    counts = np.bincount(values)
    for a in avoid:                                          # rather a length the list does not hold already
        if a < counts.size and counts.sum() > counts[a]:
            counts[a] = 0
    return int(np.argmax(counts))


def chunk_of_a_ray(ref):
    """The commonest positive n: rays whose step count is an exact multiple of the pass length."""
    return _commonest(ref["n"].reshape(-1))


def chunk_of_a_death(ref):
    """The commonest L among the rays that terminate early: their last composited step is the last of a pass."""
    L, n = ref["L"].reshape(-1), ref["n"].reshape(-1)
    return _commonest(L[L < n])


# ---- comparisons (each returns the list of what differs: empty = equal) -----------------------------------------------------------
def frame_problems(got, want, what="frame"):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [f"{what}: {got.dtype}{got.shape} for {want.dtype}{want.shape}"]
    if np.array_equal(got, want):
        return []
    bad = np.argwhere((got != want).any(axis=-1))
    y, x = (int(v) for v in bad[0])
    return [f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ, first (x={x}, y={y}): {got[y, x]} for {want[y, x]}, "
            f"max |d| {np.nanmax(np.abs(got.astype(np.float64) - want)):.3e}"]


def counter_problems(aux, ref, c, n=None, L=None, floor=False):
    """live / shaded / queries of a chunked frame against the reference (n, L: a perturbed reference's)."""
    n = ref["n"] if n is None else n
    L = ref["L"] if L is None else L
    out = []
    want = dict(live_samples=int(np.asarray(L).sum()), shaded_samples=ref["shaded"], queries=queries(n, L, c, floor))
    for k, v in want.items():
        if int(aux[k]) != v:
            out.append(f"{k}: {int(aux[k])} for {v} (pass length {c})")
    return out


def stream_problems(counts, classes, coords, feats, ref, n=None, want_classes=None):
    """What the whole-ray form emits against the reference: steps per ray, then class and MLP inputs of every row."""
    n = ref["n"] if n is None else n
    want_classes = ref["classes"] if want_classes is None else want_classes
    counts = np.asarray(counts).astype(np.int64).reshape(np.asarray(n).shape)
    if not np.array_equal(counts, n):
        bad = np.argwhere(counts != n)
        return [f"counts: {len(bad)} rays differ, first {tuple(int(v) for v in bad[0])}: {int(counts[tuple(bad[0])])} for {int(n[tuple(bad[0])])}"]
    total, out = int(np.asarray(n).sum()), []
    for what, got, want in (("classes", np.asarray(classes)[:total].astype(np.int64), want_classes), ("coords", np.asarray(coords)[:total], ref["coords"]),
                            ("feats", np.asarray(feats)[:total], ref["feats"])):
        if not np.array_equal(got, want):
            rows = np.nonzero((got != want).reshape(total, -1).any(axis=1))[0]
            out.append(f"{what}: {rows.size} of {total} rows differ, first row {int(rows[0])}: {got[rows[0]]} for {want[rows[0]]}")
    return out
