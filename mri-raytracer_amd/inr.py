"""INR forward on the GPU, with the reference's names and argument meaning.

Mirrors ``inr/inr/model.py`` as the viewer and notebooks use it (``from inr.model import
model_load, predict_volume``: inr/interactive.ipynb cell 5, inr/viewer/brats_viewer.py:261,293):

  model_load(npz_path, config_override=None) -> (params, config)        model.py:217-301
  build_input(coords, intensities, fourier_freqs) -> (B, 3+6K+M)        model.py:21-23
  apply_mlp(params, x) -> logits                                        model.py:43-50
  predict_volume(params, case_data, fourier_freqs, chunk) -> (pred,seg) model.py:119-141
  dice_score(pred, true, num_classes) / coverage_dice(pred, true)          model.py:144-161
  siren_apply(params, x, w0=30)                                         neumors_inr.ipynb:1165-1178
  make_loss_and_grad(num_classes, class_weights, dice_weight, K)        model.py:57-90      (csrc/inr_train.hip)
  train_inr(config, cases_or_cache, ...) -> (params, state)             train.py:18-259     (csrc/inr_optim.hip)
  VoxelCache(cases).sample(seed, batch_index, n) / .sample_voxels(...)  dataloader.py:86-96,133-155
  siren_init / make_siren_loss_and_grad / siren_autograd / train_siren   neumors_inr.ipynb:1150-1200 (csrc/inr_train.hip)
  render_brats_inr_autograd / fit_views                                 docs/Goals.md "gradients flow: pixels -> raytracer -> MLP weights" (csrc/brats_soft.hip)
  inject_load / inject_forward / predict_full_volume /                  notebooks/improved.ipynb cells 5 - 10, 14 (csrc/inr_inject.hip)
  compute_uncertainty_mc_dropout / boundary_weights

``params`` is the reference's list of ``{"W": [in,out], "b": [out]}`` (SIREN: dict ``l{i}`` ->
``{"w","b"}``).  All arithmetic runs in the kernels behind csrc/inr_mlp.hip
(inr_stream.hip, inr_ws.hip, inr_refine.hip: bf16 MFMA, fp32 accumulate, split-bf16
first layer); ``model_load`` is host-side file parsing.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
import pathlib
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .render import _ptr, _require_gpu, _stream_ptr

KIND_FOURIER_RELU, KIND_SIREN, KIND_RAW_RELU, KIND_RAW_SIREN = 0, 1, 2, 3


def model_load(npz_path, config_override: Optional[Dict[str, Any]] = None) -> Tuple[List[Dict[str, np.ndarray]], Dict[str, Any]]:
    """Checkpoint reader: ``{name}.npz`` + sidecar ``{name}_info.json`` (model.py:248-301).

    Accepts the final-checkpoint layout (key ``params`` holding a pickled list of W/b dicts,
    train.py:386-389 — needs ``allow_pickle`` and is therefore only honoured for files the caller
    trusts: pass ``config_override={"ALLOW_PICKLE": True}``) and the periodic-checkpoint layout
    (flat ``W_i`` / ``b_i`` arrays, train.py:216-223), which needs no pickle.
    """
    path = pathlib.Path(npz_path).expanduser().resolve()
    if not path.is_file():
        raise FileNotFoundError(f"no checkpoint archive at {path}")
    cfg_path = path.with_name(f"{path.stem}_info.json")
    if not cfg_path.is_file():
        raise FileNotFoundError(f"the sidecar {cfg_path.name} (training config) is missing beside {path.name}")
    allow_pickle = bool((config_override or {}).get("ALLOW_PICKLE", False))
    with np.load(str(path), allow_pickle=allow_pickle) as z:
        names = list(z.files)
        if names and all(n.startswith(("W_", "b_")) for n in names):
            count = sum(n.startswith("W_") for n in names)
            params = [{"W": np.asarray(z[f"W_{i}"]), "b": np.asarray(z[f"b_{i}"])} for i in range(count)]
        elif "params" in names or len(names) == 1:
            key = "params" if "params" in names else names[0]
            try:
                arr = z[key]
            except ValueError as exc:
                raise ValueError(f"{path} stores pickled params; pass config_override={{'ALLOW_PICKLE': True}} "
                                 "only for checkpoints you trust") from exc
            if arr.dtype == object:
                if arr.ndim != 0 and arr.size != 1:
                    raise ValueError(f"{path}: entry '{key}' holds {arr.size} pickled objects (shape {arr.shape}), "
                                     "a checkpoint stores exactly one parameter list")
                params = arr.item()
            else:
                params = arr
        else:
            raise KeyError(f"{path} has neither a 'params' entry nor W_i/b_i arrays (entries: {names})")
    config = json.loads(cfg_path.read_text())
    if config_override is not None:
        config = {**config, **{k: v for k, v in config_override.items() if k != "ALLOW_PICKLE"}}
    return params, config


def fourier_features(coords, k: int) -> torch.Tensor:
    """model.py:11-18: per axis [sin(pi 1 c) .. sin(pi k c), cos(pi 1 c) .. cos(pi k c)] -> (B, 6k)."""
    dev = _require_gpu()
    c = _dev_f32(coords, dev)
    freqs = torch.arange(1, k + 1, device=dev, dtype=torch.float32)
    ang = c[..., None] * freqs[None, None, :] * np.float32(np.pi)
    return torch.cat([torch.sin(ang), torch.cos(ang)], dim=-1).reshape(c.shape[0], -1)


@dataclass
class PackedMLP:
    """Device-resident network: permuted bf16 weight fragments + padded fp32 biases."""
    desc: _lib.InrDesc
    weights: torch.Tensor
    biases: torch.Tensor
    in_dim: int
    out_dim: int


def with_flags(net: PackedMLP, no_weight_stationary: bool = False, no_refine: bool = False, mark_only: bool = False,
               tie_sigmas: float = 0.0) -> PackedMLP:
    """The same packed network (shared device buffers) with other ``MrirtInrDesc.flags`` / ``tieSigmas``: the A/B switches
    of measurements and tests — the streaming kernel instead of the weight-stationary one, the bf16 pass without near-tie
    marking and second pass, marking without the second pass, another mark width.  (ABI 2 read these from the process
    environment at every launch.)"""
    d = _lib.InrDesc()
    C.memmove(C.byref(d), C.byref(net.desc), C.sizeof(d))
    d.flags = ((_lib.INR_NO_WEIGHT_STATIONARY if no_weight_stationary else 0) | (_lib.INR_NO_REFINE if no_refine else 0)
               | (_lib.INR_MARK_ONLY if mark_only else 0))
    d.tieSigmas = float(tie_sigmas)
    return PackedMLP(d, net.weights, net.biases, net.in_dim, net.out_dim)


def _layers(params) -> List[Tuple[np.ndarray, np.ndarray]]:
    if isinstance(params, dict):                         # SIREN notebook layout: l0, l1, ...
        return [(np.asarray(params[f"l{i}"]["w"], np.float32), np.asarray(params[f"l{i}"]["b"], np.float32))
                for i in range(len(params))]
    return [(np.asarray(p["W"], np.float32), np.asarray(p["b"], np.float32)) for p in params]


def pack_mlp(params, kind: int, fourier_freqs: int = 0, num_mods: int = 0, w0: float = 30.0) -> PackedMLP:
    dev = _require_gpu()
    layers = _layers(params)
    if len(layers) < 2:
        raise ValueError("the MLP kernel needs at least one hidden layer")
    hidden = layers[0][0].shape[1]
    for i, (W, b) in enumerate(layers):
        want_in = layers[0][0].shape[0] if i == 0 else hidden
        want_out = hidden if i + 1 < len(layers) else W.shape[1]
        if W.shape != (want_in, want_out) or b.shape != (want_out,):
            raise ValueError(f"layer {i}: W {W.shape} / b {b.shape}; the kernel needs equal hidden widths ({hidden})")
    d = _lib.InrDesc()
    d.kind, d.numLayers, d.inDim, d.outDim, d.hidden = kind, len(layers), layers[0][0].shape[0], layers[-1][0].shape[1], hidden
    d.fourierFreqs, d.numMods, d.w0 = int(fourier_freqs), int(num_mods), float(w0)
    nbytes = int(_lib.lib().mrirt_inr_pack_bytes(C.byref(d)))
    if nbytes <= 0:
        raise ValueError(f"unsupported network shape: in {d.inDim}, hidden {hidden} x {len(layers) - 1}, out {d.outDim} "
                         "(hidden in {32,64,128,256}, in <= 128, out <= 16, <= 8 layers)")
    w_flat = torch.from_numpy(np.concatenate([W.reshape(-1) for W, _ in layers])).to(dev)
    bias = np.concatenate([np.pad(b, (0, (-b.size) % 32)) for _, b in layers]).astype(np.float32)
    packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    biases = torch.from_numpy(bias).to(dev)
    d.weights, d.biases = packed.data_ptr(), biases.data_ptr()
    _lib.check(_lib.lib().mrirt_inr_pack_weights(C.byref(d), _ptr(w_flat), _ptr(packed), _stream_ptr(None)),
               "mrirt_inr_pack_weights")
    torch.cuda.current_stream().synchronize()           # w_flat may be freed after this returns
    return PackedMLP(d, packed, biases, int(d.inDim), int(d.outDim))


def _forward(net: PackedMLP, coords, feats, n: int, want_logits: bool, want_argmax: bool, refined: bool = False):
    dev = net.weights.device
    logits = torch.empty((n, net.out_dim), dtype=torch.float32, device=dev) if want_logits else None
    arg = torch.empty(n, dtype=torch.int16, device=dev) if want_argmax else None
    fn = _lib.lib().mrirt_inr_forward_refined if refined else _lib.lib().mrirt_inr_forward
    rc = fn(C.byref(net.desc), _ptr(coords), _ptr(feats), n, _ptr(logits), _ptr(arg), _stream_ptr(None))
    _lib.check(rc, "mrirt_inr_forward_refined" if refined else "mrirt_inr_forward")
    return logits, arg


def classify(net: PackedMLP, coords, feats, refined: bool = False, want_logits: bool = False):
    """argmax class (int16) of every point — the bf16 MFMA pass, with the points whose two largest logits are within
    the network's calibrated bf16 error re-evaluated in split bf16 (``mrirt_inr_forward``); ``refined=True`` evaluates
    every point in split bf16 (``mrirt_inr_forward_refined``).  Raw-x networks (KIND_RAW_*) take ``coords=None``."""
    dev = _require_gpu()
    f = _dev_f32(feats, dev)
    c = _dev_f32(coords, dev) if coords is not None else None
    logits, arg = _forward(net, c, f, f.shape[0], want_logits, True, refined)
    return (arg, logits) if want_logits else arg


def calibration(net: PackedMLP) -> Dict[str, float]:
    """The calibration record ``mrirt_inr_pack_weights`` measured for this network: rms / max difference between the
    bf16 pass's logits and the split-bf16 pass's over 8192 pseudo-random inputs, and the largest |logit| seen."""
    tail = net.weights[-1024:].view(torch.float32)[:4].cpu().numpy()
    return dict(rms_error=float(tail[0]), max_logit=float(tail[1]), max_error=float(tail[2]), points=int(tail[3]))


def _dev_f32(x, dev):
    return torch.as_tensor(np.asarray(x, dtype=np.float32) if not isinstance(x, torch.Tensor) else x,
                           dtype=torch.float32).to(dev).contiguous()


def build_input(coords, intensities, fourier_freqs: int) -> torch.Tensor:
    """(B,3) coords in [-1,1], (B,M) intensities -> (B, 3+6K+M) input matrix in the reference's
    feature order.  Provided for API parity; ``inr_forward`` builds the same features in-kernel."""
    dev = _require_gpu()
    c, f = _dev_f32(coords, dev), _dev_f32(intensities, dev)
    return torch.cat([c, fourier_features(c, fourier_freqs), f], dim=-1)


def inr_forward(params, coords, feats, fourier_freqs: int, net: Optional[PackedMLP] = None):
    """logits (B, classes) fp32 for points: Fourier features + ReLU MLP, fused."""
    dev = _require_gpu()
    f = _dev_f32(feats, dev)
    net = net or pack_mlp(params, KIND_FOURIER_RELU, fourier_freqs, f.shape[1])
    c = _dev_f32(coords, dev)
    return _forward(net, c, f, c.shape[0], True, False)[0]


def apply_mlp(params, x, net: Optional[PackedMLP] = None) -> torch.Tensor:
    """model.py:43-50 on an already-built input matrix x (B, in_dim)."""
    dev = _require_gpu()
    xx = _dev_f32(x, dev)
    net = net or pack_mlp(params, KIND_RAW_RELU)
    return _forward(net, None, xx, xx.shape[0], True, False)[0]


def siren_apply(params, x, w0: float = 30.0, net: Optional[PackedMLP] = None) -> torch.Tensor:
    dev = _require_gpu()
    xx = _dev_f32(x, dev)
    net = net or pack_mlp(params, KIND_RAW_SIREN, w0=w0)
    return _forward(net, None, xx, xx.shape[0], True, False)[0]


def predict_volume(params, case_data: Dict[str, Any], fourier_freqs: int, chunk: int = 200000,
                   net: Optional[PackedMLP] = None, prefilter_sigma: Optional[float] = None):
    """model.py:119-141: argmax class per voxel of ``case_data["mods"]`` (M,H,W,D) -> int16 (H,W,D).
    ``chunk`` is accepted for signature parity; the kernel streams the whole volume in one launch.
    ``prefilter_sigma``: every modality first goes through scipy.ndimage.gaussian_filter(mods[m], sigma) on the device
    (volume.gaussian_filter_device, bit for bit); 0.5 is what scripts/jax_inr_brats.py:266-270 applies."""
    dev = _require_gpu()
    mods = _dev_f32(case_data["mods"], dev)
    M, H, W, D = mods.shape
    if prefilter_sigma is not None:
        from . import volume
        filtered = torch.empty_like(mods)
        for m in range(M):
            volume.gaussian_filter_device(mods[m], prefilter_sigma, out=filtered[m])
        mods = filtered
    net = net or pack_mlp(params, KIND_FOURIER_RELU, fourier_freqs, M)
    pred = torch.empty((H, W, D), dtype=torch.int16, device=dev)
    hwd = (C.c_uint32 * 3)(H, W, D)
    rc = _lib.lib().mrirt_inr_predict_volume(C.byref(net.desc), _ptr(mods), hwd, _ptr(pred), _stream_ptr(None))
    _lib.check(rc, "mrirt_inr_predict_volume")
    return pred, case_data["seg"]


def prepare_case(mods_raw, seg=None, remap_label4: bool = True) -> Dict[str, Any]:
    """A raw case -> the dict VoxelCache, predict_volume and evaluate_single_case take, prepared on the device
    (dataloader.load_case / jax_inr_brats._load_case without the host): ``mods`` the (M, H, W, D) modalities z-scored over
    their non-zero voxels (volume.zscore_nonzero_device), ``seg`` the int16 labels with 4 -> 3 (``None`` stays ``None``),
    ``zstats`` the device (4, M) record { mu, sigma, sigma + 1e-6, count bits } (volume.zscore_constants reads it)."""
    from . import volume
    dev = _require_gpu()
    m = mods_raw if isinstance(mods_raw, torch.Tensor) else np.asarray(mods_raw, dtype=np.float32)
    if m.ndim != 4:
        raise ValueError(f"mods_raw: expected (M, H, W, D), got shape {tuple(m.shape)}")
    z, stats = volume.zscore_nonzero_device(m)
    lab = None
    if seg is not None:
        lab = _label_volume(seg, dev, "seg")
        if tuple(lab.shape) != tuple(z.shape[1:]):
            raise ValueError(f"seg has shape {tuple(lab.shape)}, the modalities {tuple(z.shape[1:])}")
        if remap_label4:
            lab = torch.where(lab == 4, torch.full_like(lab, 3), lab)
    return {"mods": z, "seg": lab, "zstats": stats}


def _label_counts(pred, true, num_classes: int):
    """Joint histogram of two label volumes: counts[p, t] for labels below ``num_classes`` (others in an overflow bin).
    NumPy arrays stay on the host; torch tensors are counted where they live (one bincount, one small read-back)."""
    n = int(num_classes)
    if isinstance(pred, torch.Tensor) or isinstance(true, torch.Tensor):
        dev = pred.device if isinstance(pred, torch.Tensor) else true.device
        p = torch.as_tensor(pred, device=dev).reshape(-1).to(torch.int64)
        t = torch.as_tensor(true, device=dev).reshape(-1).to(torch.int64)
        if p.numel() != t.numel():
            raise ValueError("dice: prediction and ground truth differ in size")
        p = torch.where((p < 0) | (p >= n), torch.full_like(p, n), p)
        t = torch.where((t < 0) | (t >= n), torch.full_like(t, n), t)
        return torch.bincount(p * (n + 1) + t, minlength=(n + 1) * (n + 1)).reshape(n + 1, n + 1).cpu().numpy()
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    t = np.asarray(true).reshape(-1).astype(np.int64)
    if p.size != t.size:
        raise ValueError("dice: prediction and ground truth differ in size")
    p = np.where((p < 0) | (p >= n), n, p)
    t = np.where((t < 0) | (t >= n), n, t)
    return np.bincount(p * (n + 1) + t, minlength=(n + 1) * (n + 1)).reshape(n + 1, n + 1)


def dice_score(pred, true, num_classes: int) -> Dict[int, float]:
    """Per-class Dice of two label volumes — the third name inr/interactive.ipynb imports from inr.model next to
    model_load and predict_volume (inr/inr/model.py:144-153): ``{c: (2 |P_c & T_c| + 1e-6) / (|P_c| + |T_c| + 1e-6)}``,
    NaN for a class that occurs in neither volume.  Accepts what ``predict_volume`` returns (a device tensor) as is."""
    h = _label_counts(pred, true, num_classes)
    out: Dict[int, float] = {}
    for c in range(int(num_classes)):
        denom = int(h[c, :].sum()) + int(h[:, c].sum())
        out[c] = (2 * int(h[c, c]) + 1e-6) / (denom + 1e-6) if denom > 0 else float("nan")
    return out


def coverage_dice(pred, true) -> float:
    """Dice of the foregrounds (label > 0) of two label volumes (inr/inr/model.py:156-161); 0.0 when both are empty."""
    pf = (pred > 0)
    tf = (true > 0)
    h = _label_counts(pf.to(torch.int64) if isinstance(pf, torch.Tensor) else np.asarray(pf, dtype=np.int64),
                      tf.to(torch.int64) if isinstance(tf, torch.Tensor) else np.asarray(tf, dtype=np.int64), 2)
    denom = int(h[1, :].sum()) + int(h[:, 1].sum())
    return (2 * int(h[1, 1]) + 1e-6) / (denom + 1e-6) if denom > 0 else 0.0


def compute_multi_metrics(pred, true, num_classes: int = 4) -> Dict[str, Any]:
    """notebooks/improved.ipynb's evaluation of a predicted volume, with its keys and its expressions:
    ``dice_class_{c}`` = (2 |P_c & T_c| + 1e-6) / (|P_c| + |T_c| + 1e-6), **0.0** (not NaN) for a class in neither volume;
    ``n_components_class_{c}`` for c = 1 .. num_classes - 1, the 6-connected components of ``pred == c`` (0 for an absent
    class; ``scipy.ndimage.label``'s count); ``slice_consistency``, the mean over the indices z >= 1 of the last axis with
    U > 0 of 2 I / (U + A[z] + A[z-1] + 1e-6) (``components.slice_counts``), 0.0 when there is none.
    A tensor prediction (what ``predict_volume`` returns) is evaluated on the device — the components by csrc/components.hip,
    the sums as integers, only those read back — and a NumPy prediction on the host, without a GPU."""
    from . import components
    n = int(num_classes)
    h = _label_counts(pred, true, n)
    out: Dict[str, Any] = {}
    for c in range(n):
        union = int(h[c, :].sum()) + int(h[:, c].sum())
        out[f"dice_class_{c}"] = (2 * int(h[c, c]) + 1e-6) / (union + 1e-6) if union > 0 else 0.0
    if isinstance(pred, torch.Tensor):
        dev = pred.device if pred.is_cuda else _require_gpu()
        lab = _label_volume(pred, dev, "pred")
        for c in range(1, n):
            out[f"n_components_class_{c}"] = components.label_components(lab, c, 1)[1]
        counts = components.slice_counts(lab).cpu().numpy()
    else:
        p = np.asarray(pred)
        if p.ndim != 3:
            raise ValueError(f"pred: expected an (H, W, D) volume, got shape {p.shape}")
        for c in range(1, n):
            out[f"n_components_class_{c}"] = components.count_components_host(p == c, 1)
        pos = p > 0
        counts = np.zeros((p.shape[2], 3), dtype=np.int64)
        counts[:, 0] = pos.sum(axis=(0, 1))
        counts[1:, 1] = ((p[:, :, 1:] == p[:, :, :-1]) & pos[:, :, 1:]).sum(axis=(0, 1))
        counts[1:, 2] = (pos[:, :, 1:] | pos[:, :, :-1]).sum(axis=(0, 1))
    ratios = [np.float64(2 * int(i)) / (int(u) + int(a) + int(a_prev) + 1e-6)
              for (a, i, u), a_prev in zip(counts[1:].tolist(), counts[:-1, 0].tolist()) if u > 0]
    out["slice_consistency"] = float(np.mean(ratios)) if ratios else 0.0
    return out


def _label_volume(x, dev, what: str) -> torch.Tensor:
    """A label volume (NumPy array or tensor, any integer dtype or bool) as the contiguous int16 (H, W, D) device tensor the
    kernels read.  A value that int16 cannot hold is no class's label: it becomes -1 instead of wrapping into one."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise TypeError(f"{what}: expected integer labels, got {t.dtype}")
    if t.dim() != 3:
        raise ValueError(f"{what}: expected an (H, W, D) volume, got shape {tuple(t.shape)}")
    t = t.to(dev)
    if t.dtype not in (torch.int16, torch.int8, torch.uint8, torch.bool):
        t = torch.where((t < -32768) | (t > 32767), torch.full_like(t, -1), t)
    return t.to(torch.int16).contiguous()


def _spacing3(spacing):
    sp = [float(np.float32(s)) for s in spacing]
    if len(sp) != 3:
        raise ValueError("spacing: expected three values (one per axis)")
    return (C.c_float * 3)(*sp)


def hausdorff_directed_sq(pred, true, spacing=(1.0, 1.0, 1.0), num_classes: int = 4) -> torch.Tensor:
    """(num_classes, 2) fp64 device tensor of ``mrirt_hausdorff``: [c, 0] = max over (pred == c) of the squared distance to
    (true == c), [c, 1] the other direction; NaN where the class is absent from either volume.  No host synchronisation."""
    dev = pred.device if isinstance(pred, torch.Tensor) and pred.is_cuda else (
        true.device if isinstance(true, torch.Tensor) and true.is_cuda else _require_gpu())
    p, t = _label_volume(pred, dev, "pred"), _label_volume(true, dev, "true")
    if p.shape != t.shape:
        raise ValueError(f"hausdorff: prediction {tuple(p.shape)} and ground truth {tuple(t.shape)} differ in shape")
    hwd = (C.c_uint32 * 3)(*p.shape)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = int(lib.mrirt_edt_scratch_bytes(hwd, int(num_classes)))
        out = torch.empty((max(int(num_classes), 0), 2), dtype=torch.float64, device=dev)
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=dev)
        rc = lib.mrirt_hausdorff(_ptr(p), _ptr(t), hwd, _spacing3(spacing), int(num_classes), _ptr(out), _ptr(scratch),
                                 nbytes, _stream_ptr(None))
    _lib.check(rc, "mrirt_hausdorff")
    return out


def hausdorff_distance(pred, true, spacing=(1.0, 1.0, 1.0), num_classes: int = 4) -> Dict[int, float]:
    """Per-class symmetric Hausdorff distance of two label volumes (inr/inr/model.py:164-195) — bit for bit what the
    reference's two cKDTrees per class return, from an exact fp64 distance transform on the GPU (csrc/edt.hip).  NumPy
    arrays are uploaded, device tensors (what ``predict_volume`` returns) are used where they are; any integer dtype.
    ``{c: float}``, NaN for a class that is absent from either volume."""
    d = hausdorff_directed_sq(pred, true, spacing, num_classes).cpu().numpy()
    out: Dict[int, float] = {}
    for c in range(int(num_classes)):
        a, b = float(d[c, 0]), float(d[c, 1])
        out[c] = float(np.sqrt(np.float64(max(a, b)))) if a == a and b == b else float("nan")
    return out


def distance_transform(mask_or_labels, cls: Optional[int] = None, spacing=(1.0, 1.0, 1.0)) -> torch.Tensor:
    """Exact squared Euclidean distance transform: fp64 (H, W, D) device tensor, at every voxel the squared distance to the
    nearest voxel of the mask (itself included: 0 on the mask), +inf everywhere when the mask is empty.  ``cls=None``: the
    mask is ``mask_or_labels != 0`` (a bool mask as is); otherwise ``mask_or_labels == cls``.  Coordinates are
    ``float32(index) * float32(spacing)`` widened to fp64, as in ``hausdorff_distance``."""
    dev = mask_or_labels.device if isinstance(mask_or_labels, torch.Tensor) and mask_or_labels.is_cuda else _require_gpu()
    if cls is None:
        m = mask_or_labels if isinstance(mask_or_labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask_or_labels))
        lab, cls = _label_volume(m != 0, dev, "mask"), 1
    else:
        lab = _label_volume(mask_or_labels, dev, "labels")
    hwd = (C.c_uint32 * 3)(*lab.shape)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = int(lib.mrirt_edt_scratch_bytes(hwd, 0))
        out = torch.empty(tuple(lab.shape), dtype=torch.float64, device=dev)
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=dev)
        rc = lib.mrirt_edt_squared(_ptr(lab), hwd, int(cls), _spacing3(spacing), _ptr(out), _ptr(scratch), nbytes, _stream_ptr(None))
    _lib.check(rc, "mrirt_edt_squared")
    return out


def evaluate_single_case(case_idx: int, case_data: Dict[str, Any], params, num_classes: int, fourier_freqs: int) -> Dict[str, Any]:
    """model.py:198-214, the evaluation every notebook and train.py run after training: predict the case's volume, then
    per-class Dice, Hausdorff (unit spacing, as the reference calls it), foreground Dice and the mean of the Dice scores
    that are not NaN.  The prediction stays on the device between the steps; ``pred_vol`` is that device tensor."""
    pred, seg = predict_volume(params, case_data, fourier_freqs)
    dice = dice_score(pred, seg, num_classes)
    finite = [v for v in dice.values() if v == v]
    return dict(case_idx=case_idx, pred_vol=pred, true_vol=seg, case_data=case_data, class_scores=dice,
                coverage_dice=coverage_dice(pred, seg), mean_dice=float(np.mean(finite)) if finite else 0.0,
                hausdorff_scores=hausdorff_distance(pred, seg, num_classes=num_classes))


_C5_SCRATCH: dict = {}


def render_brats_inr(params, intensities, net: PackedMLP, zmu, zsigma, labels=None, out=None, ext=None,
                     return_aux: bool = False, chunk_steps: Optional[int] = None, one_pass: bool = False):
    """BASELINE config 5 (build-defined): K1 with the prediction overlay's label taken
    from the MLP evaluated AT every march sample (normalised sample coordinates + the four
    trilinear-sampled, z-scored modalities) instead of ``sampleLabel(gPreds)``.

    ``net`` is a packed network over 4 modalities: the reference's Fourier/ReLU MLP
    (``pack_mlp(params, KIND_FOURIER_RELU, K, 4)``, inr/inr/model.py:11-50) or the notebook's SIREN
    (``pack_mlp(params, KIND_SIREN, 0, 4)``: x = (coords, modalities), neumors_inr.ipynb:853-899,1165-1178).
    ``zmu``/``zsigma`` are the per-modality z-score constants (brats_viewer.py:281-287).

    Default: ``mrirt_render_brats_inr`` — the march advances ``chunk_steps`` per pass and only rays that are still
    alive (t < t1, T > 0.01) have their next samples classified ("all live sample points"); no host
    synchronisation inside the frame.  ``chunk_steps=None`` picks the pass length from the scene: where the intensity
    channel alone cannot take any ray to T <= ert (intensityAlpha x box diagonal <= -ln ert — the reference viewer's whole
    slider range) no sample is classified in vain whatever the pass length, and 96-step passes are the
    fastest (fewer launches and refinement rounds: 10.13 / 9.88 / 9.68 / 9.72 / 9.76 ms per frame with 32 / 64 / 96 / 128 / 256
    steps on the config-5 scene, round 4); otherwise 32
    (a terminating ray wastes at most 31 samples; 8.9 against 9.2 ms on the dense preset).  Any value gives the same bits.  ``one_pass=True`` is the three-pass form over whole rays (count every
    sample in [t0,t1) -> emit -> ONE batched forward -> composite with the class stream); both give the same
    bits, and ``return_aux`` of the one-pass form exposes the emitted inputs and classes for the layered tests.
    """
    if net.desc.kind not in (KIND_FOURIER_RELU, KIND_SIREN) or net.desc.numMods != 4:
        raise ValueError("render_brats_inr needs a Fourier/ReLU or SIREN network over 4 modalities "
                         "(pack_mlp(params, KIND_FOURIER_RELU, K, 4) / pack_mlp(params, KIND_SIREN, 0, 4))")
    lib = _lib.lib()

    def chunked(P, E, vp, lab, mu, sg, chunk, scratch, o, pitch, st, s):
        _lib.check(lib.mrirt_render_brats_inr(C.byref(P), C.byref(E), vp, _ptr(lab), C.byref(net.desc), mu, sg, chunk, _ptr(scratch),
                                              scratch.numel(), _ptr(o), pitch, _ptr(st), s), "mrirt_render_brats_inr")

    def classify_all(coords, feats, total, classes, s):
        _lib.check(lib.mrirt_inr_forward(C.byref(net.desc), _ptr(coords), _ptr(feats), total, None, _ptr(classes), s), "mrirt_inr_forward")

    return _render_c5("render_brats_inr", params, intensities, zmu, zsigma, labels, out, ext, return_aux, chunk_steps, one_pass, chunked,
                      classify_all)


def _render_c5(who, params, intensities, zmu, zsigma, labels, out, ext, return_aux, chunk_steps, one_pass, chunked, classify_all):
    """The per-sample INR frame of render_brats_inr / render_brats_inject: binding, the ``chunk_steps=None`` rule, the scratch
    cache and both forms.  ``chunked(P, E, vp, lab, mu, sg, chunk, scratch, out, pitch, stats, stream)`` enqueues the one-call
    frame, ``classify_all(coords, feats, total, classes, stream)`` the one batched forward of the ``one_pass`` form."""
    from .render import Grid, _alloc_out, _bind_brats
    dev = _require_gpu()
    if isinstance(intensities, Grid):                    # one "mod4" grid (upload_mod4) carries all four modalities
        if intensities.layout != "mod4":
            raise ValueError("a single grid must be the 'mod4' grid of upload_mod4; per-modality grids go in a list of four")
        if one_pass:
            raise ValueError("the whole-ray three-pass form marches with the K1 kernels: bind per-modality grids")
        intensities = [intensities] * 4
    if int(params["showPred"]) == 0:
        raise ValueError(f"{who} draws the prediction overlay: set gParams.showPred")
    P, E, vols, lab, _, _ = _bind_brats(params, intensities, labels, None, ext, dev, pred_stream=True)
    if any(v is None for v in vols):
        raise ValueError("the MLP reads all four modalities: bind gIntensity0..3")
    if E.tileSize > 0:
        raise ValueError(f"{who} renders whole frames")
    w, h = int(P.imageSize[0]), int(P.imageSize[1])
    lib, s = _lib.lib(), _stream_ptr(None)
    vp = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) for t in vols])
    mu = (C.c_float * 4)(*[float(np.float32(v)) for v in zmu])
    sg = (C.c_float * 4)(*[float(np.float32(v)) for v in zsigma])
    if chunk_steps is None:
        diag = float(np.sqrt(sum((float(P.voxelSize[k]) * int(P.dims[k])) ** 2 for k in range(3))))
        ert = float(E.ertThreshold) if int(E.ertOverride) else 0.01
        chunk_steps = 96 if ert > 0.0 and float(P.intensityAlpha) * diag <= -np.log(ert) else 32
    if not one_pass:
        nbytes = int(lib.mrirt_brats_inr_scratch_bytes(C.byref(P), int(chunk_steps)))
        if nbytes <= 0:
            raise ValueError(f"chunk_steps={chunk_steps}: unsupported (1..4096, image x chunk < 2^32 samples per pass)")
        key = (dev.index, torch.cuda.current_stream().cuda_stream)
        scratch = _C5_SCRATCH.get(key)                    # one scratch per (device, stream): reused frame to frame
        if scratch is None or scratch.numel() < nbytes:
            scratch = _C5_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        o, pitch = _alloc_out(w, h, E, dev, out)
        st = torch.zeros(3, dtype=torch.int64, device=dev) if return_aux else None
        chunked(P, E, vp, lab, mu, sg, int(chunk_steps), scratch, o, pitch, st, s)
        if return_aux:
            c = st.cpu()
            return o, dict(live_samples=int(c[0]), shaded_samples=int(c[1]), queries=int(c[2]), chunk_steps=int(chunk_steps))
        return o
    counts = torch.empty(h * w, dtype=torch.int32, device=dev)
    _lib.check(lib.mrirt_brats_sample_counts(C.byref(P), C.byref(E), _ptr(counts), s), "mrirt_brats_sample_counts")
    ends = torch.cumsum(counts.to(torch.int64), 0)
    offsets = (ends - counts).contiguous()
    total = int(ends[-1])
    coords = torch.empty((max(total, 1), 3), dtype=torch.float32, device=dev)
    feats = torch.empty((max(total, 1), 4), dtype=torch.float32, device=dev)
    classes = torch.zeros(max(total, 1), dtype=torch.int16, device=dev)
    _lib.check(lib.mrirt_brats_emit_samples(C.byref(P), C.byref(E), vp, mu, sg, _ptr(offsets), _ptr(coords), _ptr(feats), s),
               "mrirt_brats_emit_samples")
    if total:
        classify_all(coords, feats, total, classes, s)
    o, pitch = _alloc_out(w, h, E, dev, out)
    st = torch.zeros(2, dtype=torch.int64, device=dev) if return_aux else None
    _lib.check(lib.mrirt_render_brats_stream(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(classes), _ptr(offsets),
                                             _ptr(o), pitch, _ptr(st), s), "mrirt_render_brats_stream")
    if return_aux:
        c = st.cpu()
        return o, dict(queries=total, live_samples=int(c[0]), shaded_samples=int(c[1]), classes=classes, offsets=offsets, coords=coords,
                       feats=feats, counts=counts)
    return o


def labels_for_viewer(pred_hwd: torch.Tensor) -> torch.Tensor:
    """pred (H,W,D) -> the viewer's x-fastest uint32 label buffer (brats_viewer.py:297-299)."""
    return pred_hwd.permute(2, 1, 0).reshape(-1).to(torch.int32).contiguous()


# --- training step: fp32 forward, loss and weight gradients (csrc/inr_train.hip) ------------------------------------------------
def _step_desc(dims: Sequence[int], kind: int, fourier_freqs: int, num_mods: int, w0: float = 0.0) -> _lib.InrDesc:
    dims = [int(v) for v in dims]
    if len(dims) < 3 or any(v != dims[1] for v in dims[1:-1]):
        raise ValueError(f"layer widths {dims}: the kernels need at least one hidden layer and equal hidden widths")
    d = _lib.InrDesc()
    d.kind, d.numLayers, d.inDim, d.hidden, d.outDim = kind, len(dims) - 1, dims[0], dims[1], dims[-1]
    d.fourierFreqs, d.numMods, d.w0 = int(fourier_freqs), int(num_mods), float(w0)
    return d


def train_desc(dims: Sequence[int], fourier_freqs: Optional[int] = None, num_mods: int = 0) -> _lib.InrDesc:
    """Descriptor of a ReLU network ``dims = [in, hidden, .., hidden, out]`` for the fp32 training entry points:
    ``fourier_freqs=None`` is the raw kind (the input matrix is given), otherwise the Fourier kind over ``num_mods``
    intensities.  The packed inference images (``desc.weights`` / ``desc.biases``) stay unset: nothing here reads them."""
    return _step_desc(dims, KIND_RAW_RELU, 0, 0) if fourier_freqs is None else _step_desc(dims, KIND_FOURIER_RELU, fourier_freqs, num_mods)


def _param_dims(Ws, bs) -> List[int]:
    dims = [int(Ws[0].shape[0])] + [int(W.shape[1]) for W in Ws]
    for i, (W, b) in enumerate(zip(Ws, bs)):
        if tuple(W.shape) != (dims[i], dims[i + 1]) or tuple(b.shape) != (dims[i + 1],):
            raise ValueError(f"layer {i}: W {tuple(W.shape)} / b {tuple(b.shape)} do not chain")
    return dims


# mrirt_inr_* takes the ReLU kinds, mrirt_siren_* the SIREN kinds.  The public twins name their family, so the library still
# refuses a descriptor of the other one; the autograd function and the loss closure go by the descriptor's kind.
_SHAPE_TEXT = {"inr": ("", "ReLU kinds", ""), "siren": ("SIREN ", "SIREN kinds", ", finite w0 != 0")}


def _family(desc: _lib.InrDesc) -> str:
    return "siren" if int(desc.kind) in (KIND_SIREN, KIND_RAW_SIREN) else "inr"


def _step_symbol(desc: _lib.InrDesc, job: str, family: Optional[str] = None) -> str:
    """The C entry point of ``job`` ("train_scratch_bytes", "forward_f32", "backward") for ``family``, or for the descriptor's."""
    return f"mrirt_{family or _family(desc)}_{job}"


def _step_scratch(desc: _lib.InrDesc, n: int, dev, family: Optional[str] = None) -> torch.Tensor:
    family = family or _family(desc)
    nbytes = int(getattr(_lib.lib(), _step_symbol(desc, "train_scratch_bytes", family))(C.byref(desc), int(n)))
    if nbytes <= 0:
        what, kinds, more = _SHAPE_TEXT[family]
        raise ValueError(f"unsupported {what}training shape: in {desc.inDim}, hidden {desc.hidden} x {desc.numLayers - 1}, out {desc.outDim}, "
                         f"n {n} ({kinds}, hidden in {{32,64,128,256}}, in <= 128, out <= 16, <= 8 layers, n >= 1{more})")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _step_forward(desc, w_flat, b_flat, coords, feats, n, scratch, family=None):
    name = _step_symbol(desc, "forward_f32", family)
    logits = torch.empty((int(n), int(desc.outDim)), dtype=torch.float32, device=w_flat.device)
    rc = getattr(_lib.lib(), name)(C.byref(desc), _ptr(w_flat), _ptr(b_flat), _ptr(coords), _ptr(feats), int(n), _ptr(logits),
                                   _ptr(scratch), scratch.numel(), _stream_ptr(None))
    _lib.check(rc, name)
    return logits


def _step_backward(desc, w_flat, n, dlogits, scratch, grad_w=None, grad_b=None, accumulate=False, family=None):
    name = _step_symbol(desc, "backward", family)
    nb = int(desc.hidden) * (int(desc.numLayers) - 1) + int(desc.outDim)
    gw = grad_w if grad_w is not None else torch.empty_like(w_flat)
    gb = grad_b if grad_b is not None else torch.empty(nb, dtype=torch.float32, device=w_flat.device)
    rc = getattr(_lib.lib(), name)(C.byref(desc), _ptr(w_flat), int(n), _ptr(dlogits), _ptr(gw), _ptr(gb), 1 if accumulate else 0,
                                   _ptr(scratch), scratch.numel(), _stream_ptr(None))
    _lib.check(rc, name)
    return gw, gb


def train_scratch(desc: _lib.InrDesc, n: int, dev) -> torch.Tensor:
    return _step_scratch(desc, n, dev, "inr")


def forward_f32(desc: _lib.InrDesc, w_flat: torch.Tensor, b_flat: torch.Tensor, coords, feats, n: int, scratch: torch.Tensor):
    """``mrirt_inr_forward_f32``: fp32 logits (n, out); the activations the backward pass needs stay in ``scratch``."""
    return _step_forward(desc, w_flat, b_flat, coords, feats, n, scratch, "inr")


def loss_ext(class_weights, dice_weight: float = 0.0, per_class_dice: bool = False, focal_gamma: float = 0.0, focal_alpha=None,
             label_smoothing: float = 0.0, edema_fp_weight: float = 0.0, tversky_edema_alpha: float = 0.8, tversky_edema_beta: float = 0.2,
             tversky_edema_weight: float = 0.0, edema_logit_reg: float = 0.0, edema_class: int = 2) -> _lib.InrLossExt:
    """``MrirtInrLossExt`` from the loss flags of scripts/jax_inr_brats.py (``--dice-weight``, ``--per-class-dice``,
    ``--focal-gamma``, ``--focal-alpha``, ``--label-smoothing``, ``--edema-fp-weight``, ``--tversky-edema-alpha / -beta /
    -weight``, ``--edema-logit-reg``, ``--class-weights``) with the script's defaults: without ``per_class_dice`` the Dice is
    prevalence-weighted.  ``edema_class`` is the script's 2.  The library checks the values when the struct is used."""
    x = _lib.InrLossExt()
    cw = [float(np.float32(v)) for v in np.asarray(class_weights, dtype=np.float32).reshape(-1)]
    if len(cw) > 16:
        raise ValueError("at most 16 classes")
    for k, v in enumerate(cw):
        x.classWeights[k] = v
    flags = _lib.LOSS_PER_CLASS_DICE if per_class_dice else 0
    if focal_alpha is not None:
        fa = [float(np.float32(v)) for v in np.asarray(focal_alpha, dtype=np.float32).reshape(-1)]
        if len(fa) != len(cw):
            raise ValueError(f"focal_alpha holds {len(fa)} values for {len(cw)} class weights")
        for k, v in enumerate(fa):
            x.focalAlpha[k] = v
        flags |= _lib.LOSS_FOCAL_ALPHA
    x.diceWeight, x.focalGamma, x.labelSmoothing = float(dice_weight), float(focal_gamma), float(label_smoothing)
    x.edemaFpWeight, x.tverskyAlpha, x.tverskyBeta = float(edema_fp_weight), float(tversky_edema_alpha), float(tversky_edema_beta)
    x.tverskyWeight, x.edemaLogitReg, x.edemaClass, x.flags = float(tversky_edema_weight), float(edema_logit_reg), int(edema_class), flags
    return x


def _loss_ext_and_dlogits(logits: torch.Tensor, labels: torch.Tensor, ext: _lib.InrLossExt, want_grad: bool):
    n, nc = int(logits.shape[0]), int(logits.shape[1])
    dev = logits.device
    scratch = torch.empty(max(int(_lib.lib().mrirt_inr_loss_ext_scratch_bytes(n)), 16), dtype=torch.uint8, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    aux = torch.empty((2, nc), dtype=torch.float32, device=dev)
    terms = torch.empty(5, dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if want_grad else None
    rc = _lib.lib().mrirt_inr_loss_ext(_ptr(logits), _ptr(labels), n, nc, C.byref(ext), _ptr(loss), _ptr(aux), _ptr(terms), _ptr(dl),
                                       _ptr(scratch), scratch.numel(), _stream_ptr(None))
    _lib.check(rc, "mrirt_inr_loss_ext")
    return loss.reshape(()), aux, dl, terms


def loss_and_dlogits(logits: torch.Tensor, labels: torch.Tensor, class_weights, dice_weight: float, scratch=None,
                     want_grad: bool = True, ext: Optional[_lib.InrLossExt] = None):
    """``mrirt_inr_loss`` on (n, C) logits and int32 labels: (loss 0-d, aux (2, C): CE per class, Dice per class,
    dlogits (n, C) or None), all on the device.  With ``ext`` (``loss_ext(...)``) the loss is ``mrirt_inr_loss_ext``'s —
    ``class_weights`` / ``dice_weight`` are then not read, the loss sums get a scratch of their own — and a fourth value is
    returned: terms (5,) = CE, Dice loss, edema FP / n, Tversky index, logit-regulariser mean."""
    if ext is not None:
        return _loss_ext_and_dlogits(logits, labels, ext, want_grad)
    n, nc = int(logits.shape[0]), int(logits.shape[1])
    cw = [float(np.float32(v)) for v in class_weights]
    if len(cw) != nc:
        raise ValueError(f"class_weights holds {len(cw)} values for {nc} classes")
    dev = logits.device
    if scratch is None:
        scratch = torch.empty(max(int(_lib.lib().mrirt_inr_loss_scratch_bytes(n)), 16), dtype=torch.uint8, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    aux = torch.empty((2, nc), dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if want_grad else None
    rc = _lib.lib().mrirt_inr_loss(_ptr(logits), _ptr(labels), n, nc, (C.c_float * nc)(*cw), float(dice_weight), _ptr(loss), _ptr(aux),
                                   _ptr(dl), _ptr(scratch), scratch.numel(), _stream_ptr(None))
    _lib.check(rc, "mrirt_inr_loss")
    return loss.reshape(()), aux, dl


def backward_f32(desc: _lib.InrDesc, w_flat: torch.Tensor, n: int, dlogits: torch.Tensor, scratch: torch.Tensor,
                 grad_w: Optional[torch.Tensor] = None, grad_b: Optional[torch.Tensor] = None, accumulate: bool = False):
    """``mrirt_inr_backward``: (grad_w, grad_b) in the flat layouts of the weights / biases, from what ``forward_f32`` left in
    ``scratch``.  ``accumulate`` adds into the given buffers."""
    return _step_backward(desc, w_flat, n, dlogits, scratch, grad_w, grad_b, accumulate, "inr")


def _split_grads(gw: torch.Tensor, gb: torch.Tensor, dims: Sequence[int]):
    out, wo, bo = [], 0, 0
    for i in range(len(dims) - 1):
        a, b = dims[i], dims[i + 1]
        out.append({"W": gw[wo:wo + a * b].view(a, b), "b": gb[bo:bo + b]})
        wo, bo = wo + a * b, bo + b
    return out


def _make_step_loss_and_grad(num_classes: int, class_weights, dice_weight: float, ext: Optional[_lib.InrLossExt], make_desc):
    """The closure of ``make_loss_and_grad`` for either family: ``make_desc(dims, num_mods)`` gives the descriptor."""
    cw = [float(v) for v in np.asarray(class_weights, dtype=np.float32).reshape(-1)]
    if len(cw) != int(num_classes):
        raise ValueError(f"class_weights holds {len(cw)} values for {num_classes} classes")

    def loss_and_grad(params, coords, intensities, labels):
        dev = _require_gpu()
        Ws = [_dev_f32(p["W"], dev) for p in params]
        bs = [_dev_f32(p["b"], dev) for p in params]
        dims = _param_dims(Ws, bs)
        if dims[-1] != int(num_classes):
            raise ValueError(f"the network has {dims[-1]} outputs for {num_classes} classes")
        c, f = _dev_f32(coords, dev), (_dev_f32(intensities, dev) if intensities is not None else None)
        n = int(c.shape[0])
        lab = torch.as_tensor(labels).to(dev).to(torch.int32).contiguous()
        desc = make_desc(dims, f.shape[1] if f is not None and f.dim() == 2 else 0)
        w_flat, b_flat = torch.cat([W.reshape(-1) for W in Ws]), torch.cat(bs)
        scratch = _step_scratch(desc, n, dev)
        logits = _step_forward(desc, w_flat, b_flat, c, f, n, scratch)
        loss, aux, dl, *terms = loss_and_dlogits(logits, lab, cw, dice_weight, scratch, ext=ext)
        gw, gb = _step_backward(desc, w_flat, n, dl, scratch)
        return (loss, {"ce_per_class": aux[0], "dice_per_class": aux[1], **({"terms": terms[0]} if terms else {})}), _split_grads(gw, gb, dims)

    return loss_and_grad


def make_loss_and_grad(num_classes: int, class_weights, dice_weight: float, fourier_freqs: int, ext: Optional[_lib.InrLossExt] = None):
    """inr/inr/model.py:64-90 on the GPU: returns ``f(params, coords, intensities, labels) -> ((loss, aux), grads)`` with the
    reference's return shape — ``loss`` a 0-d device tensor, ``aux = {"ce_per_class", "dice_per_class"}`` (device, (C,)),
    ``grads`` a list of ``{"W", "b"}`` device tensors shaped like ``params`` (NumPy arrays or device tensors);
    ``intensities`` may be None for a network without modalities.  One fp32
    forward, the loss and one backward pass (csrc/inr_train.hip); nothing synchronises with the host.  ``ext``
    (``loss_ext(...)``): the loss is ``mrirt_inr_loss_ext``'s and ``aux`` gains ``"terms"`` (5,)."""
    return _make_step_loss_and_grad(num_classes, class_weights, dice_weight, ext, lambda dims, m: train_desc(dims, fourier_freqs, m))


class _StepF32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coords, feats, make_desc, num_layers, *wb):
        Ws, bs = wb[:num_layers], wb[num_layers:]
        dims = _param_dims(Ws, bs)
        desc = make_desc(dims)
        n = int((feats if int(desc.kind) in (KIND_RAW_RELU, KIND_RAW_SIREN) else coords).shape[0])
        w_flat = torch.cat([W.detach().to(torch.float32).reshape(-1) for W in Ws])
        b_flat = torch.cat([b.detach().to(torch.float32).reshape(-1) for b in bs])
        scratch = _step_scratch(desc, n, Ws[0].device)
        logits = _step_forward(desc, w_flat, b_flat, coords, feats, n, scratch)
        ctx.desc, ctx.dims, ctx.n, ctx.w_flat, ctx.scratch = desc, dims, n, w_flat, scratch
        return logits

    @staticmethod
    def backward(ctx, grad_logits):
        gw, gb = _step_backward(ctx.desc, ctx.w_flat, ctx.n, grad_logits.to(torch.float32).contiguous(), ctx.scratch)
        g = _split_grads(gw, gb, ctx.dims)
        return (None, None, None, None, *[x["W"] for x in g], *[x["b"] for x in g])


def _step_autograd(Ws, bs, coords, feats, make_desc) -> torch.Tensor:
    dev = Ws[0].device
    c = _dev_f32(coords, dev) if coords is not None else None
    f = _dev_f32(feats, dev) if feats is not None else None
    return _StepF32.apply(c, f, lambda dims: make_desc(dims, f.shape[1] if f is not None else 0), len(Ws), *Ws, *bs)


def mlp_autograd(Ws, bs, coords, feats, fourier_freqs: Optional[int] = None) -> torch.Tensor:
    """Differentiable fp32 logits (n, out) of a ReLU MLP: the forward is ``mrirt_inr_forward_f32``, the backward
    ``mrirt_inr_backward`` — gradients reach ``Ws`` (each (in, out)) and ``bs`` only, so any torch loss and optimiser can fit
    the network.  ``fourier_freqs=None``: ``feats`` is the (n, in) input matrix and ``coords`` is unused; otherwise the
    inputs are built from coords (n, 3) and intensities ``feats`` (n, M) as ``build_input`` does."""
    return _step_autograd(Ws, bs, coords, feats, lambda dims, m: train_desc(dims, fourier_freqs, m))


# --- training loop: voxel cache + sampler, clipped AdamW, train_inr (csrc/inr_optim.hip) ---------------------------------------
ADAMW_B1, ADAMW_B2, ADAMW_EPS, ADAMW_WEIGHT_DECAY = 0.9, 0.999, 1e-8, 1e-4      # optax.adamw's defaults, as train.py uses them
CHECKPOINT_BASENAME = "checkpoint_step{step:06d}.npz"


class VoxelCache:
    """Device-resident cases of one shape with a counter-based voxel sampler (``StreamingBraTSCache`` + ``sample_batch``,
    inr/inr/dataloader.py:86-96,133-155).  ``cases``: a list of ``{"mods": (M, H, W, D) float, "seg": (H, W, D) integer}``,
    NumPy arrays or tensors; the cache keeps the device copies alive and holds the two pointer tables the kernel reads."""

    def __init__(self, cases: Sequence[Dict[str, Any]]):
        dev = _require_gpu()
        if len(cases) < 1:
            raise ValueError("VoxelCache needs at least one case")
        self.mods = [_dev_f32(c["mods"], dev) for c in cases]
        self.seg = [_label_volume(c["seg"], dev, "seg") for c in cases]
        shape = tuple(self.seg[0].shape)
        M = int(self.mods[0].shape[0])
        for m, s in zip(self.mods, self.seg):
            if m.dim() != 4 or tuple(m.shape) != (M, *shape) or tuple(s.shape) != shape:
                raise ValueError(f"every case must be mods {(M, *shape)} + seg {shape}; got {tuple(m.shape)} + {tuple(s.shape)}")
        self.n_cases, self.n_modalities, self.vol_shape, self.device = len(cases), M, shape, dev
        self.cache = [{"mods": m, "seg": s} for m, s in zip(self.mods, self.seg)]
        self.seg_table = torch.tensor([s.data_ptr() for s in self.seg], dtype=torch.int64, device=dev)
        self.mods_table = torch.tensor([m.data_ptr() for m in self.mods], dtype=torch.int64, device=dev) if M > 0 else None
        c = _lib.InrCache()
        c.mods, c.seg = (self.mods_table.data_ptr() if M > 0 else None), self.seg_table.data_ptr()
        c.ncases, c.numMods = self.n_cases, M
        c.hwd[0], c.hwd[1], c.hwd[2] = shape
        self.desc = c
        self._tumour = None
        self._classes: Dict[int, Any] = {}

    def tumour_index(self) -> _lib.InrTumourIndex:
        """``MrirtInrTumourIndex`` of the cache: the flat offsets of every case's voxels with seg > 0, ascending, built on the
        first call by ``mrirt_inr_tumour_count`` (one read of the per-case counts: load time) and ``mrirt_inr_tumour_index``,
        and kept alive with the cache (``tumour_offsets`` int64 (ncases + 1,), ``tumour_voxels`` a uint32 array viewed as int32)."""
        if self._tumour is None:
            lib, dev = _lib.lib(), self.device
            counts = torch.empty(self.n_cases, dtype=torch.int64, device=dev)
            _lib.check(lib.mrirt_inr_tumour_count(C.byref(self.desc), _ptr(counts), _stream_ptr(None)), "mrirt_inr_tumour_count")
            offsets = torch.zeros(self.n_cases + 1, dtype=torch.int64)
            offsets[1:] = torch.cumsum(counts.cpu(), 0)
            self.tumour_offsets = offsets.to(dev)
            self.tumour_voxels = torch.empty(max(int(offsets[-1]), 1), dtype=torch.int32, device=dev)
            nbytes = int(lib.mrirt_inr_tumour_index_scratch_bytes(C.byref(self.desc)))
            if nbytes <= 0:
                raise ValueError("tumour_index: the volume has 2^32 voxels or more")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.mrirt_inr_tumour_index(C.byref(self.desc), _ptr(self.tumour_offsets), _ptr(self.tumour_voxels), _ptr(scratch), nbytes,
                                                  _stream_ptr(None)), "mrirt_inr_tumour_index")
            torch.cuda.current_stream(dev).synchronize()          # the scratch dies here
            self._tumour = _lib.InrTumourIndex(self.tumour_voxels.data_ptr(), self.tumour_offsets.data_ptr())
        return self._tumour

    def sample(self, seed: int, batch_index: int, n: int, n_tumour: int = 0):
        """Micro-batch ``batch_index`` of the stream ``seed`` (``mrirt_inr_sample_batch``): (coords (n, 3) fp32,
        intensities (n, M) fp32, labels (n,) int32) on the device — the return order of the reference's ``sample_batch``.
        ``n_tumour > 0``: the first ``n_tumour`` points are drawn from the tumour voxels (``mrirt_inr_sample_batch_mix``; the
        other points keep their bits)."""
        dev = self.device
        coords = torch.empty((int(n), 3), dtype=torch.float32, device=dev)
        feats = torch.empty((int(n), self.n_modalities), dtype=torch.float32, device=dev)
        labels = torch.empty(int(n), dtype=torch.int32, device=dev)
        if int(n_tumour) != 0:
            rc = _lib.lib().mrirt_inr_sample_batch_mix(C.byref(self.desc), C.byref(self.tumour_index()), int(seed) & (2 ** 64 - 1),
                                                       int(batch_index) & (2 ** 64 - 1), int(n), int(n_tumour), _ptr(coords),
                                                       _ptr(feats) if self.n_modalities else None, _ptr(labels), _stream_ptr(None))
            _lib.check(rc, "mrirt_inr_sample_batch_mix")
            return coords, feats, labels
        rc = _lib.lib().mrirt_inr_sample_batch(C.byref(self.desc), int(seed) & (2 ** 64 - 1), int(batch_index) & (2 ** 64 - 1), int(n),
                                               _ptr(coords), _ptr(feats) if self.n_modalities else None, _ptr(labels), _stream_ptr(None))
        _lib.check(rc, "mrirt_inr_sample_batch")
        return coords, feats, labels

    def set_boundary(self, maps=None) -> List[torch.Tensor]:
        """Give the cache the boundary weight maps of the notebook's cache (cell 5): ``maps`` a list of (H, W, D) fp32 volumes,
        one per case, or None to build each with ``boundary_weights(seg)``.  The cache keeps the device copies and the table
        of their pointers, which ``sample_field`` reads."""
        if maps is None:
            maps = [boundary_weights(s) for s in self.seg]
        maps = [_dev_f32(m, self.device) for m in maps]
        if len(maps) != self.n_cases or any(tuple(m.shape) != self.vol_shape for m in maps):
            raise ValueError(f"set_boundary needs {self.n_cases} maps of shape {self.vol_shape}")
        self.boundary = maps
        self.boundary_table = torch.tensor([m.data_ptr() for m in maps], dtype=torch.int64, device=self.device)
        return maps

    def sample_field(self, seed: int, batch_index: int, n: int, n_tumour: int = 0) -> torch.Tensor:
        """``mrirt_inr_sample_field``: the boundary map's values (n,) fp32 at the voxels ``sample(seed, batch_index, n,
        n_tumour)`` draws, point by point.  ``set_boundary`` must have been called."""
        if getattr(self, "boundary_table", None) is None:
            raise ValueError("sample_field: call set_boundary() first")
        out = torch.empty(int(n), dtype=torch.float32, device=self.device)
        tumour = C.byref(self.tumour_index()) if int(n_tumour) != 0 else None
        rc = _lib.lib().mrirt_inr_sample_field(C.byref(self.desc), tumour, _ptr(self.boundary_table), int(seed) & (2 ** 64 - 1),
                                               int(batch_index) & (2 ** 64 - 1), int(n), int(n_tumour), _ptr(out), _stream_ptr(None))
        _lib.check(rc, "mrirt_inr_sample_field")
        return out

    def class_index(self, num_classes: int) -> _lib.InrClassIndex:
        """``MrirtInrClassIndex`` of the cache for ``num_classes`` classes: the flat offsets of the voxels with a label in
        ``0 .. num_classes - 1``, by class, then case, then ascending, built on the first call for that ``num_classes`` by
        ``mrirt_inr_class_count`` (one read of the (case, class) counts: load time) and ``mrirt_inr_class_index``, and kept
        alive with the cache (``class_offsets[C]`` int64 (C ncases + 1,), ``class_voxels[C]`` a uint32 array viewed as int32)."""
        nc = int(num_classes)
        if nc not in self._classes:
            lib, dev = _lib.lib(), self.device
            nbytes = int(lib.mrirt_inr_class_index_scratch_bytes(C.byref(self.desc), nc))
            if nbytes <= 0:
                raise ValueError("class_index: num_classes must be 1..16 and the volume smaller than 2^32 voxels")
            counts = torch.empty((self.n_cases, nc), dtype=torch.int64, device=dev)
            _lib.check(lib.mrirt_inr_class_count(C.byref(self.desc), nc, _ptr(counts), _stream_ptr(None)), "mrirt_inr_class_count")
            offsets = torch.zeros(nc * self.n_cases + 1, dtype=torch.int64)
            offsets[1:] = torch.cumsum(counts.cpu().T.reshape(-1), 0)           # (class, case) order
            d_offsets = offsets.to(dev)
            voxels = torch.empty(max(int(offsets[-1]), 1), dtype=torch.int32, device=dev)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.mrirt_inr_class_index(C.byref(self.desc), nc, _ptr(d_offsets), _ptr(voxels), _ptr(scratch), nbytes, _stream_ptr(None)),
                       "mrirt_inr_class_index")
            torch.cuda.current_stream(dev).synchronize()          # the scratch dies here
            self._classes[nc] = (_lib.InrClassIndex(voxels.data_ptr(), d_offsets.data_ptr(), nc, 0), d_offsets, voxels)
        return self._classes[nc][0]

    @property
    def class_offsets(self) -> Dict[int, torch.Tensor]:
        return {k: v[1] for k, v in self._classes.items()}

    @property
    def class_voxels(self) -> Dict[int, torch.Tensor]:
        return {k: v[2] for k, v in self._classes.items()}

    def _rows(self, n: int):
        dev = self.device
        return (torch.empty((int(n), 3), dtype=torch.float32, device=dev), torch.empty((int(n), self.n_modalities), dtype=torch.float32, device=dev),
                torch.empty(int(n), dtype=torch.int32, device=dev))

    def sample_candidates(self, seed: int, batch_index: int, n_cand: int):
        """``mrirt_inr_sample_candidates``: the ``n_cand`` candidate voxels of micro-batch ``batch_index`` (the sampler's draw at
        counter word 3 = 1) as ``sample`` returns a batch: (coords, intensities, labels) on the device."""
        coords, feats, labels = self._rows(n_cand)
        rc = _lib.lib().mrirt_inr_sample_candidates(C.byref(self.desc), int(seed) & (2 ** 64 - 1), int(batch_index) & (2 ** 64 - 1), int(n_cand),
                                                    _ptr(coords), _ptr(feats) if self.n_modalities else None, _ptr(labels), _stream_ptr(None))
        _lib.check(rc, "mrirt_inr_sample_candidates")
        return coords, feats, labels

    def sample_hybrid(self, seed: int, batch_index: int, n: int, n_uncertain: int = 0, picks=None, n_per_class: int = 0, num_classes: int = 4,
                      noise_sigma: float = 0.0, with_field: bool = False):
        """``mrirt_inr_sample_batch_hybrid``: micro-batch ``batch_index`` with its first ``n_uncertain`` rows the candidates
        ``picks`` (uint32 indices into ``sample_candidates``' stream: a device int32 tensor holding those bits, as
        ``select_largest`` returns, or anything NumPy reads as uint32), then ``n_per_class`` voxels of each of ``num_classes``
        classes from ``class_index(num_classes)``, then the rows of ``sample``; ``noise_sigma > 0`` adds ``noise_sigma *
        normal3(seed, batch_index, n)`` to the coordinates.  Returns (coords, intensities, labels), and with ``with_field`` also
        the boundary map's values (n,) at the rows' voxels (``set_boundary`` must have been called)."""
        dev = self.device
        hy = _lib.InrHybrid()
        hy.nUncertain, hy.nPerClass, hy.noiseSigma, hy.reserved = int(n_uncertain), int(n_per_class), float(noise_sigma), 0
        if int(n_uncertain) > 0:
            if picks is None:
                raise ValueError("sample_hybrid: n_uncertain > 0 needs picks")
            if not isinstance(picks, torch.Tensor):
                picks = torch.from_numpy(np.ascontiguousarray(np.asarray(picks).astype(np.uint32)).view(np.int32))
            picks = picks.to(dev).contiguous()
            if picks.dtype != torch.int32 or picks.numel() < int(n_uncertain):
                raise ValueError(f"sample_hybrid: picks must hold {n_uncertain} 32-bit indices")
            hy.picks = picks.data_ptr()
        classes = C.byref(self.class_index(num_classes)) if int(n_per_class) > 0 else None
        field = None
        if with_field:
            if getattr(self, "boundary_table", None) is None:
                raise ValueError("sample_hybrid: call set_boundary() first")
            field = torch.empty(int(n), dtype=torch.float32, device=dev)
        coords, feats, labels = self._rows(n)
        rc = _lib.lib().mrirt_inr_sample_batch_hybrid(C.byref(self.desc), classes, C.byref(hy), _ptr(self.boundary_table) if with_field else None,
                                                      int(seed) & (2 ** 64 - 1), int(batch_index) & (2 ** 64 - 1), int(n), _ptr(coords),
                                                      _ptr(feats) if self.n_modalities else None, _ptr(labels), _ptr(field), _stream_ptr(None))
        _lib.check(rc, "mrirt_inr_sample_batch_hybrid")
        return (coords, feats, labels, field) if with_field else (coords, feats, labels)

    def sample_voxels(self, case_indices, h_coords, w_coords, d_coords):
        """dataloader.py:86-96: (intensities (N, M) fp32, labels (N,) int16) of the given voxels, by plain indexing."""
        idx = [torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(self.device).to(torch.int64).reshape(-1)
               for v in (case_indices, h_coords, w_coords, d_coords)]
        mods = torch.empty((idx[0].numel(), self.n_modalities), dtype=torch.float32, device=self.device)
        seg = torch.empty(idx[0].numel(), dtype=torch.int16, device=self.device)
        for c in range(self.n_cases):                    # case by case: the volumes stay where they are
            at = torch.nonzero(idx[0] == c).reshape(-1)
            h, w, d = idx[1][at], idx[2][at], idx[3][at]
            if self.n_modalities:
                mods[at] = self.mods[c][:, h, w, d].T
            seg[at] = self.seg[c][h, w, d]
        return mods, seg


def lr_schedule(peak: float, end: float, warmup_steps: int, decay_steps: int, t: int) -> float:
    """``optax.warmup_cosine_decay_schedule(0, peak, warmup_steps, decay_steps, end)`` at ``t`` updates already applied, in
    fp64 (what ``mrirt_inr_lr_schedule`` computes).  ``decay_steps - warmup_steps <= 0`` is refused, as optax asserts."""
    import math
    peak, end, warmup, t = float(peak), float(end), int(warmup_steps), int(t)
    T = int(decay_steps) - warmup
    if T <= 0:
        raise ValueError(f"decay_steps ({decay_steps}) must exceed warmup_steps ({warmup_steps})")
    if not (math.isfinite(peak) and math.isfinite(end) and peak > 0.0 and end >= 0.0):
        raise ValueError("the schedule needs a finite peak > 0 and a finite end >= 0")
    if t < warmup:
        return peak * float(t) / float(warmup)
    u = float(min(t - warmup, T)) / float(T)
    alpha = end / peak
    return peak * ((1.0 - alpha) * (0.5 * (1.0 + math.cos(3.141592653589793 * u))) + alpha)


def init_mlp(seed: int, in_dim: int, hidden_dims: Sequence[int], out_dim: int) -> List[Dict[str, np.ndarray]]:
    """model.py:26-40 with a NumPy generator: Glorot-uniform weights, zero biases (jax's key stream is not reproduced)."""
    rng = np.random.default_rng(int(seed))
    dims = [int(in_dim)] + [int(h) for h in hidden_dims] + [int(out_dim)]
    params = []
    for a, b in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (a + b))
        params.append({"W": rng.uniform(-lim, lim, (a, b)).astype(np.float32), "b": np.zeros(b, np.float32)})
    return params


@dataclass
class AdamWState:
    """The flat fp32 master copy of a network with its AdamW moments, on the device, and the number of updates applied."""
    dims: List[int]
    w: torch.Tensor
    b: torch.Tensor
    mu_w: torch.Tensor
    mu_b: torch.Tensor
    nu_w: torch.Tensor
    nu_b: torch.Tensor
    step: int = 0

    @staticmethod
    def from_params(params, dev=None) -> "AdamWState":
        dev = dev or _require_gpu()
        layers = _layers(params) if not isinstance(params[0]["W"], torch.Tensor) else [(p["W"], p["b"]) for p in params]
        Ws, bs = [_dev_f32(W, dev) for W, _ in layers], [_dev_f32(b, dev) for _, b in layers]
        dims = _param_dims(Ws, bs)
        w, b = torch.cat([W.reshape(-1) for W in Ws]), torch.cat([x.reshape(-1) for x in bs])
        return AdamWState(dims, w, b, torch.zeros_like(w), torch.zeros_like(b), torch.zeros_like(w), torch.zeros_like(b), 0)

    def params(self) -> List[Dict[str, np.ndarray]]:
        return [{"W": g["W"].cpu().numpy().copy(), "b": g["b"].cpu().numpy().copy()} for g in _split_grads(self.w, self.b, self.dims)]

    def c_state(self) -> _lib.InrTrainState:
        return _lib.InrTrainState(*[t.data_ptr() for t in (self.w, self.b, self.mu_w, self.mu_b, self.nu_w, self.nu_b)])


def adamw_step(st: AdamWState, gw: torch.Tensor, gb: torch.Tensor, lr: float, gscale: float = 1.0, clip_norm: float = 0.0,
               b1: float = ADAMW_B1, b2: float = ADAMW_B2, eps: float = ADAMW_EPS, weight_decay: float = ADAMW_WEIGHT_DECAY) -> torch.Tensor:
    """``mrirt_inr_adamw_step`` in place on ``st`` (update number ``st.step + 1``; ``st.step`` is advanced): clip by the
    global norm of ``gscale`` x (gw, gb), then AdamW with the given rate.  Returns the fp64 device tensor [norm, clip factor]."""
    lib = _lib.lib()
    n = st.w.numel() + st.b.numel()
    nbytes = int(lib.mrirt_inr_adamw_scratch_bytes(n))
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=st.w.device)
    gnorm = torch.empty(2, dtype=torch.float64, device=st.w.device)
    hp = _lib.AdamW(lr, b1, b2, eps, weight_decay, clip_norm)
    rc = lib.mrirt_inr_adamw_step(_ptr(st.w), _ptr(st.b), _ptr(gw), _ptr(gb), _ptr(st.mu_w), _ptr(st.mu_b), _ptr(st.nu_w), _ptr(st.nu_b),
                                  st.w.numel(), st.b.numel(), C.byref(hp), int(st.step), float(gscale), _ptr(gnorm), _ptr(scratch), nbytes,
                                  _stream_ptr(None))
    _lib.check(rc, "mrirt_inr_adamw_step")
    st.step += 1
    return gnorm


def train_cfg(micro_batch: int, accum: int, seed: int, class_weights, dice_weight: float, peak_lr: float, min_lr: float,
              warmup_steps: int, decay_steps: int, clip_norm: float, b1: float = ADAMW_B1, b2: float = ADAMW_B2, eps: float = ADAMW_EPS,
              weight_decay: float = ADAMW_WEIGHT_DECAY) -> _lib.InrTrainCfg:
    c = _lib.InrTrainCfg()
    c.microBatch, c.accum, c.warmupSteps, c.decaySteps, c.seed = int(micro_batch), int(accum), int(warmup_steps), int(decay_steps), int(seed) & (2 ** 64 - 1)
    c.peakLr, c.minLr, c.diceWeight = float(peak_lr), float(min_lr), float(dice_weight)
    cw = [float(np.float32(v)) for v in class_weights]
    if len(cw) > 16:
        raise ValueError("at most 16 classes")
    for k, v in enumerate(cw):
        c.classWeights[k] = v
    c.adamw = _lib.AdamW(0.0, b1, b2, eps, weight_decay, clip_norm)
    return c


def _run_entry(desc: _lib.InrDesc, muon: Optional[_lib.Muon], ext: Optional[_lib.InrTrainExt] = None):
    """(name, scratch-size function, run function taking (desc, cache, cfg, state, ...)) of the one-call run for ``desc``."""
    lib = _lib.lib()
    if ext is not None:
        size, run = lib.mrirt_inr_train_run_ext_scratch_bytes, lib.mrirt_inr_train_run_ext
        return "mrirt_inr_train_run_ext", lambda d, c, g: size(d, c, g, C.byref(ext)), lambda d, c, g, *rest: run(d, c, g, C.byref(ext), *rest)
    if muon is not None:
        run = lib.mrirt_inr_train_run_muon
        return "mrirt_inr_train_run_muon", lib.mrirt_inr_train_run_muon_scratch_bytes, lambda d, c, g, *rest: run(d, c, g, C.byref(muon), *rest)
    family = "siren" if int(desc.kind) in (KIND_SIREN, KIND_RAW_SIREN) else "inr"
    return f"mrirt_{family}_train_run", getattr(lib, f"mrirt_{family}_train_run_scratch_bytes"), getattr(lib, f"mrirt_{family}_train_run")


def n_tumour_of(micro_batch: int, tumor_ratio: float) -> int:
    """jax_inr_brats.py:467-468: ``int(micro_batch * clip(tumor_ratio, 0, 1))`` in double."""
    return int(float(int(micro_batch)) * min(max(float(tumor_ratio), 0.0), 1.0))


def train_ext(cache: Optional[VoxelCache] = None, loss: Optional[_lib.InrLossExt] = None, muon: Optional[_lib.Muon] = None,
              n_tumour: int = 0) -> _lib.InrTrainExt:
    """``MrirtInrTrainExt`` for ``train_run(..., ext=)``: any of the extended loss (``loss_ext(...)``), Muon (``muon_hp(...)``)
    and ``n_tumour`` tumour draws per micro-batch (needs ``cache``, whose tumour index is built here).  The struct keeps the
    objects it points to alive."""
    x = _lib.InrTrainExt()
    if loss is not None:
        x.loss = C.pointer(loss)
    if muon is not None:
        x.muon = C.pointer(muon)
    if int(n_tumour) != 0:
        if cache is None:
            raise ValueError("train_ext: n_tumour needs the cache whose tumour index to use")
        x.tumour = cache.tumour_index()
    x.nTumour = int(n_tumour)
    x._keep = (loss, muon, cache)
    return x


def train_run(desc: _lib.InrDesc, cache: VoxelCache, cfg: _lib.InrTrainCfg, st: AdamWState, steps: int, scratch: Optional[torch.Tensor] = None,
              muon: Optional[_lib.Muon] = None, ext: Optional[_lib.InrTrainExt] = None):
    """``mrirt_inr_train_run`` (``mrirt_siren_train_run`` for a SIREN descriptor): ``steps`` optimiser steps from ``st.step``
    on, enqueued in one call without a host
    synchronisation.  Returns the device tensor history (steps, accum, 1 + 2 C): loss, CE per class, Dice per class of every
    micro-batch.  ``st`` is updated in place and ``st.step`` advanced.  ``muon`` (``muon_hp(...)``): the update is Muon on the
    weight matrices and AdamW on the biases (``mrirt_inr_train_run_muon``); ``cfg.adamw`` then is the bias / clip half and
    ``st.nu_w`` is left alone.  ``ext`` (``train_ext(...)``): the run is ``mrirt_inr_train_run_ext`` with its loss, optimiser
    and sampler (``muon`` is then not read: the optimiser is ``ext``'s)."""
    where, run_bytes, run = _run_entry(desc, muon, ext)
    nbytes = int(run_bytes(C.byref(desc), C.byref(cache.desc), C.byref(cfg)))
    if nbytes <= 0:
        raise ValueError("train_run: unsupported network / cache / configuration (Fourier ReLU or SIREN kind over the cache's modalities, "
                         "accum >= 1, decay_steps > warmup_steps, finite hyper-parameters; with ext: loss options in their domains, "
                         "0 <= n_tumour <= micro-batch)")
    if scratch is None or scratch.numel() < nbytes:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=st.w.device)
    hist = torch.empty((int(steps), int(cfg.accum), 1 + 2 * int(desc.outDim)), dtype=torch.float32, device=st.w.device)
    cs = st.c_state()
    rc = run(C.byref(desc), C.byref(cache.desc), C.byref(cfg), C.byref(cs), int(st.step), int(steps), _ptr(hist),
             _ptr(scratch), scratch.numel(), _stream_ptr(None))
    _lib.check(rc, where)
    st.step += int(steps)
    return hist


# --- Muon (csrc/inr_muon.hip): optax.contrib.muon's defaults ----------------------------------------------
MUON_BETA, MUON_NESTEROV, MUON_NS_STEPS, MUON_NS_COEFFS, MUON_EPS, MUON_WEIGHT_DECAY = 0.95, True, 5, (3.4445, -4.7750, 2.0315), 1e-8, 0.0
MUON_BIAS_B1, MUON_BIAS_B2, MUON_BIAS_EPS, MUON_BIAS_WEIGHT_DECAY = 0.9, 0.999, 1e-8, 0.0      # the AdamW half, on the biases


def muon_hp(beta: float = MUON_BETA, nesterov: bool = MUON_NESTEROV, ns_steps: int = MUON_NS_STEPS, ns_coeffs=MUON_NS_COEFFS, eps: float = MUON_EPS,
            weight_decay: float = MUON_WEIGHT_DECAY) -> _lib.Muon:
    c = [float(v) for v in ns_coeffs]
    if len(c) != 3:
        raise ValueError("ns_coeffs: three Newton-Schulz coefficients")
    return _lib.Muon(float(beta), float(eps), float(weight_decay), (C.c_float * 3)(*c), int(ns_steps), 1 if nesterov else 0)


def _muon_scratch(desc: _lib.InrDesc, dev) -> torch.Tensor:
    nbytes = int(_lib.lib().mrirt_muon_scratch_bytes(C.byref(desc)))
    if nbytes <= 0:
        raise ValueError(f"unsupported network shape for Muon: in {desc.inDim}, hidden {desc.hidden} x {desc.numLayers - 1}, out {desc.outDim}")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def muon_orthogonalize(dims: Sequence[int], m_flat: torch.Tensor, hp: Optional[_lib.Muon] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mrirt_muon_orthogonalize``: Newton-Schulz of every layer's matrix of the network ``dims = [in, hidden, .., out]``, from
    the flat fp32 weight layout (``AdamWState.w``'s) into a new tensor of the same layout, in one call."""
    desc = train_desc(dims)
    hp = hp if hp is not None else muon_hp()
    m = m_flat.contiguous()
    nw = sum(a * b for a, b in zip(dims[:-1], dims[1:]))
    if m.dtype != torch.float32 or m.numel() != nw or not m.is_cuda:
        raise ValueError(f"m_flat: {nw} float32 elements on the GPU")
    if scratch is None:
        scratch = _muon_scratch(desc, m.device)
    out = torch.empty_like(m)
    rc = _lib.lib().mrirt_muon_orthogonalize(C.byref(desc), _ptr(m), _ptr(out), C.byref(hp), _ptr(scratch), scratch.numel(), _stream_ptr(None))
    _lib.check(rc, "mrirt_muon_orthogonalize")
    return out


def muon_step(st: AdamWState, gw: torch.Tensor, gb: torch.Tensor, lr: float, gscale: float = 1.0, clip_norm: float = 0.0,
              hp: Optional[_lib.Muon] = None, b1: float = MUON_BIAS_B1, b2: float = MUON_BIAS_B2, eps: float = MUON_BIAS_EPS,
              weight_decay: float = MUON_BIAS_WEIGHT_DECAY) -> torch.Tensor:
    """``mrirt_muon_step`` in place on ``st`` (update number ``st.step + 1``; ``st.step`` is advanced): clip by the global norm
    of ``gscale`` x (gw, gb), Muon (``hp``, default ``muon_hp()``) on the weight matrices of ``st.dims``, AdamW (b1, b2, eps,
    weight_decay) on the biases.  ``st.nu_w`` is not touched.  Returns the fp64 device tensor [norm, clip factor]."""
    desc = train_desc(st.dims)
    hp = hp if hp is not None else muon_hp()
    scratch = _muon_scratch(desc, st.w.device)
    gnorm = torch.empty(2, dtype=torch.float64, device=st.w.device)
    adamw = _lib.AdamW(lr, b1, b2, eps, weight_decay, clip_norm)
    rc = _lib.lib().mrirt_muon_step(C.byref(desc), _ptr(st.w), _ptr(st.b), _ptr(gw), _ptr(gb), _ptr(st.mu_w), _ptr(st.mu_b), _ptr(st.nu_b),
                                    C.byref(hp), C.byref(adamw), int(st.step), float(gscale), _ptr(gnorm), _ptr(scratch), scratch.numel(),
                                    _stream_ptr(None))
    _lib.check(rc, "mrirt_muon_step")
    st.step += 1
    return gnorm


def _optimizer_of(config: Dict[str, Any]) -> Optional[_lib.Muon]:
    """train.py:36: ``OPTIMIZER_CHOICE == "muon"`` picks Muon (optional MUON_BETA, MUON_NS_STEPS, MUON_NESTEROV,
    MUON_WEIGHT_DECAY); any other value, or none, is AdamW, as in the reference's else-branch."""
    if config.get("OPTIMIZER_CHOICE") != "muon":
        return None
    return muon_hp(beta=float(config.get("MUON_BETA", MUON_BETA)), nesterov=bool(config.get("MUON_NESTEROV", MUON_NESTEROV)),
                   ns_steps=int(config.get("MUON_NS_STEPS", MUON_NS_STEPS)), weight_decay=float(config.get("MUON_WEIGHT_DECAY", MUON_WEIGHT_DECAY)))


# the optional config keys of the extended loss and the sampling mix (the flags of scripts/jax_inr_brats.py), with the value
# each takes when another of them is present
EXT_CONFIG_KEYS = dict(FOCAL_GAMMA=0.0, FOCAL_ALPHA=None, LABEL_SMOOTHING=0.0, PER_CLASS_DICE=True, EDEMA_FP_WEIGHT=0.0, TVERSKY_EDEMA_ALPHA=0.8,
                       TVERSKY_EDEMA_BETA=0.2, TVERSKY_EDEMA_WEIGHT=0.0, EDEMA_LOGIT_REG=0.0, EDEMA_CLASS=2, TUMOR_RATIO=0.0)


def _ext_keys_of(config: Dict[str, Any]) -> Dict[str, Any]:
    """The keys of EXT_CONFIG_KEYS the config holds (None values dropped): empty = today's run, untouched."""
    return {k: config[k] for k in EXT_CONFIG_KEYS if k in config and config[k] is not None}


def loss_ext_of_config(config: Dict[str, Any], nc: int) -> _lib.InrLossExt:
    """The ``MrirtInrLossExt`` a ``train_inr`` / ``train_siren`` config stands for: CLASS_WEIGHTS, DICE_WEIGHT and the optional keys
    of EXT_CONFIG_KEYS at their defaults where absent (PER_CLASS_DICE True: the Dice of model.py)."""
    g = {k: config.get(k, v) for k, v in EXT_CONFIG_KEYS.items()}
    cw = list(config["CLASS_WEIGHTS"])
    if len(cw) != nc:
        raise ValueError(f"CLASS_WEIGHTS holds {len(cw)} values for {nc} classes")
    return loss_ext(cw, float(config["DICE_WEIGHT"]), bool(g["PER_CLASS_DICE"]), float(g["FOCAL_GAMMA"]), g["FOCAL_ALPHA"], float(g["LABEL_SMOOTHING"]),
                    float(g["EDEMA_FP_WEIGHT"]), float(g["TVERSKY_EDEMA_ALPHA"]), float(g["TVERSKY_EDEMA_BETA"]), float(g["TVERSKY_EDEMA_WEIGHT"]),
                    float(g["EDEMA_LOGIT_REG"]), int(g["EDEMA_CLASS"]))


def _load_resume(path) -> Tuple[List[Dict[str, np.ndarray]], Optional[Dict[str, np.ndarray]]]:
    """A checkpoint's parameters — the periodic W_i / b_i layout read directly (no pickle), anything else through
    ``model_load`` — and, when the optimiser file this loop writes beside it exists, the moments and the step count."""
    path = pathlib.Path(path).expanduser()
    if not path.is_file():
        raise FileNotFoundError(f"resume_from: no checkpoint at {path}")
    with np.load(str(path)) as z:
        names = list(z.files)
        flat = bool(names) and all(n.startswith(("W_", "b_")) for n in names)
        if flat:
            count = sum(n.startswith("W_") for n in names)
            params = [{"W": np.asarray(z[f"W_{i}"], np.float32), "b": np.asarray(z[f"b_{i}"], np.float32)} for i in range(count)]
    if not flat:
        params, _ = model_load(path)
        params = [{"W": W, "b": b} for W, b in _layers(params)]
    opt_path = path.with_name(path.stem + "_opt.npz")
    opt = None
    if opt_path.is_file():
        with np.load(str(opt_path)) as z:
            opt = {k: np.asarray(z[k]) for k in z.files}
    return params, opt


def _train_loop(config: Dict[str, Any], cases_or_cache, val_cases, params, resume_from, log, save_path, in_dim_of, default_params, make_desc):
    """The loop ``train_inr`` and ``train_siren`` share: config parsing, cache, resume, chunked ``train_run`` calls, history and
    checkpoints.  ``in_dim_of(cache)`` -> input width, ``default_params(seed, in_dim, hidden_dims, nc)`` -> initial parameters,
    ``make_desc(dims, cache)`` -> the training descriptor.  Returns (AdamWState, state dict without "params")."""
    g, micro = int(config["GLOBAL_BATCH_SIZE"]), int(config["MICRO_BATCH_SIZE"])
    hidden_dims = [int(h) for h in config["HIDDEN_DIMS"]]
    warmup, train_steps = int(config["WARMUP_STEPS"]), int(config["TRAIN_STEPS"])
    nc, seed = int(config["NUM_CLASSES"]), int(config["RNG_SEED"])
    every = int(config.get("CHECKPOINT_EVERY_STEPS", 200))
    if micro < 1 or g < 1 or train_steps < 1 or every < 1:
        raise ValueError("GLOBAL_BATCH_SIZE, MICRO_BATCH_SIZE, TRAIN_STEPS and CHECKPOINT_EVERY_STEPS must be positive")
    accum = (g + micro - 1) // micro
    decay_steps = max(1, train_steps - warmup)
    lr_schedule(float(config["LR"]), float(config["MIN_LR"]), warmup, decay_steps, 0)          # refuses T <= 0 before any work
    muon = _optimizer_of(config)
    name = "muon" if muon is not None else "adamw"
    ext_keys = _ext_keys_of(config)
    opt = None
    if resume_from is not None:                          # read, and refused if it is the other optimiser's, before any GPU work
        params, opt = _load_resume(resume_from)
        saved = str(opt["optimizer"]) if opt is not None and "optimizer" in opt else "adamw"          # a file without the key is AdamW's
        if opt is not None and saved != name:
            raise ValueError(f"resume_from: the optimiser state beside the checkpoint is {saved}'s, the config asks for {name}")
    cache = cases_or_cache if isinstance(cases_or_cache, VoxelCache) else VoxelCache(cases_or_cache)
    val_cache = None if val_cases is None else (val_cases if isinstance(val_cases, VoxelCache) else VoxelCache(val_cases))
    in_dim = in_dim_of(cache)
    if resume_from is None and params is None:
        params = default_params(seed, in_dim, hidden_dims, nc)
    if isinstance(params, dict):                         # the SIREN notebook layout
        params = [{"W": W, "b": b} for W, b in _layers(params)]
    st = AdamWState.from_params(params, cache.device)
    if st.dims != [in_dim] + hidden_dims + [nc]:
        raise ValueError(f"the parameters have layer widths {st.dims}, the config asks for {[in_dim] + hidden_dims + [nc]}")
    if opt is not None:
        for k in ("mu_w", "mu_b", "nu_w", "nu_b"):
            getattr(st, k).copy_(torch.from_numpy(np.asarray(opt[k], np.float32)))
        st.step = int(opt["step"])
    desc = make_desc(st.dims, cache)
    bias_half = dict(b1=MUON_BIAS_B1, b2=MUON_BIAS_B2, eps=MUON_BIAS_EPS, weight_decay=MUON_BIAS_WEIGHT_DECAY) if muon is not None else {}
    cfg = train_cfg(micro, accum, seed, config["CLASS_WEIGHTS"], float(config["DICE_WEIGHT"]), float(config["LR"]), float(config["MIN_LR"]),
                    warmup, decay_steps, float(config["CLIP_NORM"]), **bias_half)
    if save_path is not None:
        save_path = pathlib.Path(save_path)
        save_path.mkdir(parents=True, exist_ok=True)
    loss_history: List[float] = []
    dice_history: List[List[float]] = [[] for _ in range(nc)]
    ce_history: List[List[float]] = [[] for _ in range(nc)]
    ext = None
    if ext_keys:                                         # any key of EXT_CONFIG_KEYS: the run is mrirt_inr_train_run_ext
        ext = train_ext(cache, loss_ext_of_config(config, nc), muon, n_tumour_of(micro, config.get("TUMOR_RATIO", 0.0)))
    nbytes = int(_run_entry(desc, muon, ext)[1](C.byref(desc), C.byref(cache.desc), C.byref(cfg)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=cache.device) if nbytes > 0 else None      # one buffer for every chunk
    while st.step < train_steps:
        first = st.step
        steps = min(train_steps, (first // every + 1) * every, first + 4096) - first
        h = train_run(desc, cache, cfg, st, steps, scratch, muon, ext).cpu().numpy().astype(np.float64).mean(axis=1)     # per-step means
        for k in range(steps):
            loss_history.append(float(h[k, 0]))
            for c in range(nc):
                ce_history[c].append(float(h[k, 1 + c]))
                dice_history[c].append(float(h[k, 1 + nc + c]))
            if log is not None:
                m = {"train/loss": float(h[k, 0]), "train/step": first + k + 1, "train/dice_mean": float(h[k, 1 + nc:].mean()),
                     "train/ce_mean": float(h[k, 1:1 + nc].mean())}
                for c in range(nc):
                    m[f"train/dice_class_{c}"], m[f"train/ce_class_{c}"] = float(h[k, 1 + nc + c]), float(h[k, 1 + c])
                log(first + k + 1, m)
        if save_path is not None and st.step % every == 0:
            flat = {}
            for i, layer in enumerate(st.params()):
                flat[f"W_{i}"], flat[f"b_{i}"] = layer["W"], layer["b"]
            ck = save_path / CHECKPOINT_BASENAME.format(step=st.step)
            np.savez_compressed(ck, **flat)
            np.savez_compressed(ck.with_name(ck.stem + "_opt.npz"), step=np.int64(st.step), **({"optimizer": np.str_("muon")} if muon is not None else {}),
                                **{"ext_" + k: np.asarray(v, np.float64) for k, v in ext_keys.items()},
                                **{k: getattr(st, k).cpu().numpy() for k in ("mu_w", "mu_b", "nu_w", "nu_b")})
    state = {"train_cache": cache, "val_cache": val_cache, "vol_shape": cache.vol_shape, "loss_history": loss_history,
             "dice_history": dice_history, "ce_history": ce_history, "best_val_dice": None, "best_step": None, "save_path": save_path,
             "checkpoint_periodic_basename": CHECKPOINT_BASENAME, "opt": st}
    return st, state


def train_inr(config: Dict[str, Any], cases_or_cache, val_cases=None, params=None, resume_from=None, log=None, save_path=None):
    """inr/inr/train.py:18-259 on the GPU with the reference's config keys (GLOBAL_BATCH_SIZE, MICRO_BATCH_SIZE, FOURIER_FREQS,
    HIDDEN_DIMS, LR, MIN_LR, WARMUP_STEPS, TRAIN_STEPS, RNG_SEED, NUM_CLASSES, DICE_WEIGHT, CLASS_WEIGHTS, CLIP_NORM,
    CHECKPOINT_EVERY_STEPS): ``accum = ceil(global / micro)`` micro-batches per update, clip_by_global_norm + AdamW under the
    warm-up / cosine schedule, all inside ``mrirt_inr_train_run`` — one call per chunk of steps, a chunk ending at every
    checkpoint step, and one read-back of the chunk's history.

    ``cases_or_cache``: a ``VoxelCache`` or the list of cases to build one from.  ``params``: initial parameters (default
    ``init_mlp(RNG_SEED, ...)``).  ``save_path``: a directory; only then ``checkpoint_step{step:06d}.npz`` (``W_i`` / ``b_i``,
    the reference's periodic layout) is written every CHECKPOINT_EVERY_STEPS steps, with the optimiser moments and the step
    in ``checkpoint_step{step:06d}_opt.npz`` beside it.  ``resume_from``: such a file (with the moments beside it the run
    continues at its step and reproduces the uninterrupted run bit for bit; without them it restarts the schedule from the
    loaded parameters, as the reference does) or a ``model_load`` checkpoint.  ``log(step, metrics)`` is called per step.
    ``OPTIMIZER_CHOICE == "muon"`` (train.py:36; the notebook's optimiser) replaces AdamW by Muon on the weight matrices with
    AdamW on the biases, inside ``mrirt_inr_train_run_muon`` (optional MUON_BETA, MUON_NS_STEPS, MUON_NESTEROV,
    MUON_WEIGHT_DECAY; optax's defaults otherwise); any other value keeps AdamW.  A Muon run's ``_opt.npz`` carries
    ``optimizer = "muon"``; resuming a state with the other optimiser raises ``ValueError``.
    The optional keys FOCAL_GAMMA, FOCAL_ALPHA, LABEL_SMOOTHING, PER_CLASS_DICE (default True: the Dice of model.py),
    EDEMA_FP_WEIGHT, TVERSKY_EDEMA_ALPHA / _BETA / _WEIGHT, EDEMA_LOGIT_REG, EDEMA_CLASS (default 2) and TUMOR_RATIO (default 0)
    are the loss and sampling options of scripts/jax_inr_brats.py: with any of them present the run is
    ``mrirt_inr_train_run_ext`` (``mrirt_inr_loss_ext``, and ``int(MICRO_BATCH_SIZE * clip(TUMOR_RATIO, 0, 1))`` tumour draws at
    the head of every micro-batch); the keys in force are recorded as ``ext_<KEY>`` in ``_opt.npz``.  Without them nothing changes.
    Returns ``(params, state)``: the reference's list of ``{"W", "b"}`` (NumPy) and a dict with ``loss_history``,
    ``dice_history`` / ``ce_history`` (per class), the caches, ``vol_shape`` and ``opt`` (the ``AdamWState``)."""
    K = int(config["FOURIER_FREQS"])
    st, state = _train_loop(config, cases_or_cache, val_cases, params, resume_from, log, save_path,
                            lambda cache: 3 + 6 * K + cache.n_modalities, init_mlp,
                            lambda dims, cache: train_desc(dims, K, cache.n_modalities))
    out = st.params()
    state = {"params": out, **state}
    return out, state


# --- SIREN training: the exact-sine fp32 step and loop (csrc/inr_train.hip, csrc/siren_sincos.h) ----------
def siren_init(seed: int, in_dim: int, hidden_dims: Sequence[int], out_dim: int, w0: float = 30.0) -> Dict[str, Dict[str, np.ndarray]]:
    """neumors_inr.ipynb:1150-1163 with a NumPy generator: layer 0 ~ U(+-sqrt(6 / in) / w0), every later layer (the head
    included) ~ U(+-sqrt(6 / in)), zero biases; the notebook's dict ``l{i} -> {"w", "b"}`` (jax's key stream is not reproduced)."""
    rng = np.random.default_rng(int(seed))
    dims = [int(in_dim)] + [int(h) for h in hidden_dims] + [int(out_dim)]
    params = {}
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        lim = np.sqrt(6.0 / a) / (float(w0) if i == 0 else 1.0)
        params[f"l{i}"] = {"w": rng.uniform(-lim, lim, (a, b)).astype(np.float32), "b": np.zeros(b, np.float32)}
    return params


def siren_train_desc(dims: Sequence[int], num_mods: Optional[int] = None, w0: float = 30.0) -> _lib.InrDesc:
    """Descriptor of a SIREN ``dims = [in, hidden, .., hidden, out]`` for the ``mrirt_siren_*`` entry points: ``num_mods=None``
    is the raw kind (the input matrix is given), otherwise x = (coords, ``num_mods`` intensities) and ``in`` must be
    ``3 + num_mods``."""
    d = _step_desc(dims, KIND_RAW_SIREN if num_mods is None else KIND_SIREN, 0, 0 if num_mods is None else num_mods, w0)
    if num_mods is not None and d.inDim != 3 + int(num_mods):
        raise ValueError(f"a SIREN over {num_mods} modalities has {3 + int(num_mods)} inputs, not {d.inDim}")
    if not np.isfinite(w0) or float(w0) == 0.0:
        raise ValueError("w0 must be finite and non-zero")
    return d


def siren_train_scratch(desc: _lib.InrDesc, n: int, dev) -> torch.Tensor:
    return _step_scratch(desc, n, dev, "siren")


def siren_forward_f32(desc: _lib.InrDesc, w_flat: torch.Tensor, b_flat: torch.Tensor, coords, feats, n: int, scratch: torch.Tensor):
    """``mrirt_siren_forward_f32``: fp32 logits (n, out); inputs, sines and cosines stay in ``scratch`` for the backward."""
    return _step_forward(desc, w_flat, b_flat, coords, feats, n, scratch, "siren")


def siren_backward_f32(desc: _lib.InrDesc, w_flat: torch.Tensor, n: int, dlogits: torch.Tensor, scratch: torch.Tensor,
                       grad_w: Optional[torch.Tensor] = None, grad_b: Optional[torch.Tensor] = None, accumulate: bool = False):
    """``mrirt_siren_backward``: (grad_w, grad_b) in the flat layouts, from what ``siren_forward_f32`` left in ``scratch``."""
    return _step_backward(desc, w_flat, n, dlogits, scratch, grad_w, grad_b, accumulate, "siren")


def _siren_dict(layers) -> Dict[str, Dict[str, Any]]:
    return {f"l{i}": {"w": p["W"], "b": p["b"]} for i, p in enumerate(layers)}


def make_siren_loss_and_grad(num_classes: int, class_weights, dice_weight: float, w0: float = 30.0, ext: Optional[_lib.InrLossExt] = None):
    """``make_loss_and_grad`` for the notebook's SIREN: ``f(params, coords, intensities, labels) -> ((loss, aux), grads)`` with
    ``params`` the dict ``l{i} -> {"w", "b"}`` and ``grads`` a dict of device tensors shaped like it.  x = (coords, intensities).
    ``ext`` as in ``make_loss_and_grad``."""
    f = _make_step_loss_and_grad(num_classes, class_weights, dice_weight, ext, lambda dims, m: siren_train_desc(dims, m, w0))

    def loss_and_grad(params, coords, intensities, labels):
        layers = [{"W": params[f"l{i}"]["w"], "b": params[f"l{i}"]["b"]} for i in range(len(params))]
        out, grads = f(layers, coords, intensities, labels)
        return out, _siren_dict(grads)

    return loss_and_grad


def siren_autograd(ws, bs, coords, feats, w0: float = 30.0) -> torch.Tensor:
    """Differentiable fp32 logits (n, out) of a SIREN: forward ``mrirt_siren_forward_f32``, backward ``mrirt_siren_backward``;
    gradients reach ``ws`` (each (in, out)) and ``bs`` only.  ``coords=None``: ``feats`` is the (n, in) input matrix; otherwise
    x = (coords (n, 3), intensities ``feats`` (n, M))."""
    return _step_autograd(ws, bs, coords, feats, lambda dims, m: siren_train_desc(dims, None if coords is None else m, float(w0)))


def train_siren(config: Dict[str, Any], cases_or_cache, val_cases=None, params=None, resume_from=None, log=None, save_path=None):
    """``train_inr`` for the notebook's SIREN (x = (coords, modalities), neumors_inr.ipynb:1150-1200): the same config keys
    without FOURIER_FREQS, plus ``W0`` (default 30); the same chunking, the same ``W_i`` / ``b_i`` + ``_opt.npz`` checkpoints
    and the same bit-for-bit resume, all inside ``mrirt_siren_train_run``.  ``params``: the notebook's dict ``l{i} -> {"w", "b"}``
    (default ``siren_init(RNG_SEED, ...)``).  Returns ``(params dict, state)``; the dict goes into
    ``pack_mlp(params, KIND_SIREN, 0, M, w0)`` as it is."""
    w0 = float(config.get("W0", 30.0))
    if not np.isfinite(w0) or w0 == 0.0:
        raise ValueError("W0 must be finite and non-zero")
    if "FOURIER_FREQS" in config and int(config["FOURIER_FREQS"]) != 0:
        raise ValueError("a SIREN takes no Fourier features: drop FOURIER_FREQS (or set it to 0)")
    st, state = _train_loop(config, cases_or_cache, val_cases, params, resume_from, log, save_path,
                            lambda cache: 3 + cache.n_modalities,
                            lambda seed, in_dim, hidden_dims, nc: siren_init(seed, in_dim, hidden_dims, nc, w0),
                            lambda dims, cache: siren_train_desc(dims, cache.n_modalities, w0))
    out = _siren_dict(st.params())
    state = {"params": out, "w0": w0, **state}
    return out, state


# --- differentiable INR render: frame gradients to the MLP weights (csrc/brats_soft.hip) ------------------
def render_brats_inr_autograd(params, vols, Ws, bs, zmu, zsigma, fourier_freqs: Optional[int] = None, w0: Optional[float] = None,
                              labels=None, ext=None) -> torch.Tensor:
    """The per-sample INR render as a differentiable frame, fp32 (H, W, 4), with a ``torch.autograd`` graph to ``Ws`` / ``bs``:
    counts -> offsets -> ``mrirt_brats_emit_samples`` -> the fp32 training forward (``mlp_autograd`` for a Fourier/ReLU network
    with ``fourier_freqs``, ``siren_autograd`` for a SIREN with ``w0``; exactly one of the two is given) -> the soft prediction
    overlay (``render_brats_soft_autograd``).  Where ``render_brats_inr`` draws the argmax class through the LUT, this frame
    draws the class probabilities, so ``frame.backward()`` reaches every weight.

    ``params``: the gParams dict; ``vols``: the four LINEAR fp32 device tensors of X*Y*Z voxels the MLP reads; ``Ws`` / ``bs``:
    the layers' (in, out) / (out,) device tensors; ``zmu`` / ``zsigma``: the viewer's per-modality z-score constants.  The
    sample total is read to the host once per call (as ``render_brats_inr(one_pass=True)``); the activations of every march
    sample of the frame stay on the device until the backward pass."""
    from .render import _bind_brats
    from .soft import render_brats_soft_autograd
    if (fourier_freqs is None) == (w0 is None):
        raise ValueError("give fourier_freqs (Fourier/ReLU network) or w0 (SIREN), not both")
    dev = _require_gpu()
    P, E, v, _, _, _ = _bind_brats(params, list(vols), labels, None, ext, dev, pred_stream=True)
    if len(v) != 4 or any(t is None for t in v):
        raise ValueError("the MLP reads all four modalities: bind four volumes")
    if E.layout != _lib.LAYOUT_LINEAR or E.tileSize > 0:
        raise ValueError("render_brats_inr_autograd: whole frames on LINEAR grids only")
    w, h = int(P.imageSize[0]), int(P.imageSize[1])
    lib, s = _lib.lib(), _stream_ptr(None)
    vp = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) for t in v])
    mu = (C.c_float * 4)(*[float(np.float32(x)) for x in zmu])
    sg = (C.c_float * 4)(*[float(np.float32(x)) for x in zsigma])
    counts = torch.empty(h * w, dtype=torch.int32, device=dev)
    _lib.check(lib.mrirt_brats_sample_counts(C.byref(P), C.byref(E), _ptr(counts), s), "mrirt_brats_sample_counts")
    ends = torch.cumsum(counts.to(torch.int64), 0)
    offsets = (ends - counts).contiguous()
    total = int(ends[-1])                                       # the one host read of the call
    n = max(total, 1)
    coords = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    feats = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    _lib.check(lib.mrirt_brats_emit_samples(C.byref(P), C.byref(E), vp, mu, sg, _ptr(offsets), _ptr(coords), _ptr(feats), s),
               "mrirt_brats_emit_samples")
    Ws, bs = list(Ws), list(bs)
    logits = siren_autograd(Ws, bs, coords, feats, float(w0)) if w0 is not None else mlp_autograd(Ws, bs, coords, feats, int(fourier_freqs))
    return render_brats_soft_autograd(params, v, logits, offsets, labels, ext)


def fit_views(config: Dict[str, Any], views: Sequence[Dict[str, Any]], targets: Sequence[torch.Tensor], vols, params, gparams, zmu, zsigma,
              labels=None, ext=None, log=None) -> Tuple[List[float], AdamWState]:
    """Fit a network to target frames: per step the mean over the pixels and the three colour channels of
    (frame - target)^2, summed over the views, through ``render_brats_inr_autograd``; one clipped AdamW update per step
    (``adamw_step``) at the rate of ``lr_schedule``.  The reference's "differentiability proof" (docs/Goals.md).

    ``views``: per view the gParams entries it overrides (``eye``, ``U``, ``V``, ``W``, ...); ``targets``: per view a device fp32
    (H, W, 4) frame; ``params``: the start, a list of ``{"W", "b"}`` (Fourier/ReLU) or the SIREN dict ``l{i} -> {"w", "b"}``.
    ``config``: ``STEPS``, ``LR`` (peak), ``MIN_LR`` (default ``LR``), ``WARMUP_STEPS`` (0), ``DECAY_STEPS`` (``STEPS`` + 1),
    ``CLIP_NORM`` (0: none), ``WEIGHT_DECAY`` (0), and ``FOURIER_FREQS`` or ``W0`` as the network's kind demands.
    Returns ``(losses, state)``: the loss of every step before its update (host floats) and the ``AdamWState``."""
    if len(views) != len(targets) or not views:
        raise ValueError("one target frame per view, at least one view")
    siren = isinstance(params, dict)
    layers = [{"W": params[f"l{i}"]["w"], "b": params[f"l{i}"]["b"]} for i in range(len(params))] if siren else list(params)
    if siren == ("FOURIER_FREQS" in config and int(config["FOURIER_FREQS"]) != 0):
        raise ValueError("a SIREN dict takes W0, a list of layers takes FOURIER_FREQS")
    kind = dict(w0=float(config.get("W0", 30.0))) if siren else dict(fourier_freqs=int(config["FOURIER_FREQS"]))
    steps, peak = int(config["STEPS"]), float(config["LR"])
    end, warmup = float(config.get("MIN_LR", peak)), int(config.get("WARMUP_STEPS", 0))
    decay, clip, wd = int(config.get("DECAY_STEPS", steps + 1)), float(config.get("CLIP_NORM", 0.0)), float(config.get("WEIGHT_DECAY", 0.0))
    st = AdamWState.from_params(layers)
    losses = []
    for step in range(steps):
        leaves = [{k: t.detach().requires_grad_(True) for k, t in g.items()} for g in _split_grads(st.w, st.b, st.dims)]
        Ws, bs = [g["W"] for g in leaves], [g["b"] for g in leaves]
        loss = None
        for view, target in zip(views, targets):
            frame = render_brats_inr_autograd({**gparams, **view}, vols, Ws, bs, zmu, zsigma, labels=labels, ext=ext, **kind)
            term = ((frame[..., :3] - target[..., :3]) ** 2).mean()
            loss = term if loss is None else loss + term
        loss.backward()
        gw, gb = (torch.cat([(t.grad if t.grad is not None else torch.zeros_like(t)).reshape(-1) for t in ts]) for ts in (Ws, bs))
        adamw_step(st, gw, gb, lr_schedule(peak, end, warmup, decay, st.step), clip_norm=clip, weight_decay=wd)
        losses.append(float(loss.detach()))
        if log is not None:
            log(step, losses[-1])
    return losses, st


# ---- the coordinate-injection INR of notebooks/improved.ipynb (csrc/inr_inject.hip) -----------------------

def inject_load(npz) -> Dict[str, Any]:
    """The notebook's flat checkpoint (cell 14: ``fourier_B``, ``mlp_W_i``, ``mlp_b_i``) as the nested ``params`` it trains:
    ``{"fourier": {"B"}, "mlp": [{"W", "b"}, ...]}``, fp32; the widths are the arrays' shapes.  ``npz``: a path or an open
    ``np.load`` mapping."""
    z = np.load(npz) if isinstance(npz, (str, pathlib.Path)) else npz
    if "fourier_B" not in z:
        raise KeyError("inject_load: no fourier_B in the checkpoint")
    mlp = []
    while f"mlp_W_{len(mlp)}" in z:
        i = len(mlp)
        mlp.append({"W": np.asarray(z[f"mlp_W_{i}"], np.float32), "b": np.asarray(z[f"mlp_b_{i}"], np.float32)})
    if len(mlp) < 2:
        raise ValueError("inject_load: expected at least two layers (mlp_W_0, mlp_W_1)")
    return {"fourier": {"B": np.asarray(z["fourier_B"], np.float32)}, "mlp": mlp}


def _inject_np(t) -> np.ndarray:
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float32)


def inject_desc(params, coord_layers=(1, 2, 3), mod_layers=(2,)) -> _lib.InjectDesc:
    """MrirtInjectDesc of ``params``.  Layer indices the notebook's loop never reaches (0, and L - 1 on: its own
    ``COORD_INJECTION_LAYERS = [1, 2, 3]`` names one) are dropped here; the C ABI refuses them.  The number of modalities is
    what layer 0's input holds beyond the Fourier features, and every other input width must follow from the two sets."""
    B = _inject_np(params["fourier"]["B"])
    Ws = [_inject_np(p["W"]) for p in params["mlp"]]
    L, F = len(Ws), 2 * B.shape[0]
    if B.ndim != 2 or B.shape[1] != 3 or not 2 <= L <= 8:
        raise ValueError(f"inject_desc: B {B.shape} with {L} layers is not a coordinate-injection net")
    M = Ws[0].shape[0] - F
    d = _lib.InjectDesc()
    d.numLayers, d.fourierDim, d.numMods = L, F, max(M, 0)
    for l, W in enumerate(Ws):
        d.width[l] = W.shape[1]
    d.coordLayers = sum(1 << l for l in set(int(v) for v in coord_layers) if 0 < l < L - 1)
    d.modLayers = sum(1 << l for l in set(int(v) for v in mod_layers) if 0 < l < L - 1)
    for l, W in enumerate(Ws):
        prev = F if l == 0 else Ws[l - 1].shape[1]
        want = prev + (M if l == 0 else 3 * ((d.coordLayers >> l) & 1) + M * ((d.modLayers >> l) & 1))
        if M < 0 or W.shape[0] != want or np.shape(params["mlp"][l]["b"]) != (W.shape[1],):
            raise ValueError(f"inject_desc: layer {l} has a {W.shape} weight, the injection sets give {want} inputs")
    return d


def _inject_flat(params, dev):
    w = np.concatenate([_inject_np(p["W"]).reshape(-1) for p in params["mlp"]])
    b = np.concatenate([_inject_np(p["b"]).reshape(-1) for p in params["mlp"]])
    return _dev_f32(_inject_np(params["fourier"]["B"]), dev), _dev_f32(w, dev), _dev_f32(b, dev)


def inject_dropout(seed: int = 0, keep: float = 0.7, samples: int = 1, sample0: int = 0, index0: int = 0) -> _lib.InjectDropout:
    d = _lib.InjectDropout()
    d.seed, d.keep, d.samples, d.sample0, d.reserved, d.index0 = int(seed) & (2 ** 64 - 1), float(keep), int(samples), int(sample0), 0, int(index0)
    return d


def _inject_scratch(desc: _lib.InjectDesc, n: int, dev):
    nbytes = int(_lib.lib().mrirt_inject_scratch_bytes(C.byref(desc), int(n)))
    if nbytes <= 0:
        raise _lib.MrirtError(-5, "mrirt_inject_scratch_bytes")
    return torch.empty(nbytes // 8, dtype=torch.int64, device=dev), nbytes


def _inject_points(coords, mods, dev, M: int):
    c = _dev_f32(coords, dev).reshape(-1, 3)
    m = _dev_f32(mods, dev).reshape(c.shape[0], M) if M else None
    return c, m


def inject_forward(params, coords, mods, *, dropout: Optional[_lib.InjectDropout] = None, coord_layers=(1, 2, 3), mod_layers=(2,),
                   want_argmax: bool = False):
    """Logits (n, C) fp32 of the notebook's ``apply_coord_injection_mlp(apply_fourier_features(...))`` at ``coords`` (n, 3),
    ``mods`` (n, M); with ``want_argmax`` also the int16 class per point.  ``dropout=None`` is ``training=False``; an
    ``inject_dropout(seed, keep, sample0=s, index0=i0)`` draws sample ``s`` of the library's mask stream."""
    dev = _require_gpu()
    desc = inject_desc(params, coord_layers, mod_layers)
    c, m = _inject_points(coords, mods, dev, desc.numMods)
    n = c.shape[0]
    B, w, b = _inject_flat(params, dev)
    logits = torch.empty((n, desc.width[desc.numLayers - 1]), dtype=torch.float32, device=dev)
    am = torch.empty(n, dtype=torch.int16, device=dev) if want_argmax else None
    scratch, nbytes = _inject_scratch(desc, n, dev)
    rc = _lib.lib().mrirt_inject_forward(C.byref(desc), _ptr(B), _ptr(w), _ptr(b), _ptr(c), _ptr(m) if m is not None else None, n,
                                         C.byref(dropout) if dropout is not None else None, _ptr(logits),
                                         _ptr(am) if am is not None else None, _ptr(scratch), nbytes, _stream_ptr(None))
    _lib.check(rc, "mrirt_inject_forward")
    return (logits, am) if want_argmax else logits


def inject_fused_ok(params, coord_layers=(1, 2, 3), mod_layers=(2,)) -> bool:
    """Whether the fused forward (``inject_classify``, ``render_brats_inject``) takes this network: its weights, padded, and the
    waves' buffers fit the 160 KiB of LDS of one compute unit.  No GPU needed."""
    desc = inject_desc(params, coord_layers, mod_layers)
    return int(_lib.lib().mrirt_inject_fused_lds_bytes(C.byref(desc))) > 0


def inject_classify(params, coords, mods, *, count: Optional[torch.Tensor] = None, want_logits: bool = False, coord_layers=(1, 2, 3),
                    mod_layers=(2,)):
    """The int16 class per point of ``inject_forward(..., want_argmax=True)`` without dropout -- the same bits -- in ONE launch
    (``mrirt_inject_classify``: the network stays in LDS, nothing but coords, mods and the outputs touches memory).  ``count``: a
    one-element int32 / uint32 device tensor; the kernel then processes ``min(count, n)`` rows and leaves the other rows of the
    outputs as they were allocated (zero).  ``want_logits``: also the logits (n, C).  A shape the fused path refuses
    (``inject_fused_ok``) raises."""
    dev = _require_gpu()
    desc = inject_desc(params, coord_layers, mod_layers)
    c, m = _inject_points(coords, mods, dev, desc.numMods)
    n = c.shape[0]
    if count is not None and (count.numel() != 1 or count.dtype not in (torch.int32, torch.uint32) or not count.is_cuda):
        raise ValueError("inject_classify: count is a one-element int32 / uint32 device tensor")
    B, w, b = _inject_flat(params, dev)
    am = torch.zeros(n, dtype=torch.int16, device=dev)
    logits = torch.zeros((n, desc.width[desc.numLayers - 1]), dtype=torch.float32, device=dev) if want_logits else None
    rc = _lib.lib().mrirt_inject_classify(C.byref(desc), _ptr(B), _ptr(w), _ptr(b), _ptr(c), _ptr(m) if m is not None else None, n,
                                          _ptr(count) if count is not None else None, _ptr(am),
                                          _ptr(logits) if logits is not None else None, _stream_ptr(None))
    _lib.check(rc, "mrirt_inject_classify")
    return (am, logits) if want_logits else am


def render_brats_inject(params, intensities, net_params, zmu, zsigma, labels=None, out=None, ext=None, return_aux: bool = False,
                        chunk_steps: Optional[int] = None, one_pass: bool = False, coord_layers=(1, 2, 3), mod_layers=(2,)):
    """``render_brats_inr`` with the coordinate-injection network ``net_params`` (``inject_load`` / ``train_inject``; four
    modalities): the prediction overlay's label is the net evaluated AT every live march sample.  Default:
    ``mrirt_render_brats_inject``, the chunked ERT-aware frame whose passes are classified by the fused forward, the batch size
    read from device memory; the same ``chunk_steps=None`` rule and scratch cache.  ``one_pass=True`` is the whole-ray form built
    from ``mrirt_brats_sample_counts``, ``mrirt_brats_emit_samples``, ``mrirt_inject_forward`` (argmax) and
    ``mrirt_render_brats_stream``: the definition the chunked frame is tested against, with the same ``aux``."""
    dev = _require_gpu()
    desc = inject_desc(net_params, coord_layers, mod_layers)
    if desc.numMods != 4:
        raise ValueError("render_brats_inject needs a coordinate-injection network over 4 modalities")
    lib = _lib.lib()
    if not one_pass and int(lib.mrirt_inject_fused_lds_bytes(C.byref(desc))) <= 0:
        raise ValueError("render_brats_inject: the fused forward refuses this shape (inject_fused_ok)")
    B, w, b = _inject_flat(net_params, dev)

    def chunked(P, E, vp, lab, mu, sg, chunk, scratch, o, pitch, st, s):
        _lib.check(lib.mrirt_render_brats_inject(C.byref(P), C.byref(E), vp, _ptr(lab), C.byref(desc), _ptr(B), _ptr(w), _ptr(b), mu, sg,
                                                 chunk, _ptr(scratch), scratch.numel(), _ptr(o), pitch, _ptr(st), s),
                   "mrirt_render_brats_inject")

    def classify_all(coords, feats, total, classes, s):
        scratch, nbytes = _inject_scratch(desc, total, dev)
        _lib.check(lib.mrirt_inject_forward(C.byref(desc), _ptr(B), _ptr(w), _ptr(b), _ptr(coords), _ptr(feats), total, None, None,
                                            _ptr(classes), _ptr(scratch), nbytes, s), "mrirt_inject_forward")

    return _render_c5("render_brats_inject", params, intensities, zmu, zsigma, labels, out, ext, return_aux, chunk_steps, one_pass, chunked,
                      classify_all)


def compute_uncertainty_mc_dropout(params, coords, mods, n_samples: int = 5, seed: int = 0, dropout_rate: float = 0.3, *,
                                   coord_layers=(1, 2, 3), mod_layers=(2,), want_mean: bool = False, index0: int = 0):
    """The notebook's MC-dropout uncertainty (cell 9): the entropy (n,) fp32 of the mean softmax of ``n_samples`` dropout
    passes, under the library's Philox mask stream keyed by ``seed`` (not JAX's key stream).  ``want_mean``: also the mean
    probabilities (n, C)."""
    dev = _require_gpu()
    desc = inject_desc(params, coord_layers, mod_layers)
    c, m = _inject_points(coords, mods, dev, desc.numMods)
    n = c.shape[0]
    B, w, b = _inject_flat(params, dev)
    dp = inject_dropout(seed, float(np.float32(1.0) - np.float32(dropout_rate)), n_samples, 0, index0)
    ent = torch.empty(n, dtype=torch.float32, device=dev)
    mean = torch.empty((n, desc.width[desc.numLayers - 1]), dtype=torch.float32, device=dev) if want_mean else None
    scratch, nbytes = _inject_scratch(desc, n, dev)
    rc = _lib.lib().mrirt_inject_uncertainty(C.byref(desc), _ptr(B), _ptr(w), _ptr(b), _ptr(c), _ptr(m) if m is not None else None, n,
                                             C.byref(dp), _ptr(ent), _ptr(mean) if mean is not None else None, _ptr(scratch), nbytes,
                                             _stream_ptr(None))
    _lib.check(rc, "mrirt_inject_uncertainty")
    return (ent, mean) if want_mean else ent


def predict_full_volume(params, case_data: Dict[str, Any], chunk_size: int = 50000, *, uncertainty: Optional[_lib.InjectDropout] = None,
                        coord_layers=(1, 2, 3), mod_layers=(2,)):
    """The notebook's ``predict_full_volume`` (cell 10): ``(pred int16 (H, W, D), case_data["seg"])`` for ``case_data["mods"]``
    (M, H, W, D), ``chunk_size`` voxels per pass (the result does not depend on it).  ``uncertainty=inject_dropout(seed, keep,
    samples=S)`` adds the MC-dropout entropy volume (H, W, D) fp32 as a third value: an ordinary scalar grid, which
    ``volume.upload_grid`` and ``render_brats(tf=tf_preset("hot"))`` draw as they draw a modality."""
    dev = _require_gpu()
    desc = inject_desc(params, coord_layers, mod_layers)
    mods = _dev_f32(case_data["mods"], dev)
    if mods.dim() != 4 or mods.shape[0] != desc.numMods:
        raise ValueError(f"predict_full_volume: mods {tuple(mods.shape)} for a net of {desc.numMods} modalities")
    _, H, W, D = mods.shape
    chunk = max(1, min(int(chunk_size), H * W * D))
    B, w, b = _inject_flat(params, dev)
    pred = torch.empty((H, W, D), dtype=torch.int16, device=dev)
    ent = torch.empty((H, W, D), dtype=torch.float32, device=dev) if uncertainty is not None else None
    scratch, nbytes = _inject_scratch(desc, chunk, dev)
    hwd = (C.c_uint32 * 3)(H, W, D)
    rc = _lib.lib().mrirt_inject_predict_volume(C.byref(desc), _ptr(B), _ptr(w), _ptr(b), _ptr(mods) if desc.numMods else None, hwd, chunk,
                                                C.byref(uncertainty) if uncertainty is not None else None, _ptr(pred),
                                                _ptr(ent) if ent is not None else None, _ptr(scratch), nbytes, _stream_ptr(None))
    _lib.check(rc, "mrirt_inject_predict_volume")
    return (pred, case_data["seg"], ent) if ent is not None else (pred, case_data["seg"])


def boundary_weights(seg, num_classes: int = 4) -> torch.Tensor:
    """The boundary weight map of the notebook's cache (cell 5): ``max_c 1 / (1 + edt(seg != c))`` over the tumour classes
    c = 1 .. num_classes - 1 that occur, fp32 (H, W, D) on the device, 0 where none does; bit for bit SciPy's
    ``distance_transform_edt`` loop, from the exact fp64 distance transform of csrc/edt.hip."""
    dev = seg.device if isinstance(seg, torch.Tensor) and seg.is_cuda else _require_gpu()
    lab = _label_volume(seg, dev, "seg")
    hwd = (C.c_uint32 * 3)(*lab.shape)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = int(lib.mrirt_boundary_weights_scratch_bytes(hwd))
        out = torch.empty(tuple(lab.shape), dtype=torch.float32, device=dev)
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=dev)
        rc = lib.mrirt_boundary_weights(_ptr(lab), hwd, int(num_classes), _ptr(out), _ptr(scratch), nbytes, _stream_ptr(None))
    _lib.check(rc, "mrirt_boundary_weights")
    return out


# ---- training the coordinate-injection INR (csrc/inr_inject_train.hip) -----------------------------------

def _inject_in_dims(F: int, M: int, widths: Sequence[int], coord_layers, mod_layers) -> List[int]:
    L = len(widths)
    cl = {int(v) for v in coord_layers if 0 < int(v) < L - 1}
    ml = {int(v) for v in mod_layers if 0 < int(v) < L - 1}
    return [F + M if l == 0 else widths[l - 1] + (3 if l in cl else 0) + (M if l in ml else 0) for l in range(L)]


def inject_init(seed: int, fourier_dim: int = 128, num_mods: int = 4, hidden_dims: Sequence[int] = (64, 64, 64), out_dim: int = 4,
                coord_layers=(1, 2, 3), mod_layers=(2,), sigma: float = 5.0, voxel_spacing=(1.0, 1.0, 1.0)) -> Dict[str, Any]:
    """The notebook's initial ``params`` (cells 6 - 7) with a NumPy generator: ``{"fourier": {"B"}, "mlp": [{"W", "b"}, ...]}``,
    ``B ~ N(0, sigma) / voxel_spacing`` of shape (fourier_dim / 2, 3), Glorot-uniform weights over the injected input widths,
    zero biases.  The library's own rule, as ``init_mlp`` and ``siren_init``: JAX's key stream is not reproduced."""
    rng = np.random.default_rng(int(seed))
    F, M = int(fourier_dim), int(num_mods)
    widths = [int(h) for h in hidden_dims] + [int(out_dim)]
    B = rng.normal(0.0, 1.0, (F // 2, 3)) * float(sigma) / np.asarray(voxel_spacing, np.float64).reshape(1, 3)
    mlp = []
    for a, b in zip(_inject_in_dims(F, M, widths, coord_layers, mod_layers), widths):
        lim = np.sqrt(6.0 / (a + b))
        mlp.append({"W": rng.uniform(-lim, lim, (a, b)).astype(np.float32), "b": np.zeros(b, np.float32)})
    return {"fourier": {"B": B.astype(np.float32)}, "mlp": mlp}


def inject_train_scratch(desc: _lib.InjectDesc, n: int, dev) -> torch.Tensor:
    """The step's scratch (``mrirt_inject_train_scratch_bytes``) as a uint8 tensor: forward, loss and backward share it."""
    nbytes = int(_lib.lib().mrirt_inject_train_scratch_bytes(C.byref(desc), int(n)))
    if nbytes <= 0:
        raise _lib.MrirtError(-5, "mrirt_inject_train_scratch_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def inject_forward_train(desc: _lib.InjectDesc, B: torch.Tensor, w_flat: torch.Tensor, b_flat: torch.Tensor, coords: torch.Tensor, mods,
                         n: int, scratch: torch.Tensor, dropout: Optional[_lib.InjectDropout] = None) -> torch.Tensor:
    """``mrirt_inject_forward_train``: the logits (n, C) of ``mrirt_inject_forward``, bit for bit; the features and every
    post-dropout activation stay in ``scratch`` for ``inject_backward``."""
    logits = torch.empty((int(n), desc.width[desc.numLayers - 1]), dtype=torch.float32, device=w_flat.device)
    rc = _lib.lib().mrirt_inject_forward_train(C.byref(desc), _ptr(B), _ptr(w_flat), _ptr(b_flat), _ptr(coords),
                                               _ptr(mods) if mods is not None else None, int(n),
                                               C.byref(dropout) if dropout is not None else None, _ptr(logits), _ptr(scratch),
                                               scratch.numel(), _stream_ptr(None))
    _lib.check(rc, "mrirt_inject_forward_train")
    return logits


def inject_backward(desc: _lib.InjectDesc, B: torch.Tensor, w_flat: torch.Tensor, coords: torch.Tensor, mods, n: int, dlogits: torch.Tensor,
                    scratch: torch.Tensor, dropout: Optional[_lib.InjectDropout] = None, grad_B: Optional[torch.Tensor] = None,
                    grad_w: Optional[torch.Tensor] = None, grad_b: Optional[torch.Tensor] = None, accumulate: bool = False):
    """``mrirt_inject_backward``: (grad_B (F / 2, 3), grad_w, grad_b in the flat layouts of the weights / biases) from what
    ``inject_forward_train`` left in ``scratch``; ``dropout`` must be the forward's.  ``accumulate`` adds into the given buffers."""
    dev = w_flat.device
    nb = sum(desc.width[l] for l in range(desc.numLayers))
    grad_B = torch.empty_like(B) if grad_B is None else grad_B
    grad_w = torch.empty_like(w_flat) if grad_w is None else grad_w
    grad_b = torch.empty(nb, dtype=torch.float32, device=dev) if grad_b is None else grad_b
    rc = _lib.lib().mrirt_inject_backward(C.byref(desc), _ptr(B), _ptr(w_flat), _ptr(coords), _ptr(mods) if mods is not None else None, int(n),
                                          C.byref(dropout) if dropout is not None else None, _ptr(dlogits), _ptr(grad_B), _ptr(grad_w),
                                          _ptr(grad_b), 1 if accumulate else 0, _ptr(scratch), scratch.numel(), _stream_ptr(None))
    _lib.check(rc, "mrirt_inject_backward")
    return grad_B, grad_w, grad_b


def _inject_split(desc: _lib.InjectDesc, t_B: torch.Tensor, t_w: torch.Tensor, t_b: torch.Tensor) -> Dict[str, Any]:
    """Flat (B, w, b) tensors as views in ``params``' structure."""
    L, F, M = desc.numLayers, desc.fourierDim, desc.numMods
    widths = [desc.width[l] for l in range(L)]
    ins = _inject_in_dims(F, M, widths, [l for l in range(L) if (desc.coordLayers >> l) & 1], [l for l in range(L) if (desc.modLayers >> l) & 1])
    mlp, wo, bo = [], 0, 0
    for a, b in zip(ins, widths):
        mlp.append({"W": t_w[wo:wo + a * b].view(a, b), "b": t_b[bo:bo + b]})
        wo, bo = wo + a * b, bo + b
    return {"fourier": {"B": t_B.view(F // 2, 3)}, "mlp": mlp}


# the notebook's own loss (csrc/inr_unified.hip)

def unified_loss(class_weights, gamma: float = 0.5, lam: float = 0.5, alpha: float = 0.3, beta: float = 0.7, ufl_weight: float = 0.5,
                 dice_weight: float = 0.5, tv_weight: float = 0.02, boundary_weight: float = 0.1) -> _lib.UnifiedLoss:
    """``MrirtUnifiedLoss`` with the notebook's constants (cell 2: UNIFIED_FOCAL_GAMMA, UNIFIED_FOCAL_LAMBDA, TV_WEIGHT_STAGE1,
    BOUNDARY_WEIGHT; cell 8: the Tversky 0.3 / 0.7 and the 0.5 / 0.5 mix).  UNIFIED_FOCAL_DELTA is not read by the notebook's
    loss and has no member.  The library checks the values when the struct is used."""
    x = _lib.UnifiedLoss()
    cw = [float(np.float32(v)) for v in np.asarray(class_weights, dtype=np.float32).reshape(-1)]
    if len(cw) > 16:
        raise ValueError("at most 16 classes")
    for k, v in enumerate(cw):
        x.classWeights[k] = v
    x.gamma, x.lambda_, x.tverskyAlpha, x.tverskyBeta = float(gamma), float(lam), float(alpha), float(beta)
    x.uflWeight, x.diceWeight, x.tvWeight, x.boundaryWeight, x.flags = float(ufl_weight), float(dice_weight), float(tv_weight), float(boundary_weight), 0
    return x


def unified_loss_scratch(n: int, dev) -> torch.Tensor:
    """The scratch of ``mrirt_unified_loss`` for ``n`` points (``mrirt_unified_loss_scratch_bytes``) as a uint8 tensor."""
    nbytes = int(_lib.lib().mrirt_unified_loss_scratch_bytes(int(n)))
    if nbytes <= 0:
        raise _lib.MrirtError(-5, "mrirt_unified_loss_scratch_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _unified_aux(aux: torch.Tensor) -> Dict[str, torch.Tensor]:
    """aux [8 + C] of ``mrirt_unified_loss`` under the keys of the notebook's ``loss_fn`` (views, on the device)."""
    keys = ("ufl", "mFTL", "mFL", "dice_loss", "tv_loss", "boundary_loss", "dice_mean_tumor", "accuracy")
    return {**{k: aux[i] for i, k in enumerate(keys)}, "dice_per_class": aux[8:]}


def unified_loss_and_dlogits(logits: torch.Tensor, labels: torch.Tensor, cfg: _lib.UnifiedLoss, boundary_w: Optional[torch.Tensor] = None,
                             scratch: Optional[torch.Tensor] = None, want_grad: bool = True):
    """``mrirt_unified_loss`` on (n, C) fp32 logits, int32 labels and (n,) fp32 boundary weights (or None): (loss 0-d, aux,
    dlogits (n, C) or None), all on the device; ``aux`` is a dict with the keys of the notebook's ``loss_fn``: ufl, mFTL, mFL,
    dice_loss, tv_loss, boundary_loss, dice_per_class (C,), dice_mean_tumor, accuracy.  ``scratch``: a uint8 tensor of at
    least ``mrirt_unified_loss_scratch_bytes(n)`` bytes (``unified_loss_scratch``), allocated when None."""
    n, nc = int(logits.shape[0]), int(logits.shape[1])
    dev = logits.device
    if boundary_w is not None and (boundary_w.dtype != torch.float32 or boundary_w.numel() != n or not boundary_w.is_contiguous()):
        raise ValueError(f"boundary_w must be {n} contiguous fp32 values")
    if scratch is None:
        scratch = unified_loss_scratch(n, dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    aux = torch.empty(8 + nc, dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if want_grad else None
    rc = _lib.lib().mrirt_unified_loss(_ptr(logits), _ptr(labels), _ptr(boundary_w), n, nc, C.byref(cfg), _ptr(loss), _ptr(aux), _ptr(dl),
                                       _ptr(scratch), scratch.numel(), _stream_ptr(None))
    _lib.check(rc, "mrirt_unified_loss")
    return loss.reshape(()), _unified_aux(aux), dl


def make_inject_loss_and_grad(num_classes: int, class_weights, dice_weight: float, coord_layers=(1, 2, 3), mod_layers=(2,),
                              ext: Optional[Any] = None):
    """``jax.value_and_grad(loss_fn, has_aux=True)`` for the coordinate-injection network with the library's loss: returns
    ``fn(params, coords, mods, labels, dropout=None) -> ((loss, aux), grads)``; ``loss`` a 0-d device tensor, ``aux =
    {"ce_per_class", "dice_per_class"}`` and ``grads`` device tensors in ``params``' structure (``{"fourier": {"B"}, "mlp":
    [{"W", "b"}]}``).  One ``mrirt_inject_forward_train``, ``mrirt_inr_loss`` (``mrirt_inr_loss_ext`` with ``ext``, which adds
    ``aux["terms"]``) and one ``mrirt_inject_backward``; nothing synchronises with the host.  When ``ext`` is a
    ``MrirtUnifiedLoss`` (``unified_loss(...)``) the loss is the notebook's own, ``mrirt_unified_loss``: ``class_weights`` /
    ``dice_weight`` are then not read, ``fn`` takes one more argument ``boundary_weights`` ((n,) fp32 or None: no boundary
    term) and ``aux`` carries the keys of the notebook's ``loss_fn`` (``unified_loss_and_dlogits``)."""
    unified = ext if isinstance(ext, _lib.UnifiedLoss) else None
    cw = [float(v) for v in np.asarray(class_weights, dtype=np.float32).reshape(-1)]
    if len(cw) != int(num_classes):
        raise ValueError(f"class_weights holds {len(cw)} values for {num_classes} classes")

    def unified_loss_and_grad(params, coords, mods, labels, dropout=None, boundary_weights=None):
        dev = _require_gpu()
        desc = inject_desc(params, coord_layers, mod_layers)
        if desc.width[desc.numLayers - 1] != int(num_classes):
            raise ValueError(f"the network has {desc.width[desc.numLayers - 1]} outputs for {num_classes} classes")
        c, m = _inject_points(coords, mods, dev, desc.numMods)
        n = int(c.shape[0])
        B, w, b = _inject_flat(params, dev)
        lab = torch.as_tensor(labels).to(dev).to(torch.int32).contiguous()
        bw = torch.as_tensor(boundary_weights).to(dev).to(torch.float32).contiguous() if boundary_weights is not None else None
        scratch = inject_train_scratch(desc, n, dev)
        logits = inject_forward_train(desc, B, w, b, c, m, n, scratch, dropout)
        loss, aux, dl = unified_loss_and_dlogits(logits, lab, unified, bw)
        gB, gw, gb = inject_backward(desc, B, w, c, m, n, dl, scratch, dropout)
        return (loss, aux), _inject_split(desc, gB, gw, gb)

    if unified is not None:
        return unified_loss_and_grad

    def loss_and_grad(params, coords, mods, labels, dropout=None):
        dev = _require_gpu()
        desc = inject_desc(params, coord_layers, mod_layers)
        if desc.width[desc.numLayers - 1] != int(num_classes):
            raise ValueError(f"the network has {desc.width[desc.numLayers - 1]} outputs for {num_classes} classes")
        c, m = _inject_points(coords, mods, dev, desc.numMods)
        n = int(c.shape[0])
        B, w, b = _inject_flat(params, dev)
        lab = torch.as_tensor(labels).to(dev).to(torch.int32).contiguous()
        scratch = inject_train_scratch(desc, n, dev)
        logits = inject_forward_train(desc, B, w, b, c, m, n, scratch, dropout)
        loss, aux, dl, *terms = loss_and_dlogits(logits, lab, cw, dice_weight, scratch, ext=ext)
        gB, gw, gb = inject_backward(desc, B, w, c, m, n, dl, scratch, dropout)
        return (loss, {"ce_per_class": aux[0], "dice_per_class": aux[1], **({"terms": terms[0]} if terms else {})}), _inject_split(desc, gB, gw, gb)

    return loss_and_grad


class _InjectStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coords, mods, coord_layers, mod_layers, dropout, num_layers, B, *wb):
        Ws, bs = wb[:num_layers], wb[num_layers:]
        params = {"fourier": {"B": B.detach()}, "mlp": [{"W": W.detach(), "b": b.detach()} for W, b in zip(Ws, bs)]}
        desc = inject_desc(params, coord_layers, mod_layers)
        dev = B.device
        n = int(coords.shape[0])
        Bf = B.detach().to(torch.float32).contiguous()
        w_flat = torch.cat([W.detach().to(torch.float32).reshape(-1) for W in Ws])
        b_flat = torch.cat([b.detach().to(torch.float32).reshape(-1) for b in bs])
        scratch = inject_train_scratch(desc, n, dev)
        logits = inject_forward_train(desc, Bf, w_flat, b_flat, coords, mods, n, scratch, dropout)
        ctx.saved = (desc, Bf, w_flat, coords, mods, n, scratch, dropout)
        return logits

    @staticmethod
    def backward(ctx, grad_logits):
        desc, Bf, w_flat, coords, mods, n, scratch, dropout = ctx.saved
        gB, gw, gb = inject_backward(desc, Bf, w_flat, coords, mods, n, grad_logits.to(torch.float32).contiguous(), scratch, dropout)
        g = _inject_split(desc, gB, gw, gb)
        return (None, None, None, None, None, None, g["fourier"]["B"], *[x["W"] for x in g["mlp"]], *[x["b"] for x in g["mlp"]])


def inject_autograd(B, Ws, bs, coords, mods, coord_layers=(1, 2, 3), mod_layers=(2,), dropout: Optional[_lib.InjectDropout] = None) -> torch.Tensor:
    """Differentiable fp32 logits (n, C) of the coordinate-injection network: the forward is ``mrirt_inject_forward_train``,
    the backward ``mrirt_inject_backward`` -- gradients reach ``B`` (F / 2, 3), ``Ws`` (each (in, out)) and ``bs``, none the
    inputs, so any torch loss and optimiser can fit the network."""
    dev = B.device
    M = int(Ws[0].shape[0]) - 2 * int(B.shape[0])
    c, m = _inject_points(coords, mods, dev, max(M, 0))
    return _InjectStep.apply(c, m, tuple(coord_layers), tuple(mod_layers), dropout, len(Ws), B, *Ws, *bs)


# the notebook's hybrid sampler and coordinate noise (csrc/inr_hybrid.hip)

def select_largest(values: torch.Tensor, k: int) -> torch.Tensor:
    """``mrirt_select_largest``: the indices of the ``k`` largest of the fp32 device values (n <= 65536), in ascending index
    order, as a device int32 tensor (k,): ``sorted(np.argsort(key, kind="stable")[-k:])`` under the order that puts -0 below +0
    and every NaN last; among equals the higher index wins."""
    v = values.reshape(-1)
    if not v.is_cuda or v.dtype != torch.float32 or not v.is_contiguous():
        raise ValueError("select_largest needs a contiguous fp32 device tensor")
    out = torch.empty(max(int(k), 0), dtype=torch.int32, device=v.device)
    _lib.check(_lib.lib().mrirt_select_largest(_ptr(v), int(v.numel()), int(k), _ptr(out), _stream_ptr(None)), "mrirt_select_largest")
    return out


def normal3(seed: int, batch_index: int, n: int) -> torch.Tensor:
    """``mrirt_inr_normal3``: the (n, 3) fp32 unit normals the hybrid sampler scales by its sigma for ``(seed, batch_index)``."""
    out = torch.empty((int(n), 3), dtype=torch.float32, device=_require_gpu())
    _lib.check(_lib.lib().mrirt_inr_normal3(int(seed) & (2 ** 64 - 1), int(batch_index) & (2 ** 64 - 1), int(n), _ptr(out), _stream_ptr(None)),
               "mrirt_inr_normal3")
    return out


def hybrid_counts(micro: int, uncertainty_ratio: float, balanced_ratio: float, num_classes: int, use_uncertainty: bool,
                  max_candidates: int = 10000) -> Tuple[int, int, int]:
    """``(n_uncertain, n_per_class, n_cand)`` of the notebook's ``sample_batch_hybrid`` (cell 9), with its truncations:
    ``int(micro * uncertainty_ratio)`` (0 without uncertainty), ``int(micro * balanced_ratio) // num_classes`` and
    ``min(max_candidates, 10 * n_uncertain)``."""
    n_unc = int(int(micro) * float(uncertainty_ratio)) if use_uncertainty else 0
    n_per = int(int(micro) * float(balanced_ratio)) // int(num_classes)
    return n_unc, n_per, min(int(max_candidates), 10 * n_unc)


def inject_uncertainty(desc: _lib.InjectDesc, B: torch.Tensor, w_flat: torch.Tensor, b_flat: torch.Tensor, coords: torch.Tensor, mods, n: int,
                       dropout: _lib.InjectDropout, scratch=None) -> torch.Tensor:
    """``mrirt_inject_uncertainty`` on flat parameters: the MC-dropout entropy (n,) fp32 of ``dropout.samples`` passes.
    ``scratch``: what ``_inject_scratch(desc, n', dev)`` returned for some ``n' >= n``, allocated when None."""
    ent = torch.empty(int(n), dtype=torch.float32, device=w_flat.device)
    scratch, nbytes = scratch if scratch is not None else _inject_scratch(desc, int(n), w_flat.device)
    rc = _lib.lib().mrirt_inject_uncertainty(C.byref(desc), _ptr(B), _ptr(w_flat), _ptr(b_flat), _ptr(coords), _ptr(mods) if mods is not None else None,
                                             int(n), C.byref(dropout), _ptr(ent), None, _ptr(scratch), nbytes, _stream_ptr(None))
    _lib.check(rc, "mrirt_inject_uncertainty")
    return ent


HYBRID_KEYS = ("UNCERTAINTY_RATIO", "BALANCED_RATIO")
NOISE_KEYS = ("COORD_NOISE_SIGMA_INIT", "COORD_NOISE_SIGMA_FINAL")


class _HybridBatches:
    """The micro-batches of ``train_inject`` under the notebook's hybrid keys and / or its noise keys (cells 9 and 12)."""

    def __init__(self, config, cache: VoxelCache, desc: _lib.InjectDesc, keep: float, with_field: bool):
        self.cache, self.desc, self.keep, self.with_field = cache, desc, keep, with_field
        self.nc, self.seed, self.micro = int(config["NUM_CLASSES"]), int(config["RNG_SEED"]), int(config["MICRO_BATCH_SIZE"])
        self.warmup, self.stage1 = int(config["WARMUP_STEPS"]), int(config["STAGE1_STEPS"])
        self.total = self.stage1 + int(config["STAGE2_STEPS"])
        self.hybrid = "UNCERTAINTY_RATIO" in config
        self.ratios = (float(config.get("UNCERTAINTY_RATIO", 0.0)), float(config.get("UNCERTAINTY_RATIO_STAGE2", 0.75)))
        self.balanced = float(config.get("BALANCED_RATIO", 0.0))
        self.samples = int(config.get("UNCERTAINTY_MC_SAMPLES", 5))
        self.sigmas = (float(config.get("COORD_NOISE_SIGMA_INIT", 0.0)), float(config.get("COORD_NOISE_SIGMA_FINAL", 0.0)))
        self.scratch = None
        if self.hybrid:
            if not 1 <= self.samples < 2 ** 24:
                raise ValueError("UNCERTAINTY_MC_SAMPLES must be 1 .. 2^24 - 1")
            most = 0
            for r in self.ratios:
                U, P, n_cand = self.counts(r, True)
                if U < 0 or P < 0 or U > self.micro or U > n_cand or n_cand > 65536:
                    raise ValueError(f"an uncertainty ratio of {r} with BALANCED_RATIO {self.balanced} gives {U} + {self.nc} x {P} of {self.micro} "
                                     f"points from {n_cand} candidates")
                most = max(most, n_cand)
            if most > 0:
                self.scratch = _inject_scratch(desc, most, cache.device)

    def counts(self, ratio: float, use_uncertainty: bool) -> Tuple[int, int, int]:
        """``hybrid_counts`` with the balanced segment cut to what the uncertain one leaves: the notebook's stage-2 ratios
        (0.75 + 0.3) let its batch grow past MICRO_BATCH_SIZE; here a micro-batch always has MICRO_BATCH_SIZE points."""
        U, P, n_cand = hybrid_counts(self.micro, ratio, self.balanced, self.nc, use_uncertainty)
        return U, min(P, max(self.micro - U, 0) // self.nc), n_cand

    def sigma(self, t: int) -> float:
        p = t / self.total
        return float(np.float32(self.sigmas[0] * (1.0 - p) + self.sigmas[1] * p))

    def __call__(self, t: int, g: int, B: torch.Tensor, w: torch.Tensor, b: torch.Tensor):
        """(coords, mods, labels, boundary weights or None) of global micro-batch ``g`` in step ``t``, scored by the parameters given."""
        U = P = 0
        picks = None
        if self.hybrid:
            U, P, n_cand = self.counts(self.ratios[0] if t < self.stage1 else self.ratios[1], t > self.warmup)
        if U > 0:
            cc, cm, _ = self.cache.sample_candidates(self.seed, g, n_cand)
            S = self.samples
            dp = inject_dropout(self.seed + 1, self.keep, S, (g * S) % (2 ** 24 - S), 0)
            ent = inject_uncertainty(self.desc, B, w, b, cc, cm if self.desc.numMods else None, n_cand, dp, self.scratch)
            picks = select_largest(ent, U)
        out = self.cache.sample_hybrid(self.seed, g, self.micro, U, picks, P, self.nc, self.sigma(t), self.with_field)
        return out if self.with_field else (*out, None)


def _hybrid_of_config(config) -> Tuple[bool, bool]:
    """(hybrid keys present, noise keys present); refuses half a group and TUMOR_RATIO beside either."""
    hybrid, noise = [k in config for k in HYBRID_KEYS], [k in config for k in NOISE_KEYS]
    if any(hybrid) != all(hybrid) or any(noise) != all(noise):
        raise ValueError("UNCERTAINTY_RATIO goes with BALANCED_RATIO, COORD_NOISE_SIGMA_INIT with COORD_NOISE_SIGMA_FINAL")
    if (any(hybrid) or any(noise)) and "TUMOR_RATIO" in config:
        raise ValueError("TUMOR_RATIO cannot be combined with the hybrid sampler's keys or the coordinate noise keys")
    if any(noise):
        for k in NOISE_KEYS:
            if not (np.isfinite(float(config[k])) and float(config[k]) >= 0.0):
                raise ValueError(f"{k} must be finite and >= 0")
    return any(hybrid), any(noise)


def two_stage_schedule(stage1_steps: int, stage2_steps: int, lr_stage1: float, lr_stage2: float, warmup_steps: int, min_lr: float):
    """The notebook's two-stage rate (cell 11) as ``schedule(step) -> float`` in host fp64: a linear warm-up to ``lr_stage1``,
    a linear blend to ``lr_stage2`` at ``stage1_steps``, then to ``min_lr`` over ``stage2_steps``.  With ``stage2_steps == 0``
    the last stage is never evaluated below ``stage1_steps``; from there on the rate is ``min_lr``."""
    s1, s2, warm = int(stage1_steps), int(stage2_steps), int(warmup_steps)
    lr1, lr2, lo = float(lr_stage1), float(lr_stage2), float(min_lr)

    def schedule(step):
        if step < warm:
            return lr1 * (step / warm)
        if step < s1:
            u = (step - warm) / (s1 - warm)
            return lr1 * (1.0 - u) + lr2 * u
        if s2 == 0:
            return lo
        u = (step - s1) / s2
        return lr2 * (1.0 - u) + lo * u

    return schedule


def inject_save(path, params) -> None:
    """The notebook's flat checkpoint (cell 14: ``fourier_B``, ``mlp_W_i``, ``mlp_b_i``), which ``inject_load`` reads back."""
    flat = {"fourier_B": _inject_np(params["fourier"]["B"])}
    for i, layer in enumerate(params["mlp"]):
        flat[f"mlp_W_{i}"], flat[f"mlp_b_{i}"] = _inject_np(layer["W"]), _inject_np(layer["b"])
    np.savez_compressed(path, **flat)


def train_inject(config: Dict[str, Any], cases_or_cache, params=None, log=None, save_path=None):
    """The notebook's training loop (cells 11 - 13) over the library's calls, with its config keys: FOURIER_DIM, HIDDEN_DIMS,
    COORD_INJECTION_LAYERS, MODALITY_INJECTION_LAYERS, DROPOUT_RATE, MICRO_BATCH_SIZE, ACCUM_STEPS, STAGE1_STEPS, STAGE2_STEPS,
    LR_STAGE1, LR_STAGE2, MIN_LR, WARMUP_STEPS, WEIGHT_DECAY, CLIP_NORM, CLASS_WEIGHTS (and NUM_CLASSES, DICE_WEIGHT, RNG_SEED as
    ``train_inr`` reads them; the optional FOCAL_GAMMA ... TUMOR_RATIO keys of ``loss_ext_of_config`` switch to
    ``mrirt_inr_loss_ext`` and the tumour-ratio sampler).  Step ``t`` (0-based) of STAGE1_STEPS + STAGE2_STEPS runs ACCUM_STEPS
    micro-batches -- ``VoxelCache.sample(RNG_SEED, g, MICRO_BATCH_SIZE)`` with ``g`` the global micro-batch index,
    ``mrirt_inject_forward_train`` (dropout at keep ``1 - DROPOUT_RATE`` only for ``t > WARMUP_STEPS``, as cell 12 has it, with
    ``sample0 = g`` and ``index0 = 0``), the loss, ``mrirt_inject_backward`` accumulating after the first -- and one
    ``mrirt_inr_adamw_step`` over the flat parameters ``[w | B]`` and ``b`` with ``gscale = 1 / ACCUM_STEPS``, ``clipNorm =
    CLIP_NORM`` and the rate of ``two_stage_schedule`` at ``t``.  A config that holds UNIFIED_FOCAL_GAMMA trains with the
    notebook's own loss (cell 8) instead, ``mrirt_unified_loss``: gamma and UNIFIED_FOCAL_LAMBDA (0.5 when absent), the Dice over
    CLASS_WEIGHTS, BOUNDARY_WEIGHT (0.1 when absent) on the boundary weights ``cache.sample_field`` returns for the micro-batch's
    own ``(RNG_SEED, g, n_tumour)`` (``cache.set_boundary()`` is called when the cache has no maps yet), and the TV weight of
    cell 12: TV_WEIGHT_STAGE1 for ``t < STAGE1_STEPS``, else TV_WEIGHT_STAGE2; DICE_WEIGHT and the ``loss_ext_of_config`` loss
    keys are then not read (TUMOR_RATIO still is), and ``log`` also gets ``train/ufl``, ``train/dice_loss``, ``train/tv_loss`` and
    ``train/boundary_loss``, each the mean over the step's micro-batches.  A config without that key runs exactly as before.
    UNCERTAINTY_RATIO with BALANCED_RATIO switches either loop to the notebook's hybrid sampler (cell 9; UNIFORM_RATIO is accepted
    and not read, as there): with ``(U, P, n_cand) = hybrid_counts(MICRO_BATCH_SIZE, ratio, BALANCED_RATIO, NUM_CLASSES, t >
    WARMUP_STEPS)`` and ``ratio`` UNCERTAINTY_RATIO for ``t < STAGE1_STEPS``, else UNCERTAINTY_RATIO_STAGE2 (0.75 when absent), a
    micro-batch with ``U > 0`` draws ``cache.sample_candidates(RNG_SEED, g, n_cand)``, scores them with
    ``mrirt_inject_uncertainty`` on the current parameters (``S`` = UNCERTAINTY_MC_SAMPLES, 5 when absent, passes at keep ``1 -
    DROPOUT_RATE``, dropout seed ``RNG_SEED + 1``, ``sample0 = (g S) % (2^24 - S)``, ``index0 = 0``), keeps ``select_largest(entropy,
    U)`` and trains on ``cache.sample_hybrid(RNG_SEED, g, MICRO_BATCH_SIZE, U, picks, P, NUM_CLASSES, sigma)``; where ``U + NUM_CLASSES
    P`` would exceed the micro-batch (the notebook's stage 2: 0.75 + 0.3), ``P`` is cut to ``(MICRO_BATCH_SIZE - U) // NUM_CLASSES``.
    COORD_NOISE_SIGMA_INIT with COORD_NOISE_SIGMA_FINAL, alone or beside the hybrid keys, add cell 12's coordinate noise: ``sigma =
    INIT (1 - p) + FINAL p`` with ``p = t / (STAGE1_STEPS + STAGE2_STEPS)`` in double, passed as fp32.  With either group the
    unified loop takes its boundary weights from the same launch (``with_field``) and does not call ``sample_field``; TUMOR_RATIO
    beside either group raises ``ValueError`` before a cache is built.  A config without these keys runs exactly as before.
    ``save_path``: a directory; ``model_final.npz`` (the notebook's layout) is written there.
    Returns ``(params, state)``: NumPy ``params`` and a dict with ``loss_history`` and ``opt`` (the ``AdamWState`` over
    ``[w | B]`` and ``b``)."""
    nc, seed = int(config["NUM_CLASSES"]), int(config["RNG_SEED"])
    micro, accum = int(config["MICRO_BATCH_SIZE"]), int(config["ACCUM_STEPS"])
    warmup, total = int(config["WARMUP_STEPS"]), int(config["STAGE1_STEPS"]) + int(config["STAGE2_STEPS"])
    if micro < 1 or accum < 1 or total < 1:
        raise ValueError("MICRO_BATCH_SIZE, ACCUM_STEPS and STAGE1_STEPS + STAGE2_STEPS must be positive")
    cl, ml = tuple(config["COORD_INJECTION_LAYERS"]), tuple(config["MODALITY_INJECTION_LAYERS"])
    schedule = two_stage_schedule(config["STAGE1_STEPS"], config["STAGE2_STEPS"], config["LR_STAGE1"], config["LR_STAGE2"], warmup, config["MIN_LR"])
    keep = float(np.float32(1.0) - np.float32(config["DROPOUT_RATE"]))
    ext_keys = _ext_keys_of(config)
    hybrid, noise = _hybrid_of_config(config)
    ext = loss_ext_of_config(config, nc) if ext_keys and "UNIFIED_FOCAL_GAMMA" not in config else None
    cache = cases_or_cache if isinstance(cases_or_cache, VoxelCache) else VoxelCache(cases_or_cache)
    n_tumour = n_tumour_of(micro, config.get("TUMOR_RATIO", 0.0)) if ext_keys else 0
    dev = cache.device
    if params is None:
        params = inject_init(seed, int(config["FOURIER_DIM"]), cache.n_modalities, config["HIDDEN_DIMS"], nc, cl, ml)
    desc = inject_desc(params, cl, ml)
    if desc.numMods != cache.n_modalities or desc.width[desc.numLayers - 1] != nc:
        raise ValueError(f"the parameters take {desc.numMods} modalities and give {desc.width[desc.numLayers - 1]} classes; the cache holds "
                         f"{cache.n_modalities}, the config asks for {nc}")
    B, w, b = _inject_flat(params, dev)
    nw = w.numel()
    wB = torch.cat([w, B.reshape(-1)])                   # one flat allocation [w | B]: one optimiser call updates everything
    st = AdamWState([], wB, b, torch.zeros_like(wB), torch.zeros_like(b), torch.zeros_like(wB), torch.zeros_like(b), 0)
    gwB, gb = torch.empty_like(wB), torch.empty_like(b)
    scratch = inject_train_scratch(desc, micro, dev)
    cw = [float(v) for v in config["CLASS_WEIGHTS"]]
    loss_history: List[Any] = []
    unified = "UNIFIED_FOCAL_GAMMA" in config
    batches = _HybridBatches(config, cache, desc, keep, unified) if hybrid or noise else None
    if unified:
        return _train_inject_unified(config, cache, desc, st, wB, b, nw, gwB, gb, scratch, schedule, keep, n_tumour, log, save_path, batches)
    for t in range(total):
        losses = []
        for k in range(accum):
            g = t * accum + k
            c, m, lab = cache.sample(seed, g, micro, n_tumour) if batches is None else batches(t, g, wB[nw:], wB[:nw], b)[:3]
            drop = inject_dropout(seed, keep, 1, g, 0) if t > warmup else None
            m = m if desc.numMods else None
            logits = inject_forward_train(desc, wB[nw:], wB[:nw], b, c, m, micro, scratch, drop)
            loss, _, dl, *_ = loss_and_dlogits(logits, lab, cw, float(config["DICE_WEIGHT"]), scratch, ext=ext)
            inject_backward(desc, wB[nw:], wB[:nw], c, m, micro, dl, scratch, drop, gwB[nw:], gwB[:nw], gb, accumulate=k > 0)
            losses.append(loss)
        adamw_step(st, gwB, gb, schedule(t), 1.0 / accum, float(config["CLIP_NORM"]), weight_decay=float(config["WEIGHT_DECAY"]))
        loss_history.append(torch.stack(losses).mean())      # stays on the device: without a log nothing waits for a step
        if log is not None:
            log(t + 1, {"train/loss": float(loss_history[-1]), "train/step": t + 1, "train/lr": schedule(t)})
    return _train_inject_finish(desc, st, wB, b, nw, cache, loss_history, save_path)


def _train_inject_finish(desc, st, wB, b, nw, cache, loss_history, save_path):
    """What ``train_inject`` returns and writes, from the flat state of either of its loops."""
    loss_history = [float(v) for v in torch.stack(loss_history).cpu()]
    out = _inject_split(desc, wB[nw:].clone(), wB[:nw].clone(), b.clone())
    out = {"fourier": {"B": _inject_np(out["fourier"]["B"])}, "mlp": [{"W": _inject_np(p["W"]), "b": _inject_np(p["b"])} for p in out["mlp"]]}
    if save_path is not None:
        save_path = pathlib.Path(save_path)
        save_path.mkdir(parents=True, exist_ok=True)
        inject_save(save_path / "model_final.npz", out)
    return out, {"params": out, "train_cache": cache, "loss_history": loss_history, "opt": st, "save_path": save_path}


UNIFIED_LOG_KEYS = ("ufl", "dice_loss", "tv_loss", "boundary_loss")


def _train_inject_unified(config, cache, desc, st, wB, b, nw, gwB, gb, scratch, schedule, keep, n_tumour, log, save_path, batches=None):
    """``train_inject``'s loop with the notebook's loss (cells 8 and 12): the same sampler, forward, backward and optimiser calls
    with ``mrirt_unified_loss`` between forward and backward, on a scratch of its own.  ``batches``: the hybrid sampler's, which
    returns the boundary weights with the batch."""
    nc, seed = int(config["NUM_CLASSES"]), int(config["RNG_SEED"])
    micro, accum = int(config["MICRO_BATCH_SIZE"]), int(config["ACCUM_STEPS"])
    warmup, stage1 = int(config["WARMUP_STEPS"]), int(config["STAGE1_STEPS"])
    total = stage1 + int(config["STAGE2_STEPS"])
    cw = list(config["CLASS_WEIGHTS"])
    if len(cw) != nc:
        raise ValueError(f"CLASS_WEIGHTS holds {len(cw)} values for {nc} classes")
    stages = [unified_loss(cw, float(config["UNIFIED_FOCAL_GAMMA"]), float(config.get("UNIFIED_FOCAL_LAMBDA", 0.5)), tv_weight=float(config[key]),
                           boundary_weight=float(config.get("BOUNDARY_WEIGHT", 0.1))) for key in ("TV_WEIGHT_STAGE1", "TV_WEIGHT_STAGE2")]
    if getattr(cache, "boundary_table", None) is None:
        cache.set_boundary()
    loss_scratch = unified_loss_scratch(micro, cache.device)
    loss_history: List[Any] = []
    for t in range(total):
        cfg = stages[0] if t < stage1 else stages[1]
        losses, terms = [], []
        for k in range(accum):
            g = t * accum + k
            if batches is None:
                c, m, lab = cache.sample(seed, g, micro, n_tumour)
                bw = cache.sample_field(seed, g, micro, n_tumour)
            else:
                c, m, lab, bw = batches(t, g, wB[nw:], wB[:nw], b)
            drop = inject_dropout(seed, keep, 1, g, 0) if t > warmup else None
            m = m if desc.numMods else None
            logits = inject_forward_train(desc, wB[nw:], wB[:nw], b, c, m, micro, scratch, drop)
            loss, aux, dl = unified_loss_and_dlogits(logits, lab, cfg, bw, loss_scratch)
            inject_backward(desc, wB[nw:], wB[:nw], c, m, micro, dl, scratch, drop, gwB[nw:], gwB[:nw], gb, accumulate=k > 0)
            losses.append(loss)
            terms.append(torch.stack([aux[key] for key in UNIFIED_LOG_KEYS]))
        adamw_step(st, gwB, gb, schedule(t), 1.0 / accum, float(config["CLIP_NORM"]), weight_decay=float(config["WEIGHT_DECAY"]))
        loss_history.append(torch.stack(losses).mean())
        if log is not None:
            mean = [float(v) for v in torch.stack(terms).mean(0).cpu()]
            log(t + 1, {"train/loss": float(loss_history[-1]), "train/step": t + 1, "train/lr": schedule(t),
                        **{"train/" + key: v for key, v in zip(UNIFIED_LOG_KEYS, mean)}})
    return _train_inject_finish(desc, st, wB, b, nw, cache, loss_history, save_path)
