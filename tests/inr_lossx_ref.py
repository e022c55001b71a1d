"""References for the extended INR loss and the tumour-ratio sampler (csrc/inr_lossx.hip).  No GPU.

  loss_terms      scripts/jax_inr_brats.py:179-257 restated in torch in its operation order, on given logits, in a chosen dtype
                  (fp64: what the kernels approximate; fp32: the yardstick of the tolerances); autograd supplies dlogits
  loss_alone      the same as NumPy results: loss, aux, terms, dlogits
  ext_loss        a ``loss_of_logits`` for inr_train_ref.step / inr_siren_ref's step
  tumour_index    np.flatnonzero(seg > 0) per case, concatenated, with the offsets
  sample_mix      the mixed sampler on top of the Philox restatement of inr_loop_ref.py

The options travel as a dict ``opt`` with the keys of OPT_DEFAULT; the float options are rounded to float32 first — what the C
struct holds — so that both dtypes evaluate the same function (``round32=False`` keeps them as given: the goldens' fp64).
"""
import numpy as np
import torch

import inr_loop_ref as lp

EPS = 1e-6
OPT_DEFAULT = dict(dice_weight=0.0, focal_gamma=0.0, focal_alpha=None, label_smoothing=0.0, per_class_dice=True, edema_fp_weight=0.0,
                   tversky_alpha=0.8, tversky_beta=0.2, tversky_weight=0.0, edema_logit_reg=0.0, edema_class=2, round32=True)
NEUTRAL = dict(OPT_DEFAULT)


def options(**kw):
    bad = set(kw) - set(OPT_DEFAULT)
    if bad:
        raise KeyError(sorted(bad))
    return dict(OPT_DEFAULT, **kw)


def _rounder(opt):
    return (lambda v: np.asarray(v, np.float32).astype(np.float64)) if opt["round32"] else (lambda v: np.asarray(v, np.float64))


def loss_terms(logits, labels, cw, opt):
    """(loss, ce_per_class, dice_per_class, terms[5]) as torch values of logits' dtype."""
    dtype = logits.dtype
    n, C = logits.shape
    e = int(opt["edema_class"])
    rnd = _rounder(opt)
    _f32 = lambda v: float(rnd(v))                        # noqa: E731
    eps, dw, gamma = _f32(opt["label_smoothing"]), _f32(opt["dice_weight"]), _f32(opt["focal_gamma"])
    lab = torch.as_tensor(np.asarray(labels), dtype=torch.int64)
    valid = (lab >= 0) & (lab < C)
    yh = torch.nn.functional.one_hot(torch.where(valid, lab, torch.zeros_like(lab)), C).to(dtype) * valid[:, None].to(dtype)
    y = yh * (1.0 - eps) + eps / C if eps > 0 else yh
    logp = torch.log_softmax(logits, -1)
    p = torch.softmax(logits, -1)
    ce_vec = -(y * logp).sum(-1)
    cwt = torch.as_tensor(rnd(cw), dtype=dtype)
    w = (yh * cwt[None, :]).sum(-1)                      # classWeights[label], 0 outside the range
    if gamma > 0:
        pt = (y * p).sum(-1)
        mod = torch.clamp(1.0 - pt, min=0.0) ** gamma
        if opt["focal_alpha"] is not None:
            mod = mod * (y * torch.as_tensor(rnd(opt["focal_alpha"]), dtype=dtype)[None, :]).sum(-1)
        ce = (mod * ce_vec).mean() * w.mean()            # jax_inr_brats.py:227-233: a scalar times the weight vector, averaged
    else:
        ce = (ce_vec * w).mean()
    inter = (p * y).sum(0)
    Y = y.sum(0)
    dice = (2 * inter + EPS) / (p.sum(0) + Y + EPS)
    if opt["per_class_dice"]:
        dl = 1.0 - dice.mean()
    else:
        v = (Y / (Y.sum() + EPS)).detach()
        dl = 1.0 - (dice * v).sum()
    loss = (1.0 - dw) * ce + dw * dl if dw > 0 else ce
    zero = torch.zeros((), dtype=dtype)
    fp_mean, tv, reg = zero, zero, zero
    if e < C:
        g = (lab == e).to(dtype)
        q = p[:, e]
        tp, fp, fn = (q * g).sum(), (q * (1 - g)).sum(), ((1 - q) * g).sum()
        fp_mean = fp / n
        tv = tp / (tp + _f32(opt["tversky_alpha"]) * fp + _f32(opt["tversky_beta"]) * fn + EPS)
        ze = logits[:, e]
        reg = ((torch.clamp(ze, min=0.0) + torch.log1p(torch.exp(-ze.abs()))) * (1 - g)).mean()
    if opt["edema_fp_weight"] > 0:
        loss = loss + _f32(opt["edema_fp_weight"]) * fp_mean
    if opt["tversky_weight"] > 0:
        loss = loss + _f32(opt["tversky_weight"]) * (1.0 - tv)
    if opt["edema_logit_reg"] > 0:
        loss = loss + _f32(opt["edema_logit_reg"]) * reg
    counts = yh.sum(0)
    ce_k = (ce_vec[:, None] * yh).sum(0) / torch.clamp(counts, min=1.0)
    terms = torch.stack([ce, dl if dw > 0 else zero, fp_mean, tv, reg])
    return loss, ce_k, dice, terms


def _np(t):
    return t.detach().numpy().copy()


def loss_alone(logits, labels, cw, opt, dtype=torch.float64, perm=None):
    """dict(loss, aux (2, C), terms (5,), dlogits (n, C)); ``perm`` evaluates the batch in another order (dlogits come back in
    the original one)."""
    z0 = np.asarray(logits)
    lab = np.asarray(labels)
    if perm is not None:
        z0, lab = z0[np.asarray(perm)], lab[np.asarray(perm)]
    z = torch.as_tensor(z0, dtype=dtype).clone().requires_grad_(True)
    loss, ce_k, dice, terms = loss_terms(z, lab, cw, opt)
    loss.backward()
    dl = _np(z.grad)
    if perm is not None:
        dl = dl[np.argsort(np.asarray(perm))]
    return dict(loss=float(loss.detach()), aux=np.stack([_np(ce_k), _np(dice)]), terms=_np(terms), dlogits=dl)


def ext_loss(labels, cw, opt, perm=None):
    """``loss_of_logits`` for inr_train_ref.step: (loss, (ce_per_class, dice_per_class))."""
    lab = np.asarray(labels) if perm is None else np.asarray(labels)[np.asarray(perm)]

    def f(logits):
        loss, ce_k, dice, _ = loss_terms(logits, lab, cw, opt)
        return loss, (ce_k, dice)
    return f


# ---- tumour index and the mixed sampler ---------------------------------------------------------------------------------------------
def tumour_index(cases):
    """(index uint32, offsets int64 [ncases + 1]): flat offsets x W D + y D + z of the voxels with seg > 0, ascending per case."""
    per = [np.flatnonzero(np.asarray(c["seg"]).reshape(-1) > 0).astype(np.uint32) for c in cases]
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in per])]).astype(np.int64)
    return (np.concatenate(per) if per else np.zeros(0, np.uint32)), offsets


def n_tumour_of(n, ratio):
    """jax_inr_brats.py:468: int(n * clip(ratio, 0, 1)) in double."""
    return int(float(n) * min(max(float(ratio), 0.0), 1.0))


def draw_mix(seed, batch_index, n, n_tumour, ncases, hwd, index, offsets):
    """(case, x, y, z, from_index) of the n points: the uniform draw of inr_loop_ref.draw, with the first n_tumour points taken
    from the tumour index where their case has any tumour voxel."""
    seed, b = int(seed) & (2 ** 64 - 1), int(batch_index) & (2 ** 64 - 1)
    i = np.arange(n, dtype=np.uint64)
    r = lp.philox4x32_10((i, b & lp.MASK, b >> 32, 0), (seed & lp.MASK, seed >> 32))
    cs, x, y, z = lp.mulhi32(r[0], ncases), lp.mulhi32(r[1], hwd[0]), lp.mulhi32(r[2], hwd[1]), lp.mulhi32(r[3], hwd[2])
    used = np.zeros(n, bool)
    if n_tumour > 0:
        offsets = np.asarray(offsets, np.int64)
        cnt = offsets[cs + 1] - offsets[cs]
        used = (np.arange(n) < n_tumour) & (cnt > 0)
        slot = offsets[cs] + ((r[1].astype(np.uint64) * cnt.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        v = np.asarray(index, np.int64)[np.where(used, slot, 0)] if len(index) else np.zeros(n, np.int64)
        W, D = int(hwd[1]), int(hwd[2])
        x = np.where(used, v // (W * D), x)
        y = np.where(used, (v // D) % W, y)
        z = np.where(used, v % D, z)
    return cs, x, y, z, used


def sample_mix(cases, seed, batch_index, n, n_tumour, index=None, offsets=None):
    """coords (n, 3) fp32, feats (n, M) fp32, labels (n,) int32, and which points came from the index."""
    hwd = cases[0]["seg"].shape
    if index is None:
        index, offsets = tumour_index(cases)
    cs, x, y, z, used = draw_mix(seed, batch_index, n, n_tumour, len(cases), hwd, index, offsets)
    coords = np.stack([(v.astype(np.float32) / np.float32(e - 1)) * np.float32(2.0) - np.float32(1.0) for v, e in zip((x, y, z), hwd)], 1)
    mods = np.stack([np.asarray(c["mods"], np.float32) for c in cases])
    seg = np.stack([np.asarray(c["seg"]) for c in cases])
    feats = mods[cs, :, x, y, z].astype(np.float32).reshape(n, mods.shape[1])
    labels = seg[cs, x, y, z].astype(np.int32)
    return coords.astype(np.float32), feats, labels, used
