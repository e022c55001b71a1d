"""References for the INR training step (csrc/inr_train.hip).  No GPU.

  step           torch CPU autograd over the formulas of the step (inr/inr/model.py:64-88 for the loss) in a chosen dtype:
                 fp64 is what the kernels approximate, fp32 is the yardstick of the tolerances (a
                 tolerance is 8 x what the same formula does in fp32 on the CPU, never what the kernel gives)
  loss_terms     the loss alone on given logits
  int_step       integer ReLU nets in int64: logits, dW, db, with the bound that makes fp32 exact in any summation order
  kink_free      the points of a case that keep every hidden pre-activation away from the ReLU kink
"""
import numpy as np
import torch

EPS = 1e-6


def build_input(coords, feats, K, dtype):
    """model.py:11-23 in torch: (coords, per axis [sin k = 1..K, cos k = 1..K], intensities)."""
    c = torch.as_tensor(np.asarray(coords), dtype=dtype)
    ang = c[..., None] * torch.arange(1, K + 1, dtype=dtype)[None, None, :] * torch.tensor(np.pi, dtype=dtype)
    ff = torch.cat([torch.sin(ang), torch.cos(ang)], -1).reshape(c.shape[0], -1)
    parts = [c, ff]
    if feats is not None:
        parts.append(torch.as_tensor(np.asarray(feats), dtype=dtype).reshape(c.shape[0], -1))
    return torch.cat(parts, 1)


def loss_terms(logits, labels, cw, dw, num_classes):
    """model.py:70-88 in its operation order on torch tensors: (loss, ce_per_class, dice_per_class)."""
    dtype = logits.dtype
    lab = torch.as_tensor(np.asarray(labels), dtype=torch.int64)
    y = torch.nn.functional.one_hot(lab, num_classes).to(dtype)
    ce_vec = -(y * torch.log_softmax(logits, -1)).sum(-1)
    w = torch.as_tensor(np.asarray(cw), dtype=dtype)[lab]
    ce = (ce_vec * w).mean()
    probs = torch.softmax(logits, -1)
    inter = (probs * y).sum(0)
    sums = probs.sum(0) + y.sum(0)
    dice = (2 * inter + EPS) / (sums + EPS)
    loss = (1 - dw) * ce + dw * (1 - dice.mean()) if dw > 0 else ce
    counts = y.sum(0)
    ce_k = (ce_vec[:, None] * y).sum(0) / torch.clamp(counts, min=1.0)
    return loss, ce_k, dice


def _np(t):
    return t.detach().numpy().copy()


def loss_alone(logits, labels, cw, dw, dtype=torch.float64):
    z = torch.as_tensor(np.asarray(logits), dtype=dtype).clone().requires_grad_(True)
    loss, ce_k, dice = loss_terms(z, labels, cw, dw, z.shape[1])
    loss.backward()
    return dict(loss=float(loss.detach()), aux=np.stack([_np(ce_k), _np(dice)]), dlogits=_np(z.grad))


def step(layers, x, loss_of_logits, dtype=torch.float64, perm=None):
    """Forward + autograd of ``loss_of_logits(logits) -> (loss, aux or None)`` through the ReLU MLP on the input matrix x.
    Returns logits, loss, aux, dlogits, grads [(dW, db)], and per layer the scales A_W = |h_{l-1}|^T |dz_l|, A_b = sum_p |dz_l|
    and the pre-activations z.  ``perm`` reorders the batch first (sums over the batch then run in another order); logits
    and dlogits come back in the original order."""
    xx = torch.as_tensor(np.asarray(x), dtype=dtype)
    if perm is not None:
        xx = xx[torch.as_tensor(perm)]
    Ws = [torch.as_tensor(np.asarray(p["W"]), dtype=dtype).clone().requires_grad_(True) for p in layers]
    bs = [torch.as_tensor(np.asarray(p["b"]), dtype=dtype).clone().requires_grad_(True) for p in layers]
    h, hs, zs = xx, [], []
    for i, (W, b) in enumerate(zip(Ws, bs)):
        hs.append(h)
        z = h @ W + b
        z.retain_grad()
        zs.append(z)
        h = torch.relu(z) if i + 1 < len(Ws) else z
    loss, aux = loss_of_logits(h)
    loss.backward()
    inv = None if perm is None else np.argsort(np.asarray(perm))
    back = (lambda a: a) if inv is None else (lambda a: a[inv])
    return dict(logits=back(_np(h)), loss=float(loss.detach()), aux=None if aux is None else np.stack([_np(a) for a in aux]),
                dlogits=back(_np(zs[-1].grad)), grads=[(_np(W.grad), _np(b.grad)) for W, b in zip(Ws, bs)],
                A=[(_np(hh.abs().T @ z.grad.abs()), _np(z.grad.abs().sum(0))) for hh, z in zip(hs, zs)],
                z=[back(_np(z)) for z in zs])


def model_loss(labels, cw, dw, num_classes, perm=None):
    lab = np.asarray(labels) if perm is None else np.asarray(labels)[np.asarray(perm)]

    def f(logits):
        loss, ce_k, dice = loss_terms(logits, lab, cw, dw, num_classes)
        return loss, (ce_k, dice)
    return f


def kink_free(layers, x, margin=2e-5):
    """Boolean mask of the points whose every hidden |z| (fp64) is at least ``margin`` x rms(z of that layer)."""
    h = np.asarray(x, np.float64)
    keep = np.ones(h.shape[0], bool)
    for p in layers[:-1]:
        z = h @ np.asarray(p["W"], np.float64) + np.asarray(p["b"], np.float64)
        keep &= (np.abs(z) >= margin * np.sqrt(np.mean(z * z))).all(1)
        h = np.maximum(z, 0.0)
    return keep


def int_step(layers, x, dlogits):
    """int64 forward and backward of an integer ReLU net: dict(logits, grads [(dW, db)], bound, zero_units, dead_units) where
    bound = the largest sum of |terms| over every dot product of the step (the batch sums included) — below 2^24 every
    partial sum is an integer fp32 holds exactly, whatever the order — zero_units counts hidden pre-activations that are
    exactly 0 and dead_units hidden units that are <= 0 for every point."""
    Ws = [np.asarray(p["W"]).astype(np.int64) for p in layers]
    bs = [np.asarray(p["b"]).astype(np.int64) for p in layers]
    h = np.asarray(x).astype(np.int64)
    hs, zs, bound, zero, dead = [], [], 0, 0, 0
    for i, (W, b) in enumerate(zip(Ws, bs)):
        hs.append(h)
        z = h @ W + b
        bound = max(bound, int((np.abs(h) @ np.abs(W) + np.abs(b)).max()))
        zs.append(z)
        if i + 1 < len(Ws):
            zero += int((z == 0).sum())
            dead += int((z <= 0).all(0).sum())
            h = np.maximum(z, 0)
    dz = np.asarray(dlogits).astype(np.int64)
    grads = [None] * len(Ws)
    for i in range(len(Ws) - 1, -1, -1):
        grads[i] = (hs[i].T @ dz, dz.sum(0))
        bound = max(bound, int((np.abs(hs[i]).T @ np.abs(dz)).max()), int(np.abs(dz).sum(0).max()))
        if i > 0:
            bound = max(bound, int((np.abs(dz) @ np.abs(Ws[i]).T).max()))
            dz = (dz @ Ws[i].T) * (zs[i - 1] > 0)
    return dict(logits=zs[-1], grads=grads, bound=bound, zero_units=zero, dead_units=dead)


def central_differences(f, theta, idx, h=1e-6):
    """d f / d theta[idx] by central differences in fp64 (f takes the flat parameter vector)."""
    out = []
    for i in idx:
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        out.append((f(tp) - f(tm)) / (2 * h))
    return np.array(out)


def deviation(ref, got):
    """Worst |g - g_ref| / A over all gradients of a step, A the fp64 scales (entries with A = 0 must agree exactly)."""
    worst = 0.0
    for (gw, gb), (rw, rb), (Aw, Ab) in zip(got["grads"], ref["grads"], ref["A"]):
        for g, r, A in ((gw, rw, Aw), (gb, rb, Ab)):
            d = np.abs(np.asarray(g, np.float64) - r)
            nz = A > 0
            if (d[~nz] != 0).any():
                return np.inf
            if nz.any():
                worst = max(worst, float((d[nz] / A[nz]).max()))
    return worst
