"""The unified focal + Dice + TV + boundary loss of include/mrirt.h (``mrirt_unified_loss``) restated on the CPU: torch in fp64
(the reference of the GPU tests) and with fp32 per-point values (what the kernels compute, batch sums in fp64), ``dlogits`` from
autograd with the closed-interval clip rule written out, and the derivative's closed form in NumPy with the sum of the absolute
values of its terms, which scales the per-element tolerance.  A config is a dict: cw, gamma, lam, alpha, beta, ufl_w, dice_w,
tv_w, bd_w."""
import numpy as np
import torch

AUX_KEYS = ("ufl", "mFTL", "mFL", "dice_loss", "tv_loss", "boundary_loss", "dice_mean_tumor", "accuracy")
LOGIT_CLIP = 10.0


def config(cw, gamma=0.5, lam=0.5, alpha=0.3, beta=0.7, ufl_w=0.5, dice_w=0.5, tv_w=0.02, bd_w=0.1, round32=True):
    """The values the library reads: every float rounded to fp32 as the struct holds it (``round32=False``: the Python floats
    as they are, which is what the notebook computes with)."""
    f = (lambda v: float(np.float32(v))) if round32 else float
    return dict(cw=[f(v) for v in cw], gamma=f(gamma), lam=f(lam), alpha=f(alpha), beta=f(beta), ufl_w=f(ufl_w), dice_w=f(dice_w),
                tv_w=f(tv_w), bd_w=f(bd_w))


class ClosedClip(torch.autograd.Function):
    """clip(x, lo, hi) whose gradient passes where lo <= x <= hi and nowhere else (at an exact tie JAX halves it)."""

    @staticmethod
    def forward(ctx, x, lo, hi):
        ctx.save_for_backward((x >= lo) & (x <= hi))
        return torch.minimum(torch.maximum(x, torch.as_tensor(lo, dtype=x.dtype)), torch.as_tensor(hi, dtype=x.dtype))

    @staticmethod
    def backward(ctx, g):
        (inside,) = ctx.saved_tensors
        return g * inside.to(g.dtype), None, None


def prob_clips(dtype):
    one, eps = torch.tensor(1.0, dtype=dtype), torch.tensor(1e-7, dtype=dtype)
    return float(eps), float(one - eps)


def finite_rows(z):
    return np.isfinite(np.asarray(z, np.float64)).all(1)


def argmax_first(z):
    """The first index of the largest logit of each row (NumPy's rule)."""
    return np.argmax(np.asarray(z), axis=1)


def forward(z, labels, bw, cfg, dtype=torch.float64, want_grad=True):
    """(loss, aux dict, dlogits or None, totals dict) with per-point values in ``dtype`` and everything after the batch sums in
    fp64; all results NumPy fp64.  Rows with a non-finite logit take no part and get a zero gradient row."""
    z_all = np.asarray(z, np.float32)
    n, C = z_all.shape
    labels = np.asarray(labels, np.int64)
    keep = np.nonzero(finite_rows(z_all))[0]
    zt = torch.tensor(z_all[keep].astype(np.float64), dtype=dtype, requires_grad=want_grad)
    lab = torch.tensor(labels[keep])
    lo, hi = prob_clips(dtype)
    zc = ClosedClip.apply(zt, -LOGIT_CLIP, LOGIT_CLIP)
    ps = torch.softmax(zc, 1)
    pc = ClosedClip.apply(ps, lo, hi)
    pu = torch.softmax(zt, 1)
    inr = (lab >= 0) & (lab < C)
    t = torch.zeros((len(keep), C), dtype=dtype)
    t[inr, lab[inr]] = 1.0
    d = lambda x: x.to(torch.float64)
    P, A, T, S, Q = d(pc).sum(0), d(pc * t).sum(0), d(t).sum(0), d(pu).sum(0), (d(pu) * d(pu)).sum(0)
    q = (pc * t).sum(1)[inr]                                        # pc_y of the points whose label is in the range
    eps7, eps10 = torch.tensor(1e-7, dtype=dtype), torch.tensor(1e-10, dtype=dtype)
    fl = torch.pow((1.0 - q) + eps7, torch.tensor(cfg["gamma"], dtype=dtype)) * -torch.log(q + eps10)
    FL = d(fl).sum()
    am = torch.tensor(argmax_first(z_all[keep]) if len(keep) else np.zeros(0, np.int64))
    dist = (am - lab).abs().to(torch.float64)
    Bd = (torch.tensor(np.asarray(bw, np.float64)[keep]) * dist).sum() if bw is not None else torch.tensor(0.0, dtype=torch.float64)
    Acc = (am == lab).to(torch.float64).sum()
    al, be, ga, lam = cfg["alpha"], cfg["beta"], cfg["gamma"], cfg["lam"]
    TI = ClosedClip.apply(A / (A + al * (P - A) + be * (T - A) + 1e-7), 0.0, 1.0)
    mFTL = torch.pow(1.0 - TI + 1e-7, 1.0 / ga).mean()
    mFL = FL / n
    ufl = ClosedClip.apply(lam * mFTL + (1.0 - lam) * mFL, 0.0, 1e6)
    dice = (2.0 * A + 1.0) / (P + T + 1.0)
    cw = torch.tensor(cfg["cw"], dtype=torch.float64)
    dl = ClosedClip.apply(1.0 - (dice * cw).sum() / (cw.sum() + 1e-10), 0.0, 10.0)
    tv = (Q / n - (S / n) ** 2).sum()
    bl = Bd / n
    loss = cfg["ufl_w"] * ufl + cfg["dice_w"] * dl + cfg["tv_w"] * tv + cfg["bd_w"] * bl
    grad = None
    if want_grad:
        grad = np.zeros((n, C), np.float64)
        if len(keep):
            loss.backward()
            grad[keep] = zt.grad.detach().to(torch.float64).numpy()
    v = lambda x: float(x.detach())
    aux = dict(ufl=v(ufl), mFTL=v(mFTL), mFL=v(mFL), dice_loss=v(dl), tv_loss=v(tv), boundary_loss=v(bl),
               dice_mean_tumor=float(dice[1:].mean().detach()) if C > 1 else 0.0, accuracy=v(Acc / n),
               dice_per_class=dice.detach().numpy().copy())
    tot = dict(P=P.detach().numpy(), A=A.detach().numpy(), T=T.detach().numpy(), S=S.detach().numpy(), Q=Q.detach().numpy(), FL=v(FL), Bd=v(Bd),
               Acc=v(Acc))
    return v(loss), aux, grad, tot


def aux_vector(aux):
    """aux in the ABI's order: the eight scalars, then Dice per class."""
    return np.concatenate([[aux[k] for k in AUX_KEYS], aux["dice_per_class"]])


def closed_form(z, labels, bw, cfg):
    """(dlogits, A) in NumPy fp64 from the closed form the kernel evaluates; A[i][j] is the sum of the absolute values of the
    terms of element (i, j)'s derivative."""
    z = np.asarray(z, np.float32).astype(np.float64)
    n, C = z.shape
    labels = np.asarray(labels, np.int64)
    fin = finite_rows(z)
    lo, hi = 1e-7, 1.0 - 1e-7
    zs = np.where(fin[:, None], z, 0.0)

    def softmax(x):
        e = np.exp(x - x.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)

    ps, pu = softmax(np.clip(zs, -LOGIT_CLIP, LOGIT_CLIP)), softmax(zs)
    pc = np.clip(ps, lo, hi)
    t = np.zeros((n, C))
    inr = (labels >= 0) & (labels < C) & fin
    t[inr, labels[inr]] = 1.0
    m = fin[:, None].astype(np.float64)
    P, A, T, S = (pc * m).sum(0), (pc * t).sum(0), t.sum(0), (pu * m).sum(0)
    q = (pc * t).sum(1)
    al, be, ga, lam = cfg["alpha"], cfg["beta"], cfg["gamma"], cfg["lam"]
    FL = (np.power(1.0 - q[inr] + 1e-7, ga) * -np.log(q[inr] + 1e-10)).sum()
    D = A + al * (P - A) + be * (T - A) + 1e-7
    ti = A / D
    base = 1.0 - np.clip(ti, 0.0, 1.0) + 1e-7
    ftl = np.power(base, 1.0 / ga)
    dftl = np.where((ti >= 0) & (ti <= 1), -(1.0 / ga) * np.power(base, 1.0 / ga - 1.0), 0.0)
    ufl_raw = lam * ftl.mean() + (1.0 - lam) * FL / n
    gu = 1.0 if 0.0 <= ufl_raw <= 1e6 else 0.0
    den = P + T + 1.0
    dice = (2.0 * A + 1.0) / den
    cw = np.asarray(cfg["cw"], np.float64)
    dl_raw = 1.0 - (dice * cw).sum() / (cw.sum() + 1e-10)
    gd = 1.0 / (cw.sum() + 1e-10) if 0.0 <= dl_raw <= 10.0 else 0.0
    cT = cfg["ufl_w"] * gu * lam / C * dftl
    cD = -cfg["dice_w"] * gd * cw
    tiA, tiP = (D - A * (1.0 - al - be)) / D ** 2, -A * al / D ** 2
    GP = [cT * tiP, -cD * dice / den]
    GA = [cT * tiA, cD * 2.0 / den]
    cF = cfg["ufl_w"] * gu * (1.0 - lam) / n
    qs = np.where(inr, q, 0.5)
    bq = 1.0 - qs + 1e-7
    df = [-(ga * np.power(bq, ga - 1.0)) * -np.log(qs + 1e-10), -np.power(bq, ga) / (qs + 1e-10)]
    h = ((ps >= lo) & (ps <= hi)).astype(np.float64)
    G = h * (GP[0] + GP[1] + t * (GA[0] + GA[1] + (cF * (df[0] + df[1]))[:, None]))
    Gabs = h * (abs(GP[0]) + abs(GP[1]) + t * (abs(GA[0]) + abs(GA[1]) + (abs(cF) * (abs(df[0]) + abs(df[1])))[:, None]))
    tvc = 2.0 * cfg["tv_w"] / n
    V, Vabs = tvc * (pu - S / n), tvc * (pu + S / n)
    gate = ((zs >= -LOGIT_CLIP) & (zs <= LOGIT_CLIP)).astype(np.float64)
    g = gate * ps * (G - (G * ps).sum(1, keepdims=True)) + pu * (V - (V * pu).sum(1, keepdims=True))
    a = gate * ps * (Gabs + (Gabs * ps).sum(1, keepdims=True)) + pu * (Vabs + (Vabs * pu).sum(1, keepdims=True))
    return g * m, a * m


def central_differences(z, labels, bw, cfg, elems, h):
    """D(h) and D(h / 2) of the fp64 loss at the listed (i, j) elements, which must be finite logits away from every clip edge."""
    z = np.asarray(z, np.float32).astype(np.float64)
    out = np.zeros((len(elems), 2))

    def loss_at(zz):
        # the restatement rounds its input to fp32: evaluate the fp64 graph on fp64 logits directly
        return _loss64_on_double(zz, labels, bw, cfg)

    for e, (i, j) in enumerate(elems):
        for s, step in enumerate((h, h / 2)):
            zp, zm = z.copy(), z.copy()
            zp[i, j] += step
            zm[i, j] -= step
            out[e, s] = (loss_at(zp) - loss_at(zm)) / (2 * step)
    return out


def _loss64_on_double(z, labels, bw, cfg):
    """The loss in fp64 on fp64 logits (finite rows only): NumPy, no autograd -- for the difference quotients."""
    n, C = z.shape
    labels = np.asarray(labels, np.int64)
    e = np.exp(np.clip(z, -LOGIT_CLIP, LOGIT_CLIP) - np.clip(z, -LOGIT_CLIP, LOGIT_CLIP).max(1, keepdims=True))
    pc = np.clip(e / e.sum(1, keepdims=True), 1e-7, 1.0 - 1e-7)
    e = np.exp(z - z.max(1, keepdims=True))
    pu = e / e.sum(1, keepdims=True)
    inr = (labels >= 0) & (labels < C)
    t = np.zeros((n, C))
    t[inr, labels[inr]] = 1.0
    P, A, T, S, Q = pc.sum(0), (pc * t).sum(0), t.sum(0), pu.sum(0), (pu * pu).sum(0)
    q = (pc * t).sum(1)[inr]
    FL = (np.power(1.0 - q + 1e-7, cfg["gamma"]) * -np.log(q + 1e-10)).sum()
    TI = np.clip(A / (A + cfg["alpha"] * (P - A) + cfg["beta"] * (T - A) + 1e-7), 0.0, 1.0)
    ufl = np.clip(cfg["lam"] * np.power(1.0 - TI + 1e-7, 1.0 / cfg["gamma"]).mean() + (1.0 - cfg["lam"]) * FL / n, 0.0, 1e6)
    cw = np.asarray(cfg["cw"], np.float64)
    dl = np.clip(1.0 - (((2.0 * A + 1.0) / (P + T + 1.0)) * cw).sum() / (cw.sum() + 1e-10), 0.0, 10.0)
    tv = (Q / n - (S / n) ** 2).sum()
    bl = 0.0 if bw is None else (np.asarray(bw, np.float64) * np.abs(np.argmax(z, 1) - labels)).sum() / n
    return cfg["ufl_w"] * ufl + cfg["dice_w"] * dl + cfg["tv_w"] * tv + cfg["bd_w"] * bl


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
