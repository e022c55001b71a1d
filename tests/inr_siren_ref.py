"""References for SIREN training (csrc/siren_sincos.h, the sine / cosine epilogues of csrc/inr_train.hip).
No GPU.

  sincos32        csrc/siren_sincos.h restated in NumPy float64, operation by operation: the same bits as the device
  SINCOS_SETS     the argument sets the restatement (CPU) and siren_sincos itself (device probe) are run over: the sweep, every
                  fp32 of [2^19, 2^20] in both signs, every quadrant switch with its neighbours, zeros / denormals / powers of
                  two, and beyond the domain; bits_differ and libm_figures are the two comparisons made on them
  siren_layout    SirenLayout of csrc/inr_train.h restated: where the step's scratch keeps x', h_l, c_l and the slabs
  step            torch CPU autograd over the definition of section 16 in a chosen dtype: fp64 (torch.sin) is what the kernels
                  approximate; fp32 with the restated sine is the yardstick of the tolerances
  np_step         the definition in NumPy float32 with the restated sine: on a selection net every dot product has one
                  non-zero term, so this is what the kernels must give bit for bit, whatever the order of their sums
  selection_net   weights in {0, 1}: W_0 column j selects input j mod in, hidden matrices are permutations, the head selects
                  `out` distinct hidden units; biases normal fp32
  np_step_slabs   np_step with dW / db summed slab by slab in fp32, in slab order (tr_slab_reduce_kernel's order)
  single_term     the proof of np_step's claim for a case: the most non-zero terms of any dot product, the smallest |sine|
  train           the loop of inr_loop_ref.train with the SIREN step
"""
import functools

import numpy as np

DOMAIN = 2.0 ** 20
TWO_OVER_PI = float.fromhex("0x1.45f306dc9c883p-1")
P1 = float.fromhex("0x1.921fb54400000p+0")
P2 = float.fromhex("0x1.0b4611a600000p-34")
P3 = float.fromhex("0x1.3198a2e037073p-69")
S_COEF = [float.fromhex(h) for h in ("0x1.952c77030ad4ap-49", "-0x1.ae7f3e733b81fp-41", "0x1.6124613a86d09p-33", "-0x1.ae64567f544e4p-26",
                                     "0x1.71de3a556c734p-19", "-0x1.a01a01a01a01ap-13", "0x1.1111111111111p-7", "-0x1.5555555555555p-3")]
C_COEF = [float.fromhex(h) for h in ("0x1.ae7f3e733b81fp-45", "-0x1.93974a8c07c9dp-37", "0x1.1eed8eff8d898p-29", "-0x1.27e4fb7789f5cp-22",
                                     "0x1.a01a01a01a01ap-16", "-0x1.6c16c16c16c17p-10", "0x1.5555555555555p-5", "-0x1.0p-1")]


_CHUNK = 1 << 20                   # elements of one pass of the restatement: its fp64 temporaries stay in cache


def sincos32(a):
    """(sin32(a), cos32(a)) as float32 arrays: siren_sincos of csrc/siren_sincos.h, one NumPy operation per C operation.
    sin32(-0) and the sine of every finite argument beyond the domain, negative ones included, are +0: there x = -0, k = -0 and
    r = -0 - (-0 * P1) = -0 - (-0) = +0."""
    a = np.asarray(a, np.float32)
    if a.size > _CHUNK:                                   # element-wise: the same values, piece by piece
        flat = a.reshape(-1)
        so, co = np.empty(flat.size, np.float32), np.empty(flat.size, np.float32)
        for i in range(0, flat.size, _CHUNK):
            so[i:i + _CHUNK], co[i:i + _CHUNK] = sincos32(flat[i:i + _CHUNK])
        return so.reshape(a.shape), co.reshape(a.shape)
    with np.errstate(invalid="ignore"):
        x = a.astype(np.float64)
        x = np.where(np.abs(x) <= DOMAIN, x, x * 0.0)
        k = np.rint(x * TWO_OVER_PI)
        r = x - k * P1
        r = r - k * P2
        r = r - k * P3
        r2 = r * r
        s = S_COEF[0] * r2
        for c in S_COEF[1:]:
            s = (s + c) * r2
        s = r + r * s
        c = C_COEF[0] * r2
        for v in C_COEF[1:]:
            c = (c + v) * r2
        c = 1.0 + c
        q = k - 4.0 * np.rint(k * 0.25)
        so = np.where(q == 0.0, s, np.where(q == 1.0, c, np.where((q == 2.0) | (q == -2.0), -s, -c)))
        co = np.where(q == 0.0, c, np.where(q == 1.0, -s, np.where((q == 2.0) | (q == -2.0), -c, s)))
    return so.astype(np.float32), co.astype(np.float32)


def sincos_arguments(seed=0, per_range=500_000, multiples=200_000):
    """The make-up of the sweep: uniform in +-4, +-100, +-65536, +-2^20, and the fp32 neighbours of the first multiples of pi/2."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-lim, lim, per_range).astype(np.float32) for lim in (4.0, 100.0, 65536.0, DOMAIN)]
    m = (np.arange(1, multiples + 1) * (np.pi / 2)).astype(np.float32)
    for sign in (1.0, -1.0):
        mm = (sign * m).astype(np.float32)
        parts += [mm, np.nextafter(mm, np.float32(np.inf)), np.nextafter(mm, np.float32(-np.inf))]
    edge = np.float32(DOMAIN)
    parts.append(np.array([edge, -edge, np.nextafter(edge, np.float32(0)), -np.nextafter(edge, np.float32(0)), 0.0, -0.0], np.float32))
    a = np.concatenate(parts)
    return a[np.abs(a) <= DOMAIN]


def ulps(got, want64):
    """|got - want| in units of the fp32 spacing at want."""
    want64 = np.asarray(want64, np.float64)
    sp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / sp


# ---- the argument sets of the sine's sweeps: shared by the CPU tests and the device probe -----------------------------------------

QUADRANT_KS = 667_544              # (k + 1/2) pi/2 < 2^20 for k = 0 .. 667 543


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def top_binade_arguments(sign):
    """Every fp32 of [2^19, 2^20] with the given sign (8 388 609): the largest k and the coarsest spacing of the domain."""
    a = np.arange(0x49000000, 0x49800001, dtype=np.uint32).view(np.float32)
    return a if sign > 0 else -a


def quadrant_switch_arguments():
    """(2 x QUADRANT_KS, 5): float32((k + 1/2) pi/2), where rint(a 2/pi) steps from k to k + 1, between its two fp32 neighbours
    on each side; the second half of the rows is the first negated."""
    m = ((np.arange(QUADRANT_KS) + 0.5) * (np.pi / 2)).astype(np.float32)
    pos = (m.view(np.uint32).astype(np.int64)[:, None] + np.arange(-2, 3)).astype(np.uint32).view(np.float32)
    return np.concatenate([pos, -pos])


def quadrant_index(a):
    """k = rint(a 2/pi) as the restatement computes it."""
    return np.rint(np.asarray(a, np.float32).astype(np.float64) * TWO_OVER_PI)


def small_and_special_arguments():
    """+-0, every 4099th denormal, 2^e for e = -149 .. 20, +-2^20 and its inner neighbours; each in both signs."""
    den = np.arange(1, 0x00800000, 4099, dtype=np.uint32).view(np.float32)
    p2 = np.ldexp(1.0, np.arange(-149, 21)).astype(np.float32)
    edge = np.float32(DOMAIN)
    pos = np.concatenate([np.zeros(1, np.float32), den, p2, np.array([edge, np.nextafter(edge, np.float32(0))], np.float32)])
    return np.concatenate([pos, -pos])


def outside_arguments():
    """Beyond the domain: the first float above 2^20, 2^20 + 1, 2^24, 1e10, FLT_MAX, inf in both signs; quiet NaNs of both signs."""
    edge = np.float32(DOMAIN)
    pos = np.array([np.nextafter(edge, np.float32(np.inf)), DOMAIN + 1.0, 2.0 ** 24, 1e10, np.finfo(np.float32).max, np.inf], np.float32)
    return np.concatenate([pos, -pos, _f32([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC54321])])


SINCOS_SETS = {
    "sweep": lambda: sincos_arguments(),
    "top_binade_pos": lambda: top_binade_arguments(1),
    "top_binade_neg": lambda: top_binade_arguments(-1),
    "quadrant_switches": lambda: quadrant_switch_arguments().reshape(-1),
    "small_and_special": small_and_special_arguments,
    "outside": outside_arguments,
}
INSIDE_SETS = ("sweep", "top_binade_pos", "top_binade_neg", "quadrant_switches", "small_and_special")


@functools.lru_cache(maxsize=None)
def sincos_set(name):
    """(a, sin32(a), cos32(a)) of one argument set; computed once per process, not to be written to."""
    a = np.ascontiguousarray(SINCOS_SETS[name]())
    s, c = sincos32(a)
    for v in (a, s, c):
        v.setflags(write=False)
    return a, s, c


def bits_differ(got, want):
    """Indices where ``got`` has not the bit pattern of ``want`` (the sign of zero included); where ``want`` is a NaN, where
    ``got`` is none (payloads are not compared)."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    nan = np.isnan(want)
    return np.flatnonzero(np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32)))


def libm_figures(a, s, c):
    """Per function: (results that differ from float32(np.sin / np.cos(float64(a))), worst error in fp32 ulp, largest |result|)."""
    fig = {"sin": [0, 0.0, 0.0], "cos": [0, 0.0, 0.0]}
    a, s, c = (np.asarray(v, np.float32).reshape(-1) for v in (a, s, c))
    for i in range(0, a.size, _CHUNK):
        x = a[i:i + _CHUNK].astype(np.float64)
        for what, got, want in (("sin", s[i:i + _CHUNK], np.sin(x)), ("cos", c[i:i + _CHUNK], np.cos(x))):
            f = fig[what]
            f[0] += int((got != want.astype(np.float32)).sum())
            f[1] = float(np.maximum(f[1], ulps(got, want).max()))          # np.maximum: a NaN stays
            f[2] = float(np.maximum(f[2], np.abs(got).max()))
    return {k: tuple(v) for k, v in fig.items()}


def assert_libm_figures(name, what_ran, a, s, c):
    """Print and hold the by-value figures of one argument set: at most 1 result in 10^5 off the rounded libm value, none by
    more than 1 fp32 ulp, none above 1 in magnitude."""
    fig = libm_figures(a, s, c)
    for what, (differ, worst, largest) in fig.items():
        print(f"{what_ran} {name} {what}: {differ} of {a.size} differ from float32(np.{what}(float64(a))); worst error {worst:.7f} fp32 ulp")
    for what, (differ, worst, largest) in fig.items():
        assert differ <= a.size // 100000, (name, what, differ)
        assert worst <= 1.0, (name, what, worst)
        assert largest <= 1.0, (name, what, largest)
    return fig


# ---- the scratch of a step (csrc/inr_train.h: train_layout, siren_layout) ---------------------------------------------------------

SLAB_MIN, MAX_SLABS, LOSS_THREADS, LOSS_MAX_BLOCKS, LOSS_VALS = 256, 64, 256, 256, 4 * 16 + 1


def tr_align(nbytes):
    return (int(nbytes) + 255) & ~255


def slab_len(n):
    ln = SLAB_MIN
    while -(-n // ln) > MAX_SLABS:
        ln *= 2
    return ln


def slabs(n):
    return -(-n // slab_len(n))


def slab_ranges(n):
    ln = slab_len(n)
    return [(k0, min(k0 + ln, n)) for k0 in range(0, n, ln)]


def loss_scratch_bytes(n):
    return tr_align((min(-(-n // LOSS_THREADS), LOSS_MAX_BLOCKS) + 1) * LOSS_VALS * 8)


def siren_layout(dims, n):
    """Byte offsets of the regions of a SIREN step's scratch for dims = [in, hidden, .., hidden, out] and n points: the loss
    sums, x' at offX, h_l at offH + l act, the two dz buffers at offDz, the slabs at offSlab (room for the most slabs any
    smaller n uses), and behind the ReLU step's size the cosines c_l at offC + l act."""
    depth, ind, hid = len(dims) - 1, dims[0], dims[1]
    act = tr_align(n * hid * 4)
    off_x = loss_scratch_bytes(n)
    off_h = off_x + tr_align(n * ind * 4)
    off_dz = off_h + (depth - 1) * act
    off_slab = off_dz + 2 * act
    slab_elems = max((a + 1) * b for a, b in zip(dims[:-1], dims[1:]))
    most = min(-(-n // SLAB_MIN), MAX_SLABS)
    off_c = off_slab + tr_align(most * slab_elems * 4)
    return dict(offX=off_x, offH=off_h, offDz=off_dz, offSlab=off_slab, offC=off_c, act=act, bytes=off_c + (depth - 1) * act,
                slabLen=slab_len(n), slabs=slabs(n))


# ---- the definition in torch ------------------------------------------------------------------------------------------------------

def _np(t):
    return t.detach().numpy().copy()


def _sine(dtype):
    import torch
    if dtype == torch.float64:
        return torch.sin

    class RestatedSine(torch.autograd.Function):         # h = sin32(a); da = fl32(dh * cos32(a))
        @staticmethod
        def forward(ctx, a):
            s, c = sincos32(a.detach().numpy())
            ctx.save_for_backward(torch.from_numpy(c))
            return torch.from_numpy(s)

        @staticmethod
        def backward(ctx, g):
            return g * ctx.saved_tensors[0]
    return RestatedSine.apply


def step(layers, x, w0, loss_of_logits, dtype=None, perm=None):
    """Forward + autograd of ``loss_of_logits(logits) -> (loss, aux or None)`` through the SIREN of section 16 on the input
    matrix x: x' = w0 x, a_l = in_l W_l + b_l, h_l = sin a_l, linear head.  Returns logits, loss, aux, dlogits, grads
    [(dW, db)], the scales A = [(|in_l|^T |da_l|, sum_p |da_l|)] and the pre-activations a.  ``perm`` reorders the batch."""
    import torch
    dtype = dtype or torch.float64
    xx = torch.as_tensor(np.asarray(x), dtype=dtype)
    if perm is not None:
        xx = xx[torch.as_tensor(perm)]
    sine = _sine(dtype)
    Ws = [torch.as_tensor(np.asarray(p["W"]), dtype=dtype).clone().requires_grad_(True) for p in layers]
    bs = [torch.as_tensor(np.asarray(p["b"]), dtype=dtype).clone().requires_grad_(True) for p in layers]
    h, hs, zs = xx * torch.tensor(w0, dtype=dtype), [], []
    for i, (W, b) in enumerate(zip(Ws, bs)):
        hs.append(h)
        z = h @ W + b
        z.retain_grad()
        zs.append(z)
        h = sine(z) if i + 1 < len(Ws) else z
    loss, aux = loss_of_logits(h)
    loss.backward()
    inv = None if perm is None else np.argsort(np.asarray(perm))
    back = (lambda a: a) if inv is None else (lambda a: a[inv])
    return dict(logits=back(_np(h)), loss=float(loss.detach()), aux=None if aux is None else np.stack([_np(a) for a in aux]),
                dlogits=back(_np(zs[-1].grad)), grads=[(_np(W.grad), _np(b.grad)) for W, b in zip(Ws, bs)],
                A=[(_np(hh.detach().abs().T @ z.grad.abs()), _np(z.grad.abs().sum(0))) for hh, z in zip(hs, zs)],
                z=[back(_np(z)) for z in zs])


def forward64(layers, x, w0):
    h = np.asarray(x, np.float64) * float(w0)
    for p in layers[:-1]:
        h = np.sin(h @ np.asarray(p["W"], np.float64) + np.asarray(p["b"], np.float64))
    return h @ np.asarray(layers[-1]["W"], np.float64) + np.asarray(layers[-1]["b"], np.float64)


def input_matrix(coords, feats):
    c = np.asarray(coords, np.float32)
    return c if feats is None else np.concatenate([c, np.asarray(feats, np.float32).reshape(c.shape[0], -1)], 1)


def as_dict(layers):
    return {f"l{i}": {"w": p["W"], "b": p["b"]} for i, p in enumerate(layers)}


def siren_layers(rng, dims, w0=30.0, bias=0.05):
    """siren_init's weights (U(+-sqrt(6 / in) / w0) for layer 0, U(+-sqrt(6 / in)) after it) with small non-zero biases."""
    return [{"W": (rng.uniform(-1, 1, (a, b)) * np.sqrt(6.0 / a) / (w0 if i == 0 else 1.0)).astype(np.float32),
             "b": rng.uniform(-bias, bias, b).astype(np.float32)} for i, (a, b) in enumerate(zip(dims[:-1], dims[1:]))]


# ---- the exact tier ---------------------------------------------------------------------------------------------------------------

def selection_net(rng, dims, shift=0):
    """See the module docstring; ``shift`` rotates which hidden units the head selects."""
    layers = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        W = np.zeros((a, b), np.float32)
        if i == 0:
            W[np.arange(b) % a, np.arange(b)] = 1.0
        elif i + 1 < len(dims) - 1:
            W[rng.permutation(a), np.arange(b)] = 1.0
        else:
            W[(shift + np.arange(b)) % a, np.arange(b)] = 1.0
        layers.append({"W": W, "b": rng.standard_normal(b).astype(np.float32)})
    return layers


def np_forward(layers, x, w0):
    """The forward of np_step: (logits, ins = [x', h_0, ..], cos = [c_0, ..]), float32 with the restated sine."""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        h = (f(w0) * np.asarray(x, f)).astype(f)
        ins, cs = [], []
        for i, p in enumerate(layers):
            ins.append(h)
            a = ((h @ p["W"].astype(f)).astype(f) + p["b"].astype(f)).astype(f)
            if i + 1 < len(layers):
                h, c = sincos32(a)
                cs.append(c)
            else:
                logits = a
    return logits, ins, cs


def np_step(layers, x, w0, dlogits, init_w=None, init_b=None):
    """The definition in float32 NumPy with the restated sine: dict(logits, gw, gb flat, ins, cos).  Exact for selection nets."""
    f = np.float32
    logits, ins, cs = np_forward(layers, x, w0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(dlogits, f)
        gw, gb = [None] * len(layers), [None] * len(layers)
        for i in range(len(layers) - 1, -1, -1):
            gw[i], gb[i] = (ins[i].T @ d).astype(f), d.sum(0, dtype=f)
            if i > 0:
                d = ((d @ layers[i]["W"].astype(f).T).astype(f) * cs[i - 1]).astype(f)
    gwf, gbf = np.concatenate([g.reshape(-1) for g in gw]), np.concatenate(gb)
    if init_w is not None:
        gwf, gbf = (np.asarray(init_w, f) + gwf).astype(f), (np.asarray(init_b, f) + gbf).astype(f)
    return dict(logits=logits, gw=gwf, gb=gbf, ins=ins, cos=cs)


def np_step_slabs(layers, x, w0, dlogits, slab_len, init_w=None, init_b=None, reverse=False, forward=None):
    """np_step with the gradients summed the way the kernels sum them (tr_slab_reduce_kernel): per layer, the batch is cut into
    slabs of ``slab_len`` points, partial_z = ins[slab z]^T d[slab z] and sum_p d[slab z], and g = (init or 0) + partial_0 +
    partial_1 + ... in fp32 in slab order.  Exact where every partial has one non-zero term (one non-zero dlogits row per slab
    of a selection net), however many slabs carry one.  dict(logits, gw, gb flat, ins, cos).  ``reverse``: the slabs from the last
    to the first, which is NOT what the kernels do (the tests use it to show that the order is visible in a case).  ``forward``:
    np_forward's result for these inputs, where the caller has it."""
    f = np.float32
    logits, ins, cs = forward if forward is not None else np_forward(layers, x, w0)
    r = dict(logits=logits, ins=ins, cos=cs)
    n = logits.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(dlogits, f)
        gw, gb = [None] * len(layers), [None] * len(layers)
        wo, bo = 0, 0
        offs = []
        for p in layers:
            offs.append((wo, bo))
            wo, bo = wo + p["W"].size, bo + p["W"].shape[1]
        for i in range(len(layers) - 1, -1, -1):
            a, b = layers[i]["W"].shape
            wo, bo = offs[i]
            g = np.zeros((a, b), f) if init_w is None else np.asarray(init_w, f)[wo:wo + a * b].reshape(a, b).copy()
            s = np.zeros(b, f) if init_b is None else np.asarray(init_b, f)[bo:bo + b].copy()
            for k0 in sorted(range(0, n, slab_len), reverse=reverse):
                sl = slice(k0, min(k0 + slab_len, n))
                g = (g + (r["ins"][i][sl].T @ d[sl]).astype(f)).astype(f)
                s = (s + d[sl].sum(0, dtype=f)).astype(f)
            gw[i], gb[i] = g, s
            if i > 0:
                d = ((d @ layers[i]["W"].astype(f).T).astype(f) * r["cos"][i - 1]).astype(f)
    return dict(logits=r["logits"], gw=np.concatenate([g.reshape(-1) for g in gw]), gb=np.concatenate(gb), ins=r["ins"], cos=r["cos"])


def single_term(layers, x, w0, dlogits, r=None):
    """(most non-zero terms over every dot product of the step, smallest |sine| stored, largest |pre-activation|): np_step is
    order-independent — hence what a k-ordered fma chain gives — when the first is <= 1, the second >= 2^-126 (no denormal
    operand) and the third <= 2^20 (the sine's domain).  ``r``: np_step's ins and cos of these very rows, where the caller has
    them already.  The counts are sums of 0 / 1 indicators in fp32: exact below 2^24 terms."""
    f = np.float32
    if r is None:
        r = np_step(layers, x, w0, dlogits)
    most, smallest, largest = 0, np.inf, 0.0
    d = np.asarray(dlogits, f) != 0
    assert d.shape[0] < 2 ** 24
    nz_d = [None] * len(layers)
    for i in range(len(layers) - 1, -1, -1):
        nz_d[i] = d
        if i > 0:
            terms = d.astype(f) @ (layers[i]["W"] != 0).astype(f).T
            most = max(most, int(terms.max()))
            d = (terms > 0) & (r["cos"][i - 1] != 0)
    for i, p in enumerate(layers):
        hin = r["ins"][i]
        most = max(most, int(((hin != 0).astype(f) @ (p["W"] != 0).astype(f)).max()))
        most = max(most, int(((hin != 0).astype(f).T @ nz_d[i].astype(f)).max()), int(nz_d[i].sum(0).max()))
        with np.errstate(invalid="ignore", over="ignore"):
            a = (hin @ p["W"]).astype(f) + p["b"]
        if i + 1 < len(layers):
            largest = max(largest, float(np.abs(a).max()))
            smallest = min(smallest, float(np.abs(r["ins"][i + 1]).min()))
    return most, smallest, largest


# ---- the loop -------------------------------------------------------------------------------------------------------------------

def train(layers, cases, cfg, steps, dtype_name="float64", order_seed=None, first_step=0):
    """inr_loop_ref.train with the SIREN step: cfg as there, plus w0 (K is not read).  Returns dict(w, b, losses, dims)."""
    import torch
    import inr_loop_ref as lr
    import inr_train_ref as tr
    tdt, ndt = getattr(torch, dtype_name), getattr(np, dtype_name)
    dims = [layers[0]["W"].shape[0]] + [p["W"].shape[1] for p in layers]
    w, b = lr.flat(layers, ndt)
    mu_w, mu_b, nu_w, nu_b = np.zeros_like(w), np.zeros_like(b), np.zeros_like(w), np.zeros_like(b)
    rng = np.random.default_rng(order_seed) if order_seed is not None else None
    losses = []
    for k in range(steps):
        t = first_step + k
        gw, gb, row = np.zeros_like(w), np.zeros_like(b), []
        for a in range(cfg["accum"]):
            coords, feats, labels, _ = lr.sample(cases, cfg["seed"], t * cfg["accum"] + a, cfg["micro"])
            if rng is not None:
                perm = rng.permutation(cfg["micro"])
                coords, feats, labels = coords[perm], feats[perm], labels[perm]
            x = input_matrix(coords, feats if feats.shape[1] else None)
            r = step(lr.unflat(w, b, dims), x, cfg["w0"], tr.model_loss(labels, cfg["cw"], cfg["dw"], cfg["classes"]), tdt)
            gw = gw + np.concatenate([g[0].reshape(-1) for g in r["grads"]]).astype(ndt)
            gb = gb + np.concatenate([g[1].reshape(-1) for g in r["grads"]]).astype(ndt)
            row.append(r["loss"])
        losses.append(row)
        gs = ndt(1.0) / ndt(cfg["accum"])
        g = np.concatenate([gw, gb]) * gs
        norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        s = lr.clip_factor(norm, cfg["clip"], ndt)
        rate = lr.lr_schedule(cfg["peak"], cfg["end"], cfg["warmup"], cfg["decay_steps"], t)
        w, mu_w, nu_w = lr.adamw_update(w, mu_w, nu_w, gw, s, rate, t, gs, dtype=ndt)
        b, mu_b, nu_b = lr.adamw_update(b, mu_b, nu_b, gb, s, rate, t, gs, dtype=ndt)
    return dict(w=w, b=b, losses=np.asarray(losses, np.float64), dims=dims)
