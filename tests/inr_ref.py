"""Plain NumPy references for the INR forward (csrc/inr_mlp.hip and its kernel units inr_stream.hip, inr_ws.hip, inr_refine.hip),
the networks of the shape sweep, and the packed weight image.  No GPU, no torch.

  forward64      the network in fp64: what the kernels approximate
  emulate_bf16   the error model of the bf16 pass: every operand rounded where the kernel rounds it (layer-0 inputs, weights
                 with the folded scale, activations -> bf16; a SIREN's first layer as hi + lo, three products), everything
                 else (accumulation, sine, ReLU) in fp64.  The kernel differs from it by fp32 accumulation and v_sin_f32 only.
  integer_relu_net   ReLU networks with weights in {-1, 0, +1}, biases in {-1, 0, 1} and small integer inputs: every product,
                 every partial sum and every activation is an integer of magnitude <= 256, i.e. exact in bf16 and in fp32 in
                 whatever order it is accumulated, so the kernel's logits must EQUAL forward64 and its classes must equal
                 np.argmax (first maximum) -- a dropped, duplicated or swapped row / column of the packed image changes an
                 integer somewhere, because every row of every matrix is used.

The sweep's nets (EXACT_NETS, FOURIER0_NETS, SINE_NETS) are listed here so that the host test can check their preconditions on
the CPU for exactly the seeds the GPU test uses.

  pack_image     the packed weight image of mrirt_inr_pack_weights (main and refine), written from the layout comments;
                 PACK_NETS / pack_case are the networks tests/test_gpu_inr_pack.py packs."""
import numpy as np

KIND_FOURIER_RELU, KIND_SIREN, KIND_RAW_RELU, KIND_RAW_SIREN = 0, 1, 2, 3
N_POINTS = 573                      # two full 256-point batches and a ragged 61
TWO_PI_F32 = 6.283185307179586


def bf16_round(a):
    """Round-to-nearest-even to bfloat16 (8 significant bits, fp32's exponent range, denormals kept), as float64."""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        _, e = np.frexp(np.where(np.isfinite(a), a, 0.0))                  # |a| = m 2^e, 0.5 <= m < 1
        q = np.ldexp(1.0, np.maximum(e, -125) - 8)                         # spacing of bf16 at a (2^-133 below 2^-126)
        r = np.rint(a / q) * q                                             # np.rint rounds halves to even
        r = np.where(np.abs(r) >= 2.0 ** 128, np.copysign(np.inf, a), r)
    return np.where(np.isfinite(a), r, a)


def fourier_features64(coords, K):
    """inr/inr/model.py:11-18: per axis [sin(pi 1 c) .. sin(pi K c), cos(pi 1 c) .. cos(pi K c)] -> (n, 6K)."""
    c = np.asarray(coords, np.float64)
    ang = c[..., None] * np.arange(1, K + 1, dtype=np.float64)[None, None, :] * np.pi
    return np.concatenate([np.sin(ang), np.cos(ang)], -1).reshape(c.shape[0], -1)


def build_input64(coords, feats, K):
    """model.py:21-23: (coords, Fourier features, intensities) -> (n, 3 + 6K + M); feats None = no intensities."""
    c = np.asarray(coords, np.float64)
    parts = [c, fourier_features64(c, K)]
    if feats is not None:
        parts.append(np.asarray(feats, np.float64).reshape(c.shape[0], -1))
    return np.concatenate(parts, 1)


def _wb(layers):
    return [(np.asarray(p["W"]), np.asarray(p["b"])) for p in layers]


def _is_siren(kind):
    return kind in (KIND_SIREN, KIND_RAW_SIREN)


def forward64(layers, x, kind, w0=30.0, return_hidden=False):
    """fp64 logits of the network on the input MATRIX x (n, in): build_input64 for the kinds that build it on the device.
    ReLU kinds: model.py:43-50.  SIREN kinds: sin(w0 (x W0) + b0), sin(h W + b), linear head."""
    wb = _wb(layers)
    h = np.asarray(x, np.float64)
    hidden = []
    for i, (W, b) in enumerate(wb[:-1]):
        z = h @ W.astype(np.float64)
        if _is_siren(kind):
            h = np.sin((float(w0) if i == 0 else 1.0) * z + b.astype(np.float64))
        else:
            h = np.maximum(z + b.astype(np.float64), 0.0)
        hidden.append(h)
    out = h @ wb[-1][0].astype(np.float64) + wb[-1][1].astype(np.float64)
    return (out, hidden) if return_hidden else out


def emulate_bf16(layers, x, kind, w0=30.0):
    """The bf16 pass with exact arithmetic between its roundings.  The kernel folds scale = w0 / 2 pi (first SIREN layer),
    1 / 2 pi (hidden SIREN layers), 1 (ReLU layers, every head) into the fp32 weight before rounding it to bf16, scales the
    biases by 1 / 2 pi in fp32, and takes the sine of revolutions."""
    wb = _wb(layers)
    siren = _is_siren(kind)
    h = np.asarray(x, np.float64)
    for i, (W, b) in enumerate(wb):
        head = i + 1 == len(wb)
        fold = siren and not head
        scale = np.float32(((float(w0) if i == 0 else 1.0) / TWO_PI_F32) if fold else 1.0)
        bscale = np.float32(1.0 / TWO_PI_F32 if fold else 1.0)
        Wf = (W.astype(np.float32) * scale).astype(np.float64)             # the fp32 product the packer rounds
        bf = (b.astype(np.float32) * bscale).astype(np.float64)
        Whi = bf16_round(Wf)
        hhi = bf16_round(h)
        if i == 0 and siren:                                               # hi*hi + lo*hi + hi*lo
            Wlo, hlo = bf16_round(Wf - Whi), bf16_round(h - hhi)
            z = hhi @ Whi + hlo @ Whi + hhi @ Wlo + bf
        else:
            z = hhi @ Whi + bf
        if head:
            return z
        h = np.sin(2.0 * np.pi * z) if siren else np.maximum(z, 0.0)


def top2_gap(logits):
    """Difference of the two largest logits per point (inf for a single class)."""
    if logits.shape[1] < 2:
        return np.full(logits.shape[0], np.inf)
    s = np.sort(logits, axis=1)
    return s[:, -1] - s[:, -2]


# ---- exact nets --------------------------------------------------------------------------------------------------------------

def _sparse_sign_matrix(rng, rows, cols, nnz):
    """(rows, cols) with entries in {-1, 0, +1}: every column has k = max(min(nnz, rows), ceil(rows / cols)) non-zeros and
    every row at least one.  (k exceeds nnz only where nnz x cols slots cannot reach every row: a wide input into a narrow
    layer, a hidden layer into a head of few classes.)"""
    k = max(min(nnz, rows), -(-rows // cols))
    W = np.zeros((rows, cols), np.float32)
    order = rng.permutation(rows)
    owned = [list(order[c::cols]) for c in range(cols)]                    # every row is dealt to one column
    for c in range(cols):
        rest = np.setdiff1d(np.arange(rows), owned[c])
        pick = owned[c] + list(rng.choice(rest, k - len(owned[c]), replace=False))
        W[pick, c] = rng.choice(np.array([-1.0, 1.0], np.float32), k)
    return W


def integer_relu_net(rng, dims, nnz=3):
    """dims = [in, hidden, .., hidden, out] -> layers [{"W", "b"}], fp32, see the module docstring."""
    return [{"W": _sparse_sign_matrix(rng, dims[i], dims[i + 1], nnz),
             "b": rng.integers(-1, 2, dims[i + 1]).astype(np.float32)} for i in range(len(dims) - 1)]


def integer_inputs(rng, n, width):
    return rng.integers(-2, 3, (n, width)).astype(np.float32)


def total_frags(in_dim, hidden, layers, out_dim=4, split0=False):
    """1-KiB fragments of the bf16 image (make_layout): decides LDS-resident (<= 56, hidden <= 64) or streamed."""
    kt0 = 1 if in_dim <= 32 else 4
    f = (hidden // 32) * kt0 * 2 * (2 if split0 else 1)
    f += (layers - 2) * (hidden // 32) * (hidden // 32) * 2
    return f + ((out_dim + 31) // 32) * (hidden // 32) * 2


def variant(kind, in_dim, hidden, layers, out_dim, num_mods=0):
    """The kernel instantiation a shape reaches, derived from launch_inr_kt0 / ws_eligible (never probed on a device)."""
    siren = _is_siren(kind)
    aug = kind == KIND_SIREN and in_dim <= 8
    frags = total_frags(in_dim, hidden, layers, out_dim, siren and not aug)
    res = hidden <= 64 and frags <= 56
    ws = aug and hidden == 256 and layers == 5 and out_dim <= 4 and num_mods == 4
    return dict(HID=hidden, KT0=1 if in_dim <= 32 else 4, act="aug-siren" if aug else "split-siren" if siren else "relu",
                resident=res, frags=frags, ws=ws)


def _exact_nets():
    """(in, hidden, layers, out): every (hidden, in), (hidden, layers) and (hidden, out) pair of
    {32,64,128,256} x {1,16,17,32,33,96,97,128} / {2,3,8} / {1,3,4,5,16}, and the two hidden-64 nets that sit on
    either side of the resident / streaming switch (56 and 60 fragments)."""
    ins, depths, outs = (1, 16, 17, 32, 33, 96, 97, 128), (2, 3, 8), (1, 3, 4, 5, 16)
    nets = []
    for hi, hid in enumerate((32, 64, 128, 256)):
        for ii, ind in enumerate(ins):
            # in = 32 at depth 8 for every width (hidden 64: the 56-fragment net); the offsets rotate the pairing per width
            depth = 8 if ind == 32 else depths[(ii + hi) % 3]
            nets.append((ind, hid, depth, outs[(ii + hi) % 5]))
    nets.append((33, 64, 7, 4))                                           # 60 fragments: streamed
    nets.append((1, 32, 8, 16))
    nets.append((128, 128, 8, 1))
    return nets


EXACT_NETS = _exact_nets()
# KIND_FOURIER_RELU with K = 0 (inputs built on the device from coords + feats): (numMods, hidden, layers, out)
FOURIER0_NETS = [(0, 32, 3, 4), (1, 128, 2, 3), (5, 32, 8, 16), (8, 128, 3, 5), (8, 32, 2, 1), (0, 128, 3, 2)]
# Net i uses seed EXACT_SEED + i (+ 500 for FOURIER0_NETS); the nets listed below use that + 100 instead, because their first
# draw misses a precondition of tests/test_inr_ref_host.py (no exact top-2 tie among the 573 points, or a value above 256).
EXACT_SEED = 1000
EXACT_RESEED = {(32, 32, 8, 5), (17, 256, 8, 1), (32, 256, 8, 3), (1, 32, 8, 16)}
FOURIER0_RESEED = {(5, 32, 8, 16)}


def exact_id(net):
    return "in%d_h%d_L%d_o%d" % net


def fourier0_id(net):
    return "m%d_h%d_L%d_o%d" % net


def exact_case(i):
    """Net i of EXACT_NETS: (layers, x)."""
    ind, hid, depth, out = EXACT_NETS[i]
    rng = np.random.default_rng(EXACT_SEED + i + (100 if EXACT_NETS[i] in EXACT_RESEED else 0))
    layers = integer_relu_net(rng, [ind] + [hid] * (depth - 1) + [out])
    return layers, integer_inputs(rng, N_POINTS, ind)


def fourier0_case(i):
    """Net i of FOURIER0_NETS: (layers, coords, feats or None).  Coordinates are multiples of 1/2, so every value of the
    network is a multiple of 1/2: exact in bf16 up to magnitude 128."""
    M, hid, depth, out = FOURIER0_NETS[i]
    rng = np.random.default_rng(EXACT_SEED + 500 + i + (100 if FOURIER0_NETS[i] in FOURIER0_RESEED else 0))
    layers = integer_relu_net(rng, [3 + M] + [hid] * (depth - 1) + [out])
    coords = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0], np.float32), (N_POINTS, 3))
    feats = integer_inputs(rng, N_POINTS, M) if M else None
    return layers, coords, feats


# ---- nets with a sine ----------------------------------------------------------------------------------------------------------

def siren_params(rng, dims):
    """The initialisation of test_classes_agree_with_fp64_after_refinement (tests/test_gpu_inr.py)."""
    return [{"W": (rng.uniform(-1, 1, (dims[i], dims[i + 1])) * np.sqrt(6.0 / dims[i]) / (30.0 if i == 0 else 1.0)).astype(np.float32),
             "b": rng.uniform(-0.05, 0.05, dims[i + 1]).astype(np.float32)} for i in range(len(dims) - 1)]


def fourier_params(rng, dims):
    return [{"W": (rng.uniform(-1, 1, (dims[i], dims[i + 1])) * np.sqrt(6 / (dims[i] + dims[i + 1]))).astype(np.float32),
             "b": rng.uniform(-0.1, 0.1, dims[i + 1]).astype(np.float32)} for i in range(len(dims) - 1)]


def _sine_nets():
    """dicts: kind, K, M, in, hidden, layers, out, w0.  Every listed value and every (kind, hidden), (kind, KT0) pair occurs."""
    nets = []
    depths, outs, w0s = (2, 3, 5), (1, 4, 16), (30.0, 1.0)
    i = 0
    for hid in (32, 64, 128, 256):                        # KIND_SIREN: in 3, 7, 8 k-folded ("aug"); 9, 11 split
        for M in (0, 4, 5, 6, 8):
            nets.append(dict(kind=KIND_SIREN, K=0, M=M, ind=3 + M, hidden=hid, layers=depths[i % 3], out=outs[(i // 3 + i) % 3],
                             w0=w0s[(i // 2) % 2]))
            i += 1
    for out in (1, 3):                                    # the weight-stationary shape, fewer than 4 classes
        nets.append(dict(kind=KIND_SIREN, K=0, M=4, ind=7, hidden=256, layers=5, out=out, w0=30.0))
    nets.append(dict(kind=KIND_SIREN, K=0, M=6, ind=9, hidden=64, layers=8, out=4, w0=30.0))
    raw = [(1, 32), (8, 64), (9, 128), (32, 256), (33, 32), (128, 64), (33, 128), (128, 256), (9, 32), (32, 64), (1, 128), (33, 256)]
    for j, (ind, hid) in enumerate(raw):                  # KIND_RAW_SIREN: split kernels at KT0 = 1 and 4
        nets.append(dict(kind=KIND_RAW_SIREN, K=0, M=0, ind=ind, hidden=hid, layers=depths[j % 3], out=outs[(j + 1) % 3],
                         w0=w0s[(j // 3) % 2]))
    j = 0
    for K, M in ((1, 0), (3, 4), (4, 5), (4, 6), (5, 0), (16, 8), (20, 5)):      # in 9, 25, 32 | 33, 33, 107, 128
        for hid in (32, 128, 256):
            nets.append(dict(kind=KIND_FOURIER_RELU, K=K, M=M, ind=3 + 6 * K + M, hidden=hid, layers=depths[j % 3],
                             out=(2, 4, 16)[(j // 3 + j) % 3], w0=0.0))
            j += 1
    return nets


SINE_NETS = _sine_nets()
SINE_SEED = 2000                    # net i uses seed SINE_SEED + i
KIND_NAMES = {KIND_FOURIER_RELU: "fourier", KIND_SIREN: "siren", KIND_RAW_SIREN: "rawsiren"}


def sine_id(net):
    tag = "k%dm%d" % (net["K"], net["M"]) if net["kind"] != KIND_RAW_SIREN else "in%d" % net["ind"]
    return "%s_%s_h%d_L%d_o%d_w%g" % (KIND_NAMES[net["kind"]], tag, net["hidden"], net["layers"], net["out"], net["w0"])


def sine_case(i):
    """Net i of SINE_NETS: (layers, coords or None, feats or None, x64) with x64 the fp64 input matrix of the references.
    Coordinates uniform in [-1, 1], intensities standard normal; a raw-input SIREN's matrix has the same make-up
    (three coordinate columns, then intensities)."""
    net = SINE_NETS[i]
    rng = np.random.default_rng(SINE_SEED + i)
    dims = [net["ind"]] + [net["hidden"]] * (net["layers"] - 1) + [net["out"]]
    layers = fourier_params(rng, dims) if net["kind"] == KIND_FOURIER_RELU else siren_params(rng, dims)
    coords = (rng.random((N_POINTS, 3)) * 2 - 1).astype(np.float32)
    if net["kind"] == KIND_RAW_SIREN:
        x = np.concatenate([coords, rng.standard_normal((N_POINTS, max(net["ind"] - 3, 0))).astype(np.float32)], 1)[:, :net["ind"]]
        x = np.ascontiguousarray(x)
        return layers, None, x, x.astype(np.float64)
    feats = rng.standard_normal((N_POINTS, net["M"])).astype(np.float32) if net["M"] else None
    return layers, coords, feats, build_input64(coords, feats, net["K"])


# ---- the packed image ------------------------------------------------------------------------------------------------------------
# Written from the layout comments of csrc/inr_mlp.hip / csrc/inr_fwd.h, not from the pack kernel: a 1-KiB fragment is one
# (out tile o, k tile t, k step s) of a layer as 64 lanes x 8 bf16; lane 32 h + r holds output column 32 o + r, and its element j
# input row  32 t + 16 s + 8 (j >> 2) + 4 h + (j & 3).  The layer's scale is folded into the fp32 weight before rounding;
# hi = bf16(v), lo = bf16(v - hi); rows and columns beyond the layer's true widths are zero.
#   main image:    layer 0 of a split SIREN [o][t][s][hi, lo], every other layer [o][t][s] (hi only)
#   refine image:  every layer [o][t][s][hi, lo]
#   both:          layer 0 of a KIND_SIREN net with <= 8 inputs ("augmented") is ONE k tile whose 32 rows are
#                  k step 0 = [W_hi ; W_hi ; 0] (16 rows), k step 1 = [W_lo ; 0] (16 rows): [o][s]
PACK_SLACK_FRAGS, REF_SLACK_FRAGS = 64, 32          # after the main image / after the refine image; then one calibration fragment


def _bf16_bits(a64):
    """uint16 patterns of values that are exactly representable in bf16."""
    f = np.asarray(a64, np.float64).astype(np.float32)
    assert np.array_equal(f.astype(np.float64), a64)
    return (f.view(np.uint32) >> 16).astype(np.uint16)


def _fragments(rows_bits, kt, ot):
    """(32 kt, 32 ot) uint16 -> (ot, kt, 2, 64, 8): fragment [o][t][s], lane, element."""
    j, h = np.arange(8), np.arange(2)
    k_in_step = 8 * (j[None, :] >> 2) + 4 * h[:, None] + (j[None, :] & 3)                   # [h][j]
    out = np.zeros((ot, kt, 2, 64, 8), np.uint16)
    for o in range(ot):
        for t in range(kt):
            for s in range(2):
                blk = rows_bits[32 * t + 16 * s + k_in_step][:, :, 32 * o:32 * o + 32]        # [h][j][r]
                out[o, t, s] = blk.transpose(0, 2, 1).reshape(64, 8)
    return out


def pack_image(layers, kind, w0=30.0, refine=False):
    """The main (refine=False) or the refine image of the network as (fragments, 64, 8) uint16."""
    wb = _wb(layers)
    siren = _is_siren(kind)
    in_dim, hidden = wb[0][0].shape
    aug = kind == KIND_SIREN and in_dim <= 8
    frags = []
    for i, (W, _) in enumerate(wb):
        head = i + 1 == len(wb)
        fold = siren and not head
        scale = np.float32(((float(w0) if i == 0 else 1.0) / TWO_PI_F32) if fold else 1.0)
        v = (W.astype(np.float32) * scale).astype(np.float64)                                 # the fp32 product that is rounded
        hi = bf16_round(v)
        lo = bf16_round(v - hi)
        kt = (1 if in_dim <= 32 else 4) if i == 0 else hidden // 32
        ot = (W.shape[1] + 31) // 32

        def padded(m):
            p = np.zeros((32 * kt, 32 * ot), np.uint16)
            p[:m.shape[0], :m.shape[1]] = _bf16_bits(m)
            return p
        if i == 0 and aug:
            z = np.zeros((16 - 2 * in_dim, W.shape[1]))
            folded = np.concatenate([hi, hi, z, lo, np.zeros((16 - in_dim, W.shape[1]))], 0)     # 32 rows
            frags.append(_fragments(padded(folded), 1, ot).reshape(-1, 64, 8))
        elif refine or (i == 0 and siren):
            both = np.stack([_fragments(padded(hi), kt, ot), _fragments(padded(lo), kt, ot)], 3)  # [o][t][s][hi, lo]
            frags.append(both.reshape(-1, 64, 8))
        else:
            frags.append(_fragments(padded(hi), kt, ot).reshape(-1, 64, 8))
    return np.concatenate(frags, 0)


# The smallest networks that reach every branch of the pack kernel: kind, K, M, in, hidden, layers, out, w0
PACK_NETS = [
    dict(kind=KIND_FOURIER_RELU, K=1, M=1, ind=10, hidden=32, layers=2, out=1, w0=0.0),      # one k tile, no split
    dict(kind=KIND_FOURIER_RELU, K=5, M=0, ind=33, hidden=32, layers=3, out=16, w0=0.0),     # kt0 = 4, zero padding to 128, padded head columns
    dict(kind=KIND_SIREN, K=0, M=4, ind=7, hidden=32, layers=3, out=4, w0=30.0),             # augmented split
    dict(kind=KIND_SIREN, K=0, M=5, ind=8, hidden=32, layers=3, out=4, w0=1.0),              # augmented split with k step 0 full
    dict(kind=KIND_SIREN, K=0, M=6, ind=9, hidden=64, layers=3, out=4, w0=30.0),             # hi/lo split of layer 0, scale on hidden layers
    dict(kind=KIND_RAW_RELU, K=0, M=0, ind=1, hidden=32, layers=2, out=2, w0=0.0),           # raw ReLU
    dict(kind=KIND_RAW_SIREN, K=0, M=0, ind=33, hidden=64, layers=3, out=3, w0=30.0),        # raw sine, split with kt0 = 4
]
PACK_SEED = 3000                    # net i uses seed PACK_SEED + i
# Exactly half-way between two bf16 numbers (round-to-nearest-even: down to 1, up to 1 + 2^-6, down in magnitude to -0.5, up
# to 2^-20 (1 + 2^-6)), and one whose lo part is itself a tie (1 + 2^-10 + 2^-18: hi = 1, lo -> 2^-10).  Planted in the layers
# whose folded scale is 1, where the fp32 product is the value itself.
PACK_TIES = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(0.5 + 2.0 ** -9), 2.0 ** -20 * (1.0 + 3 * 2.0 ** -8),
                      1.0 + 2.0 ** -10 + 2.0 ** -18], np.float32)


def pack_id(net):
    return "kind%d_in%d_h%d_L%d_o%d" % (net["kind"], net["ind"], net["hidden"], net["layers"], net["out"])


def pack_case(i):
    """Net i of PACK_NETS: layers [{"W", "b"}] of seeded normals with PACK_TIES planted in every layer of scale 1."""
    net = PACK_NETS[i]
    rng = np.random.default_rng(PACK_SEED + i)
    dims = [net["ind"]] + [net["hidden"]] * (net["layers"] - 1) + [net["out"]]
    layers = []
    for l in range(len(dims) - 1):
        W = rng.standard_normal((dims[l], dims[l + 1])).astype(np.float32)
        if not _is_siren(net["kind"]) or l + 2 == len(dims):
            flat = W.reshape(-1)
            n = min(len(PACK_TIES), flat.size)
            flat[rng.choice(flat.size, n, replace=False)] = PACK_TIES[:n]
        layers.append({"W": W, "b": np.zeros(dims[l + 1], np.float32)})
    return layers
