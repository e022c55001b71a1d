"""The NumPy references of the INR shape sweep (tests/inr_ref.py), checked without a GPU: bf16 rounding against torch's cast,
the bf16 error model against the stored reference logits, and the preconditions that make the sweep's nets mean what
tests/test_gpu_inr_shapes.py takes them to mean (exactness of the integer nets, the share of near-ties the toleranced nets
exclude), for exactly the nets and seeds that test uses."""
import itertools

import numpy as np
import pytest

import inr_ref as ir

LOGIT_REL_TOL = 1e-2        # tests/test_gpu_inr.py
REFINED_REL_TOL = 1e-4


def test_bf16_round_equals_torch_cast():
    import torch
    rng = np.random.default_rng(3)
    vals = [rng.standard_normal(20000).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 20000).astype(np.float32),
            rng.standard_normal(4000).astype(np.float32) * np.float32(1e-39)]                       # bf16 denormals
    m = rng.integers(128, 256, 4000).astype(np.float64)                                            # exact ties: half an ulp
    e = rng.integers(-140, 120, 4000)
    vals.append(np.ldexp((m + 0.5) / 128.0, e).astype(np.float32) * rng.choice([-1.0, 1.0], 4000).astype(np.float32))
    vals.append(np.array([0.0, -0.0, np.inf, -np.inf, 3.3895314e38, 3.4028235e38, -3.4028235e38, 1e-45, 9.1835e-41, 4.6e-41,
                          1.0, 1.00390625, 1.01171875, 256.0, 257.0, 255.5], np.float32))
    a = np.concatenate(vals)
    want = torch.from_numpy(a).to(torch.bfloat16).to(torch.float64).numpy()
    got = ir.bf16_round(a.astype(np.float64))
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    assert int((got != a).sum()) > 20000 and np.isinf(got).sum() >= 4
    assert np.isnan(ir.bf16_round(np.array([np.nan]))).all()


@pytest.mark.parametrize("tag,nl", [("k4h64", 5), ("k16h256", 5), ("k2h32x2", 3)])
def test_emulation_is_within_the_bf16_bar_on_the_fourier_goldens(golden_dir, tag, nl):
    g = np.load(golden_dir / "inr_fourier.npz")
    layers = [{"W": g[f"{tag}_W{i}"], "b": g[f"{tag}_b{i}"]} for i in range(nl)]
    want = g[f"{tag}_logits"].astype(np.float64)
    x = ir.build_input64(g[f"{tag}_coords"], g[f"{tag}_feats"], int(g[f"{tag}_K"]))
    assert np.abs(x - g[f"{tag}_x"]).max() < 1e-6                          # the reference's own feature order
    scale = np.abs(want).max()
    emu = ir.emulate_bf16(layers, x, ir.KIND_FOURIER_RELU)
    assert 0 < np.abs(emu - want).max() <= LOGIT_REL_TOL * scale
    assert np.abs(ir.forward64(layers, x, ir.KIND_FOURIER_RELU) - want).max() <= 1e-5 * scale     # fp32 reference vs fp64


@pytest.mark.parametrize("tag,depth", [("s3x256", 3), ("s4x256", 4), ("s3x256b", 3), ("s4x256b", 4), ("s4x256w", 4)])
def test_emulation_is_within_the_bf16_bar_on_the_siren_fixtures(golden_dir, tag, depth):
    s = np.load(golden_dir / "siren.npz")
    layers = [{"W": s[f"{tag}_l{i}_w"], "b": s[f"{tag}_l{i}_b"]} for i in range(depth + 1)]
    want, w0 = s[f"{tag}_logits"].astype(np.float64), float(s[f"{tag}_w0"])
    scale = max(1.0, np.abs(want).max())
    emu = ir.emulate_bf16(layers, s[f"{tag}_x"], ir.KIND_RAW_SIREN, w0)
    assert 0 < np.abs(emu - want).max() <= LOGIT_REL_TOL * scale
    assert np.abs(ir.forward64(layers, s[f"{tag}_x"], ir.KIND_RAW_SIREN, w0) - want).max() <= REFINED_REL_TOL * scale


def test_integer_net_generator():
    rng = np.random.default_rng(0)
    for dims in ([1, 32, 1], [128, 32, 32, 16], [17, 256, 3], [2, 64, 64, 5]):
        layers = ir.integer_relu_net(rng, dims)
        for p, rows, cols in zip(layers, dims[:-1], dims[1:]):
            W, b = p["W"], p["b"]
            assert W.shape == (rows, cols) and W.dtype == np.float32 and set(np.unique(W)) <= {-1.0, 0.0, 1.0}
            k = max(min(3, rows), -(-rows // cols))
            assert ((W != 0).sum(0) == k).all() and ((W != 0).sum(1) >= 1).all()
            assert set(np.unique(b)) <= {-1.0, 0.0, 1.0}
    x = ir.integer_inputs(rng, 1000, 5)
    assert set(np.unique(x)) == {-2.0, -1.0, 0.0, 1.0, 2.0}


def _check_exact(layers, x, out_dim, unit):
    """Every value a multiple of ``unit`` and exact in bf16 (|v| <= 256 unit); every row of every matrix used; >= 10 % of every
    hidden layer live; >= 1 % of the points tied between their two largest logits."""
    logits, hidden = ir.forward64(layers, x, ir.KIND_RAW_RELU, return_hidden=True)
    for p in layers:
        assert ((p["W"] != 0).sum(1) >= 1).all()
    peak = 0.0
    for h in hidden + [logits]:
        assert np.array_equal(h, np.rint(h / unit) * unit)
        peak = max(peak, np.abs(h).max())
    assert peak <= 256 * unit, peak
    for h in hidden:
        assert np.array_equal(ir.bf16_round(h), h)
        assert (h != 0).mean() >= 0.10, (h != 0).mean()
    assert np.array_equal(logits.astype(np.float32).astype(np.float64), logits)
    emu = ir.emulate_bf16(layers, x, ir.KIND_RAW_RELU)
    assert np.array_equal(emu, logits)                                     # the bf16 pass loses nothing on these nets
    if out_dim > 1:
        tied = (ir.top2_gap(logits) == 0).mean()
        assert tied >= 0.01, tied
        assert len(np.unique(logits.argmax(1))) > 1
    return peak


@pytest.mark.parametrize("i", range(len(ir.EXACT_NETS)), ids=[ir.exact_id(n) for n in ir.EXACT_NETS])
def test_integer_nets_meet_their_preconditions(i):
    layers, x = ir.exact_case(i)
    assert x.shape == (ir.N_POINTS, ir.EXACT_NETS[i][0]) and np.abs(x).max() == 2
    _check_exact(layers, x, ir.EXACT_NETS[i][3], 1.0)


@pytest.mark.parametrize("i", range(len(ir.FOURIER0_NETS)), ids=[ir.fourier0_id(n) for n in ir.FOURIER0_NETS])
def test_fourier0_nets_meet_their_preconditions(i):
    """Coordinates are multiples of 1/2 here, so the values are half-integers: exact in bf16 up to 128 (256 halves)."""
    layers, coords, feats = ir.fourier0_case(i)
    assert set(np.unique(coords)) == {-1.0, -0.5, 0.0, 0.5, 1.0} and (feats is None) == (ir.FOURIER0_NETS[i][0] == 0)
    _check_exact(layers, ir.build_input64(coords, feats, 0), ir.FOURIER0_NETS[i][3], 0.5)


def test_exact_nets_cover_the_grid():
    nets = ir.EXACT_NETS
    assert len(nets) >= 32 and len(set(nets)) == len(nets)
    hids = (32, 64, 128, 256)
    assert {(n[1], n[0]) for n in nets} >= set(itertools.product(hids, (1, 16, 17, 32, 33, 96, 97, 128)))
    assert {(n[1], n[2]) for n in nets} >= set(itertools.product(hids, (2, 3, 8)))
    assert {(n[1], n[3]) for n in nets} >= set(itertools.product(hids, (1, 3, 4, 5, 16)))
    frags = {n: ir.total_frags(n[0], n[1], n[2], n[3]) for n in nets}
    at56 = [n for n in nets if n[1] == 64 and n[2] == 8 and n[0] <= 32 and frags[n] == 56]
    at60 = [n for n in nets if n[1] == 64 and n[2] == 7 and n[0] >= 33 and frags[n] == 60]
    assert at56 and at60
    v56, v60 = ir.variant(ir.KIND_RAW_RELU, *at56[0]), ir.variant(ir.KIND_RAW_RELU, *at60[0])
    assert v56["resident"] and v56["KT0"] == 1 and not v60["resident"] and v60["KT0"] == 4
    f0 = ir.FOURIER0_NETS
    assert {n[0] for n in f0} == {0, 1, 5, 8} and {n[1] for n in f0} == {32, 128}
    # every instantiation of the ReLU forward kernel that a valid net can reach: streamed at HID >= 128 and at (64, KT0 4),
    # LDS-resident at HID <= 64.  (No net of <= 8 layers exceeds 56 fragments at HID 32, or at HID 64 with <= 32 inputs, so the
    # streamed instantiations for those are never launched.)
    seen = {(v["HID"], v["KT0"], v["resident"]) for v in (ir.variant(ir.KIND_RAW_RELU, *n) for n in nets)}
    assert seen == ({(h, k, False) for h in (128, 256) for k in (1, 4)} | {(64, 4, False)}
                    | {(h, k, True) for h in (32, 64) for k in (1, 4)})
    assert ir.total_frags(128, 32, 8, 16, split0=True) <= 56 and ir.total_frags(32, 64, 8, 16) == 56


def test_sine_nets_cover_the_grid():
    nets = ir.SINE_NETS
    assert 50 <= len(nets) <= 70 and len({ir.sine_id(n) for n in nets}) == len(nets)
    by = {k: [n for n in nets if n["kind"] == k] for k in (ir.KIND_SIREN, ir.KIND_RAW_SIREN, ir.KIND_FOURIER_RELU)}
    hids = {32, 64, 128, 256}
    s = by[ir.KIND_SIREN]
    assert {n["M"] for n in s} == {0, 4, 5, 6, 8} and {n["ind"] for n in s} == {3, 7, 8, 9, 11}
    assert {n["hidden"] for n in s} == hids and {n["layers"] for n in s} == {2, 3, 5, 8}
    assert {n["out"] for n in s} >= {1, 4, 16} and {n["w0"] for n in s} == {30.0, 1.0}
    assert {(n["hidden"], n["M"]) for n in s} >= set(itertools.product(hids, (0, 4, 5, 6, 8)))
    ws = [n for n in s if ir.variant(n["kind"], n["ind"], n["hidden"], n["layers"], n["out"], n["M"])["ws"]]
    assert {n["out"] for n in ws} >= {1, 3}
    r = by[ir.KIND_RAW_SIREN]
    assert {n["ind"] for n in r} == {1, 8, 9, 32, 33, 128}
    assert {(n["hidden"], 1 if n["ind"] <= 32 else 4) for n in r} == set(itertools.product(hids, (1, 4)))
    f = by[ir.KIND_FOURIER_RELU]
    assert {(n["K"], n["M"]) for n in f} == {(1, 0), (3, 4), (4, 5), (4, 6), (5, 0), (16, 8), (20, 5)}
    assert {n["ind"] for n in f} == {9, 25, 32, 33, 107, 128}
    assert {n["hidden"] for n in f} == {32, 128, 256} and {n["out"] for n in f} == {2, 4, 16}
    assert {(n["hidden"], 1 if n["ind"] <= 32 else 4) for n in f} == set(itertools.product((32, 128, 256), (1, 4)))
    acts = {ir.variant(n["kind"], n["ind"], n["hidden"], n["layers"], n["out"], n["M"])["act"] for n in s}
    assert acts == {"aug-siren", "split-siren"}


@pytest.mark.parametrize("i", range(len(ir.SINE_NETS)), ids=[ir.sine_id(n) for n in ir.SINE_NETS])
def test_sine_nets_exclude_at_most_one_per_cent(i):
    """The class comparison of the split pass leaves out the points whose fp64 top-2 gap is below 2 x REFINED_REL_TOL x range:
    that must be <= 1 % of a net's points, and the emulated bf16 error must be a real, finite yardstick."""
    net = ir.SINE_NETS[i]
    layers, coords, feats, x = ir.sine_case(i)
    assert x.shape == (ir.N_POINTS, net["ind"])
    ref = ir.forward64(layers, x, net["kind"], net["w0"])
    rng_ = np.abs(ref).max()
    assert np.isfinite(ref).all() and rng_ > 0
    excluded = (ir.top2_gap(ref) < 2 * REFINED_REL_TOL * rng_).mean()
    assert excluded <= 0.01, excluded
    err = np.abs(ir.emulate_bf16(layers, x, net["kind"], net["w0"]) - ref).max()
    assert 0 < err < np.inf


@pytest.mark.parametrize("i", range(len(ir.PACK_NETS)), ids=[ir.pack_id(n) for n in ir.PACK_NETS])
def test_numpy_packer_decodes_to_the_scaled_weights(i):
    """pack_image, read back element by element with the index formula of the layout comment: hi + lo of the refine image is
    the scaled fp32 weight to 2^-16, padding is zero, the main image is the refine image's hi parts (layer 0 of a split SIREN:
    both parts), and the fragment count is make_layout's."""
    net, layers = ir.PACK_NETS[i], ir.pack_case(i)
    siren = net["kind"] in (ir.KIND_SIREN, ir.KIND_RAW_SIREN)
    aug = net["kind"] == ir.KIND_SIREN and net["ind"] <= 8
    main, ref = ir.pack_image(layers, net["kind"], net["w0"]), ir.pack_image(layers, net["kind"], net["w0"], refine=True)
    assert len(main) == ir.total_frags(net["ind"], net["hidden"], net["layers"], net["out"], siren and not aug)
    val = lambda bits: (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    fm = fr = 0
    for l, p in enumerate(layers):
        head = l + 1 == len(layers)
        scale = np.float32(((net["w0"] if l == 0 else 1.0) / ir.TWO_PI_F32) if siren and not head else 1.0)
        v = (p["W"] * scale).astype(np.float64)
        kt, ot = ((1 if net["ind"] <= 32 else 4) if l == 0 else net["hidden"] // 32), (p["W"].shape[1] + 31) // 32
        n = ot * kt * 2
        if l == 0 and aug:
            assert np.array_equal(main[fm:fm + n], ref[fr:fr + n])
            fm, fr = fm + n, fr + n
            continue
        pair = ref[fr:fr + 2 * n].reshape(ot, kt, 2, 2, 64, 8)
        split_main = l == 0 and siren
        assert np.array_equal(main[fm:fm + (2 * n if split_main else n)].reshape(-1),
                              (pair if split_main else pair[:, :, :, 0]).reshape(-1))
        for o, t, s, lane, j in itertools.product(range(ot), range(kt), range(2), range(0, 64, 7), range(8)):
            k, c = 32 * t + 16 * s + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3), 32 * o + (lane & 31)
            want = v[k, c] if k < v.shape[0] and c < v.shape[1] else 0.0
            got = val(pair[o, t, s, 0, lane, j]) + val(pair[o, t, s, 1, lane, j])
            assert abs(got - want) <= 2.0 ** -16 * abs(want), (l, o, t, s, lane, j)
        fm, fr = fm + (2 * n if split_main else n), fr + 2 * n
    assert fm == len(main) and fr == len(ref)
