"""The coordinate-injection INR without a GPU: the NumPy restatement (tests/inject_ref.py) against the logits the reference
notebook's own functions produced (tests/golden/inject.npz), the preconditions of every exact GPU case, the mask rule, and the
boundary map against SciPy's recorded one (tests/golden/boundary.npz)."""
import numpy as np
import pytest

import inject_cases as ic
import inject_ref as ref
import inr_loop_ref as lref

G = ic.load_golden()


def _golden_params():
    mlp = []
    while f"mlp_W_{len(mlp)}" in G:
        mlp.append({"W": G[f"mlp_W_{len(mlp)}"], "b": G[f"mlp_b_{len(mlp)}"]})
    return {"fourier": {"B": G["fourier_B"]}, "mlp": mlp}


def test_fp64_tier_reproduces_the_notebook_logits():
    p, hwd = _golden_params(), tuple(int(v) for v in G["hwd"])
    z64 = ref.forward64(p, ref.grid_coords(hwd), ref.volume_mods(G["mods"]), list(G["coord_layers"]), list(G["mod_layers"]))
    err = np.abs(z64 - G["logits64"]).max() / np.abs(G["logits64"]).max()
    print("relative deviation of the fp64 tier from the notebook's fp64 logits:", err)
    assert G["logits64"].dtype == np.float64 and G["logits64"].shape == (hwd[0] * hwd[1] * hwd[2], 4)
    assert err <= 1e-12


def test_notebook_fp32_logits_and_fp32_tier_are_within_the_tolerance():
    p, hwd = _golden_params(), tuple(int(v) for v in G["hwd"])
    coords, mods = ref.grid_coords(hwd), ref.volume_mods(G["mods"])
    z32 = ref.forward32(p, coords, mods, list(G["coord_layers"]), list(G["mod_layers"]))
    z64 = ref.forward64(p, coords, mods, list(G["coord_layers"]), list(G["mod_layers"]))
    tau = ic.tau(z32, z64)
    dev = np.abs(G["logits32"].astype(np.float64) - z64).max()
    print("tau", tau, "notebook fp32 deviation", dev)
    assert G["logits32"].dtype == np.float32 and dev <= tau


def test_fixture_leaves_no_voxel_out_of_the_pred_comparison():
    """Equal to the notebook's pred wherever the fp64 top-two gap exceeds 2 tau: the committed fixture has no other voxel."""
    p, hwd = _golden_params(), tuple(int(v) for v in G["hwd"])
    coords, mods = ref.grid_coords(hwd), ref.volume_mods(G["mods"])
    z32 = ref.forward32(p, coords, mods, list(G["coord_layers"]), list(G["mod_layers"]))
    z64 = G["logits64"]
    tau = ic.tau(z32, ref.forward64(p, coords, mods, list(G["coord_layers"]), list(G["mod_layers"])))
    top = np.sort(z64, 1)
    gap = top[:, -1] - top[:, -2]
    print("smallest gap", gap.min(), "2 tau", 2 * tau)
    assert int((gap <= 2 * tau).sum()) == 0
    assert G["pred"].dtype == np.int16 and G["pred"].shape == hwd
    assert np.array_equal(G["pred"].reshape(-1), ref.argmax(z64)) and np.array_equal(G["pred"].reshape(-1), ref.argmax(z32))
    assert len(np.unique(G["pred"])) >= 3                      # not a constant volume


@pytest.mark.parametrize("case", ic.EXACT, ids=[c[0] for c in ic.EXACT])
def test_exact_cases_have_one_product_per_output(case):
    params, rows, coords, mods = ic.exact_case(case)
    name, n, F, M, widths, cl, ml, _ = case
    shapes = ref.net_shape(F, M, widths, cl, ml)
    for p, (n_in, _, _, out) in zip(params["mlp"], shapes):
        W = p["W"]
        assert W.shape == (n_in, out) and np.all((W != 0).sum(0) == 1)
        nz = np.abs(W[W != 0])
        assert np.all(np.log2(nz) == np.round(np.log2(nz))) and nz.min() >= 0.25 and nz.max() <= 4
    assert coords.shape == (n, 3) and mods.shape == (n, M)
    z = ref.forward32(params, coords, mods, cl, ml)
    assert z.shape == (n, widths[-1])
    if n >= 63:
        assert np.isnan(z).any() and np.isfinite(z).any()      # the special rows are poisoned, the others are not


def test_exact_cases_cover_what_they_should():
    ns, Fs, Ms, Ls, Cs, ws = set(), set(), set(), set(), set(), set()
    reached = {"h": False, "coords": False, "mods": False}
    splits, kinds = set(), set()
    for case in ic.EXACT:
        name, n, F, M, widths, cl, ml, _ = case
        _, rows, _, _ = ic.exact_case(case)
        ns.add(n); Fs.add(F); Ms.add(M); Ls.add(len(widths)); Cs.add(widths[-1]); ws.update(widths)
        L = len(widths)
        for l, ((n_in, split, split_m, out), r) in enumerate(zip(ref.net_shape(F, M, widths, cl, ml), rows)):
            r = np.asarray(r)
            reached["h"] |= bool((r < split).any())
            reached["coords"] |= bool(((r >= split) & (r < split_m)).any())
            reached["mods"] |= bool((r >= split_m).any())
            if 0 < l < L - 1:
                kind = ("coords" if split_m > split else "") + ("mods" if n_in > split_m else "") or "none"
                where = "first" if l == 1 else "last" if l == L - 2 else "mid"
                kinds.add((kind, where))
                if L == 3:
                    kinds.add((kind, "last"))
                splits.add(split % 16)
    assert ns == {1, 63, 64, 65, 257} and Fs == {2, 14, 16, 18, 128, 256} and Ms == {0, 1, 4, 8}
    assert Ls >= {2, 3, 5, 8} and Cs >= {1, 4, 16} and ws >= {1, 13, 16, 17, 64, 65, 256}
    assert all(reached.values())
    assert splits >= {0, 13, 1}                                  # the split on, before and after a k-tile edge
    for kind in ("none", "coords", "mods", "coordsmods"):
        assert (kind, "first") in kinds and (kind, "last") in kinds, kind


def test_selection_nets_reach_every_input_between_them():
    for F, M, widths, cl, ml in ((16, 4, (17, 64, 4), (1,), (1,)), (14, 1, (16, 17, 1), (1,), ())):
        shapes = ref.net_shape(F, M, widths, cl, ml)
        seen = [set() for _ in shapes]
        for shift in range(max(s[0] for s in shapes)):
            _, rows = ref.selection_net(np.random.default_rng(shift), F, M, widths, cl, ml, shift)
            for s, r in zip(seen, rows):
                s.update(r)
        assert all(s == set(range(shape[0])) for s, shape in zip(seen, shapes))


@pytest.mark.parametrize("case", ic.INTEGER, ids=[c[0] for c in ic.INTEGER])
def test_integer_cases_stay_below_2_to_24(case):
    params, coords8, mods = ic.integer_case(case)
    z8, bound = ref.forward_int(params, coords8, mods, case[5], case[6])
    print(case[0], "largest |partial sum| bound, in eighths:", bound)
    assert bound < 2 ** 24 and np.abs(z8).max() > 8            # exact in fp32, and not trivially zero
    z32 = ref.forward32(params, (coords8 / 8.0).astype(np.float32), mods.astype(np.float32), case[5], case[6])
    assert np.array_equal((z32.astype(np.float64) * 8).astype(np.int64), z8)
    assert max((p["W"] != 0).sum(0).max() for p in params["mlp"]) > 1       # multi-term sums


def test_mask_threshold_and_kept_share():
    assert ref.threshold(1.0) == 2 ** 32 and ref.threshold(0.5) == 2 ** 31 and ref.threshold(2.0 ** -24) == 256
    assert ref.threshold(0.7) == int(np.floor(float(np.float32(0.7)) * 2.0 ** 32)) == 3006477056
    n, width = 1 << 10, 1 << 8                                   # 2^18 words
    for keep in (0.5, 0.7, 0.25, 2.0 ** -24):
        kept = ref.keep_mask(12345, np.arange(n), 3, 1, width, keep)
        p = ref.threshold(keep) / 2.0 ** 32
        sd = np.sqrt(n * width * p * (1 - p))
        print(keep, kept.sum(), n * width * p, sd)
        assert abs(int(kept.sum()) - n * width * p) <= 4 * sd
    assert ref.keep_mask(1, np.arange(5), 0, 0, 7, 1.0).all()
    # the counter: (i lo, i hi, 256 s + l, j >> 2), word j & 3, key (seed lo, seed hi)
    seed, i, s, l, j = (7 << 32) | 9, (1 << 33) + 5, 2, 3, 6
    r = lref.philox4x32_10((i & 0xFFFFFFFF, i >> 32, 256 * s + l, j >> 2), (9, 7))
    assert bool(ref.keep_mask(seed, [i], s, l, 8, 0.5)[0, j]) == bool(int(r[j & 3]) < 2 ** 31)
    a, b = ref.keep_mask(1, np.arange(64), 0, 0, 64, 0.5), ref.keep_mask(1, np.arange(64), 1, 0, 64, 0.5)
    assert (a != b).any() and (a != ref.keep_mask(2, np.arange(64), 0, 0, 64, 0.5)).any()


def test_dropout_scale_is_exact_for_the_exact_tier():
    for keep in (0.5, 0.25):
        assert np.float32(1.0) / np.float32(keep) == 1.0 / keep and float(np.log2(1.0 / keep)).is_integer()


@pytest.mark.parametrize("vol", ic.load_boundary(), ids=[v[0] for v in ic.load_boundary()])
def test_boundary_restatement_equals_scipy(vol):
    name, seg, want = vol
    assert want.dtype == np.float32 and ref.same_bits(ref.boundary_weights(seg, 4), want)


def test_boundary_fixture_covers_what_it_should():
    by = {v[0]: v for v in ic.load_boundary()}
    assert not (by["class_absent"][1] == 2).any() and (by["class_absent"][1] == 1).any()
    assert int((by["one_voxel_class"][1] == 3).sum()) == 1 and by["one_voxel_class"][2].max() == 1.0
    assert not by["no_tumour"][2].any()
    assert max(by["anisotropic"][1].shape) >= 7 * min(by["anisotropic"][1].shape)
