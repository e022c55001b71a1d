"""The restatements behind the extended-loss and tumour-sampler tests, on the CPU: inr_lossx_ref.loss_terms against the values
scripts/jax_inr_brats.py's own ``loss_fn`` returned (tests/golden/inr_lossx.npz, written by make_inr_lossx_goldens.py), the
neutral configuration against inr_train_ref.loss_terms, autograd's dlogits against central differences, one recorded
tolerance re-derived, and the sampler restatement against inr_loop_ref / np.flatnonzero."""
import numpy as np
import pytest
import torch

import inr_loop_ref as lp
import inr_lossx_cases as cases
import inr_lossx_ref as lx
import inr_train_cases as tc
import inr_train_ref as tr


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(golden_dir / "inr_lossx.npz") as z:
        return {k: z[k] for k in z.files}


def _golden_opt(g, name):
    kw = {k[len(name) + 5:]: g[k] for k in g if k.startswith(name + "_opt_")}
    opt = dict(per_class_dice=False, round32=False)          # loss_fn's own defaults
    for k, v in kw.items():
        opt[k] = v if k == "focal_alpha" else (bool(v) if k == "per_class_dice" else float(v))
    return lx.options(**opt)


def test_goldens_cover_every_option(golden):
    names = [str(n) for n in golden["names"]]
    assert len(names) >= 6
    seen = set()
    for n in names:
        seen |= {k[len(n) + 5:] for k in golden if k.startswith(n + "_opt_")}
    assert {"focal_gamma", "focal_alpha", "label_smoothing", "per_class_dice", "edema_fp_weight", "tversky_weight", "edema_logit_reg"} <= seen
    assert not (golden["all_no_edema_labels"] == 2).any() and (golden["all_edema_only_labels"] == 2).all()


def test_restatement_matches_the_reference_loss(golden):
    for name in (str(n) for n in golden["names"]):
        opt = _golden_opt(golden, name)
        z = torch.as_tensor(golden[name + "_logits"], dtype=torch.float64)
        loss = float(lx.loss_terms(z, golden[name + "_labels"], golden[name + "_cw"], opt)[0])
        want = float(golden[name + "_loss"])
        print(name, loss, want)
        assert abs(loss - want) <= 1e-12 * abs(want), (name, loss, want)


@pytest.mark.parametrize("i", [1, 5, 7])
def test_neutral_configuration_is_the_plain_loss(i):
    c = tc.loss_case(i)
    got = lx.loss_alone(c["logits"], c["labels"], c["cw"], lx.options(dice_weight=c["dw"]))
    assert got["loss"] == c["ref"]["loss"]
    assert np.array_equal(got["aux"], c["ref"]["aux"]) and np.array_equal(got["dlogits"], c["ref"]["dlogits"])
    assert got["terms"][1] == (0.0 if c["dw"] <= 0 else got["terms"][1]) and np.isfinite(got["terms"]).all()


@pytest.mark.parametrize("name", ["all_n257_c4", "all_outside_n257_c4", "focal_g1_alpha_n257_c4"])
def test_autograd_dlogits_against_central_differences(name):
    c = cases.loss_case(name)
    z0 = c["logits"].astype(np.float64).reshape(-1)
    f = lambda v: float(lx.loss_terms(torch.as_tensor(v.reshape(c["logits"].shape)), c["labels"], c["cw"], c["opt"])[0])      # noqa: E731
    idx = np.random.default_rng(3).choice(z0.size, 24, replace=False)
    cd = tr.central_differences(f, z0, idx, 1e-5)
    want = c["ref"]["dlogits"].reshape(-1)[idx]
    assert np.abs(cd - want).max() <= 1e-8 * max(np.abs(c["ref"]["dlogits"]).max(), 1e-30) + 1e-10


def test_terms_show_each_option():
    c = cases.loss_case("all_n257_c4")
    t = c["ref"]["terms"]
    assert (t > 0).all() and 0 < t[3] < 1
    o = c["opt"]
    total = (1 - o["dice_weight"]) * t[0] + o["dice_weight"] * t[1] + np.float32(o["edema_fp_weight"]) * t[2] + \
        np.float32(o["tversky_weight"]) * (1 - t[3]) + np.float32(o["edema_logit_reg"]) * t[4]
    assert abs(total - c["ref"]["loss"]) <= 1e-12
    for name, zero in (("all_no_edema_n255_c4", 3), ("all_edema_only_n255_c4", 2)):      # TP = FN = 0: index 0; FP = 0
        assert cases.loss_case(name)["ref"]["terms"][zero] == 0.0
    assert cases.loss_case("all_edema_only_n255_c4")["ref"]["terms"][4] == 0.0


def test_every_case_has_a_tolerance_below_the_cap():
    assert set(cases.LOSS_TOL) == set(cases.LOSS)
    for name, t in cases.LOSS_TOL.items():
        for k in ("loss", "aux", "terms", "dlogits"):
            assert 0 < cases.tol(t[k]) <= tc.CAP, (name, k)
            assert t[k] == 0 or t[k] >= tc.ZERO_MIN, (name, k)          # nothing an fp32 result could not be held to
    for t in cases.STEP_TOL.values():
        assert all(0 < cases.tol(v) <= tc.CAP for v in t.values())
    ns, cs = {c[0] for c in cases.LOSS.values()}, {c[1] for c in cases.LOSS.values()}
    assert {1, 255, 257, cases.BIG} <= ns and cs == {1, 3, 4, 16} and cases.BIG > tc.LOSS_FIRST_STRIDED
    assert {float(c[4].get("focal_gamma", 0)) for c in cases.LOSS.values()} >= {1.0, 2.0, 5.0}


def test_a_recorded_tolerance_is_reproduced():
    name = "all_n257_c4"
    d = cases.loss_fp32_deviation(name)
    for k, v in d.items():
        assert float("%.3g" % (8 * v)) == cases.LOSS_TOL[name][k], (k, 8 * v, cases.LOSS_TOL[name][k])


# ---- sampler --------------------------------------------------------------------------------------------------------------------
def test_tumour_index_restatement():
    cs = cases.mix_cases(1)
    index, offsets = lx.tumour_index(cs)
    hwd = int(np.prod(cases.MIX_SHAPES[1]))
    assert offsets.tolist()[:4] == [0, 0, hwd, hwd + 1] and index[hwd] == hwd - 1
    assert np.array_equal(index[:hwd], np.arange(hwd))
    last = index[offsets[3]:offsets[4]]
    assert (np.diff(last.astype(np.int64)) > 0).all() and last[0] != 0          # voxel 0 of the last case is negative: no tumour


@pytest.mark.parametrize("n", cases.MIX_NS)
def test_mixed_sampler_restatement(n):
    cs = cases.mix_cases(0)
    plain = lp.sample(cs, cases.MIX_SEED, 3, n)
    for nt in cases.mix_n_tumours(n):
        coords, feats, labels, used = lx.sample_mix(cs, cases.MIX_SEED, 3, n, nt)
        assert not used[nt:].any()
        keep = ~used
        assert np.array_equal(coords[keep], plain[0][keep]) and np.array_equal(feats[keep], plain[1][keep]) and np.array_equal(labels[keep], plain[2][keep])
        assert (labels[used] > 0).all()
        if nt == 0:
            assert not used.any()
    if n >= 255:
        _, _, _, used = lx.sample_mix(cs, cases.MIX_SEED, 3, n, n)
        assert used.any() and not used.all()              # the empty case makes the fallback fire


def test_n_tumour_is_the_reference_rounding():
    assert [lx.n_tumour_of(n, r) for n, r in ((512, 0.4), (10, 0.29), (7, 1.5), (7, -1.0), (4096, 0.4))] == [204, 2, 7, 0, 1638]
