"""The restatement of the unified loss (tests/unified_loss_ref.py) against the reference notebook's own numbers and against
central differences, and the case lists of tests/unified_loss_cases.py against the conditions they promise.  No GPU."""
import numpy as np
import pytest
import torch

import unified_loss_cases as uc
import unified_loss_ref as ref


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(uc.GOLDEN))


def test_golden_file_holds_the_cases_and_only_numbers(golden):
    assert [str(v) for v in golden["names"]] == [c[0] for c in uc.GOLDEN_CASES] and 8 <= len(uc.GOLDEN_CASES) <= 12
    for case in uc.GOLDEN_CASES:
        z, labels, bw, cfg = uc.golden_case(case)
        name = case[0]
        assert ref.same_bits(golden[name + "_logits"], z) and ref.same_bits(golden[name + "_labels"], labels), name
        assert (name + "_bw" in golden) == (bw is not None) and (bw is None or ref.same_bits(golden[name + "_bw"], bw)), name
        assert np.array_equal(golden[name + "_cfg"], [cfg["gamma"], cfg["lam"], cfg["tv_w"], cfg["bd_w"], *cfg["cw"]]), name
    for k, v in golden.items():
        assert v.dtype.kind in "fiU" and (v.dtype.kind != "U" or k == "names"), k
    # what the issue asks the configurations to cover
    Cs = {c[2] for c in uc.GOLDEN_CASES}
    feats = set().union(*[set(c[10]) for c in uc.GOLDEN_CASES])
    assert {1, 3, 4} <= Cs and {"absent", "outside", "big", "saturated"} <= feats and {0.02, 0.05} <= {c[8] for c in uc.GOLDEN_CASES}


@pytest.mark.parametrize("case", uc.GOLDEN_CASES, ids=[c[0] for c in uc.GOLDEN_CASES])
def test_restatement_in_fp64_reproduces_the_notebook(golden, case):
    name = case[0]
    z, labels, bw, cfg = uc.golden_case(case)
    loss, aux, _, _ = ref.forward(z, labels, bw, cfg, want_grad=False)
    want = np.concatenate([[golden[name + "_loss"]], golden[name + "_aux"]])
    got = np.concatenate([[loss], ref.aux_vector(aux)])
    assert got.shape == want.shape == (9 + case[2],)
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (got - want)


def test_golden_cases_reach_what_they_name():
    for case in uc.GOLDEN_CASES:
        name, n, C, *_ , features = case
        z, labels, bw, cfg = uc.golden_case(case)
        zc = np.clip(z.astype(np.float64), -10, 10)
        e = np.exp(zc - zc.max(1, keepdims=True))
        ps = e / e.sum(1, keepdims=True)
        if "absent" in features:
            assert not (labels == 2).any() and (labels == 1).any()
        if "outside" in features:
            assert (labels >= C).any() and (labels < 0).any()
        if "big" in features:
            assert (z > 10).any() and (z < -10).any() and (np.abs(z) > 10).all(1).any()
        if "saturated" in features:
            assert ((ps > 1 - 1e-7).any(1) & (np.abs(z) < 10).all(1)).any() and (ps < 1e-7).any()
        if "no_bw" in features:
            assert bw is None


@pytest.mark.parametrize("case", uc.GOLDEN_CASES + uc.TOLERANCE_CASES, ids=[c[0] for c in uc.GOLDEN_CASES + uc.TOLERANCE_CASES])
def test_inputs_meet_the_conditions(case):
    """No |z| within 1e-4 of 10, no top-two gap below 1e-4, no softmax value within 1e-9 of a probability clip -- nor, next to 1
    where fp32 values lie 6e-8 apart, within that spacing of the fp32 clip: otherwise fp32 and fp64 sit on different sides of a
    gate and no tolerance is meaningful.  The inputs are built to meet this; no point is left out of a comparison."""
    z = uc.make_inputs(*case[1:5], case[10])[0]
    assert z.dtype == np.float32 and uc.conditions_met(z)
    bad = z.copy()
    bad[0, 0] = np.float32(10.00005)
    assert not uc.conditions_met(bad)
    if z.shape[1] > 1:
        bad = z.copy()
        bad[0] = 0.0
        assert not uc.conditions_met(bad)                    # a tie
        bad = z.copy()
        bad[0] = -20.0
        bad[0, 0] = np.float32(-10.0 - np.log(1e-7 / (1 - 1e-7) / (z.shape[1] - 1)))      # softmax of the clipped row = 1 - 1e-7
        assert not uc.conditions_met(bad)


def test_tolerance_cases_cover_the_shapes_and_are_recorded():
    ns, Cs = {c[1] for c in uc.TOLERANCE_CASES}, {c[2] for c in uc.TOLERANCE_CASES}
    assert {1, 255, 256, 257, 4000, 65537} <= ns and {1, 3, 4, 16} <= Cs
    assert set(uc.TOLERANCES) == {c[0] for c in uc.TOLERANCE_CASES}
    for s, g in uc.TOLERANCES.values():
        assert 0 < s < 1e-5 and 0 <= g < 1e-2


def test_one_recorded_tolerance_is_rederived():
    """8 x the worst fp32-vs-fp64 deviation over five batch orders, measured again here.  The figure is a maximum over rounding
    patterns, which a different libm or vector width moves a little: within a factor of 2 of the recorded one either way."""
    case = next(c for c in uc.TOLERANCE_CASES if c[0] == "n255_c3")
    s, g = uc.measure(case)
    rs, rg = uc.TOLERANCES["n255_c3"]
    print(f"n255_c3: re-derived ({8 * s:.3e}, {8 * g:.3e}), recorded ({rs:.3e}, {rg:.3e})")
    assert 0.5 * rs <= 8 * s <= 2 * rs and 0.5 * rg <= 8 * g <= 2 * rg


@pytest.mark.parametrize("case", uc.GOLDEN_CASES, ids=[c[0] for c in uc.GOLDEN_CASES])
def test_autograd_equals_the_closed_form(case):
    """Two derivations of dlogits: torch's autograd through the restatement with the clip rule written out, and the closed form
    the kernel evaluates.  They agree to fp64 rounding relative to the sum of the absolute terms."""
    z, labels, bw, cfg = uc.golden_case(case, round32=True)
    _, _, g, _ = ref.forward(z, labels, bw, cfg)
    gc, A = ref.closed_form(z, labels, bw, cfg)
    assert (np.abs(g - gc) <= 1e-12 * A + 1e-300).all()
    assert (A >= np.abs(gc) * (1 - 1e-12)).all() and (case[2] == 1 or np.abs(g).max() > 0)


def _small(C, seed, features=()):
    z, labels, bw = uc.make_inputs(24, C, seed, 2.0, features)
    if C > 1:
        z[np.arange(24), np.argmax(z, 1)] += np.float32(0.05)      # no step of the differences crosses an argmax tie
    return uc.condition(z), labels, bw


@pytest.mark.parametrize("C,seed,features,kw", [(4, 1, (), {}), (3, 2, ("outside",), dict(gamma=1.0, lam=0.25)), (4, 3, ("big",), dict(gamma=0.25, lam=0.75)),
                                                 (1, 4, (), {}), (3, 5, ("saturated",), dict(tv_w=0.05))])
def test_dlogits_agrees_with_central_differences(C, seed, features, kw):
    """D(h) = (L(z + h) - L(z - h)) / 2h = L' + c h^2 + O(h^4): the truncation error of D(h / 2) is |D(h) - D(h / 2)| / 3 to
    leading order and twice that is allowed; the roundoff of a difference is at most 4 eps64 S / (h / 2) with S = 4 (the loss is
    four terms of order one, each a quotient of sums of at most 24 positive terms).  Every element is checked.  The inputs keep
    every logit 1e-4 and more from a clip edge (and h below that), so no step crosses a gate."""
    z, labels, bw = _small(C, seed, features)
    cfg = ref.config([0.1, 1.5, 1.0, 2.0][:C], **kw)
    _, _, g, _ = ref.forward(z, labels, bw, cfg)
    h = 5e-5
    elems = [(i, j) for i in range(24) for j in range(C)]
    D = ref.central_differences(z, labels, bw, cfg, elems, h)
    for (i, j), (d1, d2) in zip(elems, D):
        bound = 2.0 * abs(d1 - d2) / 3.0 + 4.0 * np.finfo(np.float64).eps * 4.0 / (h / 2)
        assert abs(g[i, j] - d2) <= bound, (i, j, g[i, j], d1, d2, bound)
    assert C == 1 or np.abs(g).max() > 1e-4


def test_closed_interval_rule_and_non_finite_rows():
    cfg = ref.config([1.0, 1.0, 1.0])
    z = np.float32([[10.0, -10.0, 0.5], [10.5, -10.5, 0.5], [1.0, 2.0, 0.0], [np.nan, 0.0, 1.0], [np.inf, 0.0, 0.0]])
    labels = np.int32([0, 1, 2, 0, 1])
    loss, aux, g, tot = ref.forward(z, labels, np.float32([1, 1, 1, 1, 1]), cfg)
    gc, _ = ref.closed_form(z, labels, None, cfg)
    assert np.isfinite(loss) and np.isfinite(g).all() and not g[3:].any() and np.abs(g[:3]).min() > 0
    assert np.abs(g - gc).max() < 1e-15
    # the rows with a non-finite logit add nothing: the same sums as the first three rows alone, n stays 5
    _, _, _, tot3 = ref.forward(z[:3], labels[:3], np.float32([1, 1, 1]), cfg)
    for k in ("P", "A", "T", "S", "Q"):
        assert np.array_equal(tot[k], tot3[k])
    assert tot["FL"] == tot3["FL"] and tot["Acc"] == tot3["Acc"] and tot["Bd"] == tot3["Bd"]
    # at exactly +-10 the pc paths pass; beyond they do not: zero tv weight isolates them
    cfg0 = ref.config([1.0, 1.0, 1.0], tv_w=0.0)
    _, _, g0, _ = ref.forward(z[:3], labels[:3], None, cfg0)
    assert np.abs(g0[0]).min() > 0 and g0[1, 0] == 0 and g0[1, 1] == 0 and g0[1, 2] != 0
    assert ref.forward(z[:3], labels[:3], None, cfg0, dtype=torch.float32)[2][1, 0] == 0
