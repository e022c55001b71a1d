"""The references of the coordinate-injection INR's training step held to each other, and every exact case's preconditions
proved, without a GPU (tests/inject_train_ref.py, tests/inject_train_cases.py)."""
import numpy as np
import pytest

import inject_cases as ic
import inject_ref as ref
import inject_train_cases as tc
import inject_train_ref as tref

U32 = 2.0 ** -24                                          # the unit roundoff of fp32


def _tiny():
    rng = np.random.default_rng(5)
    F, M, widths, cl, ml, n = 4, 1, (5, 4, 3), (1,), (1,), 7
    params = ref.glorot_net(rng, F, M, widths, cl, ml)
    params["fourier"]["B"] = rng.normal(0, 0.5, (F // 2, 3)).astype(np.float32)
    coords, mods = ic.inputs(rng, n, M, special=False)
    dl = rng.normal(0, 1, (n, widths[-1])).astype(np.float32)
    return params, coords, mods, cl, ml, dl, dict(seed=11, keep=0.7, s=2)


def test_grads64_agrees_with_central_differences():
    """f = sum(logits64 * dlogits).  D(h) = (f(x + h) - f(x - h)) / 2h = f' + c h^2 + O(h^4), so D(h) - D(h / 2) = (3/4) c h^2 and
    the truncation error of D(h / 2) is |D(h) - D(h / 2)| / 3 to leading order; twice that is allowed for the next order.
    The roundoff of a difference is at most 4 eps64 S / h with S = sum |logits * dlogits| (each f within 2 eps64 S, generously:
    the sums have under a hundred terms); it is added.  The bound is relative to nothing but the differences themselves: no
    element is skipped.  Where a step crosses a ReLU kink the two differences disagree and the bound opens by itself; that must
    stay rare."""
    params, coords, mods, cl, ml, dl, drop = _tiny()
    g = tref.grads64(params, coords, mods, cl, ml, dl, drop)
    p64 = {"fourier": {"B": params["fourier"]["B"].astype(np.float64)}, "mlp": [{"W": p["W"].astype(np.float64), "b": p["b"].astype(np.float64)} for p in params["mlp"]]}

    def f():
        z = ref.forward64(p64, coords, mods, cl, ml, drop)
        return float((z * dl).sum()), float(np.abs(z * dl).sum())

    S = f()[1]
    h = 1e-4
    rough, total = 0, 0
    arrays = [(p64["fourier"]["B"], g["B"])] + [(p["W"], gw) for p, gw in zip(p64["mlp"], g["W"])] + [(p["b"], gb) for p, gb in zip(p64["mlp"], g["b"])]
    for arr, grad in arrays:
        for idx in np.ndindex(arr.shape):
            x0 = arr[idx]
            D = []
            for step in (h, h / 2):
                arr[idx] = x0 + step
                fp = f()[0]
                arr[idx] = x0 - step
                fm = f()[0]
                D.append((fp - fm) / (2 * step))
            arr[idx] = x0
            trunc = abs(D[0] - D[1]) / 3.0
            bound = 2.0 * trunc + 4.0 * np.finfo(np.float64).eps * S / (h / 2)
            assert abs(grad[idx] - D[1]) <= bound, (idx, grad[idx], D, bound)
            total += 1
            rough += trunc > 1e-6 * max(abs(D[1]), 1e-3)
    assert total == sum(a.size for a, _ in arrays) and rough <= total // 20, (rough, total)


def _reasoned_tol(params, coords, n, shapes):
    """First-order bound on |backward32 - grads64| / A away from the ReLU kinks.  A chain of K fp32 additions is within K u of
    its exact sum relative to the sum of absolute terms (u = 2^-24): the batch sums have slab_len + slabs terms, the forward and
    the dZ . W^T products of layer l have in_l + 1 and out_l; an error made at one layer reaches a gradient through every layer
    in between, hence the sum over the layers, twice (forward and backward).  The features add the sine's argument error: a =
    2 pi32 p is formed in four fp32 operations from |p| <= 3 max|c01 B|, so |delta a| <= 5 u max|a|, and sin / cos move by as
    much; the correctly rounded sine itself adds u.  The factor 4 covers the products of these first-order terms and the
    cancellation inside A's own factors (|x| and |dz| carry the same relative errors)."""
    length = tref.slab_len(n)
    chain = length + (n + length - 1) // length
    layers = sum(s[0] + 1 + s[3] for s in shapes)
    _, a = tref.angles32(params["fourier"]["B"], coords)
    return 4.0 * U32 * (chain + 2 * layers + 5.0 * float(np.abs(a).max()) + 1.0)


def test_backward32_stays_within_the_tolerance_rule_of_grads64():
    for F, M, widths, cl, ml, n, keep in ((16, 4, (17, 13, 4), (1,), (1,), 65, 0.7), (128, 4, (64, 64, 64, 4), (1, 2), (2,), 130, 1.0)):
        rng = np.random.default_rng(n)
        params = ref.glorot_net(rng, F, M, widths, cl, ml)
        coords, mods = ic.inputs(rng, n, M, special=False)
        dl = (rng.normal(0, 1, (n, widths[-1])) / n).astype(np.float32)
        drop = tc.dropout_of(keep)
        g64 = tref.grads64(params, coords, mods, cl, ml, dl, drop)
        dl[tref.near_kink(g64["z"], 1e-4)] = 0.0           # the side of a ReLU this close to its kink is not decided in fp32
        g64 = tref.grads64(params, coords, mods, cl, ml, dl, drop)
        g32 = tref.backward32(params, coords, mods, cl, ml, dl, drop)
        dev, tol = tref.relative_deviation(g32, g64), _reasoned_tol(params, coords, n, ref.net_shape(F, M, widths, cl, ml))
        print("backward32 vs grads64: worst |g32 - g64| / A", dev, "bound", tol)
        assert dev <= tol
        # and accumulation: old + restated
        old = dict(B=rng.normal(0, 1, g32["B"].shape).astype(np.float32), W=[rng.normal(0, 1, w.shape).astype(np.float32) for w in g32["W"]],
                   b=[rng.normal(0, 1, b.shape).astype(np.float32) for b in g32["b"]])
        acc = tref.backward32(params, coords, mods, cl, ml, dl, drop, old=old)
        assert ref.same_bits(acc["B"], old["B"] + g32["B"])
        if n <= 256:                                         # one slab: old + slab is old + the whole sum
            assert all(ref.same_bits(a, o + g) for a, o, g in zip(acc["W"], old["W"], g32["W"]))


@pytest.mark.parametrize("case", tc.INTEGER, ids=[c[0] for c in tc.INTEGER])
def test_integer_cases_are_exact_in_fp32_and_carry_signal(case):
    params, c8, mods, dl, drop, old = tc.integer_case(case)
    r = tref.backward_int(params, c8, mods, case[5], case[6], dl, drop)
    assert r["bound"] < 2 ** 24, r["bound"]                   # every dot product, the batch sums included, in units of 1/8 (1/16 for dB)
    assert np.abs(dl).max() <= 2 and np.count_nonzero(dl) > 0
    assert drop is None or float(np.float32(1.0) / np.float32(drop["keep"])) in (2.0, 4.0)
    assert sum(np.count_nonzero(w) for w in r["W8"]) > 0
    if case[1] >= 63:
        assert all(np.count_nonzero(w) > 0 for w in r["W8"]) and np.count_nonzero(r["B16"]) > 0, "a gradient died on the way down"
    if old is not None:                                         # old + sum stays an exact integer multiple too
        assert max(float(np.abs(o).max()) for o in [old["B"], *old["W"], *old["b"]]) <= 4
    # the restated fp32 backward computes exactly these integers
    g32 = tref.backward32(params, (c8 / 8.0).astype(np.float32), mods.astype(np.float32), case[5], case[6], dl.astype(np.float32), drop) if case[1] <= 321 else None
    if g32 is not None:
        assert all(np.array_equal(w.astype(np.float64) * 8, w8) for w, w8 in zip(g32["W"], r["W8"]))
        assert all(np.array_equal(b.astype(np.int64), bi) for b, bi in zip(g32["b"], r["b"]))
        assert ref.same_bits(g32["B"], tref.dB_of_int(r["B16"]))


def test_integer_cases_cover_the_shapes_the_kernels_branch_on():
    ns = {c[1] for c in tc.INTEGER}
    assert {1, 63, 64, 65, 257, 321, 4000, 16385} <= ns
    assert tref.slab_len(16385) == 512 and (16385 + 511) // 512 == 33 and 16385 - 32 * 512 == 1
    assert tref.slab_len(4000) == 256 and (4000 + 255) // 256 == 16 and 4000 - 15 * 256 == 160
    widths = {w for c in tc.INTEGER for w in c[4]}
    assert {1, 13, 16, 17, 60, 61, 64, 65, 256} <= widths
    assert {2, 14, 16, 18, 128, 256} <= {c[2] for c in tc.INTEGER} and {0, 1, 4, 8} <= {c[3] for c in tc.INTEGER}
    assert {2, 3, 5, 8} <= {len(c[4]) for c in tc.INTEGER} and {1, 3, 4, 15, 16} <= {c[4][-1] for c in tc.INTEGER}
    rows = {s[0] + 1 for c in tc.INTEGER for s in ref.net_shape(c[2], c[3], c[4], c[5], c[6])}
    assert 64 in rows and 65 in rows                           # in_l + 1: the row of ones is the last of a block, and alone in the next
    first_c = any(1 in c[5] for c in tc.INTEGER); last_c = any(len(c[4]) - 2 in c[5] and len(c[4]) > 3 for c in tc.INTEGER)
    first_m = any(1 in c[6] for c in tc.INTEGER); last_m = any(len(c[4]) - 2 in c[6] and len(c[4]) > 3 for c in tc.INTEGER)
    assert first_c and last_c and first_m and last_m
    assert sum(c[9] for c in tc.INTEGER) * 4 >= len(tc.INTEGER) - 3      # about a quarter accumulate
    assert {c[8] for c in tc.INTEGER} == {1.0, 0.5, 0.25}


@pytest.mark.parametrize("case", ic.EXACT, ids=[c[0] for c in ic.EXACT])
def test_selection_cases_have_one_term_per_slab_in_every_batch_sum(case):
    name, n, F, M, widths, cl, ml, _ = case
    params, _, coords, mods = tc.selection_case(case)
    drop = tc.dropout_of(0.5)
    sv = tref.forward_saved32(params, coords, mods, cl, ml, drop)
    rng = np.random.default_rng(ic.seed_of(name))
    length = tref.slab_len(n)
    zero_units = dead_units = beyond = 0
    for row in tc.SELECTION_ROWS:
        dl = tc.one_row_per_slab(rng, n, widths[-1], row)
        g = tref.backward32(params, coords, mods, cl, ml, dl, drop, saved=sv)
        for dz in [*g["dz"], g["g"]]:                         # every A . B over the batch: at most one point per slab contributes
            live = (dz != 0).any(1)                           # (a NaN counts as non-zero)
            for z0 in range(0, n, length):
                assert live[z0:z0 + length].sum() <= 1
    for l, z in enumerate(sv["z"][:-1]):
        zero_units += int((z[:, 0] == 0).sum())
        dead_units += int(z.shape[1] > 1 and not (z[:, 1] > 0).any())
    _, a = tref.angles32(params["fourier"]["B"], coords)
    beyond = int((np.abs(a) > tref.DOMAIN).sum())
    if n >= 63:
        assert zero_units > 0 and dead_units > 0
        assert np.isnan(coords).any() and np.isinf(coords).any()
    if F >= 4:
        assert beyond > 0


@pytest.mark.parametrize("t", tc.TOLERANCE, ids=[t[0] for t in tc.TOLERANCE])
def test_tolerance_cases_remove_at_most_one_percent(t):
    params, coords, mods, dl, drop = tc.tolerance_case(t)
    g = tref.grads64(params, coords, mods, t[2][5], t[2][6], dl, drop)
    removed = int(tref.near_kink(g["z"]).sum())
    print(t[0], "points within 2e-5 rms of a ReLU kink:", removed, "of", t[1])
    assert removed <= t[1] // 100
