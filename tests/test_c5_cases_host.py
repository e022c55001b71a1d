"""The C5 case grid (tests/c5_cases.py, tests/c5_ref.py) checked on the oracle alone, without a GPU: every precondition that
makes the reference of tests/test_gpu_c5_cases.py exact, what each case claims to exercise, and that the comparisons the GPU
tests make do report a perturbed reference."""
import numpy as np
import pytest

import c5_cases as cc
import c5_ref as cr
from oracle import oracle_np as onp


def _net_params(net):
    layers = cc.layers_of(net)
    return (cc.siren_dict(layers), "siren") if net.kind == "siren" else (layers, "fourier")


@pytest.mark.parametrize("name", cc.NAMES)
def test_oracle_network_gives_the_rules_class_on_every_sample(name):
    """The oracle's own fp32 network (apply_mlp(build_input(...)) / siren_apply) through brats_main_inr: on every sample of
    every ray (early termination off) its argmax is the rule's class, strictly — the winning logit is above every other, so
    nothing rests on which of two equal logits an argmax takes; and with the case's own termination it renders the reference."""
    case, ref = cc.CASES[name], cr.reference(name)
    vols, lab, zmu, zsg = cc.volumes(case.dims, case.vol_seed)
    params, kind = _net_params(case.net)
    seen = [0]

    def record(idx, k, c, f, logits):
        want = cc.rule(case.net, c, f)
        rows = ref["offsets"][idx] + k
        assert np.array_equal(want, ref["classes"][rows])
        top = logits[np.arange(len(want)), want]
        rest = logits.copy()
        rest[np.arange(len(want)), want] = -np.inf
        assert (top > rest.max(axis=1)).all(), "a sample whose winning logit is not strictly the largest"
        assert np.array_equal(np.argmax(logits, axis=-1), want)
        seen[0] += len(want)

    labels = lab if case.labels is not None else None
    p = cc.params_of(case)
    onp.brats_main_inr(p, list(vols), params, case.net.K, zmu, zsg, labels=labels, ext=dict(cc.oracle_ext(case), ertThreshold=-1.0),
                       kind=kind, w0=cc.W0, record=record)
    assert seen[0] == int(ref["n"].sum())
    frame = onp.brats_main_inr(p, list(vols), params, case.net.K, zmu, zsg, labels=labels, ext=cc.oracle_ext(case), kind=kind, w0=cc.W0)
    assert not cr.frame_problems(frame, ref["frame"])


@pytest.mark.parametrize("name", cc.NAMES)
def test_feature_margin_and_sine_range(name):
    """min |x_f| >= 2^-20 over EVERY sample of the case (no ties, no flushed denormals, no zero sine argument: none is
    excluded), and for SIREN nets w0 s max |x_f| <= 1 (the live path stays inside (-pi/2, pi/2))."""
    case, ref = cc.CASES[name], cr.reference(name)
    x = cc.feature(case.net, ref["coords"], ref["feats"])
    if "miss_all" in case.claims:
        assert x.size == 0
        return
    assert x.size == int(ref["n"].sum()) and x.size > 0
    assert np.isfinite(x).all()
    print(f"{name}: min |x_f| = {np.abs(x).min():.3e}, max |x_f| = {np.abs(x).max():.3f} over {x.size} samples")
    assert np.abs(x).min() >= cc.MARGIN
    if case.net.kind == "siren":
        assert cc.W0 * cc.scale(case.net) * float(np.abs(x).max()) <= 1.0


def _tested(case, ref):
    return [c if c is not None else cr.default_chunk(case) for c in cr.chunks_of(case, ref)]


KNOWN_CLAIMS = {"early", "none_terminate", "miss_all", "miss_some", "all_hit", "multiple", "ert_boundary", "last_pass_empty", "both_classes",
                "clipped", "drift"}


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_exercises_what_it_claims(name):
    case, ref = cc.CASES[name], cr.reference(name)
    n, L = ref["n"].reshape(-1), ref["L"].reshape(-1)
    assert case.claims <= KNOWN_CLAIMS
    assert (L <= n).all() and ref["live"] == int(L.sum())
    assert n.size == case.frame[0] * case.frame[1]
    chunks = _tested(case, ref)
    assert n.max() <= cr.max_steps(case), "the bound on the number of passes must cover every ray"
    assert all(cr.passes(case, c) <= cr.MAX_PASSES for c in chunks)
    if case.refused_chunk is not None:
        assert cr.passes(case, case.refused_chunk) > cr.MAX_PASSES
    if case.chunks is None:
        assert {1, 2, 32, 4096} <= set(chunks) and None in cr.chunks_of(case, ref)
        assert n.max() <= 50 + 3
    if case.ert is not None and case.ert < 0:
        assert np.array_equal(L, n)
    for claim in case.claims:
        if claim == "early":
            assert (L < n).sum() >= 1
        elif claim == "none_terminate":
            assert np.array_equal(L, n) and n.sum() > 0
        elif claim == "miss_all":
            assert n.sum() == 0
        elif claim == "miss_some":
            assert (n == 0).sum() >= n.size // 8 and (n > 0).sum() >= n.size // 8
        elif claim == "all_hit":
            assert (n > 0).all()
        elif claim == "multiple":
            c = cr.chunk_of_a_ray(ref)
            assert c in chunks and ((n > 0) & (n % c == 0)).any()
        elif claim == "ert_boundary":
            c = cr.chunk_of_a_death(ref)
            assert c in chunks and ((L < n) & (L > 0) & (L % c == 0)).any()
        elif claim == "last_pass_empty":
            assert any((cr.passes(case, c) - 1) * c >= n.max() for c in chunks)
        elif claim == "both_classes":
            seen = set(np.unique(ref["classes"][cr.live_rows(ref)]).tolist())
            drawn = {c for c in (case.net.a, case.net.b) if 0 < c < 8}
            assert drawn and drawn <= seen
        elif claim == "clipped":
            # the same rays without nearT / farT march from before the slab to beyond it
            import dataclasses
            whole = dataclasses.replace(case, near=0.0, far=0.0)
            vols, lab, _, _ = cc.volumes(case.dims, case.vol_seed)
            _, aux = onp.brats_main(dict(cc.params_of(whole), showPred=0, showSeg=0), list(vols), None, None, dict(ertThreshold=-1.0), return_aux=True)
            m = aux["nsteps"].reshape(-1)
            assert ((n > 0) & (n + 4 <= m)).sum() >= (m > 0).sum() // 2
            assert case.near > 0 and case.far > case.near


def _chords_fp64(case):
    """Exact length of every ray's chord through the box: the oracle's fp32 rays, the slab test in fp64."""
    p = cc.params_of(case)
    Wd, H = case.frame
    (ox, oy, oz), d = onp.make_primary(Wd, H, p["fovY"], p["eye"], p["U"], p["V"], p["W"])
    o = np.array([ox, oy, oz], np.float64)
    d = np.stack([a.reshape(-1) for a in d], axis=-1).astype(np.float64)
    lo = np.asarray(p["volMin"], np.float32).astype(np.float64)
    hi = (np.asarray(p["volMin"], np.float32) + np.asarray(p["voxelSize"], np.float32) * np.asarray(case.dims, np.float32)).astype(np.float64)
    ta, tb = (lo - o) / d, (hi - o) / d
    t0, t1 = np.minimum(ta, tb).max(axis=1), np.maximum(ta, tb).min(axis=1)
    return np.maximum(t1 - np.maximum(t0, 0.0), 0.0)


def test_drift_case_outruns_its_chord():
    """The running fp32 sum t += stepSize takes measurably more steps than chord / stepSize where stepSize is ~20 ulps of t; the
    rays are long enough that a bound on the passes that forgot that drift would stop short of their end."""
    case, ref = cc.CASES["linear_drift_8x8"], cr.reference("linear_drift_8x8")
    assert "drift" in case.claims and case.frame == (8, 8) and case.ert == -1.0
    p = cc.params_of(case)
    step = float(np.float32(p["stepSize"]))
    t_eye = float(np.linalg.norm(np.asarray(p["eye"], np.float64)))
    ulp = float(np.spacing(np.float32(t_eye)))
    assert 15.0 <= step / ulp <= 25.0, "ulp(t) about 1/20 of stepSize"
    assert 0.2 <= (step / ulp) % 1.0 <= 0.8, "stepSize is no multiple of that ulp, nor close to one"
    n = ref["n"].reshape(-1).astype(np.float64)
    exact = _chords_fp64(case) / step
    excess = n[exact > 100] / exact[exact > 100]
    print(f"drift: n / (chord / stepSize) in [{excess.min():.4f}, {excess.max():.4f}], longest ray {int(n.max())} steps; "
          f"bound {cr.max_steps(case)} with the drift term, {cr.max_steps(case, with_drift=False)} without")
    assert excess.max() >= 1.01
    assert cr.max_steps(case, with_drift=False) < n.max() <= cr.max_steps(case)
    c, = case.chunks
    assert 200 <= cr.passes(case, c) <= 500, "a few hundred passes"
    assert (cr.passes(case, c, with_drift=False) * c < n).any(), "without the drift term the last pass would leave rays marching"


def test_queries_formula_by_hand():
    # three rays of a 3-step pass: runs to its end (5 of 5), terminates at its 2nd step, misses
    n, L = np.array([5, 5, 0]), np.array([5, 2, 0])
    assert cr.queries(n, L, 3) == 5 + 3 + 0
    assert cr.queries(n, L, 1) == 5 + 2 and cr.queries(n, L, 4096) == 10
    assert cr.queries(n, L, 2) == 5 + 2 and cr.queries(n, L, 2, floor=True) == 4 + 2
    # a termination exactly on a pass boundary plans no further pass
    assert cr.queries(np.array([9]), np.array([6]), 3) == 6 and cr.queries(np.array([9]), np.array([7]), 3) == 9


def test_comparisons_report_a_perturbed_reference():
    """No broken kernel is run: the reference is perturbed instead, and the helpers the GPU tests assert on must say so."""
    name = "linear_shaded_56x40"
    case, ref = cc.CASES[name], cr.reference(name)
    n, L = ref["n"], ref["L"]
    good = dict(live_samples=ref["live"], shaded_samples=ref["shaded"])
    for c in _tested(case, ref):
        aux = dict(good, queries=cr.queries(n, L, c))
        assert not cr.counter_problems(aux, ref, c)
    assert not cr.frame_problems(ref["frame"].copy(), ref["frame"])
    assert not cr.stream_problems(n.reshape(-1), ref["classes"], ref["coords"], ref["feats"], ref)

    # 1. the class of ONE composited sample flipped (the first sample of the longest ray)
    ray = int(np.argmax(L.reshape(-1)))
    row = int(ref["offsets"][ray])
    flipped = ref["classes"].copy()
    flipped[row] = case.net.a if flipped[row] == case.net.b else case.net.b
    frame = cr.frame_with_classes(case, flipped, ref["offsets"])
    problems = cr.frame_problems(frame, ref["frame"])
    assert len(problems) == 1 and "1 of 2240 pixels differ" in problems[0], problems
    assert any(s.startswith("classes: 1 of") for s in cr.stream_problems(n.reshape(-1), flipped, ref["coords"], ref["feats"], ref))
    one = ref["coords"].copy()
    one[row, 1] = np.nextafter(one[row, 1], np.float32(2.0))
    assert any(s.startswith("coords: 1 of") for s in cr.stream_problems(n.reshape(-1), ref["classes"], one, ref["feats"], ref))

    # 2. one ray truncated by one step
    y, x = np.unravel_index(ray, L.shape)
    Lt, nt = L.copy(), n.copy()
    Lt[y, x] -= 1
    nt[y, x] -= 1
    for c in _tested(case, ref):
        got = dict(good, queries=cr.queries(n, L, c))                    # what a correct kernel reports ...
        said = cr.counter_problems(got, ref, c, n=nt, L=Lt)        # ... against the truncated reference
        assert any(s.startswith("live_samples") for s in said), c
    assert any(s.startswith("queries") for s in cr.counter_problems(dict(good, queries=cr.queries(n, L, 1)), ref, 1, n=nt, L=Lt))
    assert any(s.startswith("counts: 1 rays differ") for s in cr.stream_problems(nt.reshape(-1), ref["classes"], ref["coords"], ref["feats"], ref))

    # 3. floor instead of ceil in the queries formula: visible at every pass length that some early termination does not fall on
    early = L[L < n]
    assert early.size
    told = 0
    for c in _tested(case, ref):
        aux = dict(good, queries=cr.queries(n, L, c, floor=True))
        if (early % c != 0).any():
            assert any(s.startswith("queries") for s in cr.counter_problems(aux, ref, c)), c
            told += 1
    assert told >= 4


def test_grid_covers_what_the_issue_lists():
    cases = list(cc.CASES.values())
    nets = [k.net for k in cases]
    assert {k.f for k in nets} == set(range(7))
    assert {k.layout for k in cases} == {"linear", "brick", "vg", "quad", "mod4"}
    assert {k.layout for k in cases if k.shade} == {"linear", "brick", "vg"}
    assert {k.labels for k in cases} == {None, "linear", "brick"}
    assert {k.enabled for k in cases} == {(1, 1, 1, 1), (0, 1, 0, 1), (0, 0, 0, 0)}
    assert all(len(set(k.weights)) > 1 for k in cases if "drift" not in k.claims)
    assert {(1, 1), (8, 8), (9, 9), (64, 1), (37, 29), (56, 40)} <= {k.frame for k in cases}
    assert max(k.frame[0] * k.frame[1] for k in cases) <= 56 * 40
    assert all(9 * 8 * 7 <= np.prod(k.dims) <= 24 * 20 * 18 for k in cases)
    assert {k.variant for k in cases} == {0, 2, 3}                       # both workgroup shapes; row-major lanes once
    assert {k.ert for k in cases} >= {None, 0.5, -1.0}
    assert min(k.alpha for k in cases) <= 0.4 and max(k.alpha for k in cases) >= 40.0
    ortho = [k for k in cases if k.cam.ortho is not None]
    assert {k.frame[0] / k.frame[1] for k in ortho} == {7.0, 1.0 / 7.0}
    assert any(k.near > 0 and k.far > 0 for k in cases)
    assert all(any(k.bg) for k in cases if k.claims & {"miss_all", "miss_some"}), "a ray that misses shows the background"
    assert {k.gamma for k in cases} >= {0.7, 1.0, 2.2}
    for claim in ("miss_all", "miss_some", "all_hit", "clipped", "drift", "early", "none_terminate", "ert_boundary", "last_pass_empty"):
        assert any(claim in k.claims for k in cases), claim
    # the eye of the all_hit case is inside the box
    inside = next(k for k in cases if "all_hit" in k.claims)
    p = cc.params_of(inside)
    assert (np.abs(np.asarray(p["eye"])) < -np.asarray(p["volMin"])).all() and inside.frame == (37, 29) and (37 * 29) % 256 != 0
    # networks: the 4 x 256 SIREN, a 2 x 64 SIREN, a 4 x 64 Fourier/ReLU, 8 and 16 outputs, a pair >= 8, a pair with class 0
    shapes = {(k.kind, k.hidden, k.depth, k.out) for k in nets}
    assert {("siren", 256, 4, 4), ("siren", 64, 2, 4), ("fourier", 64, 4, 4)} <= shapes
    assert any(k.out == 8 and min(k.a, k.b) >= 4 for k in nets) and any(k.out == 16 and min(k.a, k.b) >= 8 for k in nets)
    assert any(0 in (k.a, k.b) for k in nets) and any(k.out == 16 and min(k.a, k.b) < 8 <= max(k.a, k.b) for k in nets)
    live = {j for k in nets for j in ((k.jp,) if k.kind == "siren" else (k.jp, k.jm))}
    assert {0, 63, 255} <= live
    assert any(k.kind == "fourier" and k.jp // 32 != k.jm // 32 for k in nets) and any(k.kind == "fourier" and k.jp > k.jm for k in nets)
    assert any(k.kind == "fourier" and k.K == 0 for k in nets) and any(k.kind == "fourier" and k.K > 0 for k in nets)
    for k in nets:
        layers = cc.layers_of(k)
        if k.kind == "fourier":
            assert not layers[0]["W"][3:3 + 6 * k.K].any()
        head = layers[-1]
        assert np.count_nonzero(head["W"]) == 2 and sorted(np.unique(head["b"]).tolist()) in ([-4.0, 0.0], [0.0])
