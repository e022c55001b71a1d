"""Every K1 march kernel the launch plan can pick, rendered against the oracle.

tests/k1_plan_ref.py restates the plan and spans a grid of 2720 launchable configurations; tests/test_k1_plan_host.py proves
that the 172 kernels the grid reaches, plus the tagged twin, are exactly the march kernels in the built library.  Here every
one of them gets a pytest id of its own, and every configuration that maps to it is rendered on a tiny scene (40 x 34 x 27
voxels, 40 x 28 pixels, about 60 steps) four ways — both workgroup shapes (kernelVariant bit 1), both sides of the run-time exp
switch — and held to the oracle: STRICT to oracle_c bit for bit with equal counters, FAST to oracle_np through
test_gpu_parity's _fast_check.  Where the plan marches with a skip map the frame and the counters must be the plain launch's,
twice (the Python layer decides on the second frame whether the map is kept), and the diagnostic counter of kernelVariant
bit 7 must show samples that were not fetched: a silent fall-back to the plain kernel would otherwise pass.
"""
import numpy as np
import pytest

import k1_plan_ref as K

pytestmark = pytest.mark.gpu

CASES = K.cases_by_kernel()
KERNELS = sorted(CASES, key=K.kernel_id)
WAYS = [(flip, exp_range) for flip in (False, True) for exp_range in ("small", "large")]


class _Bound:
    """The scene's grids on the device, one upload per layout."""

    def __init__(self):
        import mrirt
        self.mrirt = mrirt
        self.s = K.shared_scene()
        self._vols, self._labels = {}, {}

    def vols(self, layout):
        if layout not in self._vols:
            m, s = self.mrirt, self.s
            self._vols[layout] = [m.upload_mod4(s["vols"], K.DIMS)] * 4 if layout == "mod4" else [m.upload_grid(v, K.DIMS, layout) for v in s["vols"]]
        return self._vols[layout]

    def labels(self, c):
        """(labels, preds) as the configuration binds them: nothing without an overlay, one label-cell grid, or plain grids
        (linear under linear intensities, bricked otherwise)."""
        if c.overlays == "none":
            return None, None
        kind = "labcell" if c.cells else "linear" if c.layout == "linear" else "brick"
        if kind not in self._labels:
            m, s = self.mrirt, self.s
            self._labels[kind] = (m.upload_label_cells(s["lab"], s["prd"], K.DIMS), None) if kind == "labcell" else \
                (m.upload_grid(s["lab"], K.DIMS, kind), m.upload_grid(s["prd"], K.DIMS, kind))
        gl, gp = self._labels[kind]
        return gl, (gp if c.overlays == "seg+pred" else None)


@pytest.fixture(scope="module")
def bound():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _Bound()


def _ext(c, flip, extra=0):
    variant = extra | (K.VARIANT_FLIP_WORKGROUP if flip else 0) | (K.VARIANT_NO_PIPE if c.nopipe else 0) | (K.VARIANT_TAG if c.tag else 0)
    return dict(K.shade_ext(c), layout=c.layout, math=c.math, kernelVariant=variant)


def _render(bound, c, p, ext, skip):
    gl, gp = bound.labels(c)
    img, st = bound.mrirt.render_brats(p, bound.vols(c.layout), gl, gp, ext=ext, stats=True, skip=skip)
    return img, st


def _robust_error(got, ref, aux):
    return float(np.abs(got - ref)[..., :3].max(axis=-1)[~aux["fragile"]].max())


def _check_against_oracle(c, exp_range, img, st, what):
    """STRICT: the oracle's bits and counters.  FAST: _fast_check, unchanged; returns the robust error."""
    from test_gpu_parity import _fast_check
    ref, aux = K.reference(c, exp_range)
    got = img.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32, what
    if c.math == "strict":
        assert np.array_equal(got, ref), f"{what}: differs from oracle_c, max-abs {np.abs(got - ref).max():.3e} in {(got != ref).any(axis=-1).sum()} pixels"
        assert st["live_samples"] == aux["live_samples"] and st["shaded_samples"] == aux["shaded_samples"], (what, st, aux)
        return 0.0
    err = _robust_error(got, ref, aux)
    _fast_check(got, ref, aux, what)
    return err


def _check_config(bound, c):
    """One configuration, four ways; returns the worst robust FAST error."""
    import torch
    from mrirt import render
    pl = K.plan(c)
    worst = 0.0
    if pl.skipping:
        render._SKIP_MAPS.clear()
    builds = render.skip_map_builds
    for n, (flip, exp_range) in enumerate(WAYS):
        what = f"{c} {'16x16' if flip else '8x8'} exp-{exp_range}"
        p = K.params(c, exp_range)
        assert K.exp_small(p["intensityAlpha"]) == (exp_range == "small")
        if not pl.skipping:
            # (a map that is offered but has no kernel to read it costs nothing: no pre-pass)
            img, st = _render(bound, c, p, _ext(c, flip), c.skip)
            worst = max(worst, _check_against_oracle(c, exp_range, img, st, what))
            assert render.skip_map_builds == builds, what
            continue
        plain, st0 = _render(bound, c, p, _ext(c, flip), False)
        worst = max(worst, _check_against_oracle(c, exp_range, plain, st0, what + " plain"))
        for frame in (1, 2):
            img, st = _render(bound, c, p, _ext(c, flip), True)
            assert torch.equal(img, plain) and st == st0, f"{what}: skipping frame {frame} differs from the plain launch ({st} vs {st0})"
            # the map does not depend on the workgroup shape or on intensityAlpha: built by the first launch, reused since
            assert render.skip_map_builds == builds + 1, f"{what}: frame {frame}, {render.skip_map_builds - builds} map builds"
        (entry,) = render._SKIP_MAPS.values()
        assert entry.built and entry.empty_fraction is not None and entry.empty_fraction > 0.5, what
        img, st = _render(bound, c, p, _ext(c, flip, K.VARIANT_COUNT_UNFETCHED), True)
        assert torch.equal(img, plain) and st["live_samples"] == st0["live_samples"], what
        assert st["shaded_samples"] - st0["shaded_samples"] > 0, f"{what}: the skipping march fetched every sample"
    return worst


@pytest.mark.parametrize("kernel", KERNELS, ids=K.kernel_id)
def test_kernel_matches_oracle(bound, kernel):
    worst = {True: 0.0, False: 0.0}
    for c in CASES[kernel]:
        assert K.plan(c).kernel == kernel
        e = _check_config(bound, c)
        worst[c.gamma == 1.0] = max(worst[c.gamma == 1.0], e)
    if not kernel[1]:
        print(f"\nK1FAST {K.kernel_id(kernel)} configs={len(CASES[kernel])} worst robust max-abs: gamma=1 {worst[True]:.3e}  gamma={K.GAMMA_NOT_1} {worst[False]:.3e}")


def test_tagged_twin_renders_the_untagged_kernels_bits(bound):
    """kernelVariant bit 15: the same code under a second symbol (the kernel behind bench.py's side measurements)."""
    import torch
    c = K.TAG_CONFIG
    assert K.plan(c).kernel[-1] is True and K.plan(c._replace(tag=False)).kernel[-1] is False
    for flip, exp_range in WAYS:
        p = K.params(c, exp_range)
        tagged, st1 = _render(bound, c, p, _ext(c, flip), False)
        plain, st0 = _render(bound, c._replace(tag=False), p, _ext(c._replace(tag=False), flip), False)
        assert torch.equal(tagged, plain) and st1 == st0
        _check_against_oracle(c, exp_range, tagged, st1, f"tagged twin {flip} {exp_range}")
