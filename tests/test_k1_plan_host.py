"""The K1 launch plan, held from the host side (no GPU): tests/k1_plan_ref.py restates plan_k1() and the kernel selection of
csrc/brats_march.hip; here the restatement is held to the library's own host-only query, the kernels its case grid reaches are
held to the kernels the built library contains, and the scene tests/test_gpu_k1_kernels.py renders is shown to be fit for its
two jobs (FAST references without knife-edge pixels, skipping volumes with empty space)."""
import collections

import numpy as np
import pytest

import k1_plan_ref as K


@pytest.fixture(scope="module")
def cases():
    return K.cases_by_kernel()


def _ext(c, variant=0):
    return dict(K.shade_ext(c), layout=c.layout, math=c.math, labelLayout="labcell" if c.cells else "brick",
                kernelVariant=variant | (K.VARIANT_NO_PIPE if c.nopipe else 0) | (K.VARIANT_TAG if c.tag else 0))


def test_restatement_agrees_with_the_library():
    """Family / skipping / label_cells of every grid configuration as mrirt_brats_kernel_family reports them (host-only: nothing
    is launched); what the restatement refuses, the library refuses."""
    import mrirt
    from mrirt import render
    grid = K.grid() + [K.TAG_CONFIG]
    refused = 0
    for c in grid:
        want = K.plan(c)
        p = K.params(c, "large")
        if want == K.REFUSED:
            refused += 1
            with pytest.raises(mrirt._lib.MrirtError):
                render.kernel_family(p, _ext(c), skip=c.skip)
            continue
        got = render.kernel_family(p, _ext(c), skip=c.skip)
        assert got == {"family": want.family, "skipping": want.skipping, "label_cells": want.label_cells}, c
        # the workgroup shape (kernelVariant bit 1) is no input of the plan
        assert render.kernel_family(p, _ext(c, K.VARIANT_FLIP_WORKGROUP), skip=c.skip) == got, c
    assert refused == 800 and len(grid) == 3521


def test_mangled_names_parse():
    assert K.parse_kernel_name("_ZN5mrirt18brats_march_kernelILb1ELi6ELb0EEEvNS_6K1ArgsE") == ("generic", True, 6, False)
    assert K.parse_kernel_name("_ZN5mrirt23brats_march_pipe_kernelILb1ELi4ELb1ELi1ELb1ELb0ELb0ELb0ELb1EEEvNS_6K1ArgsE") == \
        ("pipe", True, 4, True, 1, True, False, False, False, True)
    assert K.parse_kernel_name("_ZN5mrirt23brats_march_roll_kernelILb0ELi2ELb1ELi3ELb0ELb1ELb0EEEvNS_6K1ArgsE") == \
        ("roll", False, 2, True, 3, False, True, False)
    assert K.parse_kernel_name("_ZN5mrirt16skip_mask_kernelILb1EEEvNS_8SkipArgsE") is None
    with pytest.raises(ValueError):
        K.parse_kernel_name("_ZN5mrirt18brats_march_kernelILb1ELi6EEEvNS_6K1ArgsE")


def test_case_grid_reaches_exactly_the_kernels_the_library_contains(cases):
    """Closure: the kernel identities the plan picks over the case grid == the brats_march_kernel / _pipe_kernel / _roll_kernel
    instantiations in the built library's gfx950 code objects, the tagged twin aside (which the grid leaves to its own case).
    A kernel no case reaches, or a predicted kernel the library lacks, fails here: a change of the plan or a new instantiation
    cannot land without a case."""
    import mrirt
    built = K.library_kernels(mrirt._lib.SO_PATH)
    assert len(built) == len(set(built)), [K.kernel_id(k) for k, n in collections.Counter(built).items() if n > 1]
    tag = K.plan(K.TAG_CONFIG).kernel
    assert tag == ("pipe", True, K.LAYOUT_CODE["vga"], True, 1, True, False, False, False, True)
    assert tag not in cases, "the tagged twin is launched by its own case only"
    predicted = set(cases) | {tag}
    unreached = sorted(K.kernel_id(k) for k in set(built) - predicted)
    lacking = sorted(K.kernel_id(k) for k in predicted - set(built))
    assert not unreached and not lacking, f"kernels in the library that no case launches: {unreached}; kernels the plan picks that the library lacks: {lacking}"
    kinds = collections.Counter(k[0] for k in built)
    assert (kinds["generic"], kinds["pipe"], kinds["roll"]) == (18, 95, 60)
    assert len(cases) == 172 and sum(len(v) for v in cases.values()) == 2720


def test_exp_ranges_straddle_the_switch():
    """The two intensityAlpha values sit on either side of the kernels' run-time exp switch, |intensityAlpha * stepSize| <= 1/8:
    one just below it, one well above."""
    step = np.float32(K.step_size())
    small, large = (np.float32(K.EXP_RANGES[k]) for k in ("small", "large"))
    assert K.exp_small(small) and not K.exp_small(large)
    assert 0.124 < float(small * step) <= 0.125 and float(large * step) > 0.5


def test_fast_references_stay_inside_the_knife_edge_cap():
    """_fast_check (tests/test_gpu_parity.py) compares robust pixels at 1e-4 and demands that the oracle flags fewer than 1 %
    as knife-edge.  That condition is a property of the reference alone, so it is settled here for every FAST frame the GPU
    test uses: the scene was chosen to meet it."""
    seen = {}
    for cs in K.cases_by_kernel().values():
        for c in cs:
            if c.math == "fast":
                for r in K.EXP_RANGES:
                    seen.setdefault(K.reference_key(c, r), (c, r))
    assert len(seen) == 120
    for c, r in seen.values():
        ref, aux = K.reference(c, r)
        assert aux["fragile"].mean() < 0.01, (c, r, float(aux["fragile"].mean()))
        assert np.isfinite(ref).all()
        if c.mods or c.overlays != "none":
            assert (ref[..., :3].sum(axis=-1) > 0).mean() > 0.03, (c, r)        # the frame shows something


def test_skipping_cases_march_through_empty_space(cases):
    """Every configuration the plan marches with a skip map has a mask (grid_ref's restatement) that flags more than half of
    the volume's macro cells: the bar of test_skip_is_bit_identical."""
    seen = {}
    for cs in cases.values():
        for c in cs:
            if K.plan(c).skipping:
                seen.setdefault((c.mods, c.overlays), c)
    assert len(seen) == 12                               # 4 non-empty modality sets x 3 overlay choices
    for c in seen.values():
        frac = K.skippable_fraction(c)
        assert 0.5 < frac < 1.0, (c, frac)
