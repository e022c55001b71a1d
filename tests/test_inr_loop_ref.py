"""The definitions of the INR training loop as inr_loop_ref.py restates them, checked on the CPU against
known answers, the reference's own indexing, closed forms and torch.optim.AdamW."""
import math

import numpy as np
import pytest
import torch

import inr_loop_cases as cases
import inr_loop_ref as ref

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = ref.philox4x32_10(counter, key)
    assert tuple(int(v) for v in got) == want


def reference_sample_voxels(cache, case_indices, h_coords, w_coords, d_coords):
    """StreamingBraTSCache.sample_voxels (inr/inr/dataloader.py:86-96), restated."""
    N, M = len(case_indices), cache[0]["mods"].shape[0]
    mods_out, segs_out = np.zeros((N, M), np.float32), np.zeros(N, np.int16)
    for i in range(N):
        h, w, d = h_coords[i], w_coords[i], d_coords[i]
        mods_out[i] = cache[case_indices[i]]["mods"][:, h, w, d]
        segs_out[i] = cache[case_indices[i]]["seg"][h, w, d]
    return mods_out, segs_out


def test_sampler_is_the_references_indexing():
    cs = cases.cache_cases("addr")
    n = 500
    coords, feats, labels, (ci, x, y, z) = ref.sample(cs, 12345, 3, n)
    mods, seg = reference_sample_voxels(cs, ci, x, y, z)
    assert np.array_equal(feats, mods) and np.array_equal(labels, seg.astype(np.int32))
    # the voxels encode their own address: the draw, the gather and the encoding agree
    for m in range(2):
        assert np.array_equal(feats[:, m], ((((ci * 2 + m) * 3 + x) * 5 + y) * 7 + z).astype(np.float32))
    assert np.array_equal(labels, ci * 105 + (x * 5 + y) * 7 + z)
    assert ci.min() == 0 and ci.max() == 1 and x.max() == 2 and y.max() == 4 and z.max() == 6
    want = np.stack([x / 2.0, y / 4.0, z / 6.0], 1) * 2.0 - 1.0            # sample_batch's arithmetic (dataloader.py:149-150)
    assert coords.dtype == np.float32 and np.abs(coords - want).max() <= 2.0 ** -23
    assert coords.min() == -1.0 and coords.max() == 1.0


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_sampler_is_uniform(seed):
    n, cells = 65536, 2 * 3 * 5 * 7
    ci, x, y, z = ref.draw(seed, 0, n, 2, (3, 5, 7))
    counts = np.bincount(((ci * 3 + x) * 5 + y) * 7 + z, minlength=cells)
    assert counts.size == cells and counts.min() > 0
    chi2 = float(((counts - n / cells) ** 2 / (n / cells)).sum())
    print(f"seed {seed}: cell counts {counts.min()}..{counts.max()}, chi2 {chi2:.1f}")
    assert chi2 < 277.0                                  # the 99.9 % point of chi2 with 209 degrees of freedom


def test_schedule_closed_forms():
    peak, end, warmup, decay = 1e-3, 1e-5, 10, 110
    T = decay - warmup
    f = lambda t: ref.lr_schedule(peak, end, warmup, decay, t)
    assert f(0) == 0.0
    assert f(5) == peak * 5 / 10
    assert f(warmup) == peak
    assert math.isclose(f(warmup + T // 2), 0.5 * (peak + end), rel_tol=1e-15)
    assert math.isclose(f(warmup + T), end, rel_tol=1e-13)
    assert f(warmup + T + 1000) == f(warmup + T)
    assert all(f(t) > f(t + 1) for t in range(warmup, warmup + T))
    assert ref.lr_schedule(peak, end, 0, 50, 0) == peak                       # warmup = 0 skips the ramp
    for w, d in ((10, 10), (10, 5), (1, 1)):
        with pytest.raises(ValueError):
            ref.lr_schedule(peak, end, w, d, 0)


def test_library_schedule_and_python_schedule_are_the_restatement():
    import ctypes as C
    from mrirt import _lib, inr
    lib = _lib.lib()
    out = C.c_double()
    for peak, end, w, d in ((1e-3, 1e-5, 10, 110), (5e-3, 1e-4, 2, 12), (3e-4, 0.0, 0, 7)):
        for t in list(range(0, d + 3)) + [10 ** 9]:
            assert lib.mrirt_inr_lr_schedule(peak, end, w, d, t, C.byref(out)) == 0
            assert out.value == ref.lr_schedule(peak, end, w, d, t) == inr.lr_schedule(peak, end, w, d, t), (peak, w, d, t)
    with pytest.raises(ValueError):
        inr.lr_schedule(1e-3, 1e-5, 10, 10, 0)
    with pytest.raises(ValueError):
        inr.train_inr(dict(cases.E2E_CONFIG, WARMUP_STEPS=20), [])          # decay_steps - warmup = 0: refused before any work


def test_optimiser_is_decoupled_adamw():
    rng = np.random.default_rng(5)
    n, lr = 257, 3e-3
    p0 = rng.standard_normal(n)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([tp], lr=lr, betas=(ref.B1, ref.B2), eps=ref.EPS, weight_decay=ref.WD)
    p, mu, nu = p0.copy(), np.zeros(n), np.zeros(n)
    for t in range(5):
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-4, 2, n)
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, mu, nu = ref.adamw_update(p, mu, nu, g, 1.0, lr, t, dtype=np.float64)
        err = np.abs(p - tp.detach().numpy()).max() / np.abs(p).max()
        assert err <= 1e-12, (t, err)


def test_clip_branch():
    clip = 0.5
    gw, gb = np.array([0.0, 0.6, 0.0], np.float32), np.array([0.8], np.float32)      # norm 1 = 2 clip up to fp32 rounding of .6, .8
    norm = ref.gnorm(gw, gb)
    assert abs(norm - 2 * clip) < 1e-7
    s = ref.clip_factor(norm, clip)
    assert s.dtype == np.float32 and s == np.float32(clip / norm) and abs(float(s) - 0.5) < 1e-7
    assert ref.clip_factor(0.4, clip) == np.float32(1.0)
    assert ref.clip_factor(norm, 0.0) == np.float32(1.0) and ref.clip_factor(norm, float("inf")) == np.float32(1.0)
    assert np.isnan(ref.clip_factor(float("inf"), clip)) and np.isnan(ref.clip_factor(float("nan"), clip))
    # the clipped gradient has norm clip, and the first update moves every touched parameter by lr against its sign
    gc = np.concatenate([gw, gb]) * s
    assert abs(math.sqrt(float((gc.astype(np.float64) ** 2).sum())) - clip) < 1e-7
    p, mu, nu = ref.adamw_update(np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32), np.concatenate([gw, gb]), s, 1e-2, 0)
    assert np.allclose(p, [0.0, -1e-2, 0.0, -1e-2], rtol=1e-5, atol=0) and p[0] == 0.0
    assert np.allclose(mu, 0.1 * gc, rtol=1e-6) and np.allclose(nu, 0.001 * gc * gc, rtol=1e-5)
    assert ref.gnorm(np.array([3.0, 4.0], np.float32), np.array([12.0], np.float32), 0.5) == 6.5


def test_recorded_measurements_hold():
    assert cases.TRAJ_NEAR_KINK <= 0.02 and cases.E2E_SPARE >= 1.5
    assert 0 < cases.TRAJ_TOL["params"] <= 5e-3 and 0 < cases.TRAJ_TOL["losses"] <= 5e-3
