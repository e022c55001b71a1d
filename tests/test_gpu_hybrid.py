"""The hybrid sampler and the coordinate noise on the GPU (csrc/inr_hybrid.hip) against the restatement of
tests/hybrid_ref.py.  Every ABI call runs between guard blocks on 0x00- and 0xFF-filled buffers of exactly the stated sizes; the
two runs must give the same bits.  Class index == NumPy; select_largest == the stable-argsort rule; normal3 within one fp32 ulp
of the fp64 restatement (derived: see test_normal3_...); candidates and hybrid rows == the restatement, bit for bit; train_inject
with the new keys == the composition written out from the separate calls."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hybrid_cases as hc
import hybrid_ref as ref
from mrirt import _lib, inr
from test_gpu_inject import DEV, _ptr, _up, guarded

pytestmark = pytest.mark.gpu
NOTEBOOK_CW = [0.1, 1.5, 1.0, 2.0]


def _record(line):
    """Printed, and appended to the file MRIRT_FIGURES names (profiles/r25_hybrid/gpu_test_figures.txt was written that way)."""
    print(line)
    path = os.environ.get("MRIRT_FIGURES")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _label_cache(cases):
    """A VoxelCache of label volumes alone (no modalities)."""
    hwd = cases[0]["seg"].shape
    return inr.VoxelCache([{"mods": np.zeros((0, *hwd), np.float32), "seg": c["seg"]} for c in cases])


# ---- class index -----------------------------------------------------------------------------------------------------------------------
def _class_index_abi(cache, nc, ncases):
    lib = _lib.lib()

    def count(a):
        counts = a.alloc(8 * ncases * nc, torch.int64)
        assert lib.mrirt_inr_class_count(C.byref(cache.desc), nc, _ptr(counts), None) == 0
        return (counts,)
    counts = guarded(count)[0].reshape(ncases, nc)
    offsets = np.concatenate([[0], np.cumsum(counts.T.reshape(-1))]).astype(np.int64)
    total = int(offsets[-1])
    nbytes = int(lib.mrirt_inr_class_index_scratch_bytes(C.byref(cache.desc), nc))
    assert nbytes > 0
    d_off = _up(offsets, np.int64)

    def build(a):
        index = a.alloc(4 * max(total, 1), torch.int32)      # no voxel in range: the pointer must still be one
        scratch = a.alloc(nbytes)
        assert lib.mrirt_inr_class_index(C.byref(cache.desc), nc, _ptr(d_off), _ptr(index), _ptr(scratch), nbytes, None) == 0
        return (index[:total],)
    return counts, offsets, guarded(build)[0].view(np.uint32)


@pytest.mark.parametrize("nc", hc.INDEX_CLASSES)
@pytest.mark.parametrize("ncases", hc.INDEX_NCASES)
@pytest.mark.parametrize("hwd", hc.INDEX_SHAPES)
def test_class_index_equals_numpy(hwd, ncases, nc):
    cases = hc.index_cases(hwd, ncases, nc)
    want_index, want_offsets = ref.class_index(cases, nc)
    cache = _label_cache(cases)
    counts, offsets, index = _class_index_abi(cache, nc, ncases)
    assert np.array_equal(offsets, want_offsets) and np.array_equal(index, want_index)
    for c, case in enumerate(cases):
        assert counts[c].tolist() == [int((case["seg"] == k).sum()) for k in range(nc)]
    # the Python door: built once per num_classes and kept
    ci = cache.class_index(nc)
    assert ci is cache.class_index(nc) and ci.numClasses == nc and ci.reserved == 0
    assert np.array_equal(cache.class_offsets[nc].cpu().numpy(), want_offsets)
    assert np.array_equal(cache.class_voxels[nc].cpu().numpy().view(np.uint32)[:len(want_index)], want_index)


def test_class_index_of_a_volume_that_is_all_one_class_and_of_one_with_no_label_in_range():
    hwd = (17, 16, 16)
    for fill, nc in ((2, 4), (9, 4), (0, 1)):
        cases = [{"seg": np.full(hwd, fill, np.int16)} for _ in range(2)]
        want_index, want_offsets = ref.class_index(cases, nc)
        _, offsets, index = _class_index_abi(_label_cache(cases), nc, 2)
        assert np.array_equal(offsets, want_offsets) and np.array_equal(index, want_index)
        assert len(index) == (0 if fill >= nc else 2 * 17 * 16 * 16)


# ---- selection -------------------------------------------------------------------------------------------------------------------------
def _select(values, k):
    v = _up(values)

    def call(a):
        out = a.alloc(4 * k, torch.int32)
        assert _lib.lib().mrirt_select_largest(_ptr(v), len(values), k, _ptr(out), None) == 0
        return (out,)
    return guarded(call)[0].view(np.uint32)


@pytest.mark.parametrize("n", hc.SELECT_N)
def test_select_largest_equals_the_stable_argsort_rule(n):
    for pattern in hc.SELECT_PATTERNS:
        values = hc.select_values(pattern, n)
        for k in hc.select_ks(n):
            got = _select(values, k)
            assert np.array_equal(got, ref.select_largest(values, k)), (pattern, n, k)
    values = hc.select_values("specials", n, seed=1)
    k = hc.select_ks(n)[len(hc.select_ks(n)) // 2]
    assert np.array_equal(inr.select_largest(_up(values), k).cpu().numpy().view(np.uint32), ref.select_largest(values, k))


def test_select_largest_refuses_what_it_cannot_do():
    v = _up(np.zeros(8, np.float32))
    out = torch.empty(8, dtype=torch.int32, device=DEV)
    lib = _lib.lib()
    assert lib.mrirt_select_largest(_ptr(v), 65537, 1, _ptr(out), None) == -5 and lib.mrirt_select_largest(_ptr(v), 8, 0, _ptr(out), None) == -5
    with pytest.raises(_lib.MrirtError):
        inr.select_largest(v, 0)
    with pytest.raises(_lib.MrirtError):
        inr.select_largest(v, 9)


# ---- normals ---------------------------------------------------------------------------------------------------------------------------
def test_normal3_is_within_one_fp32_ulp_of_the_fp64_restatement():
    """The bound is derived, not measured: the device's fp64 log / sin / cos differ from NumPy's by a few fp64 ulps, 2^-26 of half
    an fp32 ulp, so the two fp64 values round to the same or to adjacent floats."""
    n = 65536
    differ = 0
    for seed, batch in ((5, 0), (2 ** 40 + 3, 2 ** 33 + 1)):
        def call(a):
            out = a.alloc(4 * 3 * n, torch.float32)
            assert _lib.lib().mrirt_inr_normal3(seed, batch, n, _ptr(out), None) == 0
            return (out,)
        got = guarded(call)[0].reshape(n, 3)
        want = ref.normal3(seed, batch, n)
        assert np.isfinite(got).all()
        ulp = np.spacing(np.maximum(np.abs(want), np.abs(got)).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
        differ += int((got != want).sum())
        assert _bits(inr.normal3(seed, batch, n)) == got.tobytes()
    _record(f"normal3: {differ} of {2 * 3 * n} values differ from the fp64 restatement rounded to fp32 (each by one ulp at most)")


# ---- candidates and hybrid rows --------------------------------------------------------------------------------------------------------
def _hybrid_abi(cache, classes, U, Pc, picks, sigma, fields, seed, batch, n):
    M = cache.n_modalities
    hy = _lib.InrHybrid()
    hy.nUncertain, hy.nPerClass, hy.noiseSigma, hy.reserved = U, Pc, sigma, 0
    d_picks = _up(np.asarray(picks, np.uint32).view(np.int32), np.int32) if U else None
    hy.picks = d_picks.data_ptr() if U else None

    def call(a):
        coords, labels = a.alloc(4 * 3 * n, torch.float32), a.alloc(4 * n, torch.int32)
        feats = a.alloc(4 * n * M, torch.float32) if M else None
        fo = a.alloc(4 * n, torch.float32) if fields else None
        rc = _lib.lib().mrirt_inr_sample_batch_hybrid(C.byref(cache.desc), C.byref(classes) if Pc else None, C.byref(hy),
                                                      _ptr(cache.boundary_table) if fields else None, seed, batch, n, _ptr(coords), _ptr(feats),
                                                      _ptr(labels), _ptr(fo), None)
        assert rc == 0, rc
        return coords, feats, labels, fo
    coords, feats, labels, fo = guarded(call)
    return coords.reshape(n, 3), (feats.reshape(n, M) if M else None), labels, fo


@pytest.mark.parametrize("M", [0, 4])
@pytest.mark.parametrize("ncases", [2, 3])
def test_candidates_and_hybrid_rows_equal_the_restatement(ncases, M):
    hwd, nc, n, n_cand = (9, 7, 6), 4, hc.ROW_N, 500
    cases = hc.sampler_cases(hwd, ncases, M, seed=ncases, empty_class=2)            # class 2 is nowhere: its rows take the fallback
    cache = inr.VoxelCache(cases)
    rng = np.random.default_rng(9)
    fields = [rng.normal(0, 1, hwd).astype(np.float32) for _ in range(ncases)]
    cache.set_boundary(fields)
    classes = cache.class_index(nc)
    index, offsets = ref.class_index(cases, nc)
    for seed, batch in ((5, 0), (2 ** 40 + 3, 2 ** 33 + 1)):
        def cand(a):
            coords, labels = a.alloc(4 * 3 * n_cand, torch.float32), a.alloc(4 * n_cand, torch.int32)
            feats = a.alloc(4 * n_cand * M, torch.float32) if M else None
            assert _lib.lib().mrirt_inr_sample_candidates(C.byref(cache.desc), seed, batch, n_cand, _ptr(coords), _ptr(feats), _ptr(labels), None) == 0
            return coords, feats, labels
        got = guarded(cand)
        want = ref.rows_of(cases, *ref.candidates(seed, batch, np.arange(n_cand), ncases, hwd))
        assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()
        assert (got[1] is None and M == 0) or got[1].tobytes() == want[1].tobytes()
        py = cache.sample_candidates(seed, batch, n_cand)
        assert _bits(py[0]) == want[0].tobytes() and _bits(py[2]) == want[2].tobytes() and tuple(py[1].shape) == (n_cand, M)
        plain = cache.sample(seed, batch, n)
        z = inr.normal3(seed, batch, n).cpu().numpy()
        for U, Pc in hc.ROW_CONFIGS:
            picks = rng.integers(0, n_cand, max(U, 4)).astype(np.uint32)
            picks[:4] = (0, n_cand - 1, 0, 0xFFFFFFFF)                                  # both ends, a repeat, a counter far outside the candidates
            coords, feats, labels, fo = _hybrid_abi(cache, classes, U, Pc, picks, 0.0, True, seed, batch, n)
            cs, x, y, zz, kind = ref.hybrid_rows(seed, batch, n, U, Pc, nc, picks, index, offsets, ncases, hwd)
            w_coords, w_feats, w_labels, w_field = ref.rows_of(cases, cs, x, y, zz, fields)
            assert coords.tobytes() == w_coords.tobytes() and labels.tobytes() == w_labels.tobytes() and fo.tobytes() == w_field.tobytes(), (U, Pc)
            assert M == 0 or feats.tobytes() == w_feats.tobytes()
            assert (kind[:U] == 0).all() and (kind[U + nc * Pc:] == 3).all()
            if Pc:
                assert (kind[U + 2 * Pc:U + 3 * Pc] == 2).all() and (kind[U:U + 2 * Pc] == 1).all() and (labels[U:U + Pc] == 0).all()
            uni = kind >= 2                                                            # uniform rows and fallbacks: VoxelCache.sample's
            assert coords[uni].tobytes() == plain[0].cpu().numpy()[uni].tobytes() and labels[uni].tobytes() == plain[2].cpu().numpy()[uni].tobytes()
            if U + nc * Pc == n:
                assert not (kind == 3).any()
            # the noise: on the bits normal3 returns, product and sum each rounded; labels, modalities and the field stay the voxel's
            for sigma in (0.3, 2.0 ** -20):
                nz = _hybrid_abi(cache, classes, U, Pc, picks, sigma, True, seed, batch, n)
                assert nz[0].tobytes() == ref.noisy(w_coords, sigma, z).tobytes(), (U, Pc, sigma)
                assert nz[2].tobytes() == labels.tobytes() and nz[3].tobytes() == fo.tobytes() and (M == 0 or nz[1].tobytes() == feats.tobytes())
            # the Python door, with and without the field
            py = cache.sample_hybrid(seed, batch, n, U, picks, Pc, nc, 0.0, with_field=True)
            assert _bits(py[0]) == coords.tobytes() and _bits(py[2]) == labels.tobytes() and _bits(py[3]) == fo.tobytes()
            py = cache.sample_hybrid(seed, batch, n, U, torch.from_numpy(picks.view(np.int32)).to(DEV) if U else None, Pc, nc, 0.3)
            assert len(py) == 3 and _bits(py[0]) == ref.noisy(w_coords, 0.3, z).tobytes()
    with pytest.raises(_lib.MrirtError):
        cache.sample_hybrid(1, 0, 100, 90, np.arange(90), 3, nc)                       # U + C P > n
    with pytest.raises(ValueError):
        cache.sample_hybrid(1, 0, 100, 5)                                               # picks missing


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _uncertainty_abi(desc, B, w, b, coords, mods, n, drop):
    lib = _lib.lib()
    nbytes = int(lib.mrirt_inject_scratch_bytes(C.byref(desc), n))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ent = torch.empty(n, dtype=torch.float32, device=DEV)
    rc = lib.mrirt_inject_uncertainty(C.byref(desc), _ptr(B), _ptr(w), _ptr(b), _ptr(coords), _ptr(mods), n, C.byref(drop), _ptr(ent), None,
                                      _ptr(scratch), nbytes, None)
    assert rc == 0, rc
    return ent


@pytest.mark.parametrize("unified", [True, False])
def test_train_inject_with_the_hybrid_keys_equals_the_composition_written_out(unified):
    rng = np.random.default_rng(12)
    hwd = (12, 10, 8)
    cases = [{"mods": rng.normal(0, 1, (4, *hwd)).astype(np.float32), "seg": (rng.integers(0, 4, hwd) * (rng.random(hwd) < 0.4)).astype(np.int16)}
             for _ in range(2)]
    seed, micro, accum, S = 21, 256, 2, 5
    config = dict(NUM_CLASSES=4, RNG_SEED=seed, FOURIER_DIM=16, HIDDEN_DIMS=[17, 16, 13], COORD_INJECTION_LAYERS=[1, 2, 3], MODALITY_INJECTION_LAYERS=[2],
                  DROPOUT_RATE=0.3, MICRO_BATCH_SIZE=micro, ACCUM_STEPS=accum, STAGE1_STEPS=2, STAGE2_STEPS=2, LR_STAGE1=2e-3, LR_STAGE2=5e-4, MIN_LR=1e-5,
                  WARMUP_STEPS=0, WEIGHT_DECAY=1e-4, CLIP_NORM=1.0, CLASS_WEIGHTS=NOTEBOOK_CW, DICE_WEIGHT=0.5, UNCERTAINTY_RATIO=0.5, BALANCED_RATIO=0.3,
                  UNIFORM_RATIO=0.2, COORD_NOISE_SIGMA_INIT=0.02, COORD_NOISE_SIGMA_FINAL=0.005)
    if unified:
        config.update(UNIFIED_FOCAL_GAMMA=0.5, UNIFIED_FOCAL_LAMBDA=0.5, TV_WEIGHT_STAGE1=0.02, TV_WEIGHT_STAGE2=0.05, BOUNDARY_WEIGHT=0.1)
    with pytest.raises(ValueError, match="TUMOR_RATIO"):
        inr.train_inject(dict(config, TUMOR_RATIO=0.25), cases)
    cache = inr.VoxelCache(cases)
    params, state = inr.train_inject(config, cache)
    cl, ml = (1, 2, 3), (2,)
    p0 = inr.inject_init(seed, 16, 4, [17, 16, 13], 4, cl, ml)
    desc = inr.inject_desc(p0, cl, ml)
    B, w, b = inr._inject_flat(p0, DEV)
    nw = w.numel()
    wB = torch.cat([w, B.reshape(-1)])
    st = inr.AdamWState([], wB, b, torch.zeros_like(wB), torch.zeros_like(b), torch.zeros_like(wB), torch.zeros_like(b), 0)
    gwB, gb = torch.empty_like(wB), torch.empty_like(b)
    scratch = inr.inject_train_scratch(desc, micro, DEV)
    sched = inr.two_stage_schedule(2, 2, 2e-3, 5e-4, 0, 1e-5)
    keep = float(np.float32(1.0) - np.float32(0.3))
    other = inr.VoxelCache(cases)
    other.set_boundary()
    losses, shapes = [], []
    for t in range(4):
        ratio = 0.5 if t < 2 else 0.75
        U, Pc, n_cand = ref.hybrid_counts(micro, ratio, 0.3, 4, t > 0)
        Pc = min(Pc, (micro - U) // 4)                       # stage 2: 192 + 4 x 19 > 256, the balanced segment is cut to fit
        shapes.append((U, Pc, n_cand))
        p = t / 4
        sigma = float(np.float32(0.02 * (1.0 - p) + 0.005 * p))
        cfg = inr.unified_loss(NOTEBOOK_CW, 0.5, 0.5, tv_weight=0.02 if t < 2 else 0.05, boundary_weight=0.1)
        per = []
        for k in range(accum):
            g = accum * t + k
            picks = None
            if U:
                cc, cm, _ = other.sample_candidates(seed, g, n_cand)
                drop_u = inr.inject_dropout(seed + 1, keep, S, (g * S) % (2 ** 24 - S), 0)
                picks = inr.select_largest(_uncertainty_abi(desc, wB[nw:], wB[:nw], b, cc, cm, n_cand, drop_u), U)
            c, m, lab, bw = other.sample_hybrid(seed, g, micro, U, picks, Pc, 4, sigma, with_field=True)
            drop = inr.inject_dropout(seed, keep, 1, g, 0) if t > 0 else None
            logits = inr.inject_forward_train(desc, wB[nw:], wB[:nw], b, c, m, micro, scratch, drop)
            if unified:
                loss, _, dl = inr.unified_loss_and_dlogits(logits, lab, cfg, bw)
            else:
                loss, _, dl, *_ = inr.loss_and_dlogits(logits, lab, [float(v) for v in NOTEBOOK_CW], 0.5, scratch)
            inr.inject_backward(desc, wB[nw:], wB[:nw], c, m, micro, dl, scratch, drop, gwB[nw:], gwB[:nw], gb, accumulate=k > 0)
            per.append(loss)
        inr.adamw_step(st, gwB, gb, sched(t), 1.0 / accum, 1.0, weight_decay=1e-4)
        losses.append(float(torch.stack(per).mean()))
    assert shapes == [(0, 19, 0), (128, 19, 1280), (192, 16, 1920), (192, 16, 1920)]
    opt = state["opt"]
    assert opt.step == 4
    for k in ("w", "b", "mu_w", "mu_b", "nu_w", "nu_b"):
        assert _bits(getattr(opt, k)) == _bits(getattr(st, k)), k
    assert state["loss_history"] == losses and all(np.isfinite(losses))
    assert params["fourier"]["B"].reshape(-1).tobytes() == wB[nw:].cpu().numpy().tobytes()
    # the keys do something: without them the same config trains on other batches
    plain = {k: v for k, v in config.items() if k not in ("UNCERTAINTY_RATIO", "BALANCED_RATIO", "UNIFORM_RATIO", "COORD_NOISE_SIGMA_INIT",
                                                          "COORD_NOISE_SIGMA_FINAL")}
    _, state0 = inr.train_inject(plain, inr.VoxelCache(cases))
    assert state0["loss_history"] != losses
    # the noise keys alone: uniform rows, displaced
    _, state1 = inr.train_inject({k: v for k, v in config.items() if k not in ("UNCERTAINTY_RATIO", "BALANCED_RATIO", "UNIFORM_RATIO")},
                                 inr.VoxelCache(cases))
    assert state1["loss_history"][0] != state0["loss_history"][0] and state1["loss_history"] != losses
