"""mrirt_unified_loss and mrirt_inr_sample_field on the GPU.  Every call of the loss runs between guard
blocks on 0x00- and 0xFF-filled buffers with a scratch of exactly mrirt_unified_loss_scratch_bytes(n); the two runs must give
the same bits.  Exact tier: accuracy, boundary term, argmax ties, labels outside the range.  Gate tier: the closed-interval
clips.  Tolerance tier: loss, aux and dlogits against the fp64 restatement (tests/unified_loss_ref.py) within the tolerances of
tests/unified_loss_cases.py.  Then the field gather, the Python composition and train_inject with the unified keys."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import unified_loss_cases as uc
import unified_loss_ref as ref
from mrirt import _lib, inr
from test_gpu_inject import DEV, _ptr, _up, guarded

pytestmark = pytest.mark.gpu
NOTEBOOK_CW = uc.NOTEBOOK_CW


def struct_of(cfg):
    return inr.unified_loss(cfg["cw"], cfg["gamma"], cfg["lam"], cfg["alpha"], cfg["beta"], cfg["ufl_w"], cfg["dice_w"], cfg["tv_w"], cfg["bd_w"])


def run(z, labels, bw, cfg, want_grad=True):
    """(loss (1,), aux (8 + C,), dlogits (n, C) or None) of one guarded call."""
    n, nc = z.shape
    x = struct_of(cfg)
    nbytes = int(_lib.lib().mrirt_unified_loss_scratch_bytes(n))
    assert nbytes > 0

    def call(arena):
        logits = arena.alloc(4 * n * nc, torch.float32); logits.copy_(_up(z).reshape(-1))
        lab = arena.alloc(4 * n, torch.int32); lab.copy_(_up(labels, np.int32))
        w = None
        if bw is not None:
            w = arena.alloc(4 * n, torch.float32); w.copy_(_up(bw))
        loss, aux = arena.alloc(4, torch.float32), arena.alloc(4 * (8 + nc), torch.float32)
        dl = arena.alloc(4 * n * nc, torch.float32) if want_grad else None
        scratch = arena.alloc(nbytes)
        rc = _lib.lib().mrirt_unified_loss(_ptr(logits), _ptr(lab), _ptr(w), n, nc, C.byref(x), _ptr(loss), _ptr(aux), _ptr(dl), _ptr(scratch),
                                           nbytes, None)
        assert rc == 0, rc
        return loss, aux, dl

    loss, aux, dl = guarded(call)
    return loss, aux, (dl.reshape(n, nc) if dl is not None else None)


def exact_inputs(n, C, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(0, 3, (n, C)).astype(np.float32)
    z[::5] = np.round(z[::5])                                # ties among small integers ...
    if C > 2:
        z[1::7, 1] = z[1::7].max(1) + 1
        z[1::7, C - 1] = z[1::7, 1]                          # ... and a tie of the largest between index 1 and the last
    z[2::11] = 0.0                                           # all equal: index 0
    labels = rng.integers(0, C, n).astype(np.int32)
    labels[3::13] = C
    labels[4::17] = -1
    labels[5::19] = np.iinfo(np.int32).max
    labels[6::23] = np.iinfo(np.int32).min
    bw = (rng.integers(0, 17, n) / 16.0).astype(np.float32)
    return z, labels, bw


@pytest.mark.parametrize("n,C", [(1, 4), (255, 3), (256, 1), (257, 16), (4000, 4), (65537, 4)])
def test_exact_tier_accuracy_boundary_and_argmax_ties(n, C):
    z, labels, bw = exact_inputs(n, C, 100 + n)
    cfg = ref.config([1.0] * C)
    loss, aux, _ = run(z, labels, bw, cfg, want_grad=False)
    am = np.argmax(z, 1).astype(np.int64)                    # NumPy takes the first index of the largest
    if n > 12 and C > 2:
        assert (am[2::11] == 0).all() and (am[1::7][z[1::7, 0] < z[1::7, 1]] == 1).all()
    lab = labels.astype(np.int64)
    acc = int((am == lab).sum())
    bd = float((bw.astype(np.float64) * np.abs(am - lab).astype(np.float64)).sum())      # dyadic weights times integers: exact in fp64
    assert aux[7] == np.float32(acc / n), (aux[7], acc / n)
    assert aux[5] == np.float32(bd / n), (aux[5], bd / n)
    assert np.isfinite(loss).all() and np.isfinite(aux).all()
    # without boundary weights the boundary term is +0 and nothing else moves
    loss0, aux0, _ = run(z, labels, None, cfg, want_grad=False)
    assert aux0[5] == 0 and not np.signbit(aux0[5]) and np.delete(aux0, 5).tobytes() == np.delete(aux, 5).tobytes()


def test_labels_outside_the_range_count_for_the_boundary_term_only():
    n, C = 300, 4
    z, _, bw = exact_inputs(n, C, 7)
    labels = np.where(np.arange(n) % 2 == 0, C + (np.arange(n) % 5), -1 - (np.arange(n) % 3)).astype(np.int32)
    cfg = ref.config(NOTEBOOK_CW)
    loss, aux, dl = run(z, labels, bw, cfg)
    am = np.argmax(z, 1).astype(np.int64)
    assert aux[2] == 0 and aux[7] == 0                       # FL and Acc: no point contributes
    assert aux[1] == np.float32((1.0 + 1e-7) ** (1.0 / cfg["gamma"]))      # T = A = 0: TI = 0 for every class
    assert aux[5] == np.float32(float((bw.astype(np.float64) * np.abs(am - labels.astype(np.int64))).sum()) / n) and aux[5] > 0
    _, a64, g64, tot = ref.forward(z, labels, bw, cfg)
    assert not tot["T"].any() and not tot["A"].any()
    assert np.abs(aux[8:] - a64["dice_per_class"]).max() < 1e-6 and np.isfinite(dl).all() and np.abs(dl).max() > 0


def test_gate_tier_closed_interval_clips():
    C = 4
    z = np.float32([[12.0, 0.5, -1.0, 0.25], [-12.0, 0.5, -1.0, 0.25], [20.0, -20.0, 1.0, 0.0], [0.5, 20.0, 12.0, -12.0],
                    [10.0, 0.5, -10.0, 0.25], [1.0, 2.0, -0.5, 0.0], [0.3, -0.2, 0.1, 2.0], [25.0, 20.0, 20.0, 20.0]])
    labels = np.int32([0, 1, 2, 3, 0, 1, 2, 3])
    outside = np.abs(z) > 10
    for tv in (0.0, 0.02):
        cfg = ref.config(NOTEBOOK_CW, tv_w=tv)
        _, _, dl = run(z, labels, None, cfg)
        if tv == 0.0:
            assert (dl[outside] == 0).all(), dl                  # beyond the clip: nothing from the pc paths
            assert (dl[4] != 0).all() and (dl[~outside] != 0).all()      # at exactly +-10 the gradient passes (closed interval)
            pc_only = dl
        else:
            assert (dl[outside][np.abs(z[outside]) < 15] != 0).any() and (dl[:2][outside[:2]] != 0).all()      # the TV path is still there
    # the same rule in the restatement: an open and a closed element differ there as they do here
    g0 = ref.forward(z, labels, None, ref.config(NOTEBOOK_CW, tv_w=0.0))[2]
    assert ((g0 == 0) == (pc_only == 0)).all()


def _record(line):
    print(line)
    path = os.environ.get("MRIRT_FIGURES")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("case", uc.TOLERANCE_CASES, ids=[c[0] for c in uc.TOLERANCE_CASES])
def test_tolerance_tier_against_the_fp64_restatement(case):
    name, n, C, seed, scale, cw, gamma, lam, tv, bd, features = case
    z, labels, bw = uc.make_inputs(n, C, seed, scale, features)
    cfg = ref.config(cw, gamma, lam, tv_w=tv, bd_w=bd)
    tol_s, tol_g = uc.TOLERANCES[name]
    loss, aux, dl = run(z, labels, bw, cfg)
    l64, a64, g64, _ = ref.forward(z, labels, bw, cfg)
    _, A = ref.closed_form(z, labels, bw, cfg)
    got, want = np.concatenate([loss, aux]).astype(np.float64), np.concatenate([[l64], ref.aux_vector(a64)])
    dev_s = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    ok = A > 0
    dev_g = np.abs(dl - g64)[ok] / A[ok] if ok.any() else np.zeros(1)
    _record(f"{name}: scalars worst {dev_s.max():.3e} (tol {tol_s:.3e}); dlogits worst {dev_g.max():.3e} of A (tol {tol_g:.3e}), "
            f"{int(ok.sum())} of {A.size} elements")
    assert np.isfinite(got).all() and np.isfinite(dl).all()
    assert (dev_s <= tol_s).all(), (dev_s, tol_s)
    assert (np.abs(dl - g64) <= tol_g * A).all(), float(dev_g.max())
    # the loss without its gradient: the same bits
    loss2, aux2, none = run(z, labels, bw, cfg, want_grad=False)
    assert none is None and loss2.tobytes() == loss.tobytes() and aux2.tobytes() == aux.tobytes()


def test_a_row_with_a_non_finite_logit_takes_no_part():
    """What include/mrirt.h documents: such a row adds nothing to any sum, its gradient row is +0, the loss stays finite."""
    case = next(c for c in uc.TOLERANCE_CASES if c[0] == "n256_c4")
    name, n, C, seed, scale, cw, gamma, lam, tv, bd, features = case
    z, labels, bw = uc.make_inputs(n, C, seed, scale, features)
    cfg = ref.config(cw, gamma, lam, tv_w=tv, bd_w=bd)
    rows = [0, 77, 255]
    z[0, 1], z[77, 3], z[255, 0] = np.nan, np.inf, -np.inf
    loss, aux, dl = run(z, labels, bw, cfg)
    assert np.isfinite(loss).all() and np.isfinite(aux).all() and np.isfinite(dl).all()
    assert dl[rows].tobytes() == np.zeros((3, C), np.float32).tobytes()
    l64, a64, g64, _ = ref.forward(z, labels, bw, cfg)
    _, A = ref.closed_form(z, labels, bw, cfg)
    tol_s, tol_g = uc.TOLERANCES[name]
    want = np.concatenate([[l64], ref.aux_vector(a64)])
    assert (np.abs(np.concatenate([loss, aux]) - want) <= tol_s * np.maximum(np.abs(want), 1.0)).all()
    assert (np.abs(dl - g64) <= tol_g * A).all()
    # whatever else such a row holds -- other logits, its label, its boundary weight -- no output bit depends on it
    z2, labels2, bw2 = z.copy(), labels.copy(), bw.copy()
    z2[0, 0], z2[77, :3], labels2[rows], bw2[rows] = 9.0, 50.0, [3, 99, -4], 7.0
    loss2, aux2, dl2 = run(z2, labels2, bw2, cfg)
    assert loss2.tobytes() == loss.tobytes() and aux2.tobytes() == aux.tobytes() and dl2.tobytes() == dl.tobytes()


# ---- field gather --------------------------------------------------------------------------------------------------------------------
def _cases(hwd, ncases, seed):
    rng = np.random.default_rng(seed)
    vox = int(np.prod(hwd))
    cases = []
    for c in range(ncases):
        ident = (c * 100000 + np.arange(vox)).reshape(hwd).astype(np.float32)      # modality 0 names the case and the voxel
        seg = np.zeros(hwd, np.int16) if c == 0 else (rng.integers(0, 4, hwd) * (rng.random(hwd) < 0.3)).astype(np.int16)
        cases.append({"mods": np.stack([ident, rng.normal(0, 1, hwd).astype(np.float32)]), "seg": seg})
    return cases


@pytest.mark.parametrize("hwd,ncases,n,n_tumour", [((5, 4, 3), 2, 300, 0), ((5, 4, 3), 2, 300, 120), ((5, 4, 3), 2, 257, 257), ((9, 7, 6), 3, 1000, 400)])
def test_sample_field_reads_the_voxels_the_sampler_draws(hwd, ncases, n, n_tumour):
    cases = _cases(hwd, ncases, 3)
    cache = inr.VoxelCache(cases)
    rng = np.random.default_rng(4)
    fields = [rng.normal(0, 1, hwd).astype(np.float32) for _ in range(ncases)]
    kept = cache.set_boundary(fields)
    assert len(kept) == ncases and cache.boundary_table.dtype == torch.int64
    for seed, batch in ((5, 0), (2 ** 40 + 3, 2 ** 33 + 1)):
        coords, feats, labels = cache.sample(seed, batch, n, n_tumour)
        got = cache.sample_field(seed, batch, n, n_tumour).cpu().numpy()
        c = coords.cpu().numpy().astype(np.float64)
        xyz = [np.round((c[:, a] + 1) / 2 * (hwd[a] - 1)).astype(np.int64) for a in range(3)]
        ident = feats[:, 0].cpu().numpy().astype(np.int64)
        cs, vox = ident // 100000, ident % 100000
        assert np.array_equal(vox, (xyz[0] * hwd[1] + xyz[1]) * hwd[2] + xyz[2])
        want = np.stack(fields)[cs, xyz[0], xyz[1], xyz[2]]
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
        lab = labels.cpu().numpy()
        if n_tumour:
            assert (lab[:n_tumour][cs[:n_tumour] != 0] > 0).all() and (cs[:n_tumour] == 0).any()      # from the index; case 0 fires the fallback fill
            assert (lab[cs == 0] == 0).all()
    with pytest.raises(ValueError):
        cache.set_boundary(fields[:1] if ncases > 1 else [fields[0][:2]])


def test_set_boundary_builds_the_maps_of_boundary_weights():
    cases = _cases((9, 7, 6), 3, 8)
    cache = inr.VoxelCache(cases)
    with pytest.raises(ValueError):
        cache.sample_field(1, 0, 10)
    maps = cache.set_boundary()
    for m, case in zip(maps, cases):
        assert m.cpu().numpy().tobytes() == inr.boundary_weights(case["seg"]).cpu().numpy().tobytes() and tuple(m.shape) == (9, 7, 6)
    assert not maps[0].any() and float(maps[1].max()) == 1.0
    got = cache.sample_field(9, 2, 500)
    assert got.shape == (500,) and float(got.max()) <= 1.0 and float(got.min()) >= 0.0 and float(got.max()) > 0


# ---- Python composition ------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def test_make_inject_loss_and_grad_with_the_unified_loss_equals_the_separate_calls():
    rng = np.random.default_rng(2)
    n, cl, ml = 500, (1, 2), (2,)
    params = inr.inject_init(3, 16, 2, [17, 16, 13], 4, cl, ml)
    coords = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    mods = rng.normal(0, 1, (n, 2)).astype(np.float32)
    labels = rng.integers(0, 4, n).astype(np.int32)
    bw = rng.random(n).astype(np.float32)
    cfg = inr.unified_loss(NOTEBOOK_CW, tv_weight=0.05)
    drop = inr.inject_dropout(5, 0.7, 1, 2, 9)
    fn = inr.make_inject_loss_and_grad(4, NOTEBOOK_CW, 0.0, cl, ml, ext=cfg)
    (loss, aux), grads = fn(params, coords, mods, labels, dropout=drop, boundary_weights=bw)
    desc = inr.inject_desc(params, cl, ml)
    B, w, b = inr._inject_flat(params, DEV)
    c, m, lab = _up(coords), _up(mods), _up(labels, np.int32)
    scratch = inr.inject_train_scratch(desc, n, DEV)
    logits = inr.inject_forward_train(desc, B, w, b, c, m, n, scratch, drop)
    want_loss, want_aux, dl = inr.unified_loss_and_dlogits(logits, lab, cfg, _up(bw))
    gB, gw, gb = inr.inject_backward(desc, B, w, c, m, n, dl, scratch, drop)
    assert _bits(loss) == _bits(want_loss) and loss.dim() == 0
    assert sorted(aux) == sorted(["ufl", "mFTL", "mFL", "dice_loss", "tv_loss", "boundary_loss", "dice_per_class", "dice_mean_tumor", "accuracy"])
    for k in aux:
        assert _bits(aux[k]) == _bits(want_aux[k]), k
    assert tuple(aux["dice_per_class"].shape) == (4,) and float(aux["boundary_loss"]) > 0
    assert _bits(grads["fourier"]["B"]) == _bits(gB)
    assert _bits(torch.cat([g["W"].reshape(-1) for g in grads["mlp"]])) == _bits(gw)
    assert _bits(torch.cat([g["b"] for g in grads["mlp"]])) == _bits(gb)
    assert float(gw.abs().sum()) > 0 and float(gB.abs().sum()) > 0
    # no boundary weights: the boundary term is 0; and the other losses are what they were
    (loss0, aux0), _ = fn(params, coords, mods, labels, dropout=drop)
    assert float(aux0["boundary_loss"]) == 0.0 and _bits(aux0["ufl"]) == _bits(aux["ufl"])
    (_, plain), _ = inr.make_inject_loss_and_grad(4, NOTEBOOK_CW, 0.3, cl, ml)(params, coords, mods, labels)
    assert sorted(plain) == ["ce_per_class", "dice_per_class"]


def test_train_inject_with_the_unified_keys_equals_the_composition_written_out():
    rng = np.random.default_rng(12)
    hwd = (12, 10, 8)
    case = {"mods": rng.normal(0, 1, (4, *hwd)).astype(np.float32), "seg": (rng.integers(0, 4, hwd) * (rng.random(hwd) < 0.4)).astype(np.int16)}
    config = dict(NUM_CLASSES=4, RNG_SEED=21, FOURIER_DIM=16, HIDDEN_DIMS=[17, 16, 13], COORD_INJECTION_LAYERS=[1, 2, 3], MODALITY_INJECTION_LAYERS=[2],
                  DROPOUT_RATE=0.3, MICRO_BATCH_SIZE=300, ACCUM_STEPS=2, STAGE1_STEPS=2, STAGE2_STEPS=2, LR_STAGE1=2e-3, LR_STAGE2=5e-4, MIN_LR=1e-5,
                  WARMUP_STEPS=1, WEIGHT_DECAY=1e-4, CLIP_NORM=1.0, CLASS_WEIGHTS=NOTEBOOK_CW, UNIFIED_FOCAL_GAMMA=0.5, UNIFIED_FOCAL_LAMBDA=0.5,
                  TV_WEIGHT_STAGE1=0.02, TV_WEIGHT_STAGE2=0.05, BOUNDARY_WEIGHT=0.1, TUMOR_RATIO=0.25)
    cache = inr.VoxelCache([case])
    logged = []
    params, state = inr.train_inject(config, cache, log=lambda s, m: logged.append((s, m)))
    assert _bits(cache.boundary[0]) == _bits(inr.boundary_weights(case["seg"]))
    cl, ml = (1, 2, 3), (2,)
    p0 = inr.inject_init(21, 16, 4, [17, 16, 13], 4, cl, ml)
    desc = inr.inject_desc(p0, cl, ml)
    B, w, b = inr._inject_flat(p0, DEV)
    nw = w.numel()
    wB = torch.cat([w, B.reshape(-1)])
    st = inr.AdamWState([], wB, b, torch.zeros_like(wB), torch.zeros_like(b), torch.zeros_like(wB), torch.zeros_like(b), 0)
    gwB, gb = torch.empty_like(wB), torch.empty_like(b)
    scratch = inr.inject_train_scratch(desc, 300, DEV)
    sched = inr.two_stage_schedule(2, 2, 2e-3, 5e-4, 1, 1e-5)
    keep = float(np.float32(1.0) - np.float32(0.3))
    nt = inr.n_tumour_of(300, 0.25)
    assert 0 < nt < 300
    other = inr.VoxelCache([case])
    other.set_boundary()
    losses, tvs, dropped = [], [], 0
    for t in range(4):
        cfg = inr.unified_loss(NOTEBOOK_CW, 0.5, 0.5, tv_weight=0.02 if t < 2 else 0.05, boundary_weight=0.1)
        per, per_tv = [], []
        for k in range(2):
            g = 2 * t + k
            c, m, lab = other.sample(21, g, 300, nt)
            bw = other.sample_field(21, g, 300, nt)
            drop = inr.inject_dropout(21, keep, 1, g, 0) if t > 1 else None
            dropped += drop is not None
            logits = inr.inject_forward_train(desc, wB[nw:], wB[:nw], b, c, m, 300, scratch, drop)
            loss, aux, dl = inr.unified_loss_and_dlogits(logits, lab, cfg, bw)
            inr.inject_backward(desc, wB[nw:], wB[:nw], c, m, 300, dl, scratch, drop, gwB[nw:], gwB[:nw], gb, accumulate=k > 0)
            per.append(loss)
            per_tv.append(aux["tv_loss"])
        inr.adamw_step(st, gwB, gb, sched(t), 0.5, 1.0, weight_decay=1e-4)
        losses.append(float(torch.stack(per).mean()))
        tvs.append(float(torch.stack(per_tv).mean()))
    assert dropped == 4
    opt = state["opt"]
    assert opt.step == 4 and [s for s, _ in logged] == [1, 2, 3, 4]
    for k in ("w", "b", "mu_w", "mu_b", "nu_w", "nu_b"):
        assert _bits(getattr(opt, k)) == _bits(getattr(st, k)), k
    assert state["loss_history"] == losses == [m["train/loss"] for _, m in logged]
    assert [m["train/tv_loss"] for _, m in logged] == tvs
    for _, m in logged:
        assert {"train/ufl", "train/dice_loss", "train/tv_loss", "train/boundary_loss", "train/lr", "train/step"} <= set(m)
        assert all(np.isfinite(v) for v in m.values())
    assert ref.same_bits(params["fourier"]["B"].reshape(-1), wB[nw:].cpu().numpy())
    assert not ref.same_bits(params["mlp"][1]["W"], p0["mlp"][1]["W"])
    # the TV weight did switch: with 0.02 throughout, step 3 sees other gradients
    flat = dict(config, TV_WEIGHT_STAGE2=0.02)
    _, state2 = inr.train_inject(flat, inr.VoxelCache([case]))
    assert state2["loss_history"][:2] == losses[:2] and state2["loss_history"][2:] != losses[2:]
