"""The fused forward of the coordinate-injection INR (csrc/inr_inject_fused.hip) on the GPU: logits and
classes are held to BIT equality with the NumPy restatement (tests/inject_ref.py) where that is exact and with the chain
mrirt_inject_forward everywhere -- no tolerance anywhere in this file.  Outputs lie between guard blocks; the row count comes
from the host or from a device word."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import inject_cases as ic
import inject_ref as ref
from mrirt import _lib, inr
from test_gpu_inject import GUARD, Net, _ptr, _up, desc_of, forward

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARG, NULL = -5, -1
FILL = 0x7B
REQUIRED = ["n1_F2_M0_L2", "n63_F14_M1_L3_coords", "n64_F16_M4_L5_both_first_mods_last", "n65_F16_M1_L4_coords_last", "n257_F16_M4_L3_none"]
NOTEBOOK = (128, 4, (64, 64, 64, 4), (1, 2), (2,))


def fused_bytes(desc):
    return int(_lib.lib().mrirt_inject_fused_lds_bytes(C.byref(desc)))


class Out:
    """argmax [n_max] and logits [n_max][C], each between two guard blocks, every byte pre-filled with FILL."""

    def __init__(self, n_max, Cn, want_am=True, want_logits=True):
        self.n, self.C = n_max, Cn
        self.am_raw = torch.full((GUARD + 2 * n_max + (-2 * n_max) % 16 + GUARD,), FILL, dtype=torch.uint8, device=DEV) if want_am else None
        self.lg_raw = torch.full((GUARD + 4 * n_max * Cn + GUARD,), FILL, dtype=torch.uint8, device=DEV) if want_logits else None
        self.am = self.am_raw[GUARD:GUARD + 2 * n_max].view(torch.int16) if want_am else None
        self.lg = self.lg_raw[GUARD:GUARD + 4 * n_max * Cn].view(torch.float32) if want_logits else None

    def read(self, rows):
        """(logits[:rows], argmax[:rows]) after checking that every other byte still holds FILL."""
        torch.cuda.synchronize()
        am = lg = None
        if self.am_raw is not None:
            raw = self.am_raw.cpu().numpy()
            assert (raw[:GUARD] == FILL).all() and (raw[GUARD + 2 * rows:] == FILL).all(), "argmax: a byte beyond the count or in a guard changed"
            am = raw[GUARD:GUARD + 2 * rows].view(np.int16).copy()
        if self.lg_raw is not None:
            raw = self.lg_raw.cpu().numpy()
            assert (raw[:GUARD] == FILL).all() and (raw[GUARD + 4 * rows * self.C:] == FILL).all(), "logits: a byte beyond the count or in a guard changed"
            lg = raw[GUARD:GUARD + 4 * rows * self.C].view(np.float32).reshape(rows, self.C).copy()
        return lg, am


def classify(net, c, m, n_max, count=None, want_am=True, want_logits=True, rows=None):
    out = Out(n_max, net.C, want_am, want_logits)
    cnt = torch.tensor([count], dtype=torch.int64, device=DEV).to(torch.int32) if count is not None else None
    rc = _lib.lib().mrirt_inject_classify(C.byref(net.desc), _ptr(net.B), _ptr(net.w), _ptr(net.b), _ptr(c), _ptr(m), n_max, _ptr(cnt),
                                          _ptr(out.am), _ptr(out.lg), None)
    assert rc == 0, rc
    return out.read(n_max if rows is None else rows)


def same(a, b):
    return a.tobytes() == b.tobytes()


# ---- the cases of tests/inject_cases.py --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in ic.EXACT])
def test_exact_cases_equal_the_restatement_and_the_chain_or_are_refused(name):
    case = next(c for c in ic.EXACT if c[0] == name)
    params, _, coords, mods = ic.exact_case(case)
    net = Net(params, desc_of(*case[2:7]))
    n = case[1]
    c, m = _up(coords), (_up(mods) if case[3] else None)
    if fused_bytes(net.desc) == 0:
        assert name not in REQUIRED, "the fit rule must accept this case"
        out = Out(n, net.C)
        rc = _lib.lib().mrirt_inject_classify(C.byref(net.desc), _ptr(net.B), _ptr(net.w), _ptr(net.b), _ptr(c), _ptr(m), n, None, _ptr(out.am),
                                              _ptr(out.lg), None)
        assert rc == ARG
        out.read(0)                                              # nothing was written
        return
    want = ref.forward32(params, coords, mods, case[5], case[6])
    logits, am = classify(net, c, m, n)
    bad = ~((logits.view(np.uint32) == want.view(np.uint32)) | (np.isnan(logits) & np.isnan(want)))
    print(name, "differing logits:", int(bad.sum()), "of", bad.size)
    assert ref.same_bits(logits, want) and np.array_equal(am, ref.argmax(want))
    chain_logits, chain_am = forward(net, coords, mods)
    assert same(logits, chain_logits) and same(am, chain_am)


def test_every_required_case_is_accepted():
    for name in REQUIRED:
        case = next(c for c in ic.EXACT if c[0] == name)
        assert 0 < fused_bytes(desc_of(*case[2:7])) <= 160 * 1024, name
    for case in ic.INTEGER:
        assert 0 < fused_bytes(desc_of(*case[2:7])) <= 160 * 1024, case[0]
    assert 0 < fused_bytes(desc_of(*NOTEBOOK)) <= 160 * 1024
    refused = next(c for c in ic.EXACT if c[0] == "n65_F18_M8_L8_coords_first_both_last")
    assert fused_bytes(desc_of(*refused[2:7])) == 0


@pytest.mark.parametrize("case", ic.INTEGER, ids=[c[0] for c in ic.INTEGER])
def test_integer_cases_are_exact_and_equal_the_chain(case):
    params, coords8, mods = ic.integer_case(case)
    z8, _ = ref.forward_int(params, coords8, mods, case[5], case[6])
    net = Net(params, desc_of(*case[2:7]))
    coords, modsf = (coords8 / 8.0).astype(np.float32), mods.astype(np.float32)
    logits, am = classify(net, _up(coords), _up(modsf), case[1])
    got8 = logits.astype(np.float64) * 8
    assert np.array_equal(got8, np.round(got8)) and np.array_equal(got8.astype(np.int64), z8)
    assert np.array_equal(am, np.argmax(z8, 1).astype(np.int16))
    chain_logits, chain_am = forward(net, coords, modsf)
    assert same(logits, chain_logits) and same(am, chain_am)


def test_tolerance_case_notebook_shape_equals_the_chain_bit_for_bit():
    case = next(c for c in ic.TOLERANCE if c[0] == "notebook_shape")
    params, coords, mods = ic.tolerance_case(case)
    net = Net(params, desc_of(*case[2:7]))
    logits, am = classify(net, _up(coords), _up(mods), case[1])
    chain_logits, chain_am = forward(net, coords, mods)
    assert same(logits, chain_logits) and same(am, chain_am)


# ---- row counts on the notebook shape ----------------------------------------------------------------------------------------
ROWS = [1, 15, 16, 17, 63, 64, 65, 257, 131073]


@functools.lru_cache(maxsize=None)
def _notebook():
    """A Glorot net of the notebook's shape, 131 073 seeded points on the device, and the chain's outputs for all of them (the
    chain is batch-position invariant -- tests/test_gpu_inject.py -- so a prefix of them is the chain's answer for that prefix)."""
    rng = np.random.default_rng(20260)
    F, M, widths, cl, ml = NOTEBOOK
    params = ref.glorot_net(rng, F, M, widths, cl, ml)
    net = Net(params, desc_of(*NOTEBOOK))
    n = ROWS[-1]
    coords = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    mods = rng.normal(0, 1, (n, M)).astype(np.float32)
    c, m = _up(coords), _up(mods)
    logits = torch.empty((n, net.C), dtype=torch.float32, device=DEV)
    am = torch.empty(n, dtype=torch.int16, device=DEV)
    nbytes = _lib.lib().mrirt_inject_scratch_bytes(C.byref(net.desc), n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = _lib.lib().mrirt_inject_forward(C.byref(net.desc), _ptr(net.B), _ptr(net.w), _ptr(net.b), _ptr(c), _ptr(m), n, None, _ptr(logits),
                                         _ptr(am), _ptr(scratch), nbytes, None)
    assert rc == 0
    torch.cuda.synchronize()
    return params, net, c, m, logits.cpu().numpy(), am.cpu().numpy()


@pytest.mark.parametrize("n", ROWS)
def test_row_counts_equal_the_chain(n):
    params, net, c, m, chain_logits, chain_am = _notebook()
    if n <= 257:                                                 # the chain on exactly these rows, not only as a prefix
        lg, am = forward(net, c[:n].cpu().numpy(), m[:n].cpu().numpy())
        assert same(lg, chain_logits[:n]) and same(am, chain_am[:n])
    logits, am = classify(net, c, m, n)
    assert len(set(am.tolist())) > 1 or n < 15, "a net that answers one class everywhere shows nothing"
    assert same(logits, chain_logits[:n]) and same(am, chain_am[:n])


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 300, 1000])
def test_count_dev_bounds_what_is_read_and_written(count):
    params, net, c, m, chain_logits, chain_am = _notebook()
    n_max, rows = 300, min(count, 300)
    cc, mm = c[:n_max].clone(), m[:n_max].clone()
    cc[rows:] = float("nan")
    mm[rows:] = float("nan")
    logits, am = classify(net, cc, mm, n_max, count=count, rows=rows)      # read() checks every byte at or beyond the count
    assert same(logits, chain_logits[:rows]) and same(am, chain_am[:rows])


def test_two_calls_give_the_same_bits_and_either_output_alone_gives_the_bits_of_both():
    params, net, c, m, chain_logits, chain_am = _notebook()
    n = 1000
    a = classify(net, c, m, n)
    b = classify(net, c, m, n)
    assert same(a[0], b[0]) and same(a[1], b[1])
    only_am = classify(net, c, m, n, want_logits=False)
    only_lg = classify(net, c, m, n, want_am=False)
    assert only_am[0] is None and only_lg[1] is None
    assert same(only_am[1], a[1]) and same(only_lg[0], a[0])


def test_refusals_leave_the_outputs_untouched():
    params, net, c, m, _, _ = _notebook()
    l = _lib.lib()
    n = 64

    def call(desc=net.desc, B=net.B, w=net.w, b=net.b, coords=c, mods=m, n_max=n, am=True, lg=True):
        out = Out(n, net.C)
        rc = l.mrirt_inject_classify(C.byref(desc) if desc is not None else None, _ptr(B), _ptr(w), _ptr(b), _ptr(coords), _ptr(mods), n_max, None,
                                     _ptr(out.am) if am else None, _ptr(out.lg) if lg else None, None)
        out.read(0)
        return rc

    for kw in ("desc", "B", "w", "b", "coords", "mods"):
        assert call(**{kw: None}) == NULL, kw
    assert call(am=False, lg=False) == NULL
    for n_max in (0, -1, 1 << 31):
        assert call(n_max=n_max) == ARG
    bad = desc_of(128, 4, (64, 64, 64, 17), (1, 2), (2,))       # 17 classes: inj_check_shape refuses
    assert call(desc=bad) == ARG and fused_bytes(bad) == 0
    for name in ("n65_F18_M8_L8_coords_first_both_last", "n257_F256_M8_L3_mods"):
        case = next(k for k in ic.EXACT if k[0] == name)
        d = desc_of(*case[2:7])
        assert fused_bytes(d) == 0 and call(desc=d) == ARG, name


def test_python_wrapper():
    params, net, c, m, chain_logits, chain_am = _notebook()
    assert inr.inject_fused_ok(params, (1, 2), (2,))
    am, logits = inr.inject_classify(params, c[:500], m[:500], want_logits=True, coord_layers=(1, 2), mod_layers=(2,))
    assert same(am.cpu().numpy(), chain_am[:500]) and same(logits.cpu().numpy(), chain_logits[:500])
    cnt = torch.tensor([70], dtype=torch.int32, device=DEV)
    am = inr.inject_classify(params, c[:500], m[:500], count=cnt, coord_layers=(1, 2), mod_layers=(2,)).cpu().numpy()
    assert same(am[:70], chain_am[:70]) and not am[70:].any()
    wide = ref.glorot_net(np.random.default_rng(1), 256, 8, (256, 65, 16), (), (1,))
    assert not inr.inject_fused_ok(wide, (), (1,))
    with pytest.raises(_lib.MrirtError):
        inr.inject_classify(wide, c[:8], torch.zeros((8, 8), device=DEV), coord_layers=(), mod_layers=(1,))
