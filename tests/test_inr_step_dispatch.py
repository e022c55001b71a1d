"""The Python side of the training step has one implementation per job (scratch, forward, backward) for both families of
entry points.  On the CPU: the private dispatch picks mrirt_inr_* for the two ReLU kinds and mrirt_siren_* for the two SIREN
kinds, and the public twins still hand a descriptor of the other family to their own entry point, which refuses it with the
ValueError text each twin always raised (the *_train_scratch_bytes functions are host code and return 0 without a device)."""
import ctypes as C

import pytest

from mrirt import _lib, inr

DIMS, N = [7, 64, 64, 4], 100
DESCS = {"fourier": lambda: inr.train_desc([3 + 6 * 2 + 4, 64, 64, 4], 2, 4), "raw_relu": lambda: inr.train_desc(DIMS),
         "siren": lambda: inr.siren_train_desc(DIMS, 4, 30.0), "raw_siren": lambda: inr.siren_train_desc(DIMS, None, 30.0)}
KINDS = {"fourier": inr.KIND_FOURIER_RELU, "raw_relu": inr.KIND_RAW_RELU, "siren": inr.KIND_SIREN, "raw_siren": inr.KIND_RAW_SIREN}
FAMILY = {"fourier": "inr", "raw_relu": "inr", "siren": "siren", "raw_siren": "siren"}
JOBS = ("train_scratch_bytes", "forward_f32", "backward")
SHAPE = "in {inDim}, hidden 64 x 2, out 4, n 100"
RELU_TEXT = "unsupported training shape: " + SHAPE + " (ReLU kinds, hidden in {{32,64,128,256}}, in <= 128, out <= 16, <= 8 layers, n >= 1)"
SIREN_TEXT = ("unsupported SIREN training shape: " + SHAPE + " (SIREN kinds, hidden in {{32,64,128,256}}, in <= 128, out <= 16, <= 8 layers, "
              "n >= 1, finite w0 != 0)")


@pytest.mark.parametrize("which", sorted(DESCS))
def test_dispatch_goes_by_the_descriptors_kind(which):
    desc = DESCS[which]()
    assert desc.kind == KINDS[which]
    for job in JOBS:
        name = inr._step_symbol(desc, job)
        assert name == f"mrirt_{FAMILY[which]}_{job}" and name in _lib.ABI_SYMBOLS
        other = "siren" if FAMILY[which] == "inr" else "inr"
        assert inr._step_symbol(desc, job, other) == f"mrirt_{other}_{job}"          # a public twin names its own family


@pytest.mark.parametrize("which", sorted(DESCS))
def test_scratch_of_the_own_family_and_refusal_by_the_other(which):
    desc = DESCS[which]()
    own, other = (inr.train_scratch, inr.siren_train_scratch) if FAMILY[which] == "inr" else (inr.siren_train_scratch, inr.train_scratch)
    want = int(getattr(_lib.lib(), f"mrirt_{FAMILY[which]}_train_scratch_bytes")(C.byref(desc), N))
    assert want > 0
    for fn in (own, inr._step_scratch):                      # the twin and the dispatch agree on the size
        got = fn(desc, N, "cpu")
        assert got.numel() == want and got.dtype == inr.torch.uint8
    text = (SIREN_TEXT if FAMILY[which] == "inr" else RELU_TEXT).format(inDim=desc.inDim)
    with pytest.raises(ValueError) as e:
        other(desc, N, "cpu")
    assert str(e.value) == text


def test_descriptors_share_the_width_checks():
    for make in (lambda d: inr.train_desc(d, 2, 4), lambda d: inr.train_desc(d), lambda d: inr.siren_train_desc(d, None), lambda d: inr.siren_train_desc(d, 4)):
        for dims in ([7, 4], [7, 64, 32, 4]):
            with pytest.raises(ValueError) as e:
                make(dims)
            assert str(e.value) == f"layer widths {dims}: the kernels need at least one hidden layer and equal hidden widths"
    with pytest.raises(ValueError, match="a SIREN over 4 modalities has 7 inputs, not 8"):
        inr.siren_train_desc([8, 64, 4], 4)
    for w0 in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="w0 must be finite and non-zero"):
            inr.siren_train_desc(DIMS, 4, w0)
