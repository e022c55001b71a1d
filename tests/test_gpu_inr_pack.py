"""The packed weight image of mrirt_inr_pack_weights, byte for byte against the NumPy packer of tests/inr_ref.py (pack_image,
written from the layout comments): the main image, the refine image and the zeroed slack behind it, for the smallest networks
that reach every branch of the pack kernel (inr_ref.PACK_NETS) with weights that include exact bf16 ties (inr_ref.PACK_TIES:
round-to-nearest-even of the hi part, the lo part of a tie, a lo part that is itself a tie).

Not compared: the 64 slack fragments between the two images (the pack never writes them) and the calibration record (the
descriptor's `weights` points elsewhere, so nothing is calibrated).  The buffer is filled with 0xFF first, so a fragment the
pack kernel skipped cannot pass as zero padding."""
import ctypes as C

import numpy as np
import pytest

import inr_ref as ir

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(ir.PACK_NETS)), ids=[ir.pack_id(n) for n in ir.PACK_NETS])
def test_packed_image_equals_the_numpy_packer(i):
    import torch
    from mrirt import _lib
    assert torch.cuda.is_available()
    net, layers = ir.PACK_NETS[i], ir.pack_case(i)
    want_main = ir.pack_image(layers, net["kind"], net["w0"])
    want_ref = ir.pack_image(layers, net["kind"], net["w0"], refine=True)
    total, ref_total = len(want_main), len(want_ref)
    ref_base = total + ir.PACK_SLACK_FRAGS
    tail = ref_base + ref_total + ir.REF_SLACK_FRAGS

    d = _lib.InrDesc()
    d.kind, d.numLayers, d.inDim, d.outDim, d.hidden = net["kind"], net["layers"], net["ind"], net["out"], net["hidden"]
    d.fourierFreqs, d.numMods, d.w0 = net["K"], net["M"], net["w0"]
    d.weights, d.biases = None, None                                       # not the buffer packed below: no calibration pass
    assert _lib.lib().mrirt_inr_pack_bytes(C.byref(d)) == (tail + 1) * 1024
    w_flat = torch.from_numpy(np.concatenate([p["W"].reshape(-1) for p in layers])).cuda()
    packed = torch.full(((tail + 1) * 1024,), 0xFF, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().mrirt_inr_pack_weights(C.byref(d), C.c_void_p(w_flat.data_ptr()), C.c_void_p(packed.data_ptr()), None),
               "mrirt_inr_pack_weights")
    torch.cuda.synchronize()
    got = packed.cpu().numpy().view(np.uint16).reshape(tail + 1, 64, 8)

    for name, have, want in (("main", got[:total], want_main), ("refine", got[ref_base:ref_base + ref_total], want_ref)):
        bad = np.argwhere(have != want)
        assert bad.size == 0, (f"{name} image: {len(bad)} of {want.size} elements differ, first at fragment {bad[0][0]} lane {bad[0][1]} "
                               f"element {bad[0][2]}: {have[tuple(bad[0])]:#06x} != {want[tuple(bad[0])]:#06x}")
    assert not got[ref_base + ref_total:tail].any(), "the slack after the refine image is not zero"
    # the ties are in the image and were rounded to even: 1 + 2^-8 -> hi 1.0 (0x3f80), lo 2^-8 (0x3b80)
    assert (want_ref == 0x3b80).any() and (want_main == 0x3f80).any()
