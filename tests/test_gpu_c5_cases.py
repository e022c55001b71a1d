"""The chunked C5 render (mrirt_render_brats_inr) against the oracle, directly and with equality, over the case grid of
tests/c5_cases.py: decisive networks make the class of every sample exact, so the frame, the counters and the whole-ray
streams all have an exact reference (tests/c5_ref.py; its preconditions: tests/test_c5_cases_host.py).  Then the raw ABI:
an exact, guarded scratch with stale contents, a pitched output, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import c5_cases as cc
import c5_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import mrirt
    assert torch.cuda.is_available()
    return dict(torch=torch, mrirt=mrirt, inr=mrirt.inr, bound={}, nets={})


def _bound(env, case):
    """The case's grids on the device (uploaded once per module): (intensities, labels)."""
    key = (case.dims, case.vol_seed, case.layout, case.labels)
    if key not in env["bound"]:
        mrirt = env["mrirt"]
        vols, lab, _, _ = cc.volumes(case.dims, case.vol_seed)
        if case.layout == "mod4":
            g = mrirt.upload_mod4([v.copy() for v in vols], case.dims)      # (copies: the cached arrays are read-only)
        else:
            g = [mrirt.upload_grid(v.copy(), case.dims, case.layout) for v in vols]
        gl = mrirt.upload_grid(lab.copy(), case.dims, case.labels) if case.labels is not None else None
        env["bound"][key] = (g, gl)
    return env["bound"][key]


def _net(env, net):
    if net not in env["nets"]:
        inr = env["inr"]
        kind = inr.KIND_SIREN if net.kind == "siren" else inr.KIND_FOURIER_RELU
        env["nets"][net] = inr.pack_mlp(cc.layers_of(net), kind, net.K, 4, w0=cc.W0)
    return env["nets"][net]


def _render(env, case, net, **kw):
    g, gl = _bound(env, case)
    _, _, zmu, zsg = cc.volumes(case.dims, case.vol_seed)
    ext = kw.pop("ext", None) or cc.gpu_ext(case)
    return env["inr"].render_brats_inr(cc.params_of(case), g, net, zmu, zsg, labels=gl, ext=ext, **kw)


@pytest.mark.parametrize("name", cc.NAMES)
def test_chunked_frame_counters_and_streams_equal_the_oracle(env, name):
    case, ref = cc.CASES[name], cr.reference(name)
    net = _net(env, case.net)
    nets = [("", net)]
    if (case.net.kind, case.net.hidden, case.net.depth) == ("siren", 256, 4):      # the same net through the streaming kernel
        nets.append(("streaming kernel, ", env["inr"].with_flags(net, no_weight_stationary=True)))
    problems = []
    for tag, nt in nets:
        for c in cr.chunks_of(case, ref):
            img, aux = _render(env, case, nt, return_aux=True, chunk_steps=c)
            if c is None:
                assert aux["chunk_steps"] == cr.default_chunk(case)
            said = cr.frame_problems(img.cpu().numpy(), ref["frame"]) + cr.counter_problems(aux, ref, aux["chunk_steps"])
            problems += [f"{tag}pass length {c}: {s}" for s in said]
    assert not problems, "\n".join(problems)
    if "all_hit" in case.claims:      # pass length 1: the first batch is exactly cap = width x height rows, no multiple of 256
        _, aux = _render(env, case, net, return_aux=True, chunk_steps=1)
        assert aux["queries"] == ref["live"] and int((ref["n"] > 0).sum()) == case.frame[0] * case.frame[1]
    if case.refused_chunk is not None:                                             # more than 1024 passes
        with pytest.raises(env["mrirt"]._lib.MrirtError) as e:
            _render(env, case, net, chunk_steps=case.refused_chunk)
        assert e.value.status == -5
    if case.layout == "mod4":
        with pytest.raises(ValueError):                                            # the whole-ray form takes per-modality grids
            _render(env, case, net, one_pass=True)
        return
    # the whole-ray form: the same frame; every row's class is the rule's, its inputs inr_sample_inputs', its count n
    for tag, nt in nets:
        img, a = _render(env, case, nt, return_aux=True, one_pass=True)
        said = cr.frame_problems(img.cpu().numpy(), ref["frame"], "one-pass frame")
        said += cr.stream_problems(a["counts"].cpu().numpy(), a["classes"].cpu().numpy(), a["coords"].cpu().numpy(), a["feats"].cpu().numpy(), ref)
        for k, want in (("queries", int(ref["n"].sum())), ("live_samples", ref["live"]), ("shaded_samples", ref["shaded"])):
            if a[k] != want:
                said.append(f"one-pass {k}: {a[k]} for {want}")
        assert np.array_equal(a["offsets"].cpu().numpy(), ref["offsets"])
        assert not said, tag + "\n".join(said)


@pytest.mark.parametrize("name", cc.FAST_CASES)
def test_fast_math_stays_within_the_existing_bar(env, name):
    """MATH_FAST is not held to equality: the bar of tests/test_gpu_inr_render.py, one case per layout."""
    case, ref = cc.CASES[name], cr.reference(name)
    img = _render(env, case, _net(env, case.net), ext=cc.gpu_ext(case, math="fast"), chunk_steps=16).cpu().numpy()
    d = np.abs(img - ref["frame"])
    assert float(d.max()) < 0.3 and float(d.mean()) < 2e-3


# ---- the raw ABI ------------------------------------------------------------------------------------------------------------------
GUARD, SENTINEL, STAT_SENTINEL = 4096, -7.25, 0x5A5A5A5A5A5A5A5A


class _Raw:
    """One case bound for direct calls of mrirt_render_brats_inr."""

    def __init__(self, env, case, net):
        from mrirt.render import _bind_brats
        torch = env["torch"]
        self.torch, self.lib, self.case, self.net = torch, env["mrirt"]._lib.lib(), case, net
        g, gl = _bound(env, case)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.P, self.E, self.vols, self.lab, _, _ = _bind_brats(cc.params_of(case), [g] * 4 if case.layout == "mod4" else g, gl, None,
                                                                cc.gpu_ext(case), dev, pred_stream=True)
        _, _, zmu, zsg = cc.volumes(case.dims, case.vol_seed)
        self.mu = (C.c_float * 4)(*[float(np.float32(v)) for v in zmu])
        self.sg = (C.c_float * 4)(*[float(np.float32(v)) for v in zsg])
        self.vp = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) for t in self.vols])
        self.W, self.H = case.frame

    def bytes(self, chunk, P=None):
        return int(self.lib.mrirt_brats_inr_scratch_bytes(C.byref(P if P is not None else self.P), chunk))

    def buffers(self, chunk):
        torch = self.torch
        n = self.bytes(chunk)
        assert n > 0
        buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.full((self.H, self.W + 3, 4), SENTINEL, dtype=torch.float32, device="cuda")
        stats = torch.tensor([0, 0, 0, STAT_SENTINEL], dtype=torch.int64, device="cuda")
        assert (buf.data_ptr() + GUARD) % 256 == 0
        return buf, n, out, stats

    def call(self, chunk, buf, n, frame, counters, stream, **over):
        """rc of one call; `over` replaces single arguments (None = a NULL pointer)."""
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        a = dict(P=C.byref(self.P), E=C.byref(self.E), vp=self.vp, lab=ptr(self.lab), net=C.byref(self.net.desc), mu=self.mu, sg=self.sg,
                 chunk=chunk, scratch=C.c_void_p(buf.data_ptr() + GUARD), nbytes=n, out=ptr(frame), pitch=frame.stride(0) // 4,
                 stats=ptr(counters))
        a.update(over)
        return int(self.lib.mrirt_render_brats_inr(a["P"], a["E"], a["vp"], a["lab"], a["net"], a["mu"], a["sg"], a["chunk"], a["scratch"],
                                                   a["nbytes"], a["out"], a["pitch"], a["stats"], C.c_void_p(stream.cuda_stream)))


@pytest.mark.parametrize("name", cc.RAW_ABI_CASES)
def test_raw_abi_exact_guarded_scratch_with_stale_contents(env, name):
    """The scratch is exactly mrirt_brats_inr_scratch_bytes long between two guard blocks, the output is pitched with sentinel
    columns, stats has a sentinel fourth word: nothing outside is written; and the frame does not depend on what the scratch held
    (zeros, then 0xFF — every stale class with its mark bit set — on the same buffer), on the default stream and on a side stream."""
    torch = env["torch"]
    case, ref = cc.CASES[name], cr.reference(name)
    raw = _Raw(env, case, _net(env, case.net))
    chunk = 1 if "all_hit" in case.claims else 3
    if chunk == 1:
        assert (case.frame[0] * case.frame[1]) % 256 != 0 and (ref["n"] > 0).all()     # the first batch is exactly cap rows
    for stream in (torch.cuda.current_stream(), torch.cuda.Stream()):
        torch.cuda.synchronize()                          # the uploads and the packed net were made on the default stream
        with torch.cuda.stream(stream):
            buf, n, out, stats = raw.buffers(chunk)
            for fill in (0x00, 0xFF):
                buf[GUARD:GUARD + n].fill_(fill)
                out.fill_(SENTINEL)
                stats[:3].zero_()
                assert raw.call(chunk, buf, n, out, stats, stream) == 0
                stream.synchronize()
                b, o, s = buf.cpu().numpy(), out.cpu().numpy(), stats.cpu().numpy()
                assert (b[:GUARD] == 0xA5).all() and (b[GUARD + n:] == 0xA5).all(), "a write outside the scratch"
                assert (o[:, raw.W:] == np.float32(SENTINEL)).all() and int(s[3]) == STAT_SENTINEL
                aux = dict(live_samples=int(s[0]), shaded_samples=int(s[1]), queries=int(s[2]))
                said = cr.frame_problems(o[:, :raw.W], ref["frame"]) + cr.counter_problems(aux, ref, chunk)
                assert not said, f"scratch pre-filled with {fill:#x}: " + "\n".join(said)


def test_every_refusal_leaves_output_and_scratch_untouched(env):
    torch, lib = env["torch"], env["mrirt"]._lib
    NULL_, LAYOUT_, ARG_ = -1, -3, -5
    case = cc.CASES["quad_overlays_8x8"]
    raw = _Raw(env, case, _net(env, case.net))
    chunk = 4
    stream = torch.cuda.current_stream()
    buf, n, out, stats = raw.buffers(chunk)
    buf.fill_(0xA5)

    def copy_of(s, **fields):
        t = type(s)()
        C.memmove(C.byref(t), C.byref(s), C.sizeof(s))
        for k, v in fields.items():
            if isinstance(v, tuple):
                for i, x in enumerate(v):
                    getattr(t, k)[i] = x
            else:
                setattr(t, k, v)
        return t

    def refused(want, what, chunk_=chunk, **over):
        rc = raw.call(chunk_, buf, over.pop("nbytes", n), out, stats, stream, **over)
        stream.synchronize()
        assert rc == want, f"{what}: status {rc} for {want}"
        assert bool((buf == 0xA5).all()), f"{what}: the scratch was written"
        assert bool((out == SENTINEL).all()), f"{what}: the output was written"
        assert stats.cpu().tolist() == [0, 0, 0, STAT_SENTINEL], f"{what}: the counters were written"

    # NULL arguments
    for k in ("P", "vp", "net", "mu", "sg", "scratch", "out"):
        refused(NULL_, f"{k} = NULL", **{k: None})
    holed = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) for t in raw.vols])
    holed[2] = None
    refused(NULL_, "gIntensity2 = NULL", vp=holed)
    refused(NULL_, "showSeg without labels", lab=None)
    # the pass length
    for c in (0, 4097):
        assert raw.bytes(c) == 0
        refused(ARG_, f"chunk {c}", chunk_=c)
    # image x chunk >= 2^32 - 2^21 rows per pass
    big = copy_of(raw.P, imageSize=(2048, 1024))
    assert raw.bytes(2046, big) > 0 and raw.bytes(2047, big) == 0 and raw.bytes(4096, big) == 0
    refused(ARG_, "2^32 - 2^21 rows per pass", chunk_=2047, P=C.byref(big), pitch=2048)
    # the scratch one byte short
    refused(ARG_, "scratch one byte short", nbytes=n - 1)
    # what the entry point does not render
    refused(ARG_, "showPred == 0", P=C.byref(copy_of(raw.P, showPred=0)))
    refused(ARG_, "tiles", E=C.byref(copy_of(raw.E, tileSize=8, tileWorld=1)))
    refused(LAYOUT_, "label cells", E=C.byref(copy_of(raw.E, labelLayout=lib.LAYOUT_LABCELL)))
    refused(LAYOUT_, "vga voxels", E=C.byref(copy_of(raw.E, layout=lib.LAYOUT_VGA)))
    refused(LAYOUT_, "shaded quad", E=C.byref(copy_of(raw.E, shadeMode=1)))
    refused(LAYOUT_, "shaded mod4", E=C.byref(copy_of(raw.E, shadeMode=1, layout=lib.LAYOUT_MOD4)))
    refused(ARG_, "a raw-input network", net=C.byref(copy_of(raw.net.desc, kind=2)))
    refused(ARG_, "a network over three modalities", net=C.byref(copy_of(raw.net.desc, numMods=3, inDim=raw.net.desc.inDim - 1)))
    refused(ARG_, "a network shape the packer refuses", net=C.byref(copy_of(raw.net.desc, hidden=48)))
    refused(NULL_, "a network without weights", net=C.byref(copy_of(raw.net.desc, weights=None)))
    # more than 1024 passes: the box diagonal in 5000 steps, four per pass
    diag = float(np.sqrt(sum((float(raw.P.voxelSize[k]) * int(raw.P.dims[k])) ** 2 for k in range(3))))
    refused(ARG_, "more than 1024 passes", P=C.byref(copy_of(raw.P, stepSize=diag / 5000.0)))
    # ... and the same call goes through once nothing is wrong with it
    assert raw.call(chunk, buf, n, out, stats, stream) == 0
    stream.synchronize()
    assert not cr.frame_problems(out.cpu().numpy()[:, :raw.W], cr.reference(case.name)["frame"])
