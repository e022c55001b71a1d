"""The per-sample render with the coordinate-injection network (mrirt_render_brats_inject; csrc/brats_c5.hip,
csrc/inr_inject_fused.hip) over scenes of tests/c5_cases.py: the chunked frame and its counters against
the one-pass composition built from calls that existed before it (sample counts, emission, mrirt_inject_forward, the stream
march), a decisive net against the oracle's frame, the raw ABI with a guarded scratch, every refusal, and the factored frame
loop behind mrirt_render_brats_inr.  Equality everywhere."""
import ctypes as C

import numpy as np
import pytest

import c5_cases as cc
import c5_ref as cr
import inject_ref as ref
from test_gpu_c5_cases import GUARD, SENTINEL, STAT_SENTINEL, _Raw, _bound, _net
from test_inject_fused_host import DECISIVE_SCENE, decisive_inject

pytestmark = pytest.mark.gpu
SCENES = cc.RAW_ABI_CASES + ("linear_shaded_56x40",)
CHUNKS = (1, 7, 96)
NETS = {
    "notebook": (128, 4, (64, 64, 64, 4), (1, 2), (2,)),
    "small": (14, 4, (17, 13, 4), (1,), (1,)),                   # widths that are no multiple of 16, inputs no multiple of 4
}


@pytest.fixture(scope="module")
def env():
    import torch
    import mrirt
    assert torch.cuda.is_available()
    return dict(torch=torch, mrirt=mrirt, inr=mrirt.inr, bound={}, nets={}, one_pass={})


def _params(which):
    F, M, widths, cl, ml = NETS[which]
    return ref.glorot_net(np.random.default_rng(len(which) + 4242), F, M, widths, cl, ml, bias=0.5), cl, ml


def _render(env, case, params, cl, ml, **kw):
    g, gl = _bound(env, case)
    _, _, zmu, zsg = cc.volumes(case.dims, case.vol_seed)
    ext = cc.gpu_ext(case)
    if kw.get("one_pass") and case.layout == "mod4":              # the whole-ray form takes per-modality grids: the same voxels, LINEAR
        vols = cc.volumes(case.dims, case.vol_seed)[0]
        key = ("linear for mod4", case.dims, case.vol_seed)
        if key not in env["bound"]:
            env["bound"][key] = [env["mrirt"].upload_grid(v.copy(), case.dims, "linear") for v in vols]
        g, ext = env["bound"][key], dict(ext, layout="linear")
    return env["inr"].render_brats_inject(cc.params_of(case), g, params, zmu, zsg, labels=gl, ext=ext, coord_layers=cl, mod_layers=ml, **kw)


def _one_pass(env, name, which):
    """The definition, once per (scene, net): frame, aux, and the composited steps per ray that the oracle march takes with
    this class stream (what c5_ref.queries needs)."""
    key = (name, which)
    if key not in env["one_pass"]:
        case = cc.CASES[name]
        params, cl, ml = _params(which)
        img, aux = _render(env, case, params, cl, ml, return_aux=True, one_pass=True)
        classes, offsets = aux["classes"].cpu().numpy().astype(np.int64), aux["offsets"].cpu().numpy()
        n = aux["counts"].cpu().numpy().astype(np.int64).reshape(case.frame[1], case.frame[0])
        frame, oaux = cr._march(case, False, lambda idx, k, qx, qy, qz: classes[offsets[idx] + k])
        env["one_pass"][key] = dict(frame=img.cpu().numpy(), aux=aux, n=n, L=oaux["nsteps"].astype(np.int64), classes=classes, oracle=frame)
    return env["one_pass"][key]


@pytest.mark.parametrize("which", list(NETS))
@pytest.mark.parametrize("name", SCENES)
def test_chunked_frame_and_counters_equal_the_one_pass_composition(env, name, which):
    case = cc.CASES[name]
    params, cl, ml = _params(which)
    one = _one_pass(env, name, which)
    assert np.array_equal(one["n"], cr.reference(name)["n"])      # the steps per ray do not depend on the net
    assert one["aux"]["live_samples"] == int(one["L"].sum())      # the oracle march with this class stream composites as many
    assert not cr.frame_problems(one["frame"], one["oracle"], "one-pass frame against the oracle with its class stream")
    problems = []
    for c in CHUNKS:
        img, aux = _render(env, case, params, cl, ml, return_aux=True, chunk_steps=c)
        problems += [f"pass length {c}: {s}" for s in cr.frame_problems(img.cpu().numpy(), one["frame"])]
        want = dict(live_samples=one["aux"]["live_samples"], shaded_samples=one["aux"]["shaded_samples"], queries=cr.queries(one["n"], one["L"], c))
        problems += [f"pass length {c}: {k}: {aux[k]} for {v}" for k, v in want.items() if int(aux[k]) != v]
    assert not problems, "\n".join(problems)


def test_the_glorot_nets_draw_more_than_one_class(env):
    """... so the frames above depend on what the classifier answers."""
    seen = set()
    for name in SCENES:
        seen |= set(np.unique(_one_pass(env, name, "notebook")["classes"]).tolist())
    assert len(seen) >= 2, seen


def test_decisive_net_equals_the_oracle(env):
    case, r = cc.CASES[DECISIVE_SCENE], cr.reference(DECISIVE_SCENE)
    params, cl, ml = decisive_inject(case.net)
    problems = []
    for c in CHUNKS + (None,):
        img, aux = _render(env, case, params, cl, ml, return_aux=True, chunk_steps=c)
        said = cr.frame_problems(img.cpu().numpy(), r["frame"]) + cr.counter_problems(aux, r, aux["chunk_steps"])
        problems += [f"pass length {c}: {s}" for s in said]
    assert not problems, "\n".join(problems)
    img, a = _render(env, case, params, cl, ml, return_aux=True, one_pass=True)
    said = cr.frame_problems(img.cpu().numpy(), r["frame"], "one-pass frame")
    said += cr.stream_problems(a["counts"].cpu().numpy(), a["classes"].cpu().numpy(), a["coords"].cpu().numpy(), a["feats"].cpu().numpy(), r)
    assert not said, "\n".join(said)


# ---- the raw ABI ------------------------------------------------------------------------------------------------------------------
class _InjNet:
    def __init__(self, env, params, cl, ml):
        torch, inr = env["torch"], env["inr"]
        self.desc = inr.inject_desc(params, cl, ml)
        w, b = ref.flat(params)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        self.B, self.w, self.b = up(params["fourier"]["B"]), up(w), up(b)


class _RawInject(_Raw):
    """One case bound for direct calls of mrirt_render_brats_inject (the buffers are _Raw's)."""

    def call(self, chunk, buf, n, frame, counters, stream, **over):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        a = dict(P=C.byref(self.P), E=C.byref(self.E), vp=self.vp, lab=ptr(self.lab), net=C.byref(self.net.desc), B=ptr(self.net.B),
                 w=ptr(self.net.w), b=ptr(self.net.b), mu=self.mu, sg=self.sg, chunk=chunk, scratch=C.c_void_p(buf.data_ptr() + GUARD),
                 nbytes=n, out=ptr(frame), pitch=frame.stride(0) // 4, stats=ptr(counters))
        a.update(over)
        return int(self.lib.mrirt_render_brats_inject(a["P"], a["E"], a["vp"], a["lab"], a["net"], a["B"], a["w"], a["b"], a["mu"], a["sg"],
                                                      a["chunk"], a["scratch"], a["nbytes"], a["out"], a["pitch"], a["stats"],
                                                      C.c_void_p(stream.cuda_stream)))


@pytest.mark.parametrize("name", cc.RAW_ABI_CASES)
def test_raw_abi_exact_guarded_scratch_with_stale_contents(env, name):
    torch = env["torch"]
    case = cc.CASES[name]
    params, cl, ml = _params("notebook")
    one = _one_pass(env, name, "notebook")
    raw = _RawInject(env, case, _InjNet(env, params, cl, ml))
    chunk = 1 if "all_hit" in case.claims else 3
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
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
        said = cr.frame_problems(o[:, :raw.W], one["frame"])
        want = (one["aux"]["live_samples"], one["aux"]["shaded_samples"], cr.queries(one["n"], one["L"], chunk))
        if tuple(int(v) for v in s[:3]) != want:
            said.append(f"counters {s[:3].tolist()} for {want}")
        assert not said, f"scratch pre-filled with {fill:#x}: " + "\n".join(said)


def test_every_refusal_leaves_output_and_scratch_untouched(env):
    torch, lib = env["torch"], env["mrirt"]._lib
    NULL_, LAYOUT_, ARG_ = -1, -3, -5
    case = cc.CASES["quad_overlays_8x8"]
    params, cl, ml = _params("notebook")
    raw = _RawInject(env, case, _InjNet(env, params, cl, ml))
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

    # what mrirt_render_brats_inr refuses of the same arguments
    for k in ("P", "vp", "net", "mu", "sg", "scratch", "out"):
        refused(NULL_, f"{k} = NULL", **{k: None})
    holed = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) for t in raw.vols])
    holed[2] = None
    refused(NULL_, "gIntensity2 = NULL", vp=holed)
    refused(NULL_, "showSeg without labels", lab=None)
    for c in (0, 4097):
        refused(ARG_, f"chunk {c}", chunk_=c)
    big = copy_of(raw.P, imageSize=(2048, 1024))
    refused(ARG_, "2^32 - 2^21 rows per pass", chunk_=2047, P=C.byref(big), pitch=2048)
    refused(ARG_, "scratch one byte short", nbytes=n - 1)
    refused(ARG_, "showPred == 0", P=C.byref(copy_of(raw.P, showPred=0)))
    refused(ARG_, "tiles", E=C.byref(copy_of(raw.E, tileSize=8, tileWorld=1)))
    refused(LAYOUT_, "label cells", E=C.byref(copy_of(raw.E, labelLayout=lib.LAYOUT_LABCELL)))
    refused(LAYOUT_, "vga voxels", E=C.byref(copy_of(raw.E, layout=lib.LAYOUT_VGA)))
    refused(LAYOUT_, "shaded quad", E=C.byref(copy_of(raw.E, shadeMode=1)))
    refused(LAYOUT_, "shaded mod4", E=C.byref(copy_of(raw.E, shadeMode=1, layout=lib.LAYOUT_MOD4)))
    diag = float(np.sqrt(sum((float(raw.P.voxelSize[k]) * int(raw.P.dims[k])) ** 2 for k in range(3))))
    refused(ARG_, "more than 1024 passes", P=C.byref(copy_of(raw.P, stepSize=diag / 5000.0)))
    # what it refuses beyond that
    for k in ("B", "w", "b"):
        refused(NULL_, f"{k} = NULL", **{k: None})
    refused(ARG_, "a network over three modalities", net=C.byref(copy_of(raw.net.desc, numMods=3)))
    refused(ARG_, "a shape inj_check_shape refuses", net=C.byref(copy_of(raw.net.desc, fourierDim=127)))
    refused(ARG_, "a shape the fused path refuses", net=C.byref(copy_of(raw.net.desc, fourierDim=256, width=(256, 256, 64, 4))))
    refused(ARG_, "2^31 rows per pass and more", chunk_=1024, P=C.byref(big), pitch=2048, nbytes=1 << 62)
    # ... and the same call goes through once nothing is wrong with it
    assert raw.call(chunk, buf, n, out, stats, stream) == 0
    stream.synchronize()
    assert not cr.frame_problems(out.cpu().numpy()[:, :raw.W], _one_pass(env, case.name, "notebook")["frame"])


def test_python_wrapper_refuses_what_it_cannot_render(env):
    case = cc.CASES["quad_overlays_8x8"]
    three = ref.glorot_net(np.random.default_rng(3), 16, 3, (17, 13, 4), (1,), (1,))
    with pytest.raises(ValueError):
        _render(env, case, three, (1,), (1,))
    wide = ref.glorot_net(np.random.default_rng(4), 256, 4, (256, 256, 4), (1,), (1,))
    with pytest.raises(ValueError):
        _render(env, case, wide, (1,), (1,))


def test_render_brats_inr_still_equals_its_own_one_pass_form(env):
    """mrirt_render_brats_inr after its frame loop was factored out: the comparison of tests/test_gpu_c5_cases.py, repeated."""
    case, r = cc.CASES["linear_shaded_56x40"], cr.reference("linear_shaded_56x40")
    net = _net(env, case.net)
    g, gl = _bound(env, case)
    _, _, zmu, zsg = cc.volumes(case.dims, case.vol_seed)
    kw = dict(labels=gl, ext=cc.gpu_ext(case), return_aux=True)
    one, a1 = env["inr"].render_brats_inr(cc.params_of(case), g, net, zmu, zsg, one_pass=True, **kw)
    for c in (1, 7, 96, None):
        img, aux = env["inr"].render_brats_inr(cc.params_of(case), g, net, zmu, zsg, chunk_steps=c, **kw)
        assert np.array_equal(img.cpu().numpy(), one.cpu().numpy()), c
        assert (aux["live_samples"], aux["shaded_samples"]) == (a1["live_samples"], a1["shaded_samples"])
        assert not cr.counter_problems(aux, r, aux["chunk_steps"])
    assert not cr.frame_problems(one.cpu().numpy(), r["frame"])
