// torch.ops.mrirt_native.* — the C ABI of libmrirt.so (include/mrirt.h) registered as PyTorch operators from C++.
//
// Same contract as the Python registrations in mrirt/torch_ops.py (torch.ops.mrirt.*): device tensors in, a device
// tensor out, launched on the current HIP stream, no synchronisation; parameter blocks travel as CPU uint8 tensors
// holding the C structs byte for byte; every size check the C side cannot make (it only sees pointers) is made here.
// No device code in this file: it is compiled by the host compiler against the torch headers and linked to
// libmrirt.so, whose kernels do the work.  Replaces kernel.dispatch of inr/viewer/brats_viewer.py:431-442,
// scripts/volumeRendering/app.py:350-358, scripts/raymarch/app.py:212-223 and scripts/mesh_rt/app.py:233-243 for callers that want operators.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <cstring>
#include <optional>
#include <tuple>
#include <vector>

#include "mrirt.h"

namespace {

using at::Tensor;
using OptTensor = std::optional<Tensor>;

template <typename T>
T unblob(const Tensor& t, const char* what) {
    TORCH_CHECK_TYPE(t.device().is_cpu() && t.scalar_type() == at::kByte && t.numel() == (int64_t)sizeof(T),
                     "expected a CPU uint8 tensor of ", sizeof(T), " bytes (", what, ")");
    T v;
    const Tensor c = t.contiguous();
    std::memcpy(&v, c.data_ptr(), sizeof(T));
    return v;
}

const void* dev_ptr(const OptTensor& t, at::ScalarType dt, const char* what) {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK_TYPE(t->is_cuda() && t->scalar_type() == dt && t->is_contiguous(), what, ": expected a contiguous device tensor of the right dtype");
    return t->data_ptr();
}

// The kernels are launched on the current stream OF THE TENSORS' DEVICE: every operator first checks that all its
// device tensors live on one GPU, then makes that GPU current for the allocation of the output and for the stream
// lookup (with device 0 current and the grids on device 1 the launch would otherwise go to device 0's
// stream with device-1 pointers).
using DeviceGuard = c10::hip::OptionalHIPGuardMasqueradingAsCUDA;

void same_device(std::optional<at::Device>& dev, const OptTensor& t, const char* what) {
    if (!t.has_value()) return;
    TORCH_CHECK_TYPE(t->is_cuda(), what, ": expected a device tensor");
    if (!dev.has_value()) dev = t->device();
    TORCH_CHECK_VALUE(t->device() == *dev, what, " is on ", t->device(), " but another operand is on ", *dev,
                      ": every device tensor of one call must live on the same GPU");
}

void* current_stream() { return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

void check(int rc, const char* where) {
    TORCH_CHECK(rc == MRIRT_OK, where, ": ", mrirt_status_string(rc), " [status ", rc, "]");
}

std::vector<int64_t> out_shape(uint32_t width, uint32_t height, const MrirtRenderExt& e) {
    if (e.tileSize > 0) {
        const int64_t local = mrirt_tiles_for_rank(width, height, e.tileSize, e.tileRank, e.tileWorld);
        return { local, (int64_t)e.tileSize, (int64_t)e.tileSize, 4 };
    }
    return { (int64_t)height, (int64_t)width, 4 };
}

int64_t grid_need(const uint32_t dims[3], uint32_t layout) {
    switch (layout) {
        case MRIRT_LAYOUT_LINEAR: return (int64_t)dims[0] * dims[1] * dims[2];
        case MRIRT_LAYOUT_BRICK:  return mrirt_brick_elems(dims);
        case MRIRT_LAYOUT_VGA:    return 4 * mrirt_vga_elems(dims);
        case MRIRT_LAYOUT_LABCELL: return 2 * mrirt_vec4_elems(dims);      // 8-byte elements, counted in int32
        default:                  return 4 * mrirt_vec4_elems(dims);
    }
}

// brats_main (inr/viewer/brats_rt.slang:85-168) through mrirt_render_brats_ex
Tensor render_brats(const Tensor& params, const Tensor& ext, const OptTensor& vol0, const OptTensor& vol1,
                    const OptTensor& vol2, const OptTensor& vol3, const OptTensor& labels, const OptTensor& preds) {
    const MrirtBratsParams P = unblob<MrirtBratsParams>(params, "MrirtBratsParams");
    const MrirtRenderExt E = unblob<MrirtRenderExt>(ext, "MrirtRenderExt");
    const OptTensor* vols[4] = { &vol0, &vol1, &vol2, &vol3 };
    const char* names[4] = { "gIntensity0", "gIntensity1", "gIntensity2", "gIntensity3" };
    const void* vp[4];
    const int64_t need = grid_need(P.dims, E.layout), lneed = grid_need(P.dims, E.labelLayout);
    std::optional<at::Device> dev;
    const bool mod4 = E.layout == MRIRT_LAYOUT_MOD4;                    // vol0 = the float4 grid of all four modalities
    for (int m = 0; m < 4; ++m) {
        vp[m] = dev_ptr(*vols[m], at::kFloat, names[m]);
        same_device(dev, *vols[m], names[m]);
        const bool wanted = mod4 ? m == 0 : P.volEnabled[m] != 0;
        TORCH_CHECK_VALUE(!wanted || (vols[m]->has_value() && (*vols[m])->numel() >= need),
                          names[m], mod4 ? " (the MOD4 grid) holds fewer than " : " is enabled but holds fewer than ", need, " elements");
    }
    TORCH_CHECK_VALUE(dev.has_value(), "no intensity grid bound");
    const void* lab = dev_ptr(labels, at::kInt, "gLabels");
    const void* prd = dev_ptr(preds, at::kInt, "gPreds");
    TORCH_CHECK_VALUE(P.showSeg == 0 || (labels.has_value() && labels->numel() >= lneed), "showSeg is set but gLabels is missing or too small");
    const bool cells = E.labelLayout == MRIRT_LAYOUT_LABCELL;          // gLabels carries both grids, gPreds is ignored
    const OptTensor& predSrc = cells ? labels : preds;
    TORCH_CHECK_VALUE(P.showPred == 0 || (predSrc.has_value() && predSrc->numel() >= lneed), "showPred is set but gPreds (or the label-cell grid) is missing or too small");
    same_device(dev, labels, "gLabels");
    same_device(dev, preds, "gPreds");
    DeviceGuard guard(*dev);
    const auto dt = E.outFormat == MRIRT_OUT_RGBA16F ? at::kHalf : at::kFloat;
    Tensor out = at::empty(out_shape(P.imageSize[0], P.imageSize[1], E), at::TensorOptions().dtype(dt).device(*dev));
    check(mrirt_render_brats_ex(&P, &E, vp, lab, prd, out.data_ptr(), (int64_t)P.imageSize[0], nullptr, current_stream()),
          "mrirt_render_brats_ex");
    return out;
}

// gradients of one K1 frame on LINEAR fp32 grids through mrirt_render_brats_backward: dL/dvol0..3 (an empty tensor for a modality
// that is disabled or not bound; an empty tensor also stands for an absent modality on the way in) and dL/d(ww, wl,
// intensityAlpha, gamma) as float64 [4]; freshly zeroed outputs
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> render_brats_backward(const Tensor& params, const Tensor& ext, const Tensor& grad_out,
                                                                         const OptTensor& vol0, const OptTensor& vol1, const OptTensor& vol2,
                                                                         const OptTensor& vol3, const OptTensor& labels, const OptTensor& preds) {
    const MrirtBratsParams P = unblob<MrirtBratsParams>(params, "MrirtBratsParams");
    const MrirtRenderExt E = unblob<MrirtRenderExt>(ext, "MrirtRenderExt");
    const auto present = [](const OptTensor& t) { return t.has_value() && t->numel() != 0 ? t : OptTensor(); };
    const OptTensor vols[4] = { present(vol0), present(vol1), present(vol2), present(vol3) };
    const OptTensor lab = present(labels), prd = present(preds);
    const char* names[4] = { "gIntensity0", "gIntensity1", "gIntensity2", "gIntensity3" };
    const int64_t nvox = (int64_t)P.dims[0] * P.dims[1] * P.dims[2];
    const int64_t W = P.imageSize[0], H = P.imageSize[1];
    std::optional<at::Device> dev;
    const float* g = static_cast<const float*>(dev_ptr(grad_out, at::kFloat, "grad_out"));
    same_device(dev, grad_out, "grad_out");
    TORCH_CHECK_VALUE(grad_out.dim() == 3 && grad_out.size(0) == H && grad_out.size(1) == W && grad_out.size(2) == 4,
                      "grad_out: expected (", H, ", ", W, ", 4)");
    const float* vp[4];
    for (int m = 0; m < 4; ++m) {
        vp[m] = static_cast<const float*>(dev_ptr(vols[m], at::kFloat, names[m]));
        same_device(dev, vols[m], names[m]);
        TORCH_CHECK_VALUE(P.volEnabled[m] == 0 || (vols[m].has_value() && vols[m]->numel() >= nvox),
                          names[m], " is enabled but holds fewer than ", nvox, " elements");
    }
    const uint32_t* lp = static_cast<const uint32_t*>(dev_ptr(lab, at::kInt, "gLabels"));
    const uint32_t* pp = static_cast<const uint32_t*>(dev_ptr(prd, at::kInt, "gPreds"));
    TORCH_CHECK_VALUE(P.showSeg == 0 || (lab.has_value() && lab->numel() >= nvox), "showSeg is set but gLabels is missing or too small");
    TORCH_CHECK_VALUE(P.showPred == 0 || (prd.has_value() && prd->numel() >= nvox), "showPred is set but gPreds is missing or too small");
    same_device(dev, lab, "gLabels");
    same_device(dev, prd, "gPreds");
    DeviceGuard guard(*dev);
    Tensor gv[4];
    float* gp[4];
    for (int m = 0; m < 4; ++m) {
        const bool on = P.volEnabled[m] != 0 && vols[m].has_value();
        gv[m] = at::zeros({ on ? nvox : 0 }, at::TensorOptions().dtype(at::kFloat).device(*dev));
        gp[m] = on ? gv[m].data_ptr<float>() : nullptr;
    }
    Tensor gtf = at::zeros({ 4 }, at::TensorOptions().dtype(at::kDouble).device(*dev));
    check(mrirt_render_brats_backward(&P, &E, vp, lp, pp, g, W, gp, gtf.data_ptr<double>(), current_stream()),
          "mrirt_render_brats_backward");
    return { gv[0], gv[1], gv[2], gv[3], gtf };
}

// The soft prediction overlay (mrirt_render_brats_soft / _backward): the checks the two operators share.  An empty tensor stands
// for an absent grid, as in render_brats_backward.
struct SoftBound {
    MrirtBratsParams P;
    MrirtRenderExt E;
    const float* vp[4];
    const uint32_t* lab;
    std::optional<at::Device> dev;
};

SoftBound bind_soft(const Tensor& params, const Tensor& ext, const Tensor& logits, const Tensor& offsets, const OptTensor& vol0,
                    const OptTensor& vol1, const OptTensor& vol2, const OptTensor& vol3, const OptTensor& labels) {
    SoftBound b;
    b.P = unblob<MrirtBratsParams>(params, "MrirtBratsParams");
    b.E = unblob<MrirtRenderExt>(ext, "MrirtRenderExt");
    const auto present = [](const OptTensor& t) { return t.has_value() && t->numel() != 0 ? t : OptTensor(); };
    const OptTensor vols[4] = { present(vol0), present(vol1), present(vol2), present(vol3) };
    const OptTensor lab = present(labels);
    const char* names[4] = { "gIntensity0", "gIntensity1", "gIntensity2", "gIntensity3" };
    const int64_t nvox = (int64_t)b.P.dims[0] * b.P.dims[1] * b.P.dims[2];
    dev_ptr(logits, at::kFloat, "logits");
    dev_ptr(offsets, at::kLong, "offsets");
    same_device(b.dev, logits, "logits");
    same_device(b.dev, offsets, "offsets");
    TORCH_CHECK_VALUE(logits.dim() == 2 && logits.size(1) >= 1 && logits.size(1) <= 16, "logits: expected (rows, 1..16 classes)");
    TORCH_CHECK_VALUE(offsets.numel() == (int64_t)b.P.imageSize[0] * b.P.imageSize[1], "offsets: expected one element per pixel");
    for (int m = 0; m < 4; ++m) {
        b.vp[m] = static_cast<const float*>(dev_ptr(vols[m], at::kFloat, names[m]));
        same_device(b.dev, vols[m], names[m]);
        TORCH_CHECK_VALUE(b.P.volEnabled[m] == 0 || (vols[m].has_value() && vols[m]->numel() >= nvox),
                          names[m], " is enabled but holds fewer than ", nvox, " elements");
    }
    b.lab = static_cast<const uint32_t*>(dev_ptr(lab, at::kInt, "gLabels"));
    TORCH_CHECK_VALUE(b.P.showSeg == 0 || (lab.has_value() && lab->numel() >= nvox), "showSeg is set but gLabels is missing or too small");
    same_device(b.dev, lab, "gLabels");
    return b;
}

Tensor render_brats_soft(const Tensor& params, const Tensor& ext, const Tensor& logits, const Tensor& offsets, const OptTensor& vol0,
                         const OptTensor& vol1, const OptTensor& vol2, const OptTensor& vol3, const OptTensor& labels) {
    const SoftBound b = bind_soft(params, ext, logits, offsets, vol0, vol1, vol2, vol3, labels);
    DeviceGuard guard(*b.dev);
    const int64_t W = b.P.imageSize[0], H = b.P.imageSize[1];
    Tensor out = at::empty({ H, W, 4 }, at::TensorOptions().dtype(at::kFloat).device(*b.dev));
    check(mrirt_render_brats_soft(&b.P, &b.E, b.vp, b.lab, logits.data_ptr<float>(), (uint32_t)logits.size(1), offsets.data_ptr<int64_t>(),
                                  out.data_ptr<float>(), W, nullptr, current_stream()),
          "mrirt_render_brats_soft");
    return out;
}

Tensor render_brats_soft_backward(const Tensor& params, const Tensor& ext, const Tensor& grad_out, const Tensor& logits,
                                  const Tensor& offsets, const OptTensor& vol0, const OptTensor& vol1, const OptTensor& vol2,
                                  const OptTensor& vol3, const OptTensor& labels) {
    SoftBound b = bind_soft(params, ext, logits, offsets, vol0, vol1, vol2, vol3, labels);
    const int64_t W = b.P.imageSize[0], H = b.P.imageSize[1];
    const float* g = static_cast<const float*>(dev_ptr(grad_out, at::kFloat, "grad_out"));
    same_device(b.dev, grad_out, "grad_out");
    TORCH_CHECK_VALUE(grad_out.dim() == 3 && grad_out.size(0) == H && grad_out.size(1) == W && grad_out.size(2) == 4,
                      "grad_out: expected (", H, ", ", W, ", 4)");
    DeviceGuard guard(*b.dev);
    Tensor dl = at::zeros_like(logits);
    check(mrirt_render_brats_soft_backward(&b.P, &b.E, b.vp, b.lab, logits.data_ptr<float>(), (uint32_t)logits.size(1),
                                           offsets.data_ptr<int64_t>(), g, W, dl.data_ptr<float>(), current_stream()),
          "mrirt_render_brats_soft_backward");
    return dl;
}

// volume_cs (scripts/volumeRendering/volume_render.slang:104-148) through mrirt_render_volume
Tensor render_volume(const Tensor& params, const Tensor& ext, const Tensor& volume, int64_t mode) {
    const MrirtVolumeParams P = unblob<MrirtVolumeParams>(params, "MrirtVolumeParams");
    const MrirtRenderExt E = unblob<MrirtRenderExt>(ext, "MrirtRenderExt");
    TORCH_CHECK_VALUE(mode >= 0 && mode <= 2, "mode must be 0 (u32x4), 1 (u8) or 2 (f32)");
    const at::ScalarType want = mode == 0 ? at::kInt : mode == 1 ? at::kByte : at::kFloat;
    const void* vol = dev_ptr(volume, want, "gVolumeU8");
    const int64_t nvox = (int64_t)P.volDim[0] * P.volDim[1] * P.volDim[2];
    TORCH_CHECK_VALUE(volume.numel() >= nvox, "gVolumeU8 holds fewer than ", nvox, " voxels");
    DeviceGuard guard(volume.device());
    const auto dt = E.outFormat == MRIRT_OUT_RGBA16F ? at::kHalf : at::kFloat;
    Tensor out = at::empty(out_shape(P.imageSize[0], P.imageSize[1], E), at::TensorOptions().dtype(dt).device(volume.device()));
    check(mrirt_render_volume(&P, &E, vol, (uint32_t)mode, out.data_ptr(), (int64_t)P.imageSize[0], nullptr, current_stream()),
          "mrirt_render_volume");
    return out;
}

// raymarch_cs (scripts/raymarch/raymarch.slang:60-99); `like` only names the device
Tensor render_sdf(const Tensor& params, int64_t width, int64_t height, const Tensor& like) {
    const MrirtSdfParams P = unblob<MrirtSdfParams>(params, "MrirtSdfParams");
    TORCH_CHECK_TYPE(like.is_cuda(), "like: expected a device tensor");
    DeviceGuard guard(like.device());
    Tensor out = at::empty({ height, width, 4 }, at::TensorOptions().dtype(at::kFloat).device(like.device()));
    check(mrirt_render_sdf(&P, (uint32_t)width, (uint32_t)height, out.data_ptr<float>(), width, current_stream()), "mrirt_render_sdf");
    return out;
}

// compute_main (scripts/mesh_rt/mesh_rt.slang:138-164) through mrirt_render_mesh; the counts are the buffers' sizes
// (nodes float32 [2N x 4], tris int32 [M x 4], verts float32 [V x 4]), so the kernel's guards keep every read inside them
Tensor render_mesh(const Tensor& params, const Tensor& ext, const Tensor& nodes, const Tensor& tris, const Tensor& verts,
                   int64_t max_depth) {
    const MrirtMeshParams P = unblob<MrirtMeshParams>(params, "MrirtMeshParams");
    const MrirtRenderExt E = unblob<MrirtRenderExt>(ext, "MrirtRenderExt");
    const float* n = static_cast<const float*>(dev_ptr(nodes, at::kFloat, "gBVHNodes"));
    const uint32_t* t = static_cast<const uint32_t*>(dev_ptr(tris, at::kInt, "gTris"));
    const float* v = static_cast<const float*>(dev_ptr(verts, at::kFloat, "gVerts"));
    std::optional<at::Device> dev;
    same_device(dev, nodes, "gBVHNodes");
    same_device(dev, tris, "gTris");
    same_device(dev, verts, "gVerts");
    TORCH_CHECK_VALUE(max_depth >= 0 && max_depth <= 64, "max_depth must be in [0, 64]");
    DeviceGuard guard(*dev);
    const auto dt = E.outFormat == MRIRT_OUT_RGBA16F ? at::kHalf : at::kFloat;
    Tensor out = at::empty({ (int64_t)P.imageSize[1], (int64_t)P.imageSize[0], 4 }, at::TensorOptions().dtype(dt).device(*dev));
    const int64_t nc = nodes.numel() / 8, tc = tris.numel() / 4, vc = verts.numel() / 4;
    TORCH_CHECK_VALUE(nc < (1 << 30) && tc < (1 << 30) && vc < (1ll << 32), "buffer too large");
    check(mrirt_render_mesh(&P, &E, n, (uint32_t)nc, t, (uint32_t)tc, v, (uint32_t)vc, (uint32_t)max_depth, out.data_ptr(),
                            (int64_t)P.imageSize[0], nullptr, nullptr, current_stream()),
          "mrirt_render_mesh");
    return out;
}

// logits [n, out_dim] of the packed MLP (inr/inr/model.py:21-50 for kind 0, notebooks/neumors_inr.ipynb:1165-1178 for
// kind 1; kinds 2 / 3 take the [n, in_dim] input matrix in `feats`) through mrirt_inr_forward
Tensor inr_forward(const Tensor& weights, const Tensor& biases, int64_t kind, int64_t num_layers, int64_t in_dim, int64_t out_dim,
                   int64_t hidden, int64_t fourier_freqs, int64_t num_mods, double w0, const OptTensor& coords,
                   const OptTensor& feats, int64_t n) {
    MrirtInrDesc d;
    std::memset(&d, 0, sizeof d);
    d.kind = (uint32_t)kind; d.numLayers = (uint32_t)num_layers; d.inDim = (uint32_t)in_dim; d.outDim = (uint32_t)out_dim;
    d.hidden = (uint32_t)hidden; d.fourierFreqs = (uint32_t)fourier_freqs; d.numMods = (uint32_t)num_mods; d.w0 = (float)w0;
    const int64_t need = mrirt_inr_pack_bytes(&d);
    TORCH_CHECK_VALUE(need > 0, "unsupported network shape");
    TORCH_CHECK_TYPE(weights.is_cuda() && weights.scalar_type() == at::kByte && weights.numel() >= need,
                     "weights: expected the ", need, "-byte packed image of mrirt_inr_pack_weights on the device");
    const int64_t nb = (num_layers - 1) * hidden + ((out_dim + 31) / 32) * 32;
    d.weights = weights.data_ptr();
    d.biases = static_cast<const float*>(dev_ptr(biases, at::kFloat, "biases"));
    TORCH_CHECK_VALUE(biases.numel() >= nb, "biases holds fewer than ", nb, " floats (each layer padded to a multiple of 32)");
    const float* co = static_cast<const float*>(dev_ptr(coords, at::kFloat, "coords"));
    const float* fe = static_cast<const float*>(dev_ptr(feats, at::kFloat, "feats"));
    TORCH_CHECK_VALUE(kind >= 2 || (coords.has_value() && coords->numel() >= 3 * n), "coords must hold [n, 3] floats");
    const int64_t width = kind >= 2 ? in_dim : num_mods;
    TORCH_CHECK_VALUE(width == 0 || (feats.has_value() && feats->numel() >= width * n), "feats must hold [n, ", width, "] floats");
    std::optional<at::Device> dev = weights.device();
    same_device(dev, biases, "biases");
    same_device(dev, coords, "coords");
    same_device(dev, feats, "feats");
    DeviceGuard guard(*dev);
    Tensor out = at::empty({ n, out_dim }, at::TensorOptions().dtype(at::kFloat).device(weights.device()));
    check(mrirt_inr_forward(&d, co, fe, n, out.data_ptr<float>(), nullptr, current_stream()), "mrirt_inr_forward");
    return out;
}

// ---- INR training step (fp32): mrirt_inr_forward_f32 / mrirt_inr_loss / mrirt_inr_backward ----
struct TrainShape { MrirtInrDesc d; int64_t bytes, nw, nb; };

TrainShape train_shape(int64_t kind, int64_t num_layers, int64_t in_dim, int64_t out_dim, int64_t hidden, int64_t fourier_freqs,
                       int64_t num_mods, int64_t n) {
    TrainShape t;
    std::memset(&t.d, 0, sizeof t.d);
    t.d.kind = (uint32_t)kind; t.d.numLayers = (uint32_t)num_layers; t.d.inDim = (uint32_t)in_dim; t.d.outDim = (uint32_t)out_dim;
    t.d.hidden = (uint32_t)hidden; t.d.fourierFreqs = (uint32_t)fourier_freqs; t.d.numMods = (uint32_t)num_mods;
    t.bytes = mrirt_inr_train_scratch_bytes(&t.d, n);
    TORCH_CHECK_VALUE(t.bytes > 0, "unsupported network kind / shape / n for the training step (ReLU kinds only)");
    t.nw = in_dim * hidden + (num_layers - 2) * hidden * hidden + hidden * out_dim;
    t.nb = (num_layers - 1) * hidden + out_dim;
    return t;
}

// (logits [n, out_dim], scratch uint8): the fp32 forward that leaves its activations for inr_backward
std::tuple<Tensor, Tensor> inr_forward_f32(const Tensor& weights, const Tensor& biases, int64_t kind, int64_t num_layers, int64_t in_dim,
                                           int64_t out_dim, int64_t hidden, int64_t fourier_freqs, int64_t num_mods,
                                           const OptTensor& coords, const OptTensor& feats, int64_t n) {
    const TrainShape t = train_shape(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n);
    const float* w = static_cast<const float*>(dev_ptr(weights, at::kFloat, "weights"));
    const float* b = static_cast<const float*>(dev_ptr(biases, at::kFloat, "biases"));
    TORCH_CHECK_VALUE(weights.numel() >= t.nw && biases.numel() >= t.nb, "weights / biases are smaller than the network (", t.nw, " / ", t.nb, " floats)");
    const float* co = static_cast<const float*>(dev_ptr(coords, at::kFloat, "coords"));
    const float* fe = static_cast<const float*>(dev_ptr(feats, at::kFloat, "feats"));
    TORCH_CHECK_VALUE(kind >= 2 || (coords.has_value() && coords->numel() >= 3 * n), "coords must hold [n, 3] floats");
    const int64_t width = kind >= 2 ? in_dim : num_mods;
    TORCH_CHECK_VALUE(width == 0 || (feats.has_value() && feats->numel() >= width * n), "feats must hold [n, ", width, "] floats");
    std::optional<at::Device> dev = weights.device();
    same_device(dev, biases, "biases");
    same_device(dev, coords, "coords");
    same_device(dev, feats, "feats");
    DeviceGuard guard(*dev);
    Tensor out = at::empty({ n, out_dim }, at::TensorOptions().dtype(at::kFloat).device(*dev));
    Tensor scratch = at::empty({ t.bytes }, at::TensorOptions().dtype(at::kByte).device(*dev));
    check(mrirt_inr_forward_f32(&t.d, w, b, co, fe, n, out.data_ptr<float>(), scratch.data_ptr(), t.bytes, current_stream()),
          "mrirt_inr_forward_f32");
    return { out, scratch };
}

// (loss [1], aux [2, C], dlogits [n, C]) of the reference's loss (inr/inr/model.py:64-88) through mrirt_inr_loss
std::tuple<Tensor, Tensor, Tensor> inr_loss(const Tensor& logits, const Tensor& labels, at::ArrayRef<double> class_weights, double dice_weight) {
    const float* z = static_cast<const float*>(dev_ptr(logits, at::kFloat, "logits"));
    const int32_t* lab = static_cast<const int32_t*>(dev_ptr(labels, at::kInt, "labels"));
    TORCH_CHECK_VALUE(logits.dim() == 2 && logits.size(0) >= 1 && labels.numel() == logits.size(0), "logits must be [n, C] with n >= 1 and labels [n]");
    const int64_t n = logits.size(0), nc = logits.size(1);
    TORCH_CHECK_VALUE(nc >= 1 && nc <= 16 && (int64_t)class_weights.size() == nc, "1..16 classes, one class weight each");
    float cw[16];
    for (int64_t k = 0; k < nc; ++k) cw[k] = (float)class_weights[k];
    std::optional<at::Device> dev = logits.device();
    same_device(dev, labels, "labels");
    DeviceGuard guard(*dev);
    const int64_t nbytes = mrirt_inr_loss_scratch_bytes(n);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(*dev);
    Tensor loss = at::empty({ 1 }, f32), aux = at::empty({ 2, nc }, f32), dl = at::empty_like(logits);
    Tensor scratch = at::empty({ nbytes }, at::TensorOptions().dtype(at::kByte).device(*dev));
    check(mrirt_inr_loss(z, lab, n, (uint32_t)nc, cw, (float)dice_weight, loss.data_ptr<float>(), aux.data_ptr<float>(), dl.data_ptr<float>(),
                         scratch.data_ptr(), nbytes, current_stream()), "mrirt_inr_loss");
    return { loss, aux, dl };
}

// (loss [1], aux [2, C], terms [5], dlogits [n, C]) of scripts/jax_inr_brats.py's loss through mrirt_inr_loss_ext; focal_alpha
// empty: flags bit 1 clear
std::tuple<Tensor, Tensor, Tensor, Tensor> inr_loss_ext(const Tensor& logits, const Tensor& labels, at::ArrayRef<double> class_weights,
                                                        at::ArrayRef<double> focal_alpha, double dice_weight, bool per_class_dice, double focal_gamma,
                                                        double label_smoothing, double edema_fp_weight, double tversky_alpha, double tversky_beta,
                                                        double tversky_weight, double edema_logit_reg, int64_t edema_class) {
    const float* z = static_cast<const float*>(dev_ptr(logits, at::kFloat, "logits"));
    const int32_t* lab = static_cast<const int32_t*>(dev_ptr(labels, at::kInt, "labels"));
    TORCH_CHECK_VALUE(logits.dim() == 2 && logits.size(0) >= 1 && labels.numel() == logits.size(0), "logits must be [n, C] with n >= 1 and labels [n]");
    const int64_t n = logits.size(0), nc = logits.size(1);
    TORCH_CHECK_VALUE(nc >= 1 && nc <= 16 && (int64_t)class_weights.size() == nc, "1..16 classes, one class weight each");
    TORCH_CHECK_VALUE(focal_alpha.empty() || (int64_t)focal_alpha.size() == nc, "focal_alpha: empty, or one value per class");
    TORCH_CHECK_VALUE(edema_class >= 0 && edema_class <= 0xffffffffll, "edema_class must fit 32 bits");
    MrirtInrLossExt x;
    std::memset(&x, 0, sizeof x);
    for (int64_t k = 0; k < nc; ++k) {
        x.classWeights[k] = (float)class_weights[k];
        if (!focal_alpha.empty()) x.focalAlpha[k] = (float)focal_alpha[k];
    }
    x.diceWeight = (float)dice_weight; x.focalGamma = (float)focal_gamma; x.labelSmoothing = (float)label_smoothing;
    x.edemaFpWeight = (float)edema_fp_weight; x.tverskyAlpha = (float)tversky_alpha; x.tverskyBeta = (float)tversky_beta;
    x.tverskyWeight = (float)tversky_weight; x.edemaLogitReg = (float)edema_logit_reg;
    x.edemaClass = (uint32_t)edema_class;
    x.flags = (per_class_dice ? 1u : 0u) | (focal_alpha.empty() ? 0u : 2u);
    std::optional<at::Device> dev = logits.device();
    same_device(dev, labels, "labels");
    DeviceGuard guard(*dev);
    const int64_t nbytes = mrirt_inr_loss_ext_scratch_bytes(n);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(*dev);
    Tensor loss = at::empty({ 1 }, f32), aux = at::empty({ 2, nc }, f32), terms = at::empty({ 5 }, f32), dl = at::empty_like(logits);
    Tensor scratch = at::empty({ nbytes }, at::TensorOptions().dtype(at::kByte).device(*dev));
    check(mrirt_inr_loss_ext(z, lab, n, (uint32_t)nc, &x, loss.data_ptr<float>(), aux.data_ptr<float>(), terms.data_ptr<float>(), dl.data_ptr<float>(),
                             scratch.data_ptr(), nbytes, current_stream()), "mrirt_inr_loss_ext");
    return { loss, aux, terms, dl };
}

// (grad_w, grad_b) through mrirt_inr_backward from dlogits and the scratch inr_forward_f32 returned
std::tuple<Tensor, Tensor> inr_backward(const Tensor& weights, const Tensor& dlogits, const Tensor& scratch, int64_t kind, int64_t num_layers,
                                        int64_t in_dim, int64_t out_dim, int64_t hidden, int64_t fourier_freqs, int64_t num_mods, int64_t n) {
    const TrainShape t = train_shape(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n);
    const float* w = static_cast<const float*>(dev_ptr(weights, at::kFloat, "weights"));
    const float* dl = static_cast<const float*>(dev_ptr(dlogits, at::kFloat, "dlogits"));
    TORCH_CHECK_VALUE(weights.numel() >= t.nw && dlogits.numel() >= n * out_dim, "weights / dlogits are smaller than the network / [n, out_dim]");
    TORCH_CHECK_TYPE(scratch.is_cuda() && scratch.scalar_type() == at::kByte && scratch.is_contiguous() && scratch.numel() >= t.bytes,
                     "scratch: expected the ", t.bytes, "-byte device buffer of inr_forward_f32");
    std::optional<at::Device> dev = weights.device();
    same_device(dev, dlogits, "dlogits");
    same_device(dev, scratch, "scratch");
    DeviceGuard guard(*dev);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(*dev);
    Tensor gw = at::empty({ t.nw }, f32), gb = at::empty({ t.nb }, f32);
    check(mrirt_inr_backward(&t.d, w, n, dl, gw.data_ptr<float>(), gb.data_ptr<float>(), 0u, scratch.data_ptr(), scratch.numel(),
                             current_stream()), "mrirt_inr_backward");
    return { gw, gb };
}

// ---- INR training loop: mrirt_inr_sample_batch / mrirt_inr_adamw_step ----
// (coords [n, 3], feats [n, num_mods], labels int32 [n]); the tables are int64 device tensors of per-case device addresses
std::tuple<Tensor, Tensor, Tensor> inr_sample_batch(const OptTensor& mods_table, const Tensor& seg_table, int64_t num_mods, int64_t h, int64_t w,
                                                    int64_t d, int64_t seed, int64_t batch_index, int64_t n) {
    const void* st = dev_ptr(seg_table, at::kLong, "seg_table");
    const void* mt = dev_ptr(mods_table, at::kLong, "mods_table");
    TORCH_CHECK_VALUE(seg_table.numel() >= 1 && (num_mods <= 0 || (mods_table.has_value() && mods_table->numel() == seg_table.numel())),
                      "seg_table must hold one address per case, and mods_table as many when num_mods > 0");
    TORCH_CHECK_VALUE(num_mods >= 0 && h >= 0 && w >= 0 && d >= 0 && n >= 0, "negative extent");
    std::optional<at::Device> dev = seg_table.device();
    same_device(dev, mods_table, "mods_table");
    DeviceGuard guard(*dev);
    MrirtInrCache c;
    std::memset(&c, 0, sizeof c);
    c.mods = num_mods > 0 ? static_cast<const float* const*>(mt) : nullptr;
    c.seg = static_cast<const int16_t* const*>(st);
    c.ncases = (uint32_t)seg_table.numel(); c.numMods = (uint32_t)num_mods;
    c.hwd[0] = (uint32_t)h; c.hwd[1] = (uint32_t)w; c.hwd[2] = (uint32_t)d;
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(*dev);
    Tensor coords = at::empty({ n, 3 }, f32), feats = at::empty({ n, num_mods }, f32);
    Tensor labels = at::empty({ n }, at::TensorOptions().dtype(at::kInt).device(*dev));
    check(mrirt_inr_sample_batch(&c, (uint64_t)seed, (uint64_t)batch_index, n, coords.data_ptr<float>(),
                                 num_mods > 0 ? feats.data_ptr<float>() : nullptr, labels.data_ptr<int32_t>(), current_stream()),
          "mrirt_inr_sample_batch");
    return { coords, feats, labels };
}

// inr_sample_batch with the first n_tumour points drawn from the tumour index (mrirt_inr_sample_batch_mix): tumour_index the
// uint32 voxel offsets held in an int32 tensor, tumour_offsets int64 [ncases + 1]; both may be absent when n_tumour == 0
std::tuple<Tensor, Tensor, Tensor> inr_sample_batch_mix(const OptTensor& mods_table, const Tensor& seg_table, const OptTensor& tumour_index,
                                                        const OptTensor& tumour_offsets, int64_t num_mods, int64_t h, int64_t w, int64_t d,
                                                        int64_t seed, int64_t batch_index, int64_t n, int64_t n_tumour) {
    const void* st = dev_ptr(seg_table, at::kLong, "seg_table");
    const void* mt = dev_ptr(mods_table, at::kLong, "mods_table");
    const void* ti = dev_ptr(tumour_index, at::kInt, "tumour_index");
    const void* to = dev_ptr(tumour_offsets, at::kLong, "tumour_offsets");
    TORCH_CHECK_VALUE(seg_table.numel() >= 1 && (num_mods <= 0 || (mods_table.has_value() && mods_table->numel() == seg_table.numel())),
                      "seg_table must hold one address per case, and mods_table as many when num_mods > 0");
    TORCH_CHECK_VALUE(num_mods >= 0 && h >= 0 && w >= 0 && d >= 0 && n >= 0 && n_tumour >= 0, "negative extent");
    TORCH_CHECK_VALUE(n_tumour == 0 || (tumour_index.has_value() && tumour_offsets.has_value() && tumour_offsets->numel() == seg_table.numel() + 1),
                      "n_tumour > 0 needs tumour_index and tumour_offsets [ncases + 1]");
    std::optional<at::Device> dev = seg_table.device();
    same_device(dev, mods_table, "mods_table");
    same_device(dev, tumour_index, "tumour_index");
    same_device(dev, tumour_offsets, "tumour_offsets");
    DeviceGuard guard(*dev);
    MrirtInrCache c;
    std::memset(&c, 0, sizeof c);
    c.mods = num_mods > 0 ? static_cast<const float* const*>(mt) : nullptr;
    c.seg = static_cast<const int16_t* const*>(st);
    c.ncases = (uint32_t)seg_table.numel(); c.numMods = (uint32_t)num_mods;
    c.hwd[0] = (uint32_t)h; c.hwd[1] = (uint32_t)w; c.hwd[2] = (uint32_t)d;
    const MrirtInrTumourIndex t = { static_cast<const uint32_t*>(ti), static_cast<const int64_t*>(to) };
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(*dev);
    Tensor coords = at::empty({ n, 3 }, f32), feats = at::empty({ n, num_mods }, f32);
    Tensor labels = at::empty({ n }, at::TensorOptions().dtype(at::kInt).device(*dev));
    check(mrirt_inr_sample_batch_mix(&c, n_tumour > 0 ? &t : nullptr, (uint64_t)seed, (uint64_t)batch_index, n, n_tumour, coords.data_ptr<float>(),
                                     num_mods > 0 ? feats.data_ptr<float>() : nullptr, labels.data_ptr<int32_t>(), current_stream()),
          "mrirt_inr_sample_batch_mix");
    return { coords, feats, labels };
}

// [w, b, mu_w, mu_b, nu_w, nu_b, gnorm] after update t + 1 on copies of the flat parameters and moments
std::vector<Tensor> inr_adamw_step(const Tensor& w, const Tensor& b, const Tensor& gw, const Tensor& gb, const Tensor& mu_w, const Tensor& mu_b,
                                   const Tensor& nu_w, const Tensor& nu_b, double lr, double b1, double b2, double eps, double weight_decay,
                                   double clip_norm, int64_t t, double gscale) {
    const Tensor* ten[8] = { &w, &b, &gw, &gb, &mu_w, &mu_b, &nu_w, &nu_b };
    static const char* names[8] = { "w", "b", "gw", "gb", "mu_w", "mu_b", "nu_w", "nu_b" };
    std::optional<at::Device> dev = w.device();
    for (int i = 0; i < 8; ++i) {
        dev_ptr(*ten[i], at::kFloat, names[i]);
        same_device(dev, *ten[i], names[i]);
        TORCH_CHECK_VALUE(ten[i]->numel() == ten[i & 1]->numel(), "gradients and moments must have the sizes of w and b");
    }
    DeviceGuard guard(*dev);
    const int64_t nw = w.numel(), nb = b.numel();
    Tensor ow = w.clone(), ob = b.clone(), omw = mu_w.clone(), omb = mu_b.clone(), onw = nu_w.clone(), onb = nu_b.clone();
    const int64_t nbytes = mrirt_inr_adamw_scratch_bytes(nw + nb);
    Tensor scratch = at::empty({ nbytes > 16 ? nbytes : 16 }, at::TensorOptions().dtype(at::kByte).device(*dev));
    Tensor gnorm = at::empty({ 2 }, at::TensorOptions().dtype(at::kDouble).device(*dev));
    const MrirtAdamW hp = { (float)lr, (float)b1, (float)b2, (float)eps, (float)weight_decay, (float)clip_norm };
    check(mrirt_inr_adamw_step(ow.data_ptr<float>(), ob.data_ptr<float>(), gw.data_ptr<float>(), gb.data_ptr<float>(), omw.data_ptr<float>(),
                               omb.data_ptr<float>(), onw.data_ptr<float>(), onb.data_ptr<float>(), nw, nb, &hp, (uint64_t)t, (float)gscale,
                               gnorm.data_ptr<double>(), scratch.data_ptr(), nbytes, current_stream()), "mrirt_inr_adamw_step");
    return { ow, ob, omw, omb, onw, onb, gnorm };
}

// the volume's extent and spacing as the C ABI takes them; every label tensor is int16 (H, W, D) on one device
void edt_args(const Tensor& first, const OptTensor& second, at::ArrayRef<double> spacing, uint32_t hwd[3], float sp[3],
              std::optional<at::Device>& dev) {
    dev_ptr(first, at::kShort, "labels");
    dev_ptr(second, at::kShort, "labels");
    same_device(dev, first, "labels");
    same_device(dev, second, "labels");
    TORCH_CHECK_VALUE(first.dim() == 3 && (!second.has_value() || second->sizes() == first.sizes()),
                      "label volumes must be (H, W, D) int16 tensors of one shape");
    TORCH_CHECK_VALUE(spacing.size() == 3, "spacing: expected three values");
    for (int k = 0; k < 3; ++k) {
        TORCH_CHECK_VALUE(first.size(k) <= 0xFFFFFFFFll, "axis too long");
        hwd[k] = (uint32_t)first.size(k);
        sp[k] = (float)spacing[k];
    }
}

Tensor scratch_for(int64_t nbytes, at::Device dev) {
    return at::empty({ std::max<int64_t>(nbytes, 8) / 8 }, at::TensorOptions().dtype(at::kLong).device(dev));
}

// exact squared Euclidean distance transform of (labels == cls) through mrirt_edt_squared
Tensor edt_squared(const Tensor& labels, int64_t cls, at::ArrayRef<double> spacing) {
    uint32_t hwd[3];
    float sp[3];
    std::optional<at::Device> dev;
    edt_args(labels, std::nullopt, spacing, hwd, sp, dev);
    TORCH_CHECK_VALUE(cls >= INT32_MIN && cls <= INT32_MAX, "cls out of range");
    DeviceGuard guard(*dev);
    const int64_t nbytes = mrirt_edt_scratch_bytes(hwd, 0);
    Tensor out = at::empty(labels.sizes(), at::TensorOptions().dtype(at::kDouble).device(*dev));
    Tensor scratch = scratch_for(nbytes, *dev);
    check(mrirt_edt_squared(static_cast<const int16_t*>(labels.data_ptr()), hwd, (int32_t)cls, sp, out.data_ptr<double>(),
                            scratch.data_ptr(), nbytes, current_stream()), "mrirt_edt_squared");
    return out;
}

// squared directed Hausdorff distances [num_classes, 2] (inr/inr/model.py:164-195) through mrirt_hausdorff
Tensor hausdorff(const Tensor& pred, const Tensor& truth, at::ArrayRef<double> spacing, int64_t num_classes) {
    uint32_t hwd[3];
    float sp[3];
    std::optional<at::Device> dev;
    edt_args(pred, truth, spacing, hwd, sp, dev);
    TORCH_CHECK_VALUE(num_classes >= 1 && num_classes <= 32, "num_classes must be in [1, 32]");
    DeviceGuard guard(*dev);
    const int64_t nbytes = mrirt_edt_scratch_bytes(hwd, (uint32_t)num_classes);
    Tensor out = at::empty({ num_classes, 2 }, at::TensorOptions().dtype(at::kDouble).device(*dev));
    Tensor scratch = scratch_for(nbytes, *dev);
    check(mrirt_hausdorff(static_cast<const int16_t*>(pred.data_ptr()), static_cast<const int16_t*>(truth.data_ptr()), hwd, sp,
                          (uint32_t)num_classes, out.data_ptr<double>(), scratch.data_ptr(), nbytes, current_stream()),
          "mrirt_hausdorff");
    return out;
}

// the surface of the voxels whose label's bit is set in class_mask (naive surface nets): a (H, W, D) int16 device volume
int64_t surface_args(const Tensor& labels, int64_t class_mask, uint32_t hwd[3]) {
    dev_ptr(labels, at::kShort, "labels");
    TORCH_CHECK_VALUE(labels.dim() == 3, "labels must be an (H, W, D) int16 tensor");
    TORCH_CHECK_VALUE(class_mask >= 0 && class_mask <= 0xFFFFFFFFll, "class_mask: expected a uint32 bit set (bit l = label l is inside)");
    for (int k = 0; k < 3; ++k) {
        TORCH_CHECK_VALUE(labels.size(k) <= 0xFFFFFFFFll, "axis too long");
        hwd[k] = (uint32_t)labels.size(k);
    }
    const int64_t nbytes = mrirt_surface_scratch_bytes(hwd);
    TORCH_CHECK_VALUE(nbytes > 0, "the volume is outside the supported sizes");
    return nbytes;
}

// int64 [2]: vertices and triangles, through mrirt_surface_count
Tensor surface_count(const Tensor& labels, int64_t class_mask) {
    uint32_t hwd[3];
    const int64_t nbytes = surface_args(labels, class_mask, hwd);
    DeviceGuard guard(labels.device());
    Tensor counts = at::empty({ 2 }, at::TensorOptions().dtype(at::kLong).device(labels.device()));
    Tensor scratch = scratch_for(nbytes + 8, labels.device());
    check(mrirt_surface_count(static_cast<const int16_t*>(labels.data_ptr()), hwd, (uint32_t)class_mask, scratch.data_ptr(), nbytes,
                              counts.data_ptr<int64_t>(), current_stream()), "mrirt_surface_count");
    return counts;
}

// (verts float32 [num_verts, 3], tris int32 [num_tris, 3]) through mrirt_surface_extract; zeroed where nothing is written
std::tuple<Tensor, Tensor> surface_extract(const Tensor& labels, int64_t class_mask, at::ArrayRef<double> spacing,
                                           at::ArrayRef<double> origin, int64_t num_verts, int64_t num_tris) {
    uint32_t hwd[3];
    const int64_t nbytes = surface_args(labels, class_mask, hwd);
    TORCH_CHECK_VALUE(spacing.size() == 3 && origin.size() == 3, "spacing / origin: expected three values each");
    TORCH_CHECK_VALUE(num_verts >= 0 && num_tris >= 0, "num_verts / num_tris must not be negative");
    float sp[3], org[3];
    for (int k = 0; k < 3; ++k) { sp[k] = (float)spacing[k]; org[k] = (float)origin[k]; }
    DeviceGuard guard(labels.device());
    Tensor verts = at::zeros({ num_verts, 3 }, at::TensorOptions().dtype(at::kFloat).device(labels.device()));
    Tensor tris = at::zeros({ num_tris, 3 }, at::TensorOptions().dtype(at::kInt).device(labels.device()));
    Tensor counts = at::empty({ 2 }, at::TensorOptions().dtype(at::kLong).device(labels.device()));
    Tensor scratch = scratch_for(nbytes + 8, labels.device());
    check(mrirt_surface_extract(static_cast<const int16_t*>(labels.data_ptr()), hwd, (uint32_t)class_mask, sp, org,
                                num_verts ? verts.data_ptr<float>() : nullptr, num_verts, num_tris ? tris.data_ptr<int32_t>() : nullptr,
                                num_tris, scratch.data_ptr(), nbytes, counts.data_ptr<int64_t>(), current_stream()),
          "mrirt_surface_extract");
    return { verts, tris };
}

}  // namespace

TORCH_LIBRARY(mrirt_native, m) {
    m.def("render_brats(Tensor params, Tensor ext, Tensor? vol0, Tensor? vol1, Tensor? vol2, Tensor? vol3, Tensor? labels, Tensor? preds) -> Tensor");
    m.def("render_brats_backward(Tensor params, Tensor ext, Tensor grad_out, Tensor? vol0, Tensor? vol1, Tensor? vol2, Tensor? vol3, "
          "Tensor? labels, Tensor? preds) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("render_brats_soft(Tensor params, Tensor ext, Tensor logits, Tensor offsets, Tensor? vol0, Tensor? vol1, Tensor? vol2, Tensor? vol3, "
          "Tensor? labels) -> Tensor");
    m.def("render_brats_soft_backward(Tensor params, Tensor ext, Tensor grad_out, Tensor logits, Tensor offsets, Tensor? vol0, Tensor? vol1, "
          "Tensor? vol2, Tensor? vol3, Tensor? labels) -> Tensor");
    m.def("render_volume(Tensor params, Tensor ext, Tensor volume, int mode) -> Tensor");
    m.def("render_sdf(Tensor params, int width, int height, Tensor like) -> Tensor");
    m.def("render_mesh(Tensor params, Tensor ext, Tensor nodes, Tensor tris, Tensor verts, int max_depth) -> Tensor");
    m.def("inr_forward(Tensor weights, Tensor biases, int kind, int num_layers, int in_dim, int out_dim, int hidden, "
          "int fourier_freqs, int num_mods, float w0, Tensor? coords, Tensor? feats, int n) -> Tensor");
    m.def("inr_forward_f32(Tensor weights, Tensor biases, int kind, int num_layers, int in_dim, int out_dim, int hidden, "
          "int fourier_freqs, int num_mods, Tensor? coords, Tensor? feats, int n) -> (Tensor, Tensor)");
    m.def("inr_loss(Tensor logits, Tensor labels, float[] class_weights, float dice_weight) -> (Tensor, Tensor, Tensor)");
    m.def("inr_loss_ext(Tensor logits, Tensor labels, float[] class_weights, float[] focal_alpha, float dice_weight, bool per_class_dice, "
          "float focal_gamma, float label_smoothing, float edema_fp_weight, float tversky_alpha, float tversky_beta, float tversky_weight, "
          "float edema_logit_reg, int edema_class) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("inr_sample_batch_mix(Tensor? mods_table, Tensor seg_table, Tensor? tumour_index, Tensor? tumour_offsets, int num_mods, int h, int w, "
          "int d, int seed, int batch_index, int n, int n_tumour) -> (Tensor, Tensor, Tensor)");
    m.def("inr_backward(Tensor weights, Tensor dlogits, Tensor scratch, int kind, int num_layers, int in_dim, int out_dim, int hidden, "
          "int fourier_freqs, int num_mods, int n) -> (Tensor, Tensor)");
    m.def("inr_sample_batch(Tensor? mods_table, Tensor seg_table, int num_mods, int h, int w, int d, int seed, int batch_index, int n) "
          "-> (Tensor, Tensor, Tensor)");
    m.def("inr_adamw_step(Tensor w, Tensor b, Tensor gw, Tensor gb, Tensor mu_w, Tensor mu_b, Tensor nu_w, Tensor nu_b, float lr, float b1, "
          "float b2, float eps, float weight_decay, float clip_norm, int t, float gscale) -> Tensor[]");
    m.def("edt_squared(Tensor labels, int cls, float[] spacing) -> Tensor");
    m.def("hausdorff(Tensor pred, Tensor truth, float[] spacing, int num_classes) -> Tensor");
    m.def("surface_count(Tensor labels, int class_mask) -> Tensor");
    m.def("surface_extract(Tensor labels, int class_mask, float[] spacing, float[] origin, int num_verts, int num_tris) -> (Tensor, Tensor)");
}

// the parameter blocks are CPU tensors and the grids device tensors: no single dispatch key fits, so the
// implementations are registered for every backend and check their arguments themselves
TORCH_LIBRARY_IMPL(mrirt_native, CompositeExplicitAutograd, m) {
    m.impl("render_brats", &render_brats);
    m.impl("render_brats_backward", &render_brats_backward);
    m.impl("render_brats_soft", &render_brats_soft);
    m.impl("render_brats_soft_backward", &render_brats_soft_backward);
    m.impl("render_volume", &render_volume);
    m.impl("render_sdf", &render_sdf);
    m.impl("render_mesh", &render_mesh);
    m.impl("inr_forward", &inr_forward);
    m.impl("inr_forward_f32", &inr_forward_f32);
    m.impl("inr_loss", &inr_loss);
    m.impl("inr_loss_ext", &inr_loss_ext);
    m.impl("inr_sample_batch_mix", &inr_sample_batch_mix);
    m.impl("inr_backward", &inr_backward);
    m.impl("inr_sample_batch", &inr_sample_batch);
    m.impl("inr_adamw_step", &inr_adamw_step);
    m.impl("edt_squared", &edt_squared);
    m.impl("hausdorff", &hausdorff);
    m.impl("surface_count", &surface_count);
    m.impl("surface_extract", &surface_extract);
}
