// torch.ops.mrirt_native.* — the C ABI of libmrirt.so (include/mrirt.h) registered as PyTorch operators from C++.
//
// Same contract as the Python registrations in mrirt/torch_ops.py (torch.ops.mrirt.*): device tensors in, a device
// tensor out, launched on the current HIP stream, no synchronisation; parameter blocks travel as CPU uint8 tensors
// holding the C structs byte for byte; every size check the C side cannot make (it only sees pointers) is made here.
// No device code in this file: it is compiled by the host compiler against the torch headers and linked to
// libmrirt.so, whose kernels do the work.  Replaces kernel.dispatch of inr/viewer/brats_viewer.py:431-442,
// scripts/volumeRendering/app.py:350-358, scripts/raymarch/app.py:212-223 and scripts/mesh_rt/app.py:233-243 for callers that want operators.
// The shared pieces mirror torch_ops.py's: bind_k1 (every K1 operator's operands), inr_desc / inr_inputs, loss_operands /
// loss_outputs, sampler_cache / sample_outputs.  tests/test_torch_ops_contract.py holds the operator list and the schemas
// to the Python door's: a new operator is added there first.
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
using OptDevice = std::optional<at::Device>;

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

void same_device(OptDevice& dev, const OptTensor& t, const char* what) {
    if (!t.has_value()) return;
    TORCH_CHECK_TYPE(t->is_cuda(), what, ": expected a device tensor");
    if (!dev.has_value()) dev = t->device();
    TORCH_CHECK_VALUE(t->device() == *dev, what, " is on ", t->device(), " but another operand is on ", *dev,
                      ": every device tensor of one call must live on the same GPU");
}

// a device operand: dtype and contiguity checked, and on the same GPU as the operands before it
const void* operand(OptDevice& dev, const OptTensor& t, at::ScalarType dt, const char* what) {
    const void* p = dev_ptr(t, dt, what);
    same_device(dev, t, what);
    return p;
}

void* current_stream() { return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

void check(int rc, const char* where) {
    TORCH_CHECK(rc == MRIRT_OK, where, ": ", mrirt_status_string(rc), " [status ", rc, "]");
}

at::TensorOptions opts(at::ScalarType dt, at::Device dev) { return at::TensorOptions().dtype(dt).device(dev); }

// an empty tensor stands for an absent one (the differentiable K1 operators)
OptTensor present(const OptTensor& t) { return t.has_value() && t->numel() != 0 ? t : OptTensor(); }

// the extent of a (H, W, D) volume as the C ABI takes it
void fill_hwd(const Tensor& t, uint32_t hwd[3]) {
    for (int k = 0; k < 3; ++k) {
        TORCH_CHECK_VALUE(t.size(k) <= 0xFFFFFFFFll, "axis too long");
        hwd[k] = (uint32_t)t.size(k);
    }
}

// the frame of K1 / K2 / K4: [H, W, 4], or this rank's tiles; fp16 when the ext asks for it
Tensor new_frame(const uint32_t imageSize[2], const MrirtRenderExt& e, at::Device dev) {
    const auto o = opts(e.outFormat == MRIRT_OUT_RGBA16F ? at::kHalf : at::kFloat, dev);
    if (e.tileSize > 0)
        return at::empty({ mrirt_tiles_for_rank(imageSize[0], imageSize[1], e.tileSize, e.tileRank, e.tileWorld), (int64_t)e.tileSize, (int64_t)e.tileSize, 4 }, o);
    return at::empty({ (int64_t)imageSize[1], (int64_t)imageSize[0], 4 }, o);
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

// the differentiable operators take LINEAR grids whatever ext says
int64_t linear_need(const uint32_t dims[3], uint32_t) { return (int64_t)dims[0] * dims[1] * dims[2]; }

// ---- K1: the operand binding every K1 operator shares ----
constexpr uint32_t kNoLayout = 0xFFFFFFFFu;

struct K1Bound {
    MrirtBratsParams P;
    MrirtRenderExt E;
    const float* vp[4];                 // null: not bound
    const uint32_t *lab, *prd;
    const float* grad_out;
    OptDevice dev;
};

// The two parameter blocks, the four intensity grids, gLabels and gPreds checked for device, dtype, contiguity and size, all on
// one GPU.  need(dims, layout): the element count a grid of that layout holds; pred_overlay: whether the operator draws the
// hard prediction overlay (showPred) at all; empty_is_absent: an empty tensor stands for an absent grid.  With ext.layout ==
// one_grid_layout gIntensity0 alone carries every modality, with ext.labelLayout == cell_label_layout gLabels carries the
// predictions too.  grad_out: the fp32 [H, W, 4] frame gradient of a backward operator.  dev: the device of the operands the
// caller has already checked.
K1Bound bind_k1(const Tensor& params, const Tensor& ext, const OptTensor* const vol[4], const OptTensor& labels, const OptTensor& preds,
                int64_t (*need)(const uint32_t[3], uint32_t), bool pred_overlay, bool empty_is_absent, uint32_t one_grid_layout,
                uint32_t cell_label_layout, const OptTensor& grad_out = std::nullopt, OptDevice dev = std::nullopt) {
    static const char* const names[4] = { "gIntensity0", "gIntensity1", "gIntensity2", "gIntensity3" };
    K1Bound b;
    b.P = unblob<MrirtBratsParams>(params, "MrirtBratsParams");
    b.E = unblob<MrirtRenderExt>(ext, "MrirtRenderExt");
    b.dev = dev;
    b.grad_out = static_cast<const float*>(operand(b.dev, grad_out, at::kFloat, "grad_out"));
    const int64_t W = b.P.imageSize[0], H = b.P.imageSize[1];
    TORCH_CHECK_VALUE(!grad_out.has_value() || (grad_out->dim() == 3 && grad_out->size(0) == H && grad_out->size(1) == W && grad_out->size(2) == 4),
                      "grad_out: expected (", H, ", ", W, ", 4)");
    const int64_t vneed = need(b.P.dims, b.E.layout), lneed = need(b.P.dims, b.E.labelLayout);
    const bool one_grid = b.E.layout == one_grid_layout;
    for (int m = 0; m < 4; ++m) {
        const OptTensor v = empty_is_absent ? present(*vol[m]) : *vol[m];
        b.vp[m] = static_cast<const float*>(operand(b.dev, v, at::kFloat, names[m]));
        const bool wanted = one_grid ? m == 0 : b.P.volEnabled[m] != 0;
        TORCH_CHECK_VALUE(!wanted || (v.has_value() && v->numel() >= vneed),
                          names[m], one_grid ? " (the one grid of all modalities) holds fewer than " : " is enabled but holds fewer than ", vneed, " elements");
    }
    TORCH_CHECK_VALUE(b.dev.has_value(), "no intensity grid bound");
    const OptTensor lab = empty_is_absent ? present(labels) : labels, prd = empty_is_absent ? present(preds) : preds;
    b.lab = static_cast<const uint32_t*>(operand(b.dev, lab, at::kInt, "gLabels"));
    b.prd = static_cast<const uint32_t*>(operand(b.dev, prd, at::kInt, "gPreds"));
    TORCH_CHECK_VALUE(b.P.showSeg == 0 || (lab.has_value() && lab->numel() >= lneed), "showSeg is set but gLabels is missing or too small");
    const OptTensor& predSrc = b.E.labelLayout == cell_label_layout ? lab : prd;
    TORCH_CHECK_VALUE(!pred_overlay || b.P.showPred == 0 || (predSrc.has_value() && predSrc->numel() >= lneed),
                      "showPred is set but gPreds (or the label-cell grid) is missing or too small");
    return b;
}

// brats_main (inr/viewer/brats_rt.slang:85-168) through mrirt_render_brats_ex.  MOD4: vol0 = the float4 grid of all four
// modalities; LABCELL: gLabels carries both grids, gPreds is ignored
Tensor render_brats(const Tensor& params, const Tensor& ext, const OptTensor& vol0, const OptTensor& vol1,
                    const OptTensor& vol2, const OptTensor& vol3, const OptTensor& labels, const OptTensor& preds) {
    const OptTensor* vols[4] = { &vol0, &vol1, &vol2, &vol3 };
    const K1Bound b = bind_k1(params, ext, vols, labels, preds, grid_need, true, false, MRIRT_LAYOUT_MOD4, MRIRT_LAYOUT_LABCELL);
    DeviceGuard guard(*b.dev);
    Tensor out = new_frame(b.P.imageSize, b.E, *b.dev);
    check(mrirt_render_brats_ex(&b.P, &b.E, reinterpret_cast<const void* const*>(b.vp), b.lab, b.prd, out.data_ptr(),
                                (int64_t)b.P.imageSize[0], nullptr, current_stream()),
          "mrirt_render_brats_ex");
    return out;
}

// gradients of one K1 frame on LINEAR fp32 grids through mrirt_render_brats_backward: dL/dvol0..3 (an empty tensor for a modality
// that is disabled or not bound; an empty tensor also stands for an absent modality on the way in) and dL/d(ww, wl,
// intensityAlpha, gamma) as float64 [4]; freshly zeroed outputs
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> render_brats_backward(const Tensor& params, const Tensor& ext, const Tensor& grad_out,
                                                                         const OptTensor& vol0, const OptTensor& vol1, const OptTensor& vol2,
                                                                         const OptTensor& vol3, const OptTensor& labels, const OptTensor& preds) {
    const OptTensor* vols[4] = { &vol0, &vol1, &vol2, &vol3 };
    const K1Bound b = bind_k1(params, ext, vols, labels, preds, linear_need, true, true, kNoLayout, kNoLayout, grad_out);
    const int64_t nvox = linear_need(b.P.dims, 0);
    DeviceGuard guard(*b.dev);
    Tensor gv[4];
    float* gp[4];
    for (int m = 0; m < 4; ++m) {
        const bool on = b.P.volEnabled[m] != 0 && b.vp[m] != nullptr;
        gv[m] = at::zeros({ on ? nvox : 0 }, opts(at::kFloat, *b.dev));
        gp[m] = on ? gv[m].data_ptr<float>() : nullptr;
    }
    Tensor gtf = at::zeros({ 4 }, opts(at::kDouble, *b.dev));
    check(mrirt_render_brats_backward(&b.P, &b.E, b.vp, b.lab, b.prd, b.grad_out, (int64_t)b.P.imageSize[0], gp, gtf.data_ptr<double>(),
                                      current_stream()),
          "mrirt_render_brats_backward");
    return { gv[0], gv[1], gv[2], gv[3], gtf };
}

// The soft prediction overlay (mrirt_render_brats_soft / _backward): what the two operators add to bind_k1 (LINEAR grids, no
// hard prediction overlay, an empty tensor stands for an absent grid).
K1Bound bind_soft(const Tensor& params, const Tensor& ext, const Tensor& logits, const Tensor& offsets, const OptTensor& vol0,
                  const OptTensor& vol1, const OptTensor& vol2, const OptTensor& vol3, const OptTensor& labels,
                  const OptTensor& grad_out = std::nullopt) {
    OptDevice dev;
    operand(dev, logits, at::kFloat, "logits");
    operand(dev, offsets, at::kLong, "offsets");
    TORCH_CHECK_VALUE(logits.dim() == 2 && logits.size(1) >= 1 && logits.size(1) <= 16, "logits: expected (rows, 1..16 classes)");
    const OptTensor* vols[4] = { &vol0, &vol1, &vol2, &vol3 };
    const K1Bound b = bind_k1(params, ext, vols, labels, std::nullopt, linear_need, false, true, kNoLayout, kNoLayout, grad_out, dev);
    TORCH_CHECK_VALUE(offsets.numel() == (int64_t)b.P.imageSize[0] * b.P.imageSize[1], "offsets: expected one element per pixel");
    return b;
}

Tensor render_brats_soft(const Tensor& params, const Tensor& ext, const Tensor& logits, const Tensor& offsets, const OptTensor& vol0,
                         const OptTensor& vol1, const OptTensor& vol2, const OptTensor& vol3, const OptTensor& labels) {
    const K1Bound b = bind_soft(params, ext, logits, offsets, vol0, vol1, vol2, vol3, labels);
    DeviceGuard guard(*b.dev);
    const int64_t W = b.P.imageSize[0], H = b.P.imageSize[1];
    Tensor out = at::empty({ H, W, 4 }, opts(at::kFloat, *b.dev));
    check(mrirt_render_brats_soft(&b.P, &b.E, b.vp, b.lab, logits.data_ptr<float>(), (uint32_t)logits.size(1), offsets.data_ptr<int64_t>(),
                                  out.data_ptr<float>(), W, nullptr, current_stream()),
          "mrirt_render_brats_soft");
    return out;
}

Tensor render_brats_soft_backward(const Tensor& params, const Tensor& ext, const Tensor& grad_out, const Tensor& logits,
                                  const Tensor& offsets, const OptTensor& vol0, const OptTensor& vol1, const OptTensor& vol2,
                                  const OptTensor& vol3, const OptTensor& labels) {
    const K1Bound b = bind_soft(params, ext, logits, offsets, vol0, vol1, vol2, vol3, labels, grad_out);
    DeviceGuard guard(*b.dev);
    Tensor dl = at::zeros_like(logits);
    check(mrirt_render_brats_soft_backward(&b.P, &b.E, b.vp, b.lab, logits.data_ptr<float>(), (uint32_t)logits.size(1),
                                           offsets.data_ptr<int64_t>(), b.grad_out, (int64_t)b.P.imageSize[0], dl.data_ptr<float>(),
                                           current_stream()),
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
    Tensor out = new_frame(P.imageSize, E, volume.device());
    check(mrirt_render_volume(&P, &E, vol, (uint32_t)mode, out.data_ptr(), (int64_t)P.imageSize[0], nullptr, current_stream()),
          "mrirt_render_volume");
    return out;
}

// raymarch_cs (scripts/raymarch/raymarch.slang:60-99); `like` only names the device
Tensor render_sdf(const Tensor& params, int64_t width, int64_t height, const Tensor& like) {
    const MrirtSdfParams P = unblob<MrirtSdfParams>(params, "MrirtSdfParams");
    TORCH_CHECK_TYPE(like.is_cuda(), "like: expected a device tensor");
    DeviceGuard guard(like.device());
    Tensor out = at::empty({ height, width, 4 }, opts(at::kFloat, like.device()));
    check(mrirt_render_sdf(&P, (uint32_t)width, (uint32_t)height, out.data_ptr<float>(), width, current_stream()), "mrirt_render_sdf");
    return out;
}

// compute_main (scripts/mesh_rt/mesh_rt.slang:138-164) through mrirt_render_mesh; the counts are the buffers' sizes
// (nodes float32 [2N x 4], tris int32 [M x 4], verts float32 [V x 4]), so the kernel's guards keep every read inside them.
// (The library refuses a tiled ext for K4.)
Tensor render_mesh(const Tensor& params, const Tensor& ext, const Tensor& nodes, const Tensor& tris, const Tensor& verts,
                   int64_t max_depth) {
    const MrirtMeshParams P = unblob<MrirtMeshParams>(params, "MrirtMeshParams");
    const MrirtRenderExt E = unblob<MrirtRenderExt>(ext, "MrirtRenderExt");
    OptDevice dev;
    const float* n = static_cast<const float*>(operand(dev, nodes, at::kFloat, "gBVHNodes"));
    const uint32_t* t = static_cast<const uint32_t*>(operand(dev, tris, at::kInt, "gTris"));
    const float* v = static_cast<const float*>(operand(dev, verts, at::kFloat, "gVerts"));
    TORCH_CHECK_VALUE(max_depth >= 0 && max_depth <= 64, "max_depth must be in [0, 64]");
    DeviceGuard guard(*dev);
    Tensor out = new_frame(P.imageSize, E, *dev);
    const int64_t nc = nodes.numel() / 8, tc = tris.numel() / 4, vc = verts.numel() / 4;
    TORCH_CHECK_VALUE(nc < (1 << 30) && tc < (1 << 30) && vc < (1ll << 32), "buffer too large");
    check(mrirt_render_mesh(&P, &E, n, (uint32_t)nc, t, (uint32_t)tc, v, (uint32_t)vc, (uint32_t)max_depth, out.data_ptr(),
                            (int64_t)P.imageSize[0], nullptr, nullptr, current_stream()),
          "mrirt_render_mesh");
    return out;
}

// ---- INR: the descriptor and the input checks of mrirt_inr_forward and of the fp32 training step ----
MrirtInrDesc inr_desc(int64_t kind, int64_t num_layers, int64_t in_dim, int64_t out_dim, int64_t hidden, int64_t fourier_freqs,
                      int64_t num_mods, double w0 = 0.0) {
    MrirtInrDesc d;
    std::memset(&d, 0, sizeof d);
    d.kind = (uint32_t)kind; d.numLayers = (uint32_t)num_layers; d.inDim = (uint32_t)in_dim; d.outDim = (uint32_t)out_dim;
    d.hidden = (uint32_t)hidden; d.fourierFreqs = (uint32_t)fourier_freqs; d.numMods = (uint32_t)num_mods; d.w0 = (float)w0;
    return d;
}

// coords [n, 3] (the coordinate kinds 0 / 1) and feats [n, num_mods] — or, for the raw kinds 2 / 3, the [n, in_dim] input
// matrix — on the device `dev` already names
void inr_inputs(int64_t kind, int64_t in_dim, int64_t num_mods, const OptTensor& coords, const OptTensor& feats, int64_t n,
                const float*& co, const float*& fe, OptDevice& dev) {
    co = static_cast<const float*>(operand(dev, coords, at::kFloat, "coords"));
    fe = static_cast<const float*>(operand(dev, feats, at::kFloat, "feats"));
    TORCH_CHECK_VALUE(kind >= 2 || (coords.has_value() && coords->numel() >= 3 * n), "coords must hold [n, 3] floats");
    const int64_t width = kind >= 2 ? in_dim : num_mods;
    TORCH_CHECK_VALUE(width == 0 || (feats.has_value() && feats->numel() >= width * n), "feats must hold [n, ", width, "] floats");
}

// logits [n, out_dim] of the packed MLP (inr/inr/model.py:21-50 for kind 0, notebooks/neumors_inr.ipynb:1165-1178 for
// kind 1; kinds 2 / 3 take the [n, in_dim] input matrix in `feats`) through mrirt_inr_forward
Tensor inr_forward(const Tensor& weights, const Tensor& biases, int64_t kind, int64_t num_layers, int64_t in_dim, int64_t out_dim,
                   int64_t hidden, int64_t fourier_freqs, int64_t num_mods, double w0, const OptTensor& coords,
                   const OptTensor& feats, int64_t n) {
    MrirtInrDesc d = inr_desc(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, w0);
    const int64_t need = mrirt_inr_pack_bytes(&d);
    TORCH_CHECK_VALUE(need > 0, "unsupported network shape");
    TORCH_CHECK_TYPE(weights.is_cuda() && weights.scalar_type() == at::kByte && weights.numel() >= need,
                     "weights: expected the ", need, "-byte packed image of mrirt_inr_pack_weights on the device");
    const int64_t nb = (num_layers - 1) * hidden + ((out_dim + 31) / 32) * 32;
    OptDevice dev = weights.device();
    d.weights = weights.data_ptr();
    d.biases = static_cast<const float*>(operand(dev, biases, at::kFloat, "biases"));
    TORCH_CHECK_VALUE(biases.numel() >= nb, "biases holds fewer than ", nb, " floats (each layer padded to a multiple of 32)");
    const float *co, *fe;
    inr_inputs(kind, in_dim, num_mods, coords, feats, n, co, fe, dev);
    DeviceGuard guard(*dev);
    Tensor out = at::empty({ n, out_dim }, opts(at::kFloat, weights.device()));
    check(mrirt_inr_forward(&d, co, fe, n, out.data_ptr<float>(), nullptr, current_stream()), "mrirt_inr_forward");
    return out;
}

// ---- INR training step (fp32): mrirt_inr_forward_f32 / mrirt_inr_loss / mrirt_inr_backward ----
struct TrainShape { MrirtInrDesc d; int64_t bytes, nw, nb; };

TrainShape train_shape(int64_t kind, int64_t num_layers, int64_t in_dim, int64_t out_dim, int64_t hidden, int64_t fourier_freqs,
                       int64_t num_mods, int64_t n) {
    TrainShape t;
    t.d = inr_desc(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods);
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
    OptDevice dev;
    const float* w = static_cast<const float*>(operand(dev, weights, at::kFloat, "weights"));
    const float* b = static_cast<const float*>(operand(dev, biases, at::kFloat, "biases"));
    TORCH_CHECK_VALUE(weights.numel() >= t.nw && biases.numel() >= t.nb, "weights / biases are smaller than the network (", t.nw, " / ", t.nb, " floats)");
    const float *co, *fe;
    inr_inputs(kind, in_dim, num_mods, coords, feats, n, co, fe, dev);
    DeviceGuard guard(*dev);
    Tensor out = at::empty({ n, out_dim }, opts(at::kFloat, *dev));
    Tensor scratch = at::empty({ t.bytes }, opts(at::kByte, *dev));
    check(mrirt_inr_forward_f32(&t.d, w, b, co, fe, n, out.data_ptr<float>(), scratch.data_ptr(), t.bytes, current_stream()),
          "mrirt_inr_forward_f32");
    return { out, scratch };
}

// The operand checks of both losses: logits [n, C] and int32 labels [n] on one GPU, 1..16 classes, one class weight each.
at::Device loss_operands(const Tensor& logits, const Tensor& labels, at::ArrayRef<double> class_weights) {
    OptDevice dev;
    operand(dev, logits, at::kFloat, "logits");
    operand(dev, labels, at::kInt, "labels");
    TORCH_CHECK_VALUE(logits.dim() == 2 && logits.size(0) >= 1 && labels.numel() == logits.size(0), "logits must be [n, C] with n >= 1 and labels [n]");
    const int64_t nc = logits.size(1);
    TORCH_CHECK_VALUE(nc >= 1 && nc <= 16 && (int64_t)class_weights.size() == nc, "1..16 classes, one class weight each");
    return *dev;
}

// loss [1], aux [2, C], terms [5] (the extended loss only: undefined otherwise), dlogits like logits, and the scratch
struct LossOut { Tensor loss, aux, terms, dl, scratch; };

LossOut loss_outputs(const Tensor& logits, int64_t nbytes, bool terms, at::Device dev) {
    const auto f32 = opts(at::kFloat, dev);
    LossOut o;
    o.loss = at::empty({ 1 }, f32);
    o.aux = at::empty({ 2, logits.size(1) }, f32);
    if (terms) o.terms = at::empty({ 5 }, f32);
    o.dl = at::empty_like(logits);
    o.scratch = at::empty({ nbytes }, opts(at::kByte, dev));
    return o;
}

// (loss [1], aux [2, C], dlogits [n, C]) of the reference's loss (inr/inr/model.py:64-88) through mrirt_inr_loss
std::tuple<Tensor, Tensor, Tensor> inr_loss(const Tensor& logits, const Tensor& labels, at::ArrayRef<double> class_weights, double dice_weight) {
    const at::Device dev = loss_operands(logits, labels, class_weights);
    const int64_t n = logits.size(0), nc = logits.size(1);
    float cw[16];
    for (int64_t k = 0; k < nc; ++k) cw[k] = (float)class_weights[k];
    DeviceGuard guard(dev);
    const int64_t nbytes = mrirt_inr_loss_scratch_bytes(n);
    LossOut o = loss_outputs(logits, nbytes, false, dev);
    check(mrirt_inr_loss(logits.data_ptr<float>(), labels.data_ptr<int32_t>(), n, (uint32_t)nc, cw, (float)dice_weight, o.loss.data_ptr<float>(),
                         o.aux.data_ptr<float>(), o.dl.data_ptr<float>(), o.scratch.data_ptr(), nbytes, current_stream()), "mrirt_inr_loss");
    return { o.loss, o.aux, o.dl };
}

// (loss [1], aux [2, C], terms [5], dlogits [n, C]) of scripts/jax_inr_brats.py's loss through mrirt_inr_loss_ext; focal_alpha
// empty: flags bit 1 clear
std::tuple<Tensor, Tensor, Tensor, Tensor> inr_loss_ext(const Tensor& logits, const Tensor& labels, at::ArrayRef<double> class_weights,
                                                        at::ArrayRef<double> focal_alpha, double dice_weight, bool per_class_dice, double focal_gamma,
                                                        double label_smoothing, double edema_fp_weight, double tversky_alpha, double tversky_beta,
                                                        double tversky_weight, double edema_logit_reg, int64_t edema_class) {
    const at::Device dev = loss_operands(logits, labels, class_weights);
    const int64_t n = logits.size(0), nc = logits.size(1);
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
    DeviceGuard guard(dev);
    const int64_t nbytes = mrirt_inr_loss_ext_scratch_bytes(n);
    LossOut o = loss_outputs(logits, nbytes, true, dev);
    check(mrirt_inr_loss_ext(logits.data_ptr<float>(), labels.data_ptr<int32_t>(), n, (uint32_t)nc, &x, o.loss.data_ptr<float>(),
                             o.aux.data_ptr<float>(), o.terms.data_ptr<float>(), o.dl.data_ptr<float>(), o.scratch.data_ptr(), nbytes,
                             current_stream()), "mrirt_inr_loss_ext");
    return { o.loss, o.aux, o.terms, o.dl };
}

// (grad_w, grad_b) through mrirt_inr_backward from dlogits and the scratch inr_forward_f32 returned
std::tuple<Tensor, Tensor> inr_backward(const Tensor& weights, const Tensor& dlogits, const Tensor& scratch, int64_t kind, int64_t num_layers,
                                        int64_t in_dim, int64_t out_dim, int64_t hidden, int64_t fourier_freqs, int64_t num_mods, int64_t n) {
    const TrainShape t = train_shape(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n);
    OptDevice dev;
    const float* w = static_cast<const float*>(operand(dev, weights, at::kFloat, "weights"));
    const float* dl = static_cast<const float*>(operand(dev, dlogits, at::kFloat, "dlogits"));
    TORCH_CHECK_VALUE(weights.numel() >= t.nw && dlogits.numel() >= n * out_dim, "weights / dlogits are smaller than the network / [n, out_dim]");
    TORCH_CHECK_TYPE(scratch.is_cuda() && scratch.scalar_type() == at::kByte && scratch.is_contiguous() && scratch.numel() >= t.bytes,
                     "scratch: expected the ", t.bytes, "-byte device buffer of inr_forward_f32");
    same_device(dev, scratch, "scratch");
    DeviceGuard guard(*dev);
    Tensor gw = at::empty({ t.nw }, opts(at::kFloat, *dev)), gb = at::empty({ t.nb }, opts(at::kFloat, *dev));
    check(mrirt_inr_backward(&t.d, w, n, dl, gw.data_ptr<float>(), gb.data_ptr<float>(), 0u, scratch.data_ptr(), scratch.numel(),
                             current_stream()), "mrirt_inr_backward");
    return { gw, gb };
}

// ---- INR training loop: mrirt_inr_sample_batch / mrirt_inr_sample_batch_mix / mrirt_inr_adamw_step ----
// The table checks and the MrirtInrCache of both samplers; the tables are int64 device tensors of per-case device addresses.
MrirtInrCache sampler_cache(const OptTensor& mods_table, const Tensor& seg_table, int64_t num_mods, int64_t h, int64_t w, int64_t d, int64_t n,
                            int64_t n_tumour, OptDevice& dev) {
    const void* st = operand(dev, seg_table, at::kLong, "seg_table");
    const void* mt = operand(dev, mods_table, at::kLong, "mods_table");
    TORCH_CHECK_VALUE(seg_table.numel() >= 1 && (num_mods <= 0 || (mods_table.has_value() && mods_table->numel() == seg_table.numel())),
                      "seg_table must hold one address per case, and mods_table as many when num_mods > 0");
    TORCH_CHECK_VALUE(num_mods >= 0 && h >= 0 && w >= 0 && d >= 0 && n >= 0 && n_tumour >= 0, "negative extent");
    MrirtInrCache c;
    std::memset(&c, 0, sizeof c);
    c.mods = num_mods > 0 ? static_cast<const float* const*>(mt) : nullptr;
    c.seg = static_cast<const int16_t* const*>(st);
    c.ncases = (uint32_t)seg_table.numel(); c.numMods = (uint32_t)num_mods;
    c.hwd[0] = (uint32_t)h; c.hwd[1] = (uint32_t)w; c.hwd[2] = (uint32_t)d;
    return c;
}

// (coords [n, 3], feats [n, num_mods], labels int32 [n])
std::tuple<Tensor, Tensor, Tensor> sample_outputs(int64_t n, int64_t num_mods, at::Device dev) {
    return { at::empty({ n, 3 }, opts(at::kFloat, dev)), at::empty({ n, num_mods }, opts(at::kFloat, dev)), at::empty({ n }, opts(at::kInt, dev)) };
}

std::tuple<Tensor, Tensor, Tensor> inr_sample_batch(const OptTensor& mods_table, const Tensor& seg_table, int64_t num_mods, int64_t h, int64_t w,
                                                    int64_t d, int64_t seed, int64_t batch_index, int64_t n) {
    OptDevice dev;
    const MrirtInrCache c = sampler_cache(mods_table, seg_table, num_mods, h, w, d, n, 0, dev);
    DeviceGuard guard(*dev);
    auto out = sample_outputs(n, num_mods, *dev);
    check(mrirt_inr_sample_batch(&c, (uint64_t)seed, (uint64_t)batch_index, n, std::get<0>(out).data_ptr<float>(),
                                 num_mods > 0 ? std::get<1>(out).data_ptr<float>() : nullptr, std::get<2>(out).data_ptr<int32_t>(), current_stream()),
          "mrirt_inr_sample_batch");
    return out;
}

// inr_sample_batch with the first n_tumour points drawn from the tumour index (mrirt_inr_sample_batch_mix): tumour_index the
// uint32 voxel offsets held in an int32 tensor, tumour_offsets int64 [ncases + 1]; both may be absent when n_tumour == 0
std::tuple<Tensor, Tensor, Tensor> inr_sample_batch_mix(const OptTensor& mods_table, const Tensor& seg_table, const OptTensor& tumour_index,
                                                        const OptTensor& tumour_offsets, int64_t num_mods, int64_t h, int64_t w, int64_t d,
                                                        int64_t seed, int64_t batch_index, int64_t n, int64_t n_tumour) {
    OptDevice dev;
    const void* ti = operand(dev, tumour_index, at::kInt, "tumour_index");
    const void* to = operand(dev, tumour_offsets, at::kLong, "tumour_offsets");
    const MrirtInrCache c = sampler_cache(mods_table, seg_table, num_mods, h, w, d, n, n_tumour, dev);
    TORCH_CHECK_VALUE(n_tumour == 0 || (tumour_index.has_value() && tumour_offsets.has_value() && tumour_offsets->numel() == seg_table.numel() + 1),
                      "n_tumour > 0 needs tumour_index and tumour_offsets [ncases + 1]");
    DeviceGuard guard(*dev);
    const MrirtInrTumourIndex t = { static_cast<const uint32_t*>(ti), static_cast<const int64_t*>(to) };
    auto out = sample_outputs(n, num_mods, *dev);
    check(mrirt_inr_sample_batch_mix(&c, n_tumour > 0 ? &t : nullptr, (uint64_t)seed, (uint64_t)batch_index, n, n_tumour,
                                     std::get<0>(out).data_ptr<float>(), num_mods > 0 ? std::get<1>(out).data_ptr<float>() : nullptr,
                                     std::get<2>(out).data_ptr<int32_t>(), current_stream()),
          "mrirt_inr_sample_batch_mix");
    return out;
}

// [w, b, mu_w, mu_b, nu_w, nu_b, gnorm] after update t + 1 on copies of the flat parameters and moments
std::vector<Tensor> inr_adamw_step(const Tensor& w, const Tensor& b, const Tensor& gw, const Tensor& gb, const Tensor& mu_w, const Tensor& mu_b,
                                   const Tensor& nu_w, const Tensor& nu_b, double lr, double b1, double b2, double eps, double weight_decay,
                                   double clip_norm, int64_t t, double gscale) {
    const Tensor* ten[8] = { &w, &b, &gw, &gb, &mu_w, &mu_b, &nu_w, &nu_b };
    static const char* names[8] = { "w", "b", "gw", "gb", "mu_w", "mu_b", "nu_w", "nu_b" };
    OptDevice dev;
    for (int i = 0; i < 8; ++i) {
        operand(dev, *ten[i], at::kFloat, names[i]);
        TORCH_CHECK_VALUE(ten[i]->numel() == ten[i & 1]->numel(), "gradients and moments must have the sizes of w and b");
    }
    DeviceGuard guard(*dev);
    const int64_t nw = w.numel(), nb = b.numel();
    Tensor ow = w.clone(), ob = b.clone(), omw = mu_w.clone(), omb = mu_b.clone(), onw = nu_w.clone(), onb = nu_b.clone();
    const int64_t nbytes = mrirt_inr_adamw_scratch_bytes(nw + nb);
    Tensor scratch = at::empty({ nbytes > 16 ? nbytes : 16 }, opts(at::kByte, *dev));
    Tensor gnorm = at::empty({ 2 }, opts(at::kDouble, *dev));
    const MrirtAdamW hp = { (float)lr, (float)b1, (float)b2, (float)eps, (float)weight_decay, (float)clip_norm };
    check(mrirt_inr_adamw_step(ow.data_ptr<float>(), ob.data_ptr<float>(), gw.data_ptr<float>(), gb.data_ptr<float>(), omw.data_ptr<float>(),
                               omb.data_ptr<float>(), onw.data_ptr<float>(), onb.data_ptr<float>(), nw, nb, &hp, (uint64_t)t, (float)gscale,
                               gnorm.data_ptr<double>(), scratch.data_ptr(), nbytes, current_stream()), "mrirt_inr_adamw_step");
    return { ow, ob, omw, omb, onw, onb, gnorm };
}

// the volume's extent and spacing as the C ABI takes them; every label tensor is int16 (H, W, D) on one device
void edt_args(const Tensor& first, const OptTensor& second, at::ArrayRef<double> spacing, uint32_t hwd[3], float sp[3], OptDevice& dev) {
    operand(dev, first, at::kShort, "labels");
    operand(dev, second, at::kShort, "labels");
    TORCH_CHECK_VALUE(first.dim() == 3 && (!second.has_value() || second->sizes() == first.sizes()),
                      "label volumes must be (H, W, D) int16 tensors of one shape");
    TORCH_CHECK_VALUE(spacing.size() == 3, "spacing: expected three values");
    fill_hwd(first, hwd);
    for (int k = 0; k < 3; ++k) sp[k] = (float)spacing[k];
}

Tensor scratch_for(int64_t nbytes, at::Device dev) { return at::empty({ std::max<int64_t>(nbytes, 8) / 8 }, opts(at::kLong, dev)); }

// exact squared Euclidean distance transform of (labels == cls) through mrirt_edt_squared
Tensor edt_squared(const Tensor& labels, int64_t cls, at::ArrayRef<double> spacing) {
    uint32_t hwd[3];
    float sp[3];
    OptDevice dev;
    edt_args(labels, std::nullopt, spacing, hwd, sp, dev);
    TORCH_CHECK_VALUE(cls >= INT32_MIN && cls <= INT32_MAX, "cls out of range");
    DeviceGuard guard(*dev);
    const int64_t nbytes = mrirt_edt_scratch_bytes(hwd, 0);
    Tensor out = at::empty(labels.sizes(), opts(at::kDouble, *dev));
    Tensor scratch = scratch_for(nbytes, *dev);
    check(mrirt_edt_squared(static_cast<const int16_t*>(labels.data_ptr()), hwd, (int32_t)cls, sp, out.data_ptr<double>(),
                            scratch.data_ptr(), nbytes, current_stream()), "mrirt_edt_squared");
    return out;
}

// squared directed Hausdorff distances [num_classes, 2] (inr/inr/model.py:164-195) through mrirt_hausdorff
Tensor hausdorff(const Tensor& pred, const Tensor& truth, at::ArrayRef<double> spacing, int64_t num_classes) {
    uint32_t hwd[3];
    float sp[3];
    OptDevice dev;
    edt_args(pred, truth, spacing, hwd, sp, dev);
    TORCH_CHECK_VALUE(num_classes >= 1 && num_classes <= 32, "num_classes must be in [1, 32]");
    DeviceGuard guard(*dev);
    const int64_t nbytes = mrirt_edt_scratch_bytes(hwd, (uint32_t)num_classes);
    Tensor out = at::empty({ num_classes, 2 }, opts(at::kDouble, *dev));
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
    fill_hwd(labels, hwd);
    const int64_t nbytes = mrirt_surface_scratch_bytes(hwd);
    TORCH_CHECK_VALUE(nbytes > 0, "the volume is outside the supported sizes");
    return nbytes;
}

// int64 [2]: vertices and triangles, through mrirt_surface_count
Tensor surface_count(const Tensor& labels, int64_t class_mask) {
    uint32_t hwd[3];
    const int64_t nbytes = surface_args(labels, class_mask, hwd);
    DeviceGuard guard(labels.device());
    Tensor counts = at::empty({ 2 }, opts(at::kLong, labels.device()));
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
    Tensor verts = at::zeros({ num_verts, 3 }, opts(at::kFloat, labels.device()));
    Tensor tris = at::zeros({ num_tris, 3 }, opts(at::kInt, labels.device()));
    Tensor counts = at::empty({ 2 }, opts(at::kLong, labels.device()));
    Tensor scratch = scratch_for(nbytes + 8, labels.device());
    check(mrirt_surface_extract(static_cast<const int16_t*>(labels.data_ptr()), hwd, (uint32_t)class_mask, sp, org,
                                num_verts ? verts.data_ptr<float>() : nullptr, num_verts, num_tris ? tris.data_ptr<int32_t>() : nullptr,
                                num_tris, scratch.data_ptr(), nbytes, counts.data_ptr<int64_t>(), current_stream()),
          "mrirt_surface_extract");
    return { verts, tris };
}

// the parameter blocks are CPU tensors and the grids device tensors: no single dispatch key fits, so every implementation is
// registered for every backend and checks its arguments itself
template <typename F>
auto everywhere(F* fn) { return torch::dispatch(c10::DispatchKey::CompositeExplicitAutograd, fn); }

}  // namespace

TORCH_LIBRARY(mrirt_native, m) {
    m.def("render_brats(Tensor params, Tensor ext, Tensor? vol0, Tensor? vol1, Tensor? vol2, Tensor? vol3, Tensor? labels, Tensor? preds) -> Tensor",
          everywhere(&render_brats));
    m.def("render_brats_backward(Tensor params, Tensor ext, Tensor grad_out, Tensor? vol0, Tensor? vol1, Tensor? vol2, Tensor? vol3, "
          "Tensor? labels, Tensor? preds) -> (Tensor, Tensor, Tensor, Tensor, Tensor)", everywhere(&render_brats_backward));
    m.def("render_brats_soft(Tensor params, Tensor ext, Tensor logits, Tensor offsets, Tensor? vol0, Tensor? vol1, Tensor? vol2, Tensor? vol3, "
          "Tensor? labels) -> Tensor", everywhere(&render_brats_soft));
    m.def("render_brats_soft_backward(Tensor params, Tensor ext, Tensor grad_out, Tensor logits, Tensor offsets, Tensor? vol0, Tensor? vol1, "
          "Tensor? vol2, Tensor? vol3, Tensor? labels) -> Tensor", everywhere(&render_brats_soft_backward));
    m.def("render_volume(Tensor params, Tensor ext, Tensor volume, int mode) -> Tensor", everywhere(&render_volume));
    m.def("render_sdf(Tensor params, int width, int height, Tensor like) -> Tensor", everywhere(&render_sdf));
    m.def("render_mesh(Tensor params, Tensor ext, Tensor nodes, Tensor tris, Tensor verts, int max_depth) -> Tensor", everywhere(&render_mesh));
    m.def("inr_forward(Tensor weights, Tensor biases, int kind, int num_layers, int in_dim, int out_dim, int hidden, "
          "int fourier_freqs, int num_mods, float w0, Tensor? coords, Tensor? feats, int n) -> Tensor", everywhere(&inr_forward));
    m.def("inr_forward_f32(Tensor weights, Tensor biases, int kind, int num_layers, int in_dim, int out_dim, int hidden, "
          "int fourier_freqs, int num_mods, Tensor? coords, Tensor? feats, int n) -> (Tensor, Tensor)", everywhere(&inr_forward_f32));
    m.def("inr_loss(Tensor logits, Tensor labels, float[] class_weights, float dice_weight) -> (Tensor, Tensor, Tensor)", everywhere(&inr_loss));
    m.def("inr_loss_ext(Tensor logits, Tensor labels, float[] class_weights, float[] focal_alpha, float dice_weight, bool per_class_dice, "
          "float focal_gamma, float label_smoothing, float edema_fp_weight, float tversky_alpha, float tversky_beta, float tversky_weight, "
          "float edema_logit_reg, int edema_class) -> (Tensor, Tensor, Tensor, Tensor)", everywhere(&inr_loss_ext));
    m.def("inr_sample_batch_mix(Tensor? mods_table, Tensor seg_table, Tensor? tumour_index, Tensor? tumour_offsets, int num_mods, int h, int w, "
          "int d, int seed, int batch_index, int n, int n_tumour) -> (Tensor, Tensor, Tensor)", everywhere(&inr_sample_batch_mix));
    m.def("inr_backward(Tensor weights, Tensor dlogits, Tensor scratch, int kind, int num_layers, int in_dim, int out_dim, int hidden, "
          "int fourier_freqs, int num_mods, int n) -> (Tensor, Tensor)", everywhere(&inr_backward));
    m.def("inr_sample_batch(Tensor? mods_table, Tensor seg_table, int num_mods, int h, int w, int d, int seed, int batch_index, int n) "
          "-> (Tensor, Tensor, Tensor)", everywhere(&inr_sample_batch));
    m.def("inr_adamw_step(Tensor w, Tensor b, Tensor gw, Tensor gb, Tensor mu_w, Tensor mu_b, Tensor nu_w, Tensor nu_b, float lr, float b1, "
          "float b2, float eps, float weight_decay, float clip_norm, int t, float gscale) -> Tensor[]", everywhere(&inr_adamw_step));
    m.def("edt_squared(Tensor labels, int cls, float[] spacing) -> Tensor", everywhere(&edt_squared));
    m.def("hausdorff(Tensor pred, Tensor truth, float[] spacing, int num_classes) -> Tensor", everywhere(&hausdorff));
    m.def("surface_count(Tensor labels, int class_mask) -> Tensor", everywhere(&surface_count));
    m.def("surface_extract(Tensor labels, int class_mask, float[] spacing, float[] origin, int num_verts, int num_tris) -> (Tensor, Tensor)",
          everywhere(&surface_extract));
}
