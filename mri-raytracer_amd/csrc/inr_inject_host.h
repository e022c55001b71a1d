// Coordinate-injection INR, host side: what csrc/inr_inject.hip checks and launches for its own entry points and for the
// training step built on its kernels (csrc/inr_inject_train.hip).  Nothing here touches the device before every check passed.
#pragma once
#include "inr_inject.h"
#include "mrirt_host.h"

namespace mrirt {

struct InjDrop { uint64_t seed, index0; uint32_t thr, s; float scale; bool on; };

// MRIRT_OK and the network, or what the entry points return for a desc they refuse
int inj_desc(const MrirtInjectDesc* d, InjNet& N);
// what every entry point refuses of a dropout struct; maxSamples: how many samples this call may take at most
int inj_check_dropout(const MrirtInjectDropout* p, uint32_t maxSamples);
// sample s of the call's mask stream; NULL or keep == 1: no mask
InjDrop inj_drop(const MrirtInjectDropout* p, uint32_t s);
// the features of n points into feat [n][F] (coords NULL: generated from voxel base + i of hwd into coordsOut)
int inj_run_features(const InjNet& N, const float* B, const float* coords, int64_t n, int64_t base, const uint32_t* hwd, float* coordsOut,
                     float* feat, hipStream_t s);
// the L layer launches over feat; act[l]: the output of hidden layer l, [n][width[l]]
int inj_run_layers(const InjNet& N, const float* feat, float* const* act, const float* w, const float* b, const float* coords,
                   const float* mods, int64_t modRow, int64_t modCol, int64_t n, const InjDrop& d, float* logits, hipStream_t s);

// csrc/inr_inject_fused.hip: the fused forward.  inj_fused_check: MRIRT_OK, or what the entry points
// return for a desc the fused path refuses (no HIP call).  inj_fused_dev_n: one launch over min(*nDev, nMax) rows (nDev NULL:
// nMax rows), 1 <= nMax < 2^31; argmax or logits may be NULL
int inj_fused_check(const MrirtInjectDesc* desc);
int inj_fused_dev_n(const MrirtInjectDesc* desc, const float* B, const float* w, const float* b, const float* coords, const float* mods,
                    int64_t nMax, const uint32_t* nDev, int16_t* argmax, float* logits, hipStream_t s);

}  // namespace mrirt
