// K4: triangle-mesh BVH ray tracer — gfx950 HIP replacement for the Slang compute shader `compute_main`
// (scripts/mesh_rt/mesh_rt.slang:138-164; ray generation :26-37, traversal :75-136 in csrc/mesh_trace.h).
//
// One ray per pixel, one 64-lane workgroup per 8x8-pixel packet (the shader's numthreads(8,8,1)).  The shader's
// `uint stack[64]` indexed at run time would live in scratch; here each lane's stack is a column of LDS sized from the
// tree's real depth (maxDepth entries: 256 B per entry per wave), so a median-split tree of 8 M triangles (~22 levels)
// takes 5.5 KiB per wave and LDS does not limit the 32 waves a CU holds until maxDepth > 20.
#include "mesh_trace.h"
#include "mrirt_host.h"

namespace mrirt {

struct K4Args {
    Camera cam;
    PixelMap map;
    MeshBufs mesh;
    uint32_t cap;               // stack entries per lane (= maxDepth)
    void* out;
    uint64_t* stats;
    uint32_t* status;
};

struct LdsStack {
    uint32_t* col;              // this lane's column: entry i at col[i * kWave]
    MRIRT_HD uint32_t get(uint32_t i) const { return col[i * kWave]; }
    MRIRT_HD void set(uint32_t i, uint32_t v) { col[i * kWave] = v; }
};

template <bool HALF>
__global__ __launch_bounds__(64) void mesh_rt_kernel(const K4Args a) {
    extern __shared__ uint32_t stackLds[];
    uint32_t px, py;
    int64_t oidx;
    const int kind = map_pixel(a.map, px, py, oidx);
    uint32_t pops = 0, tests = 0;
    if (kind == 1) {
        MeshRay ray;
        primary_ray(a.cam, px, py, ray.o, ray.d);                 // makePrimary, :26-37 (aspect = W / H)
        mesh_ray_setup(ray);
        LdsStack st{ stackLds + (threadIdx.x & (kWave - 1)) };
        MeshHit h;
        const int rc = mesh_trace(a.mesh, ray, st, a.cap, h);
        pops = h.pops; tests = h.tests;
        float r, g, b;
        if (rc != MESH_TRACE_OK) {
            if (a.status != nullptr) atomicOr(a.status, 1u);
            r = 1.0f; g = 0.0f; b = 1.0f;
        } else if (h.t < 1e29f) {
            // :149-156; the normal of the winning triangle (:69), formed once
            const uint4 idx = a.mesh.tris[h.tri];
            const float4 A = a.mesh.verts[idx.x], B = a.mesh.verts[idx.y], Cv = a.mesh.verts[idx.z];
            const float ab[3] = { B.x - A.x, B.y - A.y, B.z - A.z };
            const float ac[3] = { Cv.x - A.x, Cv.y - A.y, Cv.z - A.z };
            float n[3];
            mesh_cross(ab, ac, n);
            normalize3(n[0], n[1], n[2]);                           // triHit's normalize
            normalize3(n[0], n[1], n[2]);                           // compute_main's
            if (dot3(n[0], n[1], n[2], ray.d[0], ray.d[1], ray.d[2]) > 0.0f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
            float lx = 0.3f, ly = 0.8f, lz = 0.5f;
            normalize3(lx, ly, lz);
            const float ndotl = fmaxf(0.0f, dot3(n[0], n[1], n[2], lx, ly, lz));
            const float ao = 0.3f + 0.7f * satf(1.0f - 0.05f * h.t);
            const float k = (0.15f + ndotl) * ao;
            r = k * 0.8f; g = k * 0.7f; b = k * 0.6f;
        } else {
            float dx = ray.d[0], dy = ray.d[1], dz = ray.d[2];
            normalize3(dx, dy, dz);
            const float tbg = 0.5f * (dy + 1.0f);
            r = M<true>::lerp(0.05f, 0.2f, tbg); g = M<true>::lerp(0.06f, 0.25f, tbg); b = M<true>::lerp(0.08f, 0.3f, tbg);
        }
        store_rgba<HALF>(a.out, oidx, r, g, b, 1.0f);
    }
    if (a.stats != nullptr) {
        wave_count_add(a.stats, pops);
        wave_count_add(a.stats + 1, tests);
    }
}

}  // namespace mrirt

using namespace mrirt;

extern "C" int mrirt_render_mesh(const MrirtMeshParams* p, const MrirtRenderExt* ext,
                                 const float* nodes, uint32_t nodeCount,
                                 const uint32_t* tris, uint32_t triCount,
                                 const float* verts, uint32_t vertCount,
                                 uint32_t maxDepth, void* out_rgba, int64_t pitch_px,
                                 uint64_t* stats_dev, uint32_t* status_dev, void* stream) {
    if (!p || !nodes || !tris || !verts || !out_rgba) return MRIRT_ERR_NULL;
    // indices are stored as floats and decoded with int(x + 0.5): exact below 2^23 only
    if (nodeCount == 0 || triCount == 0 || vertCount == 0) return MRIRT_ERR_ARG;
    if (nodeCount >= (1u << 23) || triCount >= (1u << 23)) return MRIRT_ERR_ARG;
    if (maxDepth == 0 || maxDepth > kMeshMaxStack) return MRIRT_ERR_ARG;
    if (ext) {
        if (ext->math != MRIRT_MATH_STRICT || ext->tileSize != 0 || ext->kernelVariant != 0) return MRIRT_ERR_ARG;
        if (ext->outFormat > MRIRT_OUT_RGBA16F || ext->cameraMode > 1) return MRIRT_ERR_LAYOUT;
    }
    const bool half = ext && ext->outFormat == MRIRT_OUT_RGBA16F;
    K4Args a;
    fill_camera(a.cam, p->eye, p->U, p->V, p->W, p->fovY, p->imageSize[0], p->imageSize[1], ext, true);
    int rc = fill_pixel_map(a.map, p->imageSize[0], p->imageSize[1], pitch_px, nullptr, kTilePx, 0, 0);
    if (rc != MRIRT_OK) return rc;
    a.mesh.nodes = reinterpret_cast<const float4*>(nodes);
    a.mesh.tris = reinterpret_cast<const uint4*>(tris);
    a.mesh.verts = reinterpret_cast<const float4*>(verts);
    a.mesh.nodeCount = nodeCount; a.mesh.triCount = triCount; a.mesh.vertCount = vertCount;
    a.cap = maxDepth;
    a.out = out_rgba; a.stats = stats_dev; a.status = status_dev;
    if (a.map.numBlocks == 0) return MRIRT_OK;
    const size_t lds = (size_t)maxDepth * kWave * sizeof(uint32_t);
    const dim3 grid(a.map.chunk * kXcds), block(kWave);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (half) hipLaunchKernelGGL(mesh_rt_kernel<true>, grid, block, lds, s, a);
    else      hipLaunchKernelGGL(mesh_rt_kernel<false>, grid, block, lds, s, a);
    MRIRT_HIP(hipGetLastError());
    return MRIRT_OK;
}
