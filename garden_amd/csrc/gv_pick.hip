// gv_pick.hip — gfx950 kernel of gv_pick: the editor's click selection (MeshSelectorEditorSystem::render,
// editor/system/render/mesh-selector.cpp:67-122) as one pass over a pool's mirror.
//
//   pick_kernel   one lane per mirror entry: the cull's filter chain and camera-relative model (prepare_model), the model's
//                 inverse once, then every ray against the box. The smallest 64-bit key per ray goes
//                 through a wave reduction, then the workgroup's LDS, and a workgroup with a hit makes one global atomicMin
//                 per ray. Almost no workgroup has one: the atomics do not contend.
//
// Reads the full streams (65 B per entity flat, 69 with a hierarchy, +4 with a general mapping), never the sphere stream: the
// sphere bounds the box in world space, but the fp32 inverse of an ill-conditioned model is not bounded by it.
#include "gv_device.hpp"

namespace gv {

struct PickArgs {
    MeshMirror mesh;
    TransformMirror xf;
    PickLaunch p;
};

template <uint32_t MAP>
__global__ __launch_bounds__(kPickBlock) void pick_kernel(const PickArgs a)
{
    __shared__ unsigned long long wave_min[kPickBlock / 64][kPickMaxRays];
    const uint32_t i = blockIdx.x * kPickBlock + threadIdx.x;
    Mat34 m = {};
    float4 box_a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float2 box_b = make_float2(0.0f, 0.0f);
    bool candidate = i < a.mesh.count && prepare_model<MAP>(a.mesh, a.xf, a.p.cam, i, m, box_a, box_b);
    uint32_t slot = kSlotNone;
    if (candidate) {
        slot = a.mesh.orig ? a.mesh.orig[i] : i;
        if (a.p.index_map)
            slot = a.p.index_map[slot];  // GV_NONE: a hole of the share (the host checked the rest fit in 28 bits)
        candidate = slot != 0xFFFFFFFFu && slot != a.p.exclude;
    }
    Inv33 inv = affine_inverse(m);
    inv.valid = inv.valid && candidate;
    const uint32_t order_slot = a.p.order_bits | (slot & kSlotMask);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t r = 0; r < kPickMaxRays; r++)
        if (r < a.p.rays) {  // wave-uniform: the ray stays in SGPRs
            unsigned long long key = pick_key(inv, m.c3x, m.c3y, m.c3z, box_a, box_b, a.p.ray[r][0], a.p.ray[r][1], a.p.ray[r][2],
                                              a.p.ray[r][3], a.p.ray[r][4], a.p.ray[r][5], order_slot);
            if (__any(key != ~0ull)) {  // rare: most waves hold no hit for this ray
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const unsigned long long other = __shfl_xor(key, d);
                    key = other < key ? other : key;
                }
            }
            if (lane == 0)
                wave_min[wave][r] = key;
        }
    __syncthreads();
    if (threadIdx.x < a.p.rays) {
        unsigned long long key = wave_min[0][threadIdx.x];
#pragma unroll
        for (uint32_t w = 1; w < kPickBlock / 64; w++)
            key = wave_min[w][threadIdx.x] < key ? wave_min[w][threadIdx.x] : key;
        if (key != ~0ull)
            atomicMin(a.p.keys + threadIdx.x, key);  // global vector atomic (64-bit unsigned min)
    }
}

hipError_t launch_pick(const MeshMirror& mesh, const TransformMirror& xf, const PickLaunch& p, hipStream_t stream)
{
    if (mesh.count == 0)
        return hipSuccess;
    const PickArgs a{mesh, xf, p};
    const dim3 grid((mesh.count + kPickBlock - 1) / kPickBlock), block(kPickBlock);
    switch (mesh.mapping) {
    case kMapExact: hipLaunchKernelGGL((pick_kernel<kMapExact>), grid, block, 0, stream, a); break;
    case kMapSpeculate: hipLaunchKernelGGL((pick_kernel<kMapSpeculate>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((pick_kernel<kMapGeneral>), grid, block, 0, stream, a); break;
    }
    return hipGetLastError();
}

}  // namespace gv
