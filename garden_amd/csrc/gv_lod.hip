// gv_lod.hip — gfx950 kernel of gv_pool_select_lods: the level of detail of every draw of the pool's last emission (DESIGN.md §4
// item 11, §5.14), the rule in gv_device_math.hpp lod_level.
//
//   lod_kernel   one lane per draw, 256 per workgroup, ONE launch for all listed views (the shape of instance_kernel: the grid is
//                sized from the occupancies, a workgroup beyond its view's device count leaves after one wave-uniform load, D_v is
//                at most 7 count loads). Per lane: idx[k] and the record's third model row (ONE aligned 16-byte load at float
//                12 k + 8: the translation is its y, z, w) stream in; the two per-slot gathers id[s] and size[s] are issued together;
//                the 32-byte table entry (the table is at most 2 MB: cache-resident) as two 16-byte loads; seven masked compares,
//                no dynamically indexed register; one coalesced 4-byte store of g_k. Histogram: per level a ballot + popcount per
//                wave into LDS, then at most 8 integer atomicAdd per workgroup (level_counts is zeroed in front of the launch).
//
// Whatever an id holds, the table is read inside [0, table_count) only; a slot is below the occupancy the columns were checked
// against on the host.
#include "gv_device.hpp"

namespace gv {

namespace {

__global__ __launch_bounds__(kLodBlock) void lod_kernel(const LodLaunch a)
{
    constexpr uint32_t kWaves = kLodBlock / 64u;
    __shared__ uint32_t hist[kWaves][kMaxLodLevels];
    const uint32_t v = view_of_block(a.first_block, a.views, blockIdx.x);
    const LodView& vw = a.view[v];
    const uint32_t n = *vw.count;
    const uint32_t first = (blockIdx.x - a.first_block[v]) * kLodBlock;
    if (first >= n)
        return;  // (the whole workgroup, after ONE load: the grid is sized for the occupancy)
    uint32_t base = 0;  // D_v
    for (uint32_t u = 0; u < v; u++)
        base += *a.view[u].count;
    const uint32_t k = first + threadIdx.x;
    const bool live = k < n;
    uint32_t level = 0;
    if (live) {
        const uint32_t slot = stream_load(vw.idx + k);
        const float4 row = stream_load(reinterpret_cast<const float4*>(vw.model) + (size_t)k * 3 + 2);  // (c2.z, c3.x, c3.y, c3.z)
        const uint32_t b = a.ids ? a.ids[slot] : 0u;
        const float size = a.sizes ? __uint_as_float(a.sizes[slot]) : 1.0f;
        const float x = lod_distance_sq(row.y, row.z, row.w) * vw.scale;
        uint32_t levels = 1u;
        float sw[kMaxLodLevels - 1] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (b < a.table_count) {
            const float4* const e = reinterpret_cast<const float4*>(a.table + b);
            const float4 e0 = e[0], e1 = e[1];
            levels = __float_as_uint(e0.x);
            sw[0] = e0.y, sw[1] = e0.z, sw[2] = e0.w;
            sw[3] = e1.x, sw[4] = e1.y, sw[5] = e1.z, sw[6] = e1.w;
        }
        level = lod_level(x, size, levels, sw);
        a.draw_geometry[base + k] = b + level;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t l = 0; l < kMaxLodLevels; l++) {
        const unsigned long long m = __ballot(live && level == l);
        if (lane == 0)
            hist[wave][l] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    // (the adds of a workgroup leave as ONE instruction; all workgroups of a view add into one 32-byte row, and those instructions
    // are performed one after the other: measured with the adds switched off they are 7 of the kernel's 16 us at 832 workgroups,
    // and packing two levels into one 64-bit add changed nothing — profiles/r22_lod_select.md)
    if (threadIdx.x < kMaxLodLevels) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; w++)
            sum += hist[w][threadIdx.x];
        if (sum)
            atomicAdd(a.level_counts + v * kMaxLodLevels + threadIdx.x, sum);
    }
}

}  // namespace

hipError_t launch_lod(const LodLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(lod_kernel, dim3(std::max(1u, launch.first_block[launch.views])), dim3(kLodBlock), 0, stream, launch);
    return hipGetLastError();
}

}  // namespace gv
