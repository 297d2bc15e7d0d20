// gv_second.hip — gfx950 (CDNA4, wave64) kernels of gv_pool_cull_second_phase: the second phase of two-phase occlusion culling
// (DESIGN.md §4 item 13, §5.16). Three launches of its own in front of the existing compaction and record emission (gv_cull.hip):
//
//   second_seen_kernel    the first view's RECORDS -> one bit per mirror entry (the records exist for every launch form of the first
//                         cull and survive a sort, a grouping and a re-order of the mirror; its ballot words do neither).
//   second_cull_kernel    cull_kernel's per-entity work for the entries whose bit is clear, through the very functions the cull runs
//                         (prepare_model, classify_sphere, settle, hiz_occluded of gv_device.hpp: no arithmetic is restated, so every
//                         decision keeps its bits); outputs in exactly the format cull_kernel leaves — four ballot words per tile as
//                         one store, one integer add per workgroup into its chunk total — so that launch_scan / launch_emit take it
//                         from there unchanged.
//   second_union_kernel   the seen bits ORed into the second view's isVisible bytes (main pass): the frame's final answer.
//
// Policy as gv_cull.hip: static tile ids, no workgroup waits for another, atomics only add or OR integers and never decide a place.
#include "gv_device.hpp"
#include "gv_second_kernels.hpp"

#include <type_traits>

namespace gv {

// One lane per record of the first view. The device count is one wave-uniform load; lanes beyond it leave at once. A record holds a
// POOL slot (never index-mapped); inv maps it to the mirror entry whose bit is set. ORs of integers commute: the set is the same
// whatever the arrival order. (Measured: the launch is bound by its device-scope atomics, not by the workgroups that only leave —
// eight records per lane, an eighth of the grid, took 18.4 instead of 9.4 us at 10^6 entities and 37.0 instead of 36.5 us at 10^7;
// profiles/r24_second_phase.md.)
__global__ __launch_bounds__(kSecondBlock) void second_seen_kernel(const uint32_t* __restrict__ count, const uint32_t* __restrict__ idx,
                                                                    uint32_t capacity, const uint32_t* __restrict__ inv, uint32_t slots,
                                                                    uint32_t entries, unsigned long long* __restrict__ seen)
{
    const uint32_t k = blockIdx.x * kSecondBlock + threadIdx.x;
    const uint32_t n = min(*count, capacity);
    if (k >= n)
        return;
    const uint32_t slot = idx[k];
    if (slot >= slots)
        return;
    const uint32_t entry = inv ? inv[slot] : slot;
    if (entry < entries)
        atomicOr(&seen[entry >> 6], 1ull << (entry & 63u));
}

// 256 entries per workgroup, wave w of tile lb holds ballot word (lb, w), as cull_kernel. Each wave first loads the seen word of its
// 64 entries (wave-uniform; the set covers whole tiles): a wave whose entries are all seen goes straight to the tile's barrier with a
// zero word and touches no stream; in any other wave the seen lanes issue no stream loads. The rest is cull_block's plain path.
template <bool HIZ, uint32_t MAP>
__global__ __launch_bounds__(kCullBlock) void second_cull_kernel(const CullArgs args, const unsigned long long* __restrict__ seen)
{
    __shared__ unsigned long long wave_word[kCullBlock / 64];
    __shared__ uint32_t wave_count[kCullBlock / 64];
    const uint32_t lb = blockIdx.x, tid = threadIdx.x;
    const uint32_t i = lb * kCullBlock + tid;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const unsigned long long seen_word = seen[(size_t)lb * (kCullBlock / 64) + wave];
    bool visible = false;
    if (seen_word != ~0ull) {  // wave-uniform
        const bool mine = i < args.mesh.count && !((seen_word >> lane) & 1ull);
        Corners c;
        if (mine) {
            Mat34 m;
            float4 box_a;
            float2 box_b;
            uint32_t where = kSphereOutside;
            if (prepare_model<MAP>(args.mesh, args.xf, args.view.cam, i, m, box_a, box_b))
                where = classify_sphere(m, box_a, box_b, args.view.planes, args.view.plane_count);
            visible = settle<HIZ>(where, m, box_a, box_b, args.view.planes, args.view.plane_count, c);
        }
        if (HIZ && visible)
            visible = !hiz_occluded(args.hiz, args.view.vp, c);
    }
    if (i < args.mesh.count && args.view.write_is_visible)
        args.out.is_visible[i] = visible ? 1 : 0;
    const unsigned long long word = __ballot(visible);
    if (lane == 0) {
        wave_word[wave] = word;
        wave_count[wave] = (uint32_t)__popcll(word);
    }
    __syncthreads();
    if (tid < kCullBlock / 64)
        args.out.mask[(size_t)lb * (kCullBlock / 64) + tid] = wave_word[tid];
    if (tid == 0) {
        uint32_t total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kCullBlock / 64; w++)
            total += wave_count[w];
        if (total)  // integer adds commute: the sum is deterministic whatever the arrival order
            atomicAdd(&args.out.chunk_count[lb / (kEmitChunk / kCullBlock)], total);
    }
}

// Lane t owns entries 4t .. 4t + 3: a wave reads four whole words of the set and writes up to 256 contiguous bytes, a workgroup 1 KB
// of whole sectors. A lane whose four bits are clear stores nothing.
__global__ __launch_bounds__(kSecondBlock) void second_union_kernel(const unsigned long long* __restrict__ seen, uint32_t entries,
                                                                     uint8_t* __restrict__ is_visible)
{
    const uint32_t e = (blockIdx.x * kSecondBlock + threadIdx.x) * 4u;
    if (e >= entries)
        return;
    const uint32_t nibble = (uint32_t)(seen[e >> 6] >> (e & 63u)) & 15u;
    if (!nibble)
        return;
    const uint32_t bytes = (nibble & 1u) | ((nibble & 2u) << 7) | ((nibble & 4u) << 14) | ((nibble & 8u) << 21);
    if (e + 3u < entries) {
        uint32_t* p = reinterpret_cast<uint32_t*>(is_visible + e);
        *p |= bytes;
    } else {
        for (uint32_t k = 0; e + k < entries; k++)
            is_visible[e + k] |= (uint8_t)((bytes >> (8u * k)) & 1u);
    }
}

hipError_t launch_second_seen(const uint32_t* count, const uint32_t* idx, uint32_t capacity, const uint32_t* inv, uint32_t slots,
                              uint32_t entries, unsigned long long* seen, hipStream_t stream)
{
    if (capacity == 0)
        return hipSuccess;
    hipLaunchKernelGGL(second_seen_kernel, dim3((capacity + kSecondBlock - 1) / kSecondBlock), dim3(kSecondBlock), 0, stream, count, idx, capacity,
                       inv, slots, entries, seen);
    return hipGetLastError();
}

hipError_t launch_second_cull(const MeshMirror& mesh, const TransformMirror& xf, const HizDevice& hiz, const ViewParams& vp,
                              const ViewBuffers& out, const unsigned long long* seen, hipStream_t stream)
{
    if (mesh.count == 0)
        return hipSuccess;
    CullArgs a{};
    a.mesh = mesh;
    a.mesh.hot = nullptr;  // full streams only
    a.xf = xf;
    a.hiz = hiz;
    a.view = vp;
    a.out = out;
    a.nblocks = (mesh.count + kCullBlock - 1) / kCullBlock;
    const dim3 grid(a.nblocks), block(kCullBlock);
    auto with_map = [&](auto hz) {
        switch (mesh.mapping) {
        case kMapExact: hipLaunchKernelGGL((second_cull_kernel<hz, kMapExact>), grid, block, 0, stream, a, seen); break;
        case kMapSpeculate: hipLaunchKernelGGL((second_cull_kernel<hz, kMapSpeculate>), grid, block, 0, stream, a, seen); break;
        default: hipLaunchKernelGGL((second_cull_kernel<hz, kMapGeneral>), grid, block, 0, stream, a, seen); break;
        }
    };
    if (vp.use_hiz)
        with_map(std::true_type{});
    else
        with_map(std::false_type{});
    return hipGetLastError();
}

hipError_t launch_second_union(const unsigned long long* seen, uint32_t entries, uint8_t* is_visible, hipStream_t stream)
{
    if (entries == 0)
        return hipSuccess;
    const uint32_t lanes = (entries + 3u) / 4u;
    hipLaunchKernelGGL(second_union_kernel, dim3((lanes + kSecondBlock - 1) / kSecondBlock), dim3(kSecondBlock), 0, stream, seen, entries, is_visible);
    return hipGetLastError();
}

}  // namespace gv
