// gv_merge.hip — gfx950 kernel of gv_merge_sorted: the sorted lists of several mesh systems merged into the ONE array per sorted
// kind the reference keeps (transSortedMeshes / uiSortedMeshes / one translucent array per shadow pass: every system appends its
// SortedMesh records, mesh.cpp:247-261, one std::sort orders the whole array, mesh.cpp:296-326).
//
//   merge_sorted_kernel   ONE launch for every group of a frame: blockIdx.y = list (its group from group_of[]), blockIdx.x = 256
//                     consecutive records of it; a workgroup whose first record lies beyond its list's device-side count leaves
//                     after one wave-uniform load. No atomics, no waiting between workgroups, no host read of a count: record i
//                     of list j with key k finds its own place
//                         i + sum over lists l < j of #{T >= T(k)} + sum over lists l > j of #{T > T(k)}        (descending;
//                     ascending mirrored), T the sort's key order on the float's bits (gv_sort.hip float_key) — one binary
//                     search per other list, which is byte for byte what std::inplace_merge of the runs in list order gives.
//                     The searches of a wave: its 64 records are consecutive in one sorted list, so their places in any other
//                     list are monotone. Lanes 0 .. 2 L - 1 first search all L lists for the wave's FIRST and LAST key at once
//                     (one chain of log2 n dependent loads for all lists together, near the roots of the search trees that
//                     every wave shares in L2); every lane then searches only the window between the two — a handful of steps
//                     over a few cache lines when the lists are of similar length.
//                     The record (launch_pack_records' struct: componentOffset, 12 model floats, the key, bufferIndex, zeros
//                     elsewhere) is built in LDS by its own lane and leaves as 16-byte pieces, consecutive lanes writing the
//                     consecutive pieces of one record. Records at or beyond `capacity` are not written.
#include "gv_device.hpp"

namespace gv {

__device__ __forceinline__ uint32_t merge_key(uint32_t u) { return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }

// how many of keys[lo, hi) — sorted in the group's direction, all of keys[0, lo) known to go in front — go in front of a record
// of ANOTHER list whose key is t; ties: keys of a list in front win them
__device__ __forceinline__ uint32_t merge_rank(const uint32_t* __restrict__ keys, uint32_t lo, uint32_t hi, uint32_t t, bool descending,
                                               bool ties)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t x = merge_key(keys[mid]);
        const bool in_front = descending ? (ties ? x >= t : x > t) : (ties ? x <= t : x < t);
        if (in_front)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kMergeBlock) void merge_sorted_kernel(const MergeLaunch a)
{
    __shared__ uint4 stage[kMergeBlock * kMaxRecordStride / 16];
    __shared__ uint32_t place[kMergeBlock];
    __shared__ const uint32_t* keys_of[kMaxMergeGroupLists];
    __shared__ uint32_t count_of[kMaxMergeGroupLists];
    __shared__ uint32_t window[kMergeBlock / 64][2 * kMaxMergeGroupLists];
    // workgroup-uniform: this workgroup's list and group
    const uint32_t j = blockIdx.y;
    const MergeGroup& g = a.group[a.group_of[j]];
    const MergeList& mine = a.list[j];
    const uint32_t lists = min(g.lists, kMaxMergeGroupLists), my = j - g.first;
    if (blockIdx.x == 0 && my == 0 && threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t l = 0; l < lists; l++) {
            const uint32_t c = *a.list[g.first + l].count;
            g.counts[l] = c;
            total += c;
        }
        g.counts[lists] = total;
    }
    const uint32_t n = *mine.count;
    const uint32_t first = blockIdx.x * kMergeBlock;
    if (first >= n)
        return;  // (the whole workgroup, after ONE load: the grid is sized for the widest occupancy)
    const uint32_t quads = g.stride >> 4;
    for (uint32_t q = threadIdx.x; q < kMergeBlock * quads; q += kMergeBlock)
        stage[q] = make_uint4(0, 0, 0, 0);
    for (uint32_t l = 0; l < lists; l++) {  // (uniform index: scalar loads of the table)
        const MergeList& o = a.list[g.first + l];
        if (threadIdx.x == l) {
            keys_of[l] = reinterpret_cast<const uint32_t*>(o.dist);
            count_of[l] = *o.count;
        }
    }
    __syncthreads();
    const bool descending = g.descending != 0;
    const uint32_t* const my_keys = reinterpret_cast<const uint32_t*>(mine.dist);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t wave_first = first + wave * 64u;
    if (wave_first < n && lane < 2u * lists && (lane >> 1) != my) {
        const uint32_t l = lane >> 1;
        const uint32_t t = merge_key(my_keys[(lane & 1u) ? min(wave_first + 63u, n - 1u) : wave_first]);
        window[wave][lane] = merge_rank(keys_of[l], 0, count_of[l], t, descending, l < my);
    }
    __syncthreads();
    const uint32_t i = first + threadIdx.x;
    uint32_t at = 0xFFFFFFFFu;
    if (i < n) {
        const uint32_t key = my_keys[i], t = merge_key(key);
        at = i;
        for (uint32_t l = 0; l < lists; l++)
            if (l != my)
                at += merge_rank(keys_of[l], window[wave][2u * l], window[wave][2u * l + 1u], t, descending, l < my);
        if (at < g.capacity) {
            uint8_t* rec = reinterpret_cast<uint8_t*>(stage) + threadIdx.x * g.stride;
            const uint32_t slot = mine.idx[i];
            const unsigned long long offset =
                (unsigned long long)(mine.slot_map ? mine.slot_map[slot] : slot) * mine.component_stride;  // componentOffset  mesh.cpp:170
            uint32_t* w = reinterpret_cast<uint32_t*>(rec + g.component_offset);
            w[0] = (uint32_t)offset;
            w[1] = (uint32_t)(offset >> 32);
            const float4* rows = reinterpret_cast<const float4*>(mine.model) + (size_t)i * 3;
            const float4 r0 = rows[0], r1 = rows[1], r2 = rows[2];
            float* bm = reinterpret_cast<float*>(rec + g.baked_model);
            bm[0] = r0.x; bm[1] = r0.y; bm[2] = r0.z; bm[3] = r0.w;
            bm[4] = r1.x; bm[5] = r1.y; bm[6] = r1.z; bm[7] = r1.w;
            bm[8] = r2.x; bm[9] = r2.y; bm[10] = r2.z; bm[11] = r2.w;
            *reinterpret_cast<uint32_t*>(rec + g.distance_sq) = key;
            if (g.buffer_index != 0xFFFFFFFFu)
                *reinterpret_cast<uint32_t*>(rec + g.buffer_index) = mine.buffer_index;
        } else {
            at = 0xFFFFFFFFu;
        }
    }
    place[threadIdx.x] = at;
    __syncthreads();
    const uint32_t pieces = min(kMergeBlock, n - first) * quads;
    for (uint32_t q = threadIdx.x; q < pieces; q += kMergeBlock) {
        const uint32_t r = q / quads, p = q - r * quads;
        const uint32_t to = place[r];
        if (to != 0xFFFFFFFFu)
            reinterpret_cast<uint4*>(g.dst + (size_t)to * g.stride)[p] = stage[q];
    }
}

hipError_t launch_merge_sorted(const MergeLaunch& launch, uint32_t widest, hipStream_t stream)
{
    const dim3 grid(std::max(1u, (widest + kMergeBlock - 1u) / kMergeBlock), std::max(1u, launch.lists)), block(kMergeBlock);
    hipLaunchKernelGGL(merge_sorted_kernel, grid, block, 0, stream, launch);
    return hipGetLastError();
}

}  // namespace gv
