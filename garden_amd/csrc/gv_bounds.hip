// gv_bounds.hip — gfx950 (CDNA4, wave64) kernels of gv_pool_view_bounds: the bounds of a view's visible draws in a caller's basis
// (DESIGN.md §4 item 14, §5.17), the rule in gv_device_math.hpp (bounds_key, bounds_project over aabb_corners). TWO launches for
// all items of a call, no memset, no atomics:
//
//   bounds_fold_kernel    256 lanes, kBoundsRecords records per workgroup (kBoundsRecords / 256 per lane, strided so that every
//                         load of a wave is coalesced). The grid is sized from the listed views' occupancies, as lod_kernel's; a
//                         workgroup whose first record is at or beyond the device count leaves after ONE wave-uniform load and
//                         stores nothing. Per record: idx[k] and the three 16-byte model loads stream in; the gathers inv[s],
//                         then a[e] / b[e] follow (the mirror is in spatial order and so are unsorted records: mostly line-coherent).
//                         Each lane keeps six keys and a NaN-record count; integer min / max across the wave by __shfl_xor, across
//                         the four waves through LDS; one lane stores the workgroup's 8-word row of KEYS.
//   bounds_finish_kernel  one workgroup per item: reads the device count, folds the ceil(n / kBoundsRecords) rows of its item —
//                         the only rows written — decodes the keys and stores the item's GvViewBounds (n = 0: the empty answer).
//
// Policy as gv_cull.hip: static tile ids, no workgroup waits for another. Whatever a record's slot holds, inv is read below
// `slots` and the boxes below `entries` only; a record outside takes the empty box.
#include "gv_device.hpp"
#include "gv_bounds_kernels.hpp"

namespace gv {

namespace {

constexpr uint32_t kWaves = kBoundsBlock / 64u;
constexpr uint32_t kPerLane = kBoundsRecords / kBoundsBlock;

struct BoundsAcc {
    uint32_t lo[3], hi[3], nan_records;
};

__device__ __forceinline__ void fold_row(const v2f (&q)[4], uint32_t& lo, uint32_t& hi, bool& nan)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float e[2] = {q[j].x, q[j].y};
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const bool number = e[h] == e[h];
            const uint32_t key = bounds_key(e[h]);
            lo = min(lo, number ? key : kBoundsLoIdentity);
            hi = max(hi, number ? key : kBoundsHiIdentity);
            nan = nan || !number;
        }
    }
}

// the workgroup's fold of `acc`: on return lane 0 holds it
__device__ __forceinline__ void reduce_workgroup(BoundsAcc& acc, uint32_t (&part)[kWaves][8])
{
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
            acc.lo[r] = min(acc.lo[r], (uint32_t)__shfl_xor((int)acc.lo[r], (int)d, 64));
            acc.hi[r] = max(acc.hi[r], (uint32_t)__shfl_xor((int)acc.hi[r], (int)d, 64));
        }
        acc.nan_records += (uint32_t)__shfl_xor((int)acc.nan_records, (int)d, 64);
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
            part[wave][r] = acc.lo[r];
            part[wave][4 + r] = acc.hi[r];
        }
        part[wave][3] = acc.nan_records;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t w = 1; w < kWaves; w++) {
#pragma unroll
            for (int r = 0; r < 3; r++) {
                acc.lo[r] = min(acc.lo[r], part[w][r]);
                acc.hi[r] = max(acc.hi[r], part[w][4 + r]);
            }
            acc.nan_records += part[w][3];
        }
    }
}

__global__ __launch_bounds__(kBoundsBlock) void bounds_fold_kernel(const BoundsLaunch a)
{
    __shared__ uint32_t part[kWaves][8];
    if (blockIdx.x >= a.first_block[a.items])
        return;  // (a call whose views hold no slot at all still launches one workgroup)
    const uint32_t v = view_of_block(a.first_block, a.items, blockIdx.x);
    const BoundsItem& it = a.item[v];
    const uint32_t n = min(*it.count, it.capacity);
    const uint32_t first = (blockIdx.x - a.first_block[v]) * kBoundsRecords;
    if (first >= n)
        return;  // (the whole workgroup, after ONE load: the grid is sized for the occupancy)
    BoundsAcc acc;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        acc.lo[r] = kBoundsLoIdentity;
        acc.hi[r] = kBoundsHiIdentity;
    }
    acc.nan_records = 0;
    // the streams of all of the lane's records first, then the gathers that depend on them
    uint32_t slot[kPerLane];
    float4 w0[kPerLane], w1[kPerLane], w2[kPerLane];
#pragma unroll
    for (uint32_t j = 0; j < kPerLane; j++) {
        const uint32_t k = first + j * kBoundsBlock + threadIdx.x;
        slot[j] = kSlotNone;
        if (k < n) {
            slot[j] = stream_load(it.idx + k);
            const float4* const rows = reinterpret_cast<const float4*>(it.model) + (size_t)k * 3;
            w0[j] = stream_load(rows);
            w1[j] = stream_load(rows + 1);
            w2[j] = stream_load(rows + 2);
        }
    }
    uint32_t entry[kPerLane];
#pragma unroll
    for (uint32_t j = 0; j < kPerLane; j++) {
        const uint32_t k = first + j * kBoundsBlock + threadIdx.x;
        entry[j] = kSlotNone;
        if (k < n && slot[j] < a.slots)
            entry[j] = a.inv ? a.inv[slot[j]] : slot[j];
    }
#pragma unroll
    for (uint32_t j = 0; j < kPerLane; j++) {
        const uint32_t k = first + j * kBoundsBlock + threadIdx.x;
        if (k < n) {
            float4 box_a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float2 box_b = make_float2(0.0f, 0.0f);
            if (entry[j] < a.entries) {
                box_a = a.a[entry[j]];
                box_b = a.b[entry[j]];
            }
            const Mat34 m = rows_model(w0[j], w1[j], w2[j]);
            Corners c;
            aabb_corners(m, box_a.x, box_a.y, box_a.z, box_a.w, box_b.x, box_b.y, c);
            bool nan = false;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                v2f q[4];
                bounds_project(c, it.basis[r], it.basis[3 + r], it.basis[6 + r], it.basis[9 + r], q);
                fold_row(q, acc.lo[r], acc.hi[r], nan);
            }
            acc.nan_records += nan ? 1u : 0u;
        }
    }
    reduce_workgroup(acc, part);
    if (threadIdx.x == 0) {
        uint4* const row = reinterpret_cast<uint4*>(a.partial + blockIdx.x);
        row[0] = make_uint4(acc.lo[0], acc.lo[1], acc.lo[2], acc.nan_records);
        row[1] = make_uint4(acc.hi[0], acc.hi[1], acc.hi[2], 0u);
    }
}

__global__ __launch_bounds__(kBoundsBlock) void bounds_finish_kernel(const BoundsLaunch a)
{
    __shared__ uint32_t part[kWaves][8];
    const uint32_t v = blockIdx.x;
    const BoundsItem& it = a.item[v];
    const uint32_t n = min(*it.count, it.capacity);
    const uint32_t rows = min((n + kBoundsRecords - 1) / kBoundsRecords, a.first_block[v + 1] - a.first_block[v]);
    BoundsAcc acc;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        acc.lo[r] = kBoundsLoIdentity;
        acc.hi[r] = kBoundsHiIdentity;
    }
    acc.nan_records = 0;
    for (uint32_t row = threadIdx.x; row < rows; row += kBoundsBlock) {
        const uint4* const p = reinterpret_cast<const uint4*>(a.partial + a.first_block[v] + row);
        const uint4 l = p[0], h = p[1];
        acc.lo[0] = min(acc.lo[0], l.x), acc.lo[1] = min(acc.lo[1], l.y), acc.lo[2] = min(acc.lo[2], l.z);
        acc.hi[0] = max(acc.hi[0], h.x), acc.hi[1] = max(acc.hi[1], h.y), acc.hi[2] = max(acc.hi[2], h.z);
        acc.nan_records += l.w;
    }
    reduce_workgroup(acc, part);
    if (threadIdx.x == 0) {
        BoundsResult out;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            out.lo[r] = bounds_unkey(acc.lo[r]);
            out.hi[r] = bounds_unkey(acc.hi[r]);
        }
        out.draw_count = *it.count;
        out.nan_records = acc.nan_records;
        a.out[v] = out;
    }
}

}  // namespace

hipError_t launch_bounds_fold(const BoundsLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(bounds_fold_kernel, dim3(std::max(1u, launch.first_block[launch.items])), dim3(kBoundsBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_bounds_finish(const BoundsLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(bounds_finish_kernel, dim3(launch.items), dim3(kBoundsBlock), 0, stream, launch);
    return hipGetLastError();
}

}  // namespace gv
