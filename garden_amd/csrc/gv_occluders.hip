// gv_occluders.hip — gfx950 (CDNA4, wave64) kernels of gv_pool_draw_occluders: the occluder boxes of a view's draws rasterised into a
// depth image, the rule in gv_device_math.hpp (occluder_*). THREE launches per call whatever the counts:
//
//   occluder_setup_kernel   256 lanes, one record per lane; the grid is sized from the view's occupancy, and a workgroup whose first
//                           record is at or beyond the device count leaves after ONE wave-uniform load. Per record: idx[k] and the three
//                           16-byte model loads stream in, the slot's two box rows are gathered; corners, clip, depth, snap, face signs,
//                           the edge word and the pixel range follow in registers (occluder_setup). Nothing of it is stored but the
//                           class and the tile count. The tiles of a drawn occluder — the T x T cells of the image's tile grid its
//                           pixel range touches — are scanned across the workgroup (shuffles, then four wave totals through LDS):
//                           local[k] is the exclusive prefix, base[block] the total. The six counts are tallied in LDS (a ballot
//                           per class and wave) and added with one atomicAdd per non-zero field.
//   occluder_scan_kernel    one workgroup: base[] of the ceil(n / 256) setup workgroups that ran -> items in front of each, base[B]
//                           the total. 1024 entries a turn, the carry in a register.
//   occluder_raster_kernel  a FIXED grid (kOccluderRasterGroups x 4 waves): wave w takes the items [w c, (w + 1) c), c = ceil(total /
//                           waves), an item being (occluder, tile). The first item of a run is found by two binary searches (base[],
//                           then local[] of that workgroup's records) and computes the occluder's row again (occluder_setup: every
//                           lane the same words); the following items of the same occluder reuse it. Per item the active edges are evaluated at the corners of the tile's clipped rectangle: outside some edge — next
//                           item; inside all — no per-pixel test; otherwise each lane tests its pixels at the corner where the edge
//                           function is smallest (exact in int64: the same truth as the rule's four corners). A wave step is two image
//                           rows of 32 pixels: per covered pixel a plain load, and global_atomic_umax only where the stored word is
//                           smaller — two 128-byte row segments per atomic instruction (a stale smaller read costs one atomic, never a
//                           wrong value: the maximum is idempotent).
//
// Policy as gv_cull.hip: no workgroup waits for another, no atomic decides a place — the only atomics are the maximum and the counts.
// Whatever a record's slot holds, the boxes are read below `slots` only; every pixel written lies inside the range item 8 clamps to
// the image the same launch was given.
#include "gv_device.hpp"
#include "gv_occluder_kernels.hpp"

namespace gv {

namespace {

constexpr uint32_t kWaves = kOccluderBlock / 64u;
constexpr uint32_t kTileShift = 5;
static_assert((1u << kTileShift) == kOccluderTile, "tile coordinates are shifts");
constexpr uint32_t kSteps = kOccluderTile / 2u;  // wave steps per tile: two rows each

__device__ __forceinline__ uint32_t records_of_launch(const OccluderLaunch& a) { return min(*a.count, a.capacity); }

// Items 1 - 6 and 8 for record k (k below the view's count): the field of OccluderCounts the record is counted in — 0: drawn, and
// then `row` holds what the raster needs of it. Both launches call it: the setup launch for the class and the tile count, the raster
// launch again for the row, once per run of items of one occluder — the same instructions over the same words, so the same row;
// what is spared is a row per slot of the view in device memory.
__device__ __forceinline__ uint32_t occluder_setup(const OccluderLaunch& a, uint32_t k, OccluderRow& row)
{
    const uint32_t slot = stream_load(a.idx + k);
    const float4* const rows = reinterpret_cast<const float4*>(a.model) + (size_t)k * 3;
    const float4 w0 = stream_load(rows), w1 = stream_load(rows + 1), w2 = stream_load(rows + 2);
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;  // (a record outside the mirror has no box)
    if (slot < a.slots) {
        lo = a.boxes[(size_t)2 * slot];
        hi = a.boxes[(size_t)2 * slot + 1];
    }
    uint32_t cls = 0;  // the field of OccluderCounts this record is counted in
    if (!(lo.x < hi.x && lo.y < hi.y && lo.z < hi.z)) {
        cls = 1;
    } else {
        Corners c;
        aabb_corners(rows_model(w0, w1, w2), lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, c);
        float u[8], v[8], z[8];
        const bool in_front = occluder_clip(a.view_proj, c, u, v, z);
        const float d = occluder_depth(z);
        if (!in_front || !(d > 0.0f)) {
            cls = 2;
        } else {
            const float sx = (float)(16u * a.width), sy = (float)(16u * a.height);
            bool in_range = true;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                in_range = occluder_snap(u[i], sx, row.X[i]) && in_range;
                in_range = occluder_snap(v[i], sy, row.Y[i]) && in_range;
            }
            if (!in_range) {
                cls = 3;
            } else {
                row.edges = occluder_edges(row.X, row.Y);
                if (!row.edges) {
                    cls = 4;
                } else {
                    int32_t xmin = row.X[0], xmax = row.X[0], ymin = row.Y[0], ymax = row.Y[0];
#pragma unroll
                    for (int i = 1; i < 8; i++) {
                        xmin = min(xmin, row.X[i]), xmax = max(xmax, row.X[i]);
                        ymin = min(ymin, row.Y[i]), ymax = max(ymax, row.Y[i]);
                    }
                    const int32_t x0 = max(xmin >> 4, 0), x1 = min(xmax >> 4, (int32_t)a.width - 1);
                    const int32_t y0 = max(ymin >> 4, 0), y1 = min(ymax >> 4, (int32_t)a.height - 1);
                    if (x0 > x1 || y0 > y1 || (uint32_t)(x1 - x0 + 1) < a.min_pixels || (uint32_t)(y1 - y0 + 1) < a.min_pixels) {
                        cls = 5;
                    } else {
                        row.depth_bits = __float_as_uint(d);
                        row.xr = (uint32_t)x0 | ((uint32_t)x1 << 16);
                        row.yr = (uint32_t)y0 | ((uint32_t)y1 << 16);
                    }
                }
            }
        }
    }
    return cls;
}

__device__ __forceinline__ uint32_t occluder_tiles(const OccluderRow& row)
{
    const uint32_t x0 = row.xr & 0xFFFFu, x1 = row.xr >> 16, y0 = row.yr & 0xFFFFu, y1 = row.yr >> 16;
    return ((x1 >> kTileShift) - (x0 >> kTileShift) + 1) * ((y1 >> kTileShift) - (y0 >> kTileShift) + 1);
}

__global__ __launch_bounds__(kOccluderBlock) void occluder_setup_kernel(const OccluderLaunch a)
{
    __shared__ uint32_t wave_total[kWaves];
    __shared__ uint32_t tally[6];
    const uint32_t n = records_of_launch(a);
    const uint32_t first = blockIdx.x * kOccluderBlock;
    if (first >= n)
        return;  // (the whole workgroup, after ONE load: the grid is sized for the occupancy)
    if (threadIdx.x < 6)
        tally[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t k = first + threadIdx.x;
    uint32_t tiles = 0, counted = 6;  // counted: the field of OccluderCounts the lane's record goes to (6: the lane has none)
    if (k < n) {
        OccluderRow row;
        counted = occluder_setup(a, k, row);
        if (counted == 0)
            tiles = occluder_tiles(row);
    }
    // the tally: per class one ballot and one LDS add per wave (most records of a real view are of ONE class, no_box)
#pragma unroll
    for (uint32_t c = 0; c < 6; c++) {
        const uint32_t members = (uint32_t)__popcll(__ballot(counted == c));
        if ((threadIdx.x & 63u) == 0 && members)
            atomicAdd(&tally[c], members);
    }
    // the workgroup's exclusive scan of `tiles` (at most 2^20 each: 2^28 a workgroup)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = tiles;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        incl += lane >= d ? up : 0u;
    }
    if (lane == 63)
        wave_total[wave] = incl;
    __syncthreads();
    uint32_t in_front_of_wave = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; w++) {
        in_front_of_wave += w < wave ? wave_total[w] : 0u;
        total += wave_total[w];
    }
    if (k < n)
        a.local[k] = in_front_of_wave + incl - tiles;
    if (threadIdx.x == 0)
        a.base[blockIdx.x] = total;
    if (threadIdx.x < 6 && tally[threadIdx.x])
        atomicAdd(reinterpret_cast<uint32_t*>(a.counts) + threadIdx.x, tally[threadIdx.x]);
}

__global__ __launch_bounds__(kOccluderBlock) void occluder_scan_kernel(const OccluderLaunch a)
{
    __shared__ unsigned long long wave_total[kWaves];
    const uint32_t n = records_of_launch(a);
    const uint32_t blocks = (n + kOccluderBlock - 1) / kOccluderBlock;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (uint32_t start = 0; start < blocks; start += 4 * kOccluderBlock) {
        const uint32_t at = start + 4 * threadIdx.x;
        unsigned long long v[4], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            v[j] = at + j < blocks ? a.base[at + j] : 0ull;
            sum += v[j];
        }
        unsigned long long incl = sum;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d, 64);
            incl += lane >= d ? up : 0ull;
        }
        __syncthreads();  // (the previous turn's reads of wave_total)
        if (lane == 63)
            wave_total[wave] = incl;
        __syncthreads();
        unsigned long long before = carry, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; w++) {
            before += w < wave ? wave_total[w] : 0ull;
            total += wave_total[w];
        }
        before += incl - sum;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (at + j < blocks)
                a.base[at + j] = before;
            before += v[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0)
        a.base[blocks] = carry;
}

__global__ __launch_bounds__(kOccluderBlock) void occluder_raster_kernel(const OccluderLaunch a)
{
    const uint32_t n = records_of_launch(a);
    const uint32_t blocks = (n + kOccluderBlock - 1) / kOccluderBlock;
    const unsigned long long total = a.base[blocks];
    const unsigned long long waves = (unsigned long long)gridDim.x * kWaves;
    const unsigned long long share = (total + waves - 1) / waves;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + (threadIdx.x >> 6)));
    const unsigned long long i0 = wave * share, i1 = min(i0 + share, total);
    const uint32_t lane = threadIdx.x & 63u, col = lane & 31u, upper = lane >> 5;
    uint32_t* const image = reinterpret_cast<uint32_t*>(a.depth);
    unsigned long long begin = 0, end = 0;  // the items of the occluder `row` belongs to
    OccluderRow row;
    bool drawn = false;
    for (unsigned long long i = i0; i < i1; i++) {
        if (i >= end) {
            uint32_t lo = 0, hi = blocks;  // the last workgroup b with base[b] <= i (base[blocks] = total > i)
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (a.base[mid] <= i)
                    lo = mid;
                else
                    hi = mid;
            }
            const uint32_t b = lo;
            const unsigned long long base = a.base[b];
            const uint32_t rel = (uint32_t)(i - base), held = min(kOccluderBlock, n - b * kOccluderBlock);
            const uint32_t* const local = a.local + (size_t)b * kOccluderBlock;
            lo = 0, hi = held;  // the last record j of it with local[j] <= rel: the one whose tiles hold rel
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (local[mid] <= rel)
                    lo = mid;
                else
                    hi = mid;
            }
            const uint32_t behind = lo + 1 < held ? local[lo + 1] : (uint32_t)(a.base[b + 1] - base);
            begin = base + local[lo];
            end = base + behind;
            drawn = occluder_setup(a, b * kOccluderBlock + lo, row) == 0;  // (it is: only a drawn occluder has tiles)
        }
        if (!drawn)
            continue;
        const int32_t x0 = (int32_t)(row.xr & 0xFFFFu), x1 = (int32_t)(row.xr >> 16), y0 = (int32_t)(row.yr & 0xFFFFu), y1 = (int32_t)(row.yr >> 16);
        const uint32_t tiles_x = (uint32_t)((x1 >> kTileShift) - (x0 >> kTileShift) + 1);
        const uint32_t t = (uint32_t)(i - begin);
        const int32_t px0 = (int32_t)(((uint32_t)(x0 >> kTileShift) + t % tiles_x) << kTileShift);
        const int32_t py0 = (int32_t)(((uint32_t)(y0 >> kTileShift) + t / tiles_x) << kTileShift);
        // the tile clipped to the occluder's pixel range (never empty: the tile grid cell touches the range)
        const int32_t rx0 = max(px0, x0), rx1 = min(px0 + (int32_t)kOccluderTile - 1, x1);
        const int32_t ry0 = max(py0, y0), ry1 = min(py0 + (int32_t)kOccluderTile - 1, y1);
        bool inside = true, outside = false;
#pragma unroll
        for (int e = 0; e < 12; e++) {
            if ((row.edges >> e) & 1u) {
                const bool rev = (row.edges >> (12 + e)) & 1u;
                const int p = kOccluderEdgeA[e], q = kOccluderEdgeB[e];
                const OccluderEdge g = occluder_edge(rev ? row.X[q] : row.X[p], rev ? row.Y[q] : row.Y[p], rev ? row.X[p] : row.X[q], rev ? row.Y[p] : row.Y[q]);
                inside = inside && occluder_edge_lo(g, rx0, rx1 + 1, ry0, ry1 + 1) >= 0;
                outside = outside || occluder_edge_hi(g, rx0, rx1 + 1, ry0, ry1 + 1) < 0;
            }
        }
        if (outside)
            continue;
        const int32_t px = px0 + (int32_t)col, row0 = py0 + (int32_t)upper;  // the lane's pixel of step s: (px, row0 + 2 s)
        uint32_t keep = px >= rx0 && px <= rx1 ? 0xFFFFu : 0u;
        if (!inside) {
#pragma unroll
            for (int e = 0; e < 12; e++) {
                if ((row.edges >> e) & 1u) {
                    const bool rev = (row.edges >> (12 + e)) & 1u;
                    const int p = kOccluderEdgeA[e], q = kOccluderEdgeB[e];
                    const OccluderEdge g = occluder_edge(rev ? row.X[q] : row.X[p], rev ? row.Y[q] : row.Y[p], rev ? row.X[p] : row.X[q], rev ? row.Y[p] : row.Y[q]);
                    long long at = occluder_edge_lo(g, px, px + 1, row0, row0 + 1);
                    const long long step = 32 * g.ex;  // two rows down
#pragma unroll
                    for (uint32_t s = 0; s < kSteps; s++) {
                        keep &= ~((at < 0 ? 1u : 0u) << s);
                        at += step;
                    }
                }
            }
        }
        const uint32_t s_first = (uint32_t)(ry0 - py0) >> 1, s_last = (uint32_t)(ry1 - py0) >> 1;
        for (uint32_t s = s_first; s <= s_last; s++) {
            const int32_t py = row0 + 2 * (int32_t)s;
            if (((keep >> s) & 1u) && py >= ry0 && py <= ry1) {
                uint32_t* const at = image + (size_t)py * a.width + (uint32_t)px;
                if (__atomic_load_n(at, __ATOMIC_RELAXED) < row.depth_bits)
                    atomicMax(at, row.depth_bits);
            }
        }
    }
}

}  // namespace

hipError_t launch_occluder_setup(const OccluderLaunch& launch, hipStream_t stream)
{
    const uint32_t blocks = (launch.capacity + kOccluderBlock - 1) / kOccluderBlock;
    hipLaunchKernelGGL(occluder_setup_kernel, dim3(std::max(1u, blocks)), dim3(kOccluderBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_occluder_scan(const OccluderLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(occluder_scan_kernel, dim3(1), dim3(kOccluderBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_occluder_raster(const OccluderLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(occluder_raster_kernel, dim3(kOccluderRasterGroups), dim3(kOccluderBlock), 0, stream, launch);
    return hipGetLastError();
}

}  // namespace gv
