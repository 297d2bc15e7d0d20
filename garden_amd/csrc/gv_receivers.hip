// gv_receivers.hip — gfx950 (CDNA4, wave64) kernels of gv_pool_draw_receivers: the cull AABBs of a view's draws rasterised OUTWARDS
// into a receiver mask in a light's clip space, each pixel keeping the smallest of the boxes' farthest depths (DESIGN.md §4 item 17,
// §5.20), the rule in gv_device_math.hpp (receiver_*, and occluder_clip / occluder_snap / occluder_edges where the words are item
// 16's). THREE launches per call whatever the counts, the middle one gv_occluders.hip's scan:
//
//   receiver_setup_kernel   256 lanes, one record per lane; the grid is sized from the view's occupancy, and a workgroup whose first
//                           record is at or beyond the device count leaves after ONE wave-uniform load. Per record: idx[k] and the three
//                           16-byte model loads stream in, inv[s] and the entry's box are gathered (as bounds_fold_kernel reads them);
//                           corners, clip, depth, snap, face signs, the edge word and the pixel range follow in registers
//                           (receiver_setup). EVERY record of a view is a receiver, and most touch a handful of pixels: a record
//                           whose range holds at most kReceiverSmallPixels pixels is written here, by its own lane — one bit per
//                           pixel, each active edge evaluated at the pixel's best corner — and takes no further part. Of the others
//                           nothing is stored but the tile count: the T x T cells of the mask's tile grid the range touches (the
//                           whole grid for a record counted behind or range) are scanned across the workgroup: local[k] is the
//                           exclusive prefix, base[block] the total. The five counts are tallied in LDS (a ballot per class and wave)
//                           and added with one atomicAdd per non-zero field.
//   occluder_scan_kernel    (gv_occluders.hip, through launch_occluder_scan) base[] -> items in front of each workgroup, base[B] the total.
//   receiver_raster_kernel  a FIXED grid (kReceiverRasterGroups x 4 waves): wave w takes the items [w c, (w + 1) c), c = ceil(total /
//                           waves), an item being (receiver, tile). The first item of a run is found by two binary searches (base[],
//                           then local[] of that workgroup's records) and computes the receiver's row again (receiver_setup: every
//                           lane the same words); the following items of the same receiver reuse it. Per item the active edges are
//                           evaluated over the tile's clipped rectangle: no pixel passes some edge — next item; all pass all — no
//                           per-pixel test; otherwise each lane tests its pixels at their best corner (exact in int64: the same
//                           truth as the rule's four corners). A wave step is two mask rows of 32 pixels: per touched pixel a plain
//                           load, and global_atomic_umin only where the stored word is larger — the floor under a crowd is written
//                           once (a stale larger read costs one atomic, never a wrong value: the minimum is idempotent).
//
// Policy as gv_cull.hip: no workgroup waits for another, no atomic decides a place — the only atomics are the minimum and the counts.
// Whatever a record's slot holds, inv is read below `slots` and the boxes below `entries` only; every pixel written lies inside the
// range step 5 clamps to the mask the same launch was given.
#include "gv_device.hpp"
#include "gv_receiver_kernels.hpp"

namespace gv {

namespace {

constexpr uint32_t kWaves = kReceiverBlock / 64u;
constexpr uint32_t kTileShift = 5;
static_assert((1u << kTileShift) == kReceiverTile, "tile coordinates are shifts");
constexpr uint32_t kSteps = kReceiverTile / 2u;  // wave steps per tile: two rows each
constexpr uint32_t kOutside = 4;                 // the field of ReceiverCounts of a record that writes nothing

__device__ __forceinline__ uint32_t records_of_launch(const ReceiverLaunch& a) { return min(*a.count, a.capacity); }

// Steps 1 - 6 for record k (k below the view's count): the field of ReceiverCounts the record is counted in, and — unless that is
// `outside` — in `row` what writing it needs. Both launches call it: the setup launch for the class, the small ranges and the tile
// count, the raster launch again for the row, once per run of items of one receiver — the same instructions over the same words.
__device__ __forceinline__ uint32_t receiver_setup(const ReceiverLaunch& a, uint32_t k, ReceiverRow& row)
{
    const uint32_t slot = stream_load(a.idx + k);
    const float4* const rows = reinterpret_cast<const float4*>(a.model) + (size_t)k * 3;
    const float4 w0 = stream_load(rows), w1 = stream_load(rows + 1), w2 = stream_load(rows + 2);
    uint32_t entry = kSlotNone;
    if (slot < a.slots)
        entry = a.inv ? a.inv[slot] : slot;
    float4 box_a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (a record outside the mirror takes the empty box)
    float2 box_b = make_float2(0.0f, 0.0f);
    if (entry < a.entries) {
        box_a = a.a[entry];
        box_b = a.b[entry];
    }
    Corners c;
    aabb_corners(rows_model(w0, w1, w2), box_a.x, box_a.y, box_a.z, box_a.w, box_b.x, box_b.y, c);
    float u[8], v[8], z[8];
    const bool in_front = occluder_clip(a.light, c, u, v, z);
    const uint32_t whole_x = (a.width - 1) << 16, whole_y = (a.height - 1) << 16;
    row.edges = 0;
    row.xr = whole_x, row.yr = whole_y;
    if (!in_front) {
        row.depth_bits = 0;  // +0.0f
        return 2;
    }
    row.depth_bits = __float_as_uint(receiver_depth(z));
    const float sx = (float)(16u * a.width), sy = (float)(16u * a.height);
    bool in_range = true;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        in_range = occluder_snap(u[i], sx, row.X[i]) && in_range;
        in_range = occluder_snap(v[i], sy, row.Y[i]) && in_range;
    }
    if (!in_range)
        return 3;
    int32_t xmin = row.X[0], xmax = row.X[0], ymin = row.Y[0], ymax = row.Y[0];
#pragma unroll
    for (int i = 1; i < 8; i++) {
        xmin = min(xmin, row.X[i]), xmax = max(xmax, row.X[i]);
        ymin = min(ymin, row.Y[i]), ymax = max(ymax, row.Y[i]);
    }
    const int32_t x0 = max((xmin - 2) >> 4, 0), x1 = min((xmax + 2) >> 4, (int32_t)a.width - 1);
    const int32_t y0 = max((ymin - 2) >> 4, 0), y1 = min((ymax + 2) >> 4, (int32_t)a.height - 1);
    if (x0 > x1 || y0 > y1)
        return kOutside;
    row.xr = (uint32_t)x0 | ((uint32_t)x1 << 16);
    row.yr = (uint32_t)y0 | ((uint32_t)y1 << 16);
    row.edges = occluder_edges(row.X, row.Y);
    return row.edges ? 0 : 1;
}

// active edge e of the row, directed as its positive face has it
__device__ __forceinline__ OccluderEdge receiver_edge_of(const ReceiverRow& row, int e)
{
    const bool rev = (row.edges >> (12 + e)) & 1u;
    const int p = kOccluderEdgeA[e], q = kOccluderEdgeB[e];
    return receiver_edge(rev ? row.X[q] : row.X[p], rev ? row.Y[q] : row.Y[p], rev ? row.X[p] : row.X[q], rev ? row.Y[p] : row.Y[q]);
}

__device__ __forceinline__ void receiver_store(uint32_t* at, uint32_t bits)
{
    if (__atomic_load_n(at, __ATOMIC_RELAXED) > bits)
        atomicMin(at, bits);
}

__device__ __forceinline__ uint32_t receiver_tiles(const ReceiverRow& row)
{
    const uint32_t x0 = row.xr & 0xFFFFu, x1 = row.xr >> 16, y0 = row.yr & 0xFFFFu, y1 = row.yr >> 16;
    return ((x1 >> kTileShift) - (x0 >> kTileShift) + 1) * ((y1 >> kTileShift) - (y0 >> kTileShift) + 1);
}

// a range of at most kReceiverSmallPixels pixels, by the record's own lane
__device__ __forceinline__ void receiver_write_small(const ReceiverLaunch& a, const ReceiverRow& row, uint32_t wide, uint32_t pixels)
{
    const int32_t x0 = (int32_t)(row.xr & 0xFFFFu), y0 = (int32_t)(row.yr & 0xFFFFu);
    uint32_t keep = 0xFFFFFFFFu >> (32u - pixels);
#pragma unroll
    for (int e = 0; e < 12; e++) {
        if ((row.edges >> e) & 1u) {
            const OccluderEdge g = receiver_edge_of(row, e);
            for (uint32_t i = 0; i < pixels; i++)
                keep &= ~((receiver_edge_at(g, x0 + (int32_t)(i % wide), y0 + (int32_t)(i / wide)) < 0 ? 1u : 0u) << i);
        }
    }
    uint32_t* const image = reinterpret_cast<uint32_t*>(a.mask);
    for (uint32_t i = 0; i < pixels; i++)
        if ((keep >> i) & 1u)
            receiver_store(image + (size_t)(y0 + (int32_t)(i / wide)) * a.width + (uint32_t)(x0 + (int32_t)(i % wide)), row.depth_bits);
}

__global__ __launch_bounds__(kReceiverBlock) void receiver_setup_kernel(const ReceiverLaunch a)
{
    __shared__ uint32_t wave_total[kWaves];
    __shared__ uint32_t tally[5];
    const uint32_t n = records_of_launch(a);
    const uint32_t first = blockIdx.x * kReceiverBlock;
    if (first >= n)
        return;  // (the whole workgroup, after ONE load: the grid is sized for the occupancy)
    if (threadIdx.x < 5)
        tally[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t k = first + threadIdx.x;
    uint32_t tiles = 0, counted = 5;  // counted: the field of ReceiverCounts the lane's record goes to (5: the lane has none)
    if (k < n) {
        ReceiverRow row;
        counted = receiver_setup(a, k, row);
        if (counted != kOutside) {
            const uint32_t wide = (row.xr >> 16) - (row.xr & 0xFFFFu) + 1, high = (row.yr >> 16) - (row.yr & 0xFFFFu) + 1;
            if (wide * high <= kReceiverSmallPixels)  // (at most 2^15 each)
                receiver_write_small(a, row, wide, wide * high);
            else
                tiles = receiver_tiles(row);
        }
    }
    // the tally: per class one ballot and one LDS add per wave
#pragma unroll
    for (uint32_t c = 0; c < 5; c++) {
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
    if (threadIdx.x < 5 && tally[threadIdx.x])
        atomicAdd(reinterpret_cast<uint32_t*>(a.counts) + threadIdx.x, tally[threadIdx.x]);
}

__global__ __launch_bounds__(kReceiverBlock) void receiver_raster_kernel(const ReceiverLaunch a)
{
    const uint32_t n = records_of_launch(a);
    const uint32_t blocks = (n + kReceiverBlock - 1) / kReceiverBlock;
    const unsigned long long total = a.base[blocks];
    const unsigned long long waves = (unsigned long long)gridDim.x * kWaves;
    const unsigned long long share = (total + waves - 1) / waves;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + (threadIdx.x >> 6)));
    const unsigned long long i0 = wave * share, i1 = min(i0 + share, total);
    const uint32_t lane = threadIdx.x & 63u, col = lane & 31u, upper = lane >> 5;
    uint32_t* const image = reinterpret_cast<uint32_t*>(a.mask);
    unsigned long long begin = 0, end = 0;  // the items of the receiver `row` belongs to
    ReceiverRow row;
    bool listed = false;
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
            const uint32_t rel = (uint32_t)(i - base), held = min(kReceiverBlock, n - b * kReceiverBlock);
            const uint32_t* const local = a.local + (size_t)b * kReceiverBlock;
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
            listed = receiver_setup(a, b * kReceiverBlock + lo, row) != kOutside;  // (it is: only a listed receiver has tiles)
        }
        if (!listed)
            continue;
        const int32_t x0 = (int32_t)(row.xr & 0xFFFFu), x1 = (int32_t)(row.xr >> 16), y0 = (int32_t)(row.yr & 0xFFFFu), y1 = (int32_t)(row.yr >> 16);
        const uint32_t tiles_x = (uint32_t)((x1 >> kTileShift) - (x0 >> kTileShift) + 1);
        const uint32_t t = (uint32_t)(i - begin);
        const int32_t px0 = (int32_t)(((uint32_t)(x0 >> kTileShift) + t % tiles_x) << kTileShift);
        const int32_t py0 = (int32_t)(((uint32_t)(y0 >> kTileShift) + t / tiles_x) << kTileShift);
        // the tile clipped to the receiver's pixel range (never empty: the tile grid cell touches the range)
        const int32_t rx0 = max(px0, x0), rx1 = min(px0 + (int32_t)kReceiverTile - 1, x1);
        const int32_t ry0 = max(py0, y0), ry1 = min(py0 + (int32_t)kReceiverTile - 1, y1);
        bool all = true, none = false;
#pragma unroll
        for (int e = 0; e < 12; e++) {
            if ((row.edges >> e) & 1u) {
                const OccluderEdge g = receiver_edge_of(row, e);
                all = all && receiver_edge_lo(g, rx0, rx1, ry0, ry1) >= 0;
                none = none || receiver_edge_hi(g, rx0, rx1, ry0, ry1) < 0;
            }
        }
        if (none)
            continue;
        const int32_t px = px0 + (int32_t)col, row0 = py0 + (int32_t)upper;  // the lane's pixel of step s: (px, row0 + 2 s)
        uint32_t keep = px >= rx0 && px <= rx1 ? 0xFFFFu : 0u;
        if (!all) {
#pragma unroll
            for (int e = 0; e < 12; e++) {
                if ((row.edges >> e) & 1u) {
                    const OccluderEdge g = receiver_edge_of(row, e);
                    long long at = receiver_edge_at(g, px, row0);
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
            if (((keep >> s) & 1u) && py >= ry0 && py <= ry1)
                receiver_store(image + (size_t)py * a.width + (uint32_t)px, row.depth_bits);
        }
    }
}

}  // namespace

hipError_t launch_receiver_setup(const ReceiverLaunch& launch, hipStream_t stream)
{
    const uint32_t blocks = (launch.capacity + kReceiverBlock - 1) / kReceiverBlock;
    hipLaunchKernelGGL(receiver_setup_kernel, dim3(std::max(1u, blocks)), dim3(kReceiverBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_receiver_raster(const ReceiverLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(receiver_raster_kernel, dim3(kReceiverRasterGroups), dim3(kReceiverBlock), 0, stream, launch);
    return hipGetLastError();
}

}  // namespace gv
