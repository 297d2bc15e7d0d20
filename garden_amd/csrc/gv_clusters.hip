// gv_clusters.hip — gfx950 kernels of gv_pool_cull_clusters: every mesh cluster of every draw of the pool's last instance emission
// tested with the draw's own matrix, one indirect command per survivor. No new arithmetic: a cluster
// is tested as the cull tests an entity — aabb_corners, behind_frustum and hiz_occluded of gv_device.hpp, unchanged, over the
// record's bakedModel as delivered. A CANDIDATE is what may become one command: a cluster of a clustered draw, or a whole draw.
//
//   cluster_count_kernel   one lane per draw, 256 per workgroup, grid from the views' occupancies. idx -> id (or the selected id) ->
//                          range; candidates of the draw: 0 (void geometry, no instance, beyond the view's count), 1 (whole) or
//                          range.count. Workgroup-local exclusive prefix per draw (ballot-free: a wave scan and four wave totals),
//                          one candidate total and one tested total per workgroup, the draw's id kept for the launches behind.
//   cluster_scan_kernel    ONE workgroup of 1024 lanes, four entries per lane and turn, a running carry: the table becomes the
//                          exclusive prefix of itself. <0>: the count workgroups' totals (their number is host-known); also T,
//                          the candidates in front of every view, the clusters tested per view, and per tile the count workgroup
//                          that holds its first candidate. <1>: the tiles' survivor
//                          counts, ceil(T / 256) of them, read from the device; also the survivors in front of every view — a tile
//                          prefix plus the ballot bits below the view's first candidate — and with them the command counts.
//   cluster_test_kernel    one lane per candidate, tiles of 256 walked grid-stride by a grid of fixed size (8 workgroups per compute
//                          unit) with the device-read T as the limit: a bound of 6 x 10^8 candidates costs no empty workgroup.
//                          Candidate c -> (draw, j): the largest workgroup whose prefix is <= c — searched between the workgroup
//                          of the tile's first candidate and that of the next tile's, a table cluster_scan_kernel<0> leaves: a
//                          step or none — then the largest draw of it likewise (8 dependent loads, from tables the L2 holds). The 32-byte cluster as two
//                          16-byte loads, the draw's 48-byte model as three: neighbouring lanes share it, so it comes from cache.
//                          Corners once; then per view that has a lane in the wave (a tile may cross a view) the planes, the
//                          matrix and the pyramid from the kernel arguments at a wave-uniform offset, as cull_multi_hiz_kernel
//                          takes them, the six plane tests and the Hi-Z query. One ballot per wave: the word is kept (a bit per
//                          candidate), the tile's sum of popcounts is its survivor count.
//   cluster_write_kernel   the same walk. A survivor's position is its rank: the tile's prefix + the bits below it. It finds its
//                          draw again, builds the command and stores every word of the stride. With regions a second grid-stride
//                          walk writes the all-zero padding positions.
//
// Rank + scatter as gv_sort: no workgroup waits for another, no atomics, integer adds only — the order (view, draw, cluster) and
// every byte are the same run to run. Whatever an id, a range or a count holds, the tables are read inside their bounds: j is below
// the range's count by construction, a range lies inside the cluster table by the bind's check, T is at most the host's bound.
//
// Behind them, sharing their device helpers: the five kernels of gv_pool_cull_clusters_second_phase (cluster_second_*, described
// where they stand), which read what the five above left on the device and write none of it; and the three kernels of the run form
// gv_pool_cull_cluster_runs (cluster_run_*, described where they stand), which with the count, the scans and the test's walk above
// write one command per run of adjacent survivors; and the three test kernels of the normal-cone form gv_pool_cull_cluster_cones
// (cluster_cone_*: the test walks above instantiated with the cone test in their conjunction, described where they stand); and the
// six test kernels of the level-of-detail form gv_pool_cull_cluster_lods (cluster_lod_*: the same walks with the LOD cut in front).
#include "gv_device.hpp"
#include "gv_cluster_kernels.hpp"
#include "gv_cluster_second_kernels.hpp"
#include "gv_cluster_run_kernels.hpp"
#include "gv_cluster_cone_kernels.hpp"
#include "gv_cluster_lod_kernels.hpp"

namespace gv {

namespace {

typedef const ClusterLaunch __attribute__((address_space(4))) * ConstClusterArgs;
struct ClusterPlanes { float planes[6][4]; };
struct ClusterMatrix { float m[16]; };
__device__ __forceinline__ ClusterPlanes view_planes_of(ConstClusterArgs base, uint32_t v)
{
    ClusterPlanes out;
    __builtin_memcpy(&out, &base->planes[v], sizeof(out));
    return out;
}
__device__ __forceinline__ ClusterMatrix view_matrix_of(ConstClusterArgs base, uint32_t v)
{
    ClusterMatrix out;
    __builtin_memcpy(&out, &base->vp[v], sizeof(out));
    return out;
}
__device__ __forceinline__ HizDevice view_hiz_of(ConstClusterArgs base, uint32_t v)
{
    HizDevice out;
    __builtin_memcpy(&out, &base->hiz[v], sizeof(out));
    return out;
}

// The normal-cone test (gv_pool_cull_cluster_cones). The eye of view v lies in a wrapper struct behind
// the launch struct the walk reads: at byte `eye_offset` of the argument block, read at a wave-uniform offset like the planes.
struct ClusterEye { float e[4]; };
__device__ __forceinline__ ClusterEye view_eye_of(ConstClusterArgs base, uint32_t eye_offset, uint32_t v)
{
    ClusterEye out;
    __builtin_memcpy(&out, reinterpret_cast<const char __attribute__((address_space(4)))*>(base) + eye_offset + v * (uint32_t)sizeof(ClusterEye),
                     sizeof(out));
    return out;
}
// what a lane keeps of its draw and its cone for the views' tests: adj(A) and det A of the draw's 3x3 block, its translation, the cone
struct ConeLane {
    Adj33 adj;
    float t[3];
    float apex[3], cutoff, axis[3];
};
__device__ __forceinline__ ConeLane cone_lane(const Mat34& model, const float4 c0, const float4 c1)
{
    ConeLane c;
    c.adj = affine_adjugate(model);
    c.t[0] = model.c3x, c.t[1] = model.c3y, c.t[2] = model.c3z;
    c.apex[0] = c0.x, c.apex[1] = c0.y, c.apex[2] = c0.z, c.cutoff = c0.w;
    c.axis[0] = c1.x, c.axis[1] = c1.y, c.axis[2] = c1.z;
    return c;
}
// CONE-REJECTED, in model space: w = det * (apex - the eye in model space) for a point eye (eye.e[3] != 0), adj(A) * D for parallel
// rays along D. No division, no square root; a NaN anywhere, a zero axis, an eye at the apex, an overflowing square and a model
// with det <= 0 or not finite all keep the cluster (include/garden_vis.h).
__device__ __forceinline__ bool cone_rejected(const ConeLane& c, const ClusterEye& eye)
{
    const bool facing = c.adj.det > 0.0f && c.adj.det < __builtin_inff();
    float w[3];
    if (eye.e[3] != 0.0f) {  // (wave-uniform)
        const float u0 = eye.e[0] - c.t[0], u1 = eye.e[1] - c.t[1], u2 = eye.e[2] - c.t[2];
#pragma unroll
        for (uint32_t r = 0; r < 3u; r++)
            w[r] = fmaf(c.adj.det, c.apex[r], -fmaf(c.adj.j[r][0], u0, fmaf(c.adj.j[r][1], u1, c.adj.j[r][2] * u2)));
    } else {
#pragma unroll
        for (uint32_t r = 0; r < 3u; r++)
            w[r] = fmaf(c.adj.j[r][0], eye.e[0], fmaf(c.adj.j[r][1], eye.e[1], c.adj.j[r][2] * eye.e[2]));
    }
    const float s = fmaf(w[0], c.axis[0], fmaf(w[1], c.axis[1], w[2] * c.axis[2]));
    const float ww = fmaf(w[0], w[0], fmaf(w[1], w[1], w[2] * w[2]));
    const float q = s * s;
    const float r = (c.cutoff * c.cutoff) * ww;
    return facing && s > 0.0f && q > 0.0f && q < __builtin_inff() && q >= r;
}

// The level-of-detail cut (gv_pool_cull_cluster_lods). The ClusterLodView of view v lies in a wrapper
// struct behind the launch struct the walk reads: at byte `lod_offset` of the argument block, read at a wave-uniform offset.
__device__ __forceinline__ ClusterLodView view_lod_of(ConstClusterArgs base, uint32_t lod_offset, uint32_t v)
{
    ClusterLodView out;
    __builtin_memcpy(&out, reinterpret_cast<const char __attribute__((address_space(4)))*>(base) + lod_offset + v * (uint32_t)sizeof(ClusterLodView),
                     sizeof(out));
    return out;
}
// what a lane keeps of its draw and its LOD entry for the views' tests: s2, the two carried centres, the two radii and errors
struct LodLane {
    float s2;
    float self_c[3], parent_c[3];
    float self_r, parent_r, self_e, parent_e;
};
__device__ __forceinline__ LodLane lod_lane(const Mat34& model, const float4 l0, const float4 l1, const float4 l2)
{
    LodLane l;
    l.s2 = lod_scale2(model);
    lod_carry(model, l0.x, l0.y, l0.z, l.self_c);
    lod_carry(model, l1.x, l1.y, l1.z, l.parent_c);
    l.self_r = l0.w, l.parent_r = l1.w, l.self_e = l2.x, l.parent_e = l2.y;
    return l;
}
// LOD-KEPT iff !EXCEEDS(self) && EXCEEDS(parent); scale == 0 (+-0) keeps every cluster. The branches on the view are wave-uniform.
__device__ __forceinline__ bool lod_kept(const LodLane& l, const ClusterLodView& view)
{
    if (view.scale == 0.0f)
        return true;
    const bool point = view.eye[3] != 0.0f;
    return !lod_exceeds(l.self_c, l.self_r, l.self_e, l.s2, view.eye, point, view.scale, view.near_distance) &&
           lod_exceeds(l.parent_c, l.parent_r, l.parent_e, l.s2, view.eye, point, view.scale, view.near_distance);
}

// draw k of view v: the first instance the emission gave it, and how many (c_k)
__device__ __forceinline__ uint32_t first_of_draw(const ClusterLaunch& a, uint32_t v, uint32_t k)
{
    return a.first_instance_of ? a.first_instance_of[a.draw_starts[v] + k] : a.starts[v] + k;
}
__device__ __forceinline__ uint32_t instances_of_draw(const ClusterLaunch& a, uint32_t v, uint32_t k, uint32_t n, uint32_t from)
{
    const uint32_t next = k + 1u < n ? first_of_draw(a, v, k + 1u) : a.starts[v + 1];
    return next - from;
}
// what the walks need of view v when v differs from lane to lane: selected, not indexed (an argument array indexed by a lane's
// value would be copied to scratch)
struct ViewPick {
    const float* model;
    const uint32_t* count;
    uint32_t first_block;
};
__device__ __forceinline__ ViewPick pick_view(const ClusterLaunch& a, uint32_t v)
{
    ViewPick p{a.view[0].model, a.view[0].count, a.first_block[0]};
#pragma unroll
    for (uint32_t u = 1; u < kMaxInstanceViews; u++)
        if (v == u)
            p = ViewPick{a.view[u].model, a.view[u].count, a.first_block[u]};
    return p;
}
__device__ __forceinline__ ClusterRange range_of(const ClusterLaunch& a, uint32_t g)
{
    return g < a.range_count ? a.ranges[g] : ClusterRange{0u, 0u};
}

__global__ __launch_bounds__(kClusterBlock) void cluster_count_kernel(const ClusterLaunch a)
{
    __shared__ uint32_t wave_sum[2][kClusterBlock / 64u];
    if (blockIdx.x >= a.first_block[a.views])
        return;  // (a call whose views hold no slot launches one workgroup)
    const uint32_t v = view_of_block(a.first_block, a.views, blockIdx.x);
    const ClusterView& vw = a.view[v];
    const uint32_t n = *vw.count;
    const uint32_t first = (blockIdx.x - a.first_block[v]) * kClusterBlock;
    if (first >= n) {  // (the whole workgroup, after ONE load) nothing here: the prefix skips it, nobody reads its draws
        if (threadIdx.x == 0) {
            a.block_total[blockIdx.x] = 0;
            a.block_tested[blockIdx.x] = 0;
        }
        return;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t k = first + threadIdx.x;
    uint32_t g = kClusterNone, candidates = 0, tested = 0;
    if (k < n) {
        uint32_t id;
        if (a.draw_ids) {  // the selected ids, draw-indexed (wave-uniform choice)
            uint32_t at = 0;
            for (uint32_t u = 0; u < v; u++)
                at += *a.view[u].count;
            id = stream_load(a.draw_ids + at + k);
        } else {
            const uint32_t slot = stream_load(vw.idx + k);
            id = a.ids ? a.ids[slot] : 0u;
        }
        const uint32_t from = first_of_draw(a, v, k);
        if (id < a.table_count && instances_of_draw(a, v, k, n, from) != 0u) {
            g = id;
            tested = range_of(a, id).count;
            candidates = tested ? tested : 1u;
        }
    }
    // workgroup-local exclusive prefix: a draw beyond the count has no candidate, so its prefix is the total and no search ends on it
    const uint32_t upto = wave_inclusive_scan(candidates, lane);
    uint32_t t = tested;
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1)
        t += __shfl_xor(t, d, 64);
    if (lane == 63u)
        wave_sum[0][wave] = upto;
    if (lane == 0u)
        wave_sum[1][wave] = t;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t w = 0; w < kClusterBlock / 64u; w++)
        before += w < wave ? wave_sum[0][w] : 0u;
    const size_t at = (size_t)blockIdx.x * kClusterBlock + threadIdx.x;
    a.draw_geometry[at] = g;
    a.draw_local[at] = before + upto - candidates;
    if (threadIdx.x == 0) {
        a.block_total[blockIdx.x] = wave_sum[0][0] + wave_sum[0][1] + wave_sum[0][2] + wave_sum[0][3];
        a.block_tested[blockIdx.x] = wave_sum[1][0] + wave_sum[1][1] + wave_sum[1][2] + wave_sum[1][3];
    }
}

// t[0, n) becomes its own exclusive prefix, by the whole workgroup of kClusterScanBlock lanes; every lane gets the sum
__device__ __forceinline__ uint32_t scan_table(uint32_t* t, uint32_t n, uint32_t* wave_part, uint32_t* turn_sum)
{
    constexpr uint32_t kWaves = kClusterScanBlock / 64u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += kClusterScanBlock * 4u) {
        const uint32_t at = base + threadIdx.x * 4u;
        uint32_t x[4] = {0u, 0u, 0u, 0u};
        if (at + 4u <= n) {  // (the table is 16-byte aligned and `at` a multiple of four)
            const uint4 q = *reinterpret_cast<const uint4*>(t + at);
            x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
        } else {
            for (uint32_t e = 0; e < 4u; e++)
                x[e] = at + e < n ? t[at + e] : 0u;
        }
        const uint32_t own = x[0] + x[1] + x[2] + x[3];
        const uint32_t upto = wave_inclusive_scan(own, lane);
        __syncthreads();  // (the parts may still be read from the turn before)
        if (lane == 63u)
            wave_part[wave] = upto;
        __syncthreads();
        if (wave == 0) {
            const uint32_t part = lane < kWaves ? wave_part[lane] : 0u, scanned = wave_inclusive_scan(part, lane);
            if (lane < kWaves)
                wave_part[lane] = scanned - part;
            if (lane == kWaves - 1u)
                *turn_sum = scanned;
        }
        __syncthreads();
        uint32_t run = carry + wave_part[wave] + upto - own;
        if (at + 4u <= n) {
            uint4 q;
            q.x = run, q.y = run + x[0], q.z = run + x[0] + x[1], q.w = run + x[0] + x[1] + x[2];
            *reinterpret_cast<uint4*>(t + at) = q;
        } else {
            for (uint32_t e = 0; e < 4u; e++) {
                if (at + e < n)
                    t[at + e] = run;
                run += x[e];
            }
        }
        carry += *turn_sum;
    }
    __syncthreads();
    return carry;
}

// survivors in front of candidate c (c <= T): the prefix of its tile and the ballot bits below it; `all` for c == T
__device__ __forceinline__ uint32_t survivors_before(const ClusterLaunch& a, uint32_t c, uint32_t total, uint32_t all)
{
    if (c >= total)
        return all;
    const uint32_t tile = c / kClusterTile, in = c % kClusterTile;
    uint32_t s = a.tile_count[tile];  // (scanned: the survivors in front of the tile)
    for (uint32_t w = 0; w < in / 64u; w++)
        s += (uint32_t)__popcll(a.survive[(size_t)tile * 4u + w]);
    if (in % 64u)
        s += (uint32_t)__popcll(a.survive[(size_t)tile * 4u + in / 64u] & ((1ull << (in % 64u)) - 1ull));
    return s;
}

template <uint32_t kStage>
__global__ __launch_bounds__(kClusterScanBlock) void cluster_scan_kernel(const ClusterLaunch a)
{
    __shared__ uint32_t wave_part[kClusterScanBlock / 64u];
    __shared__ uint32_t turn_sum;
    __shared__ uint32_t view_sum[kMaxInstanceViews][kClusterScanBlock / 64u];
    const uint32_t blocks = a.first_block[a.views];
    if constexpr (kStage == 0) {
        // clusters tested per view, in front of the scan (sums of another table: no order to keep)
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        for (uint32_t v = 0; v < a.views; v++) {
            uint32_t x = 0;
            for (uint32_t b = a.first_block[v] + threadIdx.x; b < a.first_block[v + 1]; b += kClusterScanBlock)
                x += a.block_tested[b];
#pragma unroll
            for (uint32_t d = 32; d >= 1u; d >>= 1)
                x += __shfl_xor(x, d, 64);
            if (lane == 0u)
                view_sum[v][wave] = x;
        }
        __syncthreads();
        if (threadIdx.x < a.views) {
            uint32_t x = 0;
            for (uint32_t w = 0; w < kClusterScanBlock / 64u; w++)
                x += view_sum[threadIdx.x][w];
            a.counts[a.views + threadIdx.x] = x;
        }
        const uint32_t total = scan_table(a.block_total, blocks, wave_part, &turn_sum);
        if (threadIdx.x == 0)
            a.totals[kClusterTotalCandidates] = total;
        if (threadIdx.x == 0)  // (the scan's stores are visible to the workgroup behind scan_table's last barrier)
            for (uint32_t v = 0; v <= a.views; v++)
                a.totals[kClusterCandidateStart + v] = a.first_block[v] < blocks ? a.block_total[a.first_block[v]] : total;
        // where the search of a tile's candidates begins: every tile's first candidate lies in exactly one workgroup that has
        // candidates, and that workgroup writes the tile's entry
        for (uint32_t b = threadIdx.x; b < blocks; b += kClusterScanBlock) {
            const uint32_t from = a.block_total[b], end = b + 1u < blocks ? a.block_total[b + 1u] : total;
            if (end == from)
                continue;
            const uint32_t last = (end - 1u) / kClusterTile;
            for (uint32_t t = from / kClusterTile + (from % kClusterTile ? 1u : 0u); t <= last; t++)
                a.tile_block[t] = b;
        }
    } else {
        const uint32_t total = a.totals[kClusterTotalCandidates];
        const uint32_t tiles = total / kClusterTile + (total % kClusterTile ? 1u : 0u);
        const uint32_t all = scan_table(a.tile_count, tiles, wave_part, &turn_sum);
        if (threadIdx.x <= a.views)
            view_sum[0][threadIdx.x] = survivors_before(a, a.totals[kClusterCandidateStart + threadIdx.x], total, all);
        __syncthreads();
        if (threadIdx.x <= a.views)
            a.totals[kClusterSurvivorStart + threadIdx.x] = view_sum[0][threadIdx.x];
        if (threadIdx.x < a.views)
            a.counts[threadIdx.x] = view_sum[0][threadIdx.x + 1u] - view_sum[0][threadIdx.x];
    }
}

// candidate c < T -> the count workgroup of its draw, the draw's place in the scratch and the candidate's number inside the draw
// (of tile `tile` of `tiles`, `blocks` count workgroups: the workgroup lies between the one of the tile's first candidate and the
// one of the next tile's — mostly the same one, so the first search is a step or none)
__device__ __forceinline__ void locate(const ClusterLaunch& a, uint32_t c, uint32_t tile, uint32_t tiles, uint32_t blocks, uint32_t& block,
                                       uint32_t& at, uint32_t& j)
{
    uint32_t lo = a.tile_block[tile], hi = (tile + 1u < tiles ? a.tile_block[tile + 1u] : blocks - 1u) + 1u;
    while (hi - lo > 1u) {  // the largest workgroup in [lo, hi) whose prefix is <= c (lo's is: it holds the tile's first candidate)
        const uint32_t mid = (lo + hi) >> 1;
        if (a.block_total[mid] <= c)
            lo = mid;
        else
            hi = mid;
    }
    block = lo;
    const uint32_t rest = c - a.block_total[lo];
    const uint32_t* const local = a.draw_local + (size_t)lo * kClusterBlock;
    lo = 0, hi = kClusterBlock;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (local[mid] <= rest)
            lo = mid;
        else
            hi = mid;
    }
    at = block * kClusterBlock + lo;
    j = rest - local[lo];
}

// The walk of cluster_test_kernel. kRuns (cluster_run_test_kernel): it also ballots the LINK bit of every candidate into `link` —
// cluster j of a draw follows cluster j - 1 in the index buffer, j is no multiple of kClusterRunSpan and the cluster's own interval
// does not wrap (include/garden_vis.h). A lane holds its cluster's first and count in the .w of its two loads; the predecessor's
// are in the lane below (lane > 0 and j > 0: candidate c - 1 is cluster j - 1 of the same draw), lane 0 loads them itself.
// kCones (cluster_cone_test_kernel, cluster_cone_run_test_kernel): a cluster survives iff it passes the test above and is not
// cone-rejected. The cone's two 16-byte loads are issued with the cluster's two — one more step in the chain of dependent loads is
// what would cost — and the cone test runs behind the plane tests, in front of the Hi-Z query.
// kLod (cluster_lod_*_test_kernel): a cluster survives iff it is LOD-kept and passes the tests above. The entry's three 16-byte loads
// are issued with the cluster's two and the model's three; the LOD test runs in front of the plane tests, a LOD-rejected lane does
// neither them, nor the cone test, nor the Hi-Z query, and a wave with no LOD-kept lane for a view skips them wholesale.
template <bool kRuns, bool kCones, bool kLod>
__device__ __forceinline__ void cluster_test_tiles(const ClusterLaunch& a, unsigned long long* link, const float4* cones, uint32_t eye_offset,
                                                   const float4* lods, uint32_t lod_offset)
{
    __shared__ uint32_t wave_count[kClusterBlock / 64u];
    ConstClusterArgs base = (ConstClusterArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(base));  // (opaque: nothing read through it is moved out of the loops)
    const uint32_t total = a.totals[kClusterTotalCandidates];
    const uint32_t tiles = total / kClusterTile + (total % kClusterTile ? 1u : 0u);
    const uint32_t blocks = a.first_block[a.views];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t c = tile * kClusterTile + threadIdx.x;
        const bool live = c < total;
        bool survives = live;  // a whole draw survives untested
        bool tested = false;
        uint32_t v = 0;
        Corners corners;
        uint32_t j = 0, cl_first = 0, cl_count = 0;
        const float4* cl = nullptr;
        [[maybe_unused]] ConeLane cone{};
        [[maybe_unused]] LodLane lod{};
        if (live) {
            uint32_t block, at;
            locate(a, c, tile, tiles, blocks, block, at, j);
            v = view_of_block(a.first_block, a.views, block);
            const ClusterRange range = range_of(a, a.draw_geometry[at]);
            if (range.count) {
                tested = true;
                cl = a.clusters + ((size_t)range.first + j) * 2u;
                const float4 lo = cl[0], hi = cl[1];  // (plain loads: every draw of the geometry reads the cluster again)
                [[maybe_unused]] float4 c0, c1;
                if constexpr (kCones) {
                    const float4* const cn = cones + ((size_t)range.first + j) * 2u;  // (the cone table is as long as the cluster table)
                    c0 = cn[0], c1 = cn[1];
                }
                [[maybe_unused]] float4 l0, l1, l2;
                if constexpr (kLod) {
                    const float4* const ln = lods + ((size_t)range.first + j) * 3u;  // (the LOD table is as long as the cluster table)
                    l0 = ln[0], l1 = ln[1], l2 = ln[2];
                }
                cl_first = __float_as_uint(lo.w), cl_count = __float_as_uint(hi.w);
                const ViewPick view = pick_view(a, v);
                const uint32_t k = at - view.first_block * kClusterBlock;
                const float4* const rows = reinterpret_cast<const float4*>(view.model) + (size_t)k * 3u;
                const float4 w0 = rows[0], w1 = rows[1], w2 = rows[2];  // (... and the draw's other clusters its model)
                aabb_corners(rows_model(w0, w1, w2), lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, corners);
                if constexpr (kCones)
                    cone = cone_lane(rows_model(w0, w1, w2), c0, c1);
                if constexpr (kLod)
                    lod = lod_lane(rows_model(w0, w1, w2), l0, l1, l2);
            }
        }
#pragma unroll 1
        for (uint32_t u = 0; u < a.views; u++) {
            bool mine = tested && v == u;
            if (!__any(mine))
                continue;  // (wave-uniform)
            if constexpr (kLod) {
                const ClusterLodView lv = view_lod_of(base, lod_offset, u);
                const bool kept = mine && lod_kept(lod, lv);
                if (mine && !kept)
                    survives = false;
                mine = kept;
                if (!__any(mine))
                    continue;  // (wave-uniform: no LOD-kept lane, no plane test, no cone test, no query)
            }
            const ClusterPlanes pl = view_planes_of(base, u);
            const uint32_t plane_count = base->plane_count[u];
            const bool query = (a.hiz_views >> u) & 1u;
            [[maybe_unused]] ClusterEye eye;
            if constexpr (kCones)
                eye = view_eye_of(base, eye_offset, u);
            if (mine) {
                bool visible = !behind_frustum(corners, pl.planes, plane_count);
                if constexpr (kCones)
                    visible = visible && !cone_rejected(cone, eye);
                if (query && visible) {
                    const HizDevice hz = view_hiz_of(base, u);
                    const ClusterMatrix vm = view_matrix_of(base, u);
                    visible = !hiz_occluded(hz, vm.m, corners);
                }
                survives = visible;
            }
        }
        const unsigned long long word = __ballot(survives);
        if constexpr (kRuns) {
            // (whole draws and dead lanes: not tested, no link. The survivors are counted as heads by the launch behind.)
            const uint32_t below_first = (uint32_t)__shfl_up((int)cl_first, 1, 64), below_count = (uint32_t)__shfl_up((int)cl_count, 1, 64);
            bool linked = false;
            if (tested && j != 0u && j % kClusterRunSpan != 0u) {
                uint32_t before_first = below_first, before_count = below_count;
                if (lane == 0u)
                    before_first = __float_as_uint(cl[-2].w), before_count = __float_as_uint(cl[-1].w);  // (j > 0: inside the range)
                linked = (uint64_t)before_first + before_count == cl_first && (uint64_t)cl_first + cl_count <= 0xFFFFFFFFull;
            }
            const unsigned long long links = __ballot(linked);
            if (lane == 0u) {
                a.survive[(size_t)tile * 4u + wave] = word;
                link[(size_t)tile * 4u + wave] = links;
            }
        } else {
            if (lane == 0u) {
                a.survive[(size_t)tile * 4u + wave] = word;
                wave_count[wave] = (uint32_t)__popcll(word);
            }
            __syncthreads();
            if (threadIdx.x == 0)
                a.tile_count[tile] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
            __syncthreads();  // (the next tile rewrites the wave counts)
        }
    }
}

__global__ __launch_bounds__(kClusterBlock) void cluster_test_kernel(const ClusterLaunch a)
{
    cluster_test_tiles<false, false, false>(a, nullptr, nullptr, 0u, nullptr, 0u);
}

// every word of one command position; a field offset of kNoField matches no word
__device__ __forceinline__ void put_command(const ClusterLaunch& a, uint32_t position, uint32_t count, uint32_t instances, uint32_t first,
                                            uint32_t first_instance, uint32_t vertex_offset, uint32_t draw)
{
    uint32_t* const to = reinterpret_cast<uint32_t*>(a.dst + (size_t)position * a.stride);
    for (uint32_t w = 0; w < a.stride / 4u; w++) {
        const uint32_t byte = w * 4u;
        uint32_t x = 0u;
        x = byte == a.count ? count : x;
        x = byte == a.instance_count ? instances : x;
        x = byte == a.first ? first : x;
        x = byte == a.first_instance ? first_instance : x;
        x = byte == a.vertex_offset ? vertex_offset : x;
        x = byte == a.draw ? draw : x;
        to[w] = x;
    }
}

__global__ __launch_bounds__(kClusterBlock) void cluster_write_kernel(const ClusterLaunch a)
{
    const uint32_t total = a.totals[kClusterTotalCandidates];
    const uint32_t tiles = total / kClusterTile + (total % kClusterTile ? 1u : 0u);
    const uint32_t blocks = a.first_block[a.views];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const unsigned long long* const words = a.survive + (size_t)tile * 4u;
        const unsigned long long word = words[wave];
        if (!((word >> lane) & 1ull))
            continue;
        uint32_t rank = a.tile_count[tile] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));  // (scanned: survivors in front of the tile)
        for (uint32_t w = 0; w < wave; w++)
            rank += (uint32_t)__popcll(words[w]);
        const uint32_t c = tile * kClusterTile + threadIdx.x;
        uint32_t block, at, j;
        locate(a, c, tile, tiles, blocks, block, at, j);
        const uint32_t v = view_of_block(a.first_block, a.views, block);
        uint32_t position = rank;  // packed: the views' commands back to back are the survivors in order
        if (a.region) {
            const uint32_t in_view = rank - a.totals[kClusterSurvivorStart + v];
            if (in_view >= a.region)
                continue;
            position = v * a.region + in_view;
        }
        if (position >= a.capacity)
            continue;
        const ViewPick view = pick_view(a, v);
        const uint32_t k = at - view.first_block * kClusterBlock;
        const uint32_t g = a.draw_geometry[at];  // (below table_count: the draw has candidates)
        const CommandGeometry geometry = a.table[g];
        const ClusterRange range = range_of(a, g);
        uint32_t count = geometry.count, first = geometry.first;
        if (range.count) {
            const float4* const cl = a.clusters + ((size_t)range.first + j) * 2u;
            first += __float_as_uint(cl[0].w);
            count = __float_as_uint(cl[1].w);
        }
        const uint32_t from = first_of_draw(a, v, k);
        put_command(a, position, count, instances_of_draw(a, v, k, *view.count, from), first, from, (uint32_t)geometry.vertex_offset, k);
    }
    if (a.region) {  // the all-zero padding positions C_v <= j < R of every view
        const uint64_t positions = (uint64_t)a.views * a.region;
        for (uint64_t p = (uint64_t)blockIdx.x * kClusterBlock + threadIdx.x; p < positions && p < a.capacity; p += (uint64_t)gridDim.x * kClusterBlock) {
            const uint32_t v = (uint32_t)(p / a.region), in_view = (uint32_t)(p % a.region);
            if (in_view < a.counts[v])
                continue;
            uint32_t* const to = reinterpret_cast<uint32_t*>(a.dst + (size_t)p * a.stride);
            for (uint32_t w = 0; w < a.stride / 4u; w++)
                to[w] = 0u;
        }
    }
}

// ---- the second phase (gv_pool_cull_clusters_second_phase) ----
// A candidate of K1 is PENDING iff K1 tested it, did not keep it and queried a pyramid for its view. Whole draws are kept untested,
// so the pending candidates are the clear bits of K1's ballot words inside the candidate ranges of the queried views: no search is
// needed to know them. The five launches mirror K1's, one level up — a PENDING TILE is kClusterTile pending candidates in order:
//
//   cluster_second_count_kernel   one lane per CANDIDATE tile, grid-stride: the popcount of its four pending words.
//   cluster_second_scan_kernel    <0>: those counts become their own exclusive prefix; P, the pending in front of every view and with
//                                 them counts[m + v]; per pending tile the candidate tile that holds its first pending (as
//                                 tile_block). <1>: the pending tiles' survivor counts likewise, and counts[v].
//   cluster_second_test_kernel    one lane per PENDING candidate (dense: where phase 1 kept 99 % a walk over its candidates would
//                                 run the Hi-Z query with a lane or two per wave). Pending p -> its candidate tile, searched between
//                                 two entries of that table; the (p - prefix)-th set bit of the tile's pending words is c; then K1's
//                                 locate and K1's test, unchanged, against the pyramids in this launch's arguments.
//   cluster_second_write_kernel   the same walk; a survivor's rank is its position; the padding with regions.
//
// Nothing K1 wrote is written; no workgroup waits for another, no atomics, integer ranks only.
static_assert(offsetof(ClusterSecondLaunch, k) == 0, "the per-view arguments are read at K1's offsets");

// the pending bits of ballot word w of candidate tile `tile` (tile below the number of tiles of T)
__device__ __forceinline__ unsigned long long pending_word(const ClusterLaunch& a, uint32_t tile, uint32_t w)
{
    const uint64_t c0 = (uint64_t)tile * kClusterTile + w * 64u;
    unsigned long long in = 0ull;  // the word's candidates that lie in a queried view (whose end is at most T)
    for (uint32_t v = 0; v < a.views; v++) {
        if (!((a.hiz_views >> v) & 1u))
            continue;
        const uint64_t first = a.totals[kClusterCandidateStart + v], end = a.totals[kClusterCandidateStart + v + 1u];
        const uint64_t from = first > c0 ? first : c0, to = end < c0 + 64u ? end : c0 + 64u;
        if (from >= to)
            continue;
        const unsigned long long below_to = to - c0 == 64u ? ~0ull : (1ull << (to - c0)) - 1ull;
        in |= below_to & ~((1ull << (from - c0)) - 1ull);
    }
    return in ? ~a.survive[(size_t)tile * 4u + w] & in : 0ull;
}

__global__ __launch_bounds__(kClusterBlock) void cluster_second_count_kernel(const ClusterSecondLaunch s)
{
    const ClusterLaunch& a = s.k;
    const uint32_t total = a.totals[kClusterTotalCandidates];
    const uint32_t tiles = total / kClusterTile + (total % kClusterTile ? 1u : 0u);
    for (uint64_t tile = (uint64_t)blockIdx.x * kClusterBlock + threadIdx.x; tile < tiles; tile += (uint64_t)gridDim.x * kClusterBlock) {
        uint32_t n = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++)
            n += (uint32_t)__popcll(pending_word(a, (uint32_t)tile, w));
        s.pending_count[tile] = n;
    }
}

// pending in front of candidate c (c <= T): the prefix of its tile and the pending bits below it; `all` for c == T
__device__ __forceinline__ uint32_t pending_before(const ClusterSecondLaunch& s, uint32_t c, uint32_t total, uint32_t all)
{
    if (c >= total)
        return all;
    const uint32_t tile = c / kClusterTile, in = c % kClusterTile;
    uint32_t n = s.pending_count[tile];  // (scanned: the pending in front of the tile)
    for (uint32_t w = 0; w < in / 64u; w++)
        n += (uint32_t)__popcll(pending_word(s.k, tile, w));
    if (in % 64u)
        n += (uint32_t)__popcll(pending_word(s.k, tile, in / 64u) & ((1ull << (in % 64u)) - 1ull));
    return n;
}
// second-phase survivors in front of pending p (p <= P), likewise
__device__ __forceinline__ uint32_t kept_before(const ClusterSecondLaunch& s, uint32_t p, uint32_t pending, uint32_t all)
{
    if (p >= pending)
        return all;
    const uint32_t q = p / kClusterTile, in = p % kClusterTile;
    uint32_t n = s.kept_count[q];
    for (uint32_t w = 0; w < in / 64u; w++)
        n += (uint32_t)__popcll(s.kept[(size_t)q * 4u + w]);
    if (in % 64u)
        n += (uint32_t)__popcll(s.kept[(size_t)q * 4u + in / 64u] & ((1ull << (in % 64u)) - 1ull));
    return n;
}

template <uint32_t kStage>
__global__ __launch_bounds__(kClusterScanBlock) void cluster_second_scan_kernel(const ClusterSecondLaunch s)
{
    __shared__ uint32_t wave_part[kClusterScanBlock / 64u];
    __shared__ uint32_t turn_sum;
    __shared__ uint32_t view_start[kMaxInstanceViews + 1];
    const ClusterLaunch& a = s.k;
    if constexpr (kStage == 0) {
        const uint32_t total = a.totals[kClusterTotalCandidates];
        const uint32_t tiles = total / kClusterTile + (total % kClusterTile ? 1u : 0u);
        const uint32_t pending = scan_table(s.pending_count, tiles, wave_part, &turn_sum);
        if (threadIdx.x == 0)
            s.totals[kSecondTotalPending] = pending;
        if (threadIdx.x <= a.views)
            view_start[threadIdx.x] = pending_before(s, a.totals[kClusterCandidateStart + threadIdx.x], total, pending);
        __syncthreads();
        if (threadIdx.x <= a.views)
            s.totals[kSecondPendingStart + threadIdx.x] = view_start[threadIdx.x];
        if (threadIdx.x < a.views)
            a.counts[a.views + threadIdx.x] = view_start[threadIdx.x + 1u] - view_start[threadIdx.x];
        // where the search of a pending tile's candidates begins: every pending tile's first pending lies in exactly one candidate
        // tile that has pending, and that tile writes the entry
        for (uint32_t t = threadIdx.x; t < tiles; t += kClusterScanBlock) {
            const uint32_t from = s.pending_count[t], end = t + 1u < tiles ? s.pending_count[t + 1u] : pending;
            if (end == from)
                continue;
            const uint32_t last = (end - 1u) / kClusterTile;
            for (uint32_t q = from / kClusterTile + (from % kClusterTile ? 1u : 0u); q <= last; q++)
                s.pending_tile[q] = t;
        }
    } else {
        const uint32_t pending = s.totals[kSecondTotalPending];
        const uint32_t ptiles = pending / kClusterTile + (pending % kClusterTile ? 1u : 0u);
        const uint32_t all = scan_table(s.kept_count, ptiles, wave_part, &turn_sum);
        if (threadIdx.x <= a.views)
            view_start[threadIdx.x] = kept_before(s, s.totals[kSecondPendingStart + threadIdx.x], pending, all);
        __syncthreads();
        if (threadIdx.x <= a.views)
            s.totals[kSecondSurvivorStart + threadIdx.x] = view_start[threadIdx.x];
        if (threadIdx.x < a.views)
            a.counts[threadIdx.x] = view_start[threadIdx.x + 1u] - view_start[threadIdx.x];
    }
}

// pending p < P of pending tile q -> its candidate tile and the candidate c: the largest candidate tile whose prefix is <= p,
// searched between the tile of q's first pending and that of the next pending tile's; then the (p - prefix)-th set bit of its words
__device__ __forceinline__ void find_pending(const ClusterSecondLaunch& s, uint32_t p, uint32_t q, uint32_t ptiles, uint32_t tiles, uint32_t& tile,
                                             uint32_t& c)
{
    uint32_t lo = s.pending_tile[q], hi = (q + 1u < ptiles ? s.pending_tile[q + 1u] : tiles - 1u) + 1u;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s.pending_count[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    tile = lo;
    uint32_t rest = p - s.pending_count[lo];  // (below the tile's pending count: the next tile's prefix is above p)
    uint32_t in = 0;
    bool found = false;
#pragma unroll
    for (uint32_t w = 0; w < 4u; w++) {
        const unsigned long long word = pending_word(s.k, lo, w);
        const uint32_t n = (uint32_t)__popcll(word);
        if (!found && rest < n) {
            uint32_t at = 0;  // the rest-th set bit: halve the word six times
#pragma unroll
            for (uint32_t width = 32; width >= 1u; width >>= 1) {
                const uint32_t below = (uint32_t)__popcll((word >> at) & ((1ull << width) - 1ull));
                if (rest >= below) {
                    rest -= below;
                    at += width;
                }
            }
            in = w * 64u + at;
            found = true;
        }
        rest -= found ? 0u : n;
    }
    c = lo * kClusterTile + in;
}

// kCones (cluster_cone_second_test_kernel): behind a cone result a pending cluster survives iff the unchanged test keeps it and it is
// not cone-rejected, with the eyes and the cone table of K1 (as cluster_test_tiles).
// kLod (cluster_lod_second_test_kernel, cluster_lod_cone_second_test_kernel): the LOD cut of K1's views in front, likewise.
template <bool kCones, bool kLod>
__device__ __forceinline__ void cluster_second_test_tiles(const ClusterSecondLaunch& s, const float4* cones, uint32_t eye_offset, const float4* lods,
                                                          uint32_t lod_offset)
{
    __shared__ uint32_t wave_count[kClusterBlock / 64u];
    const ClusterLaunch& a = s.k;
    ConstClusterArgs base = (ConstClusterArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(base));  // (opaque: nothing read through it is moved out of the loops)
    const uint32_t total = a.totals[kClusterTotalCandidates];
    const uint32_t tiles = total / kClusterTile + (total % kClusterTile ? 1u : 0u);
    const uint32_t pending = s.totals[kSecondTotalPending];
    const uint32_t ptiles = pending / kClusterTile + (pending % kClusterTile ? 1u : 0u);
    const uint32_t blocks = a.first_block[a.views];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t q = blockIdx.x; q < ptiles; q += gridDim.x) {
        const uint32_t p = q * kClusterTile + threadIdx.x;
        bool tested = false, survives = false;
        uint32_t v = 0;
        Corners corners;
        [[maybe_unused]] ConeLane cone{};
        [[maybe_unused]] LodLane lod{};
        if (p < pending) {
            uint32_t tile, c, block, at, j;
            find_pending(s, p, q, ptiles, tiles, tile, c);
            locate(a, c, tile, tiles, blocks, block, at, j);
            v = view_of_block(a.first_block, a.views, block);
            const ClusterRange range = range_of(a, a.draw_geometry[at]);
            if (range.count) {  // (a pending candidate is a cluster: K1 tested it)
                tested = true;
                const float4* const cl = a.clusters + ((size_t)range.first + j) * 2u;
                const float4 lo = cl[0], hi = cl[1];
                [[maybe_unused]] float4 c0, c1;
                if constexpr (kCones) {
                    const float4* const cn = cones + ((size_t)range.first + j) * 2u;
                    c0 = cn[0], c1 = cn[1];
                }
                [[maybe_unused]] float4 l0, l1, l2;
                if constexpr (kLod) {
                    const float4* const ln = lods + ((size_t)range.first + j) * 3u;  // (the LOD table is as long as the cluster table)
                    l0 = ln[0], l1 = ln[1], l2 = ln[2];
                }
                const ViewPick view = pick_view(a, v);
                const uint32_t k = at - view.first_block * kClusterBlock;
                const float4* const rows = reinterpret_cast<const float4*>(view.model) + (size_t)k * 3u;
                const float4 w0 = rows[0], w1 = rows[1], w2 = rows[2];
                aabb_corners(rows_model(w0, w1, w2), lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, corners);
                if constexpr (kCones)
                    cone = cone_lane(rows_model(w0, w1, w2), c0, c1);
                if constexpr (kLod)
                    lod = lod_lane(rows_model(w0, w1, w2), l0, l1, l2);
            }
        }
#pragma unroll 1
        for (uint32_t u = 0; u < a.views; u++) {
            bool mine = tested && v == u;
            if (!__any(mine))
                continue;  // (wave-uniform)
            if constexpr (kLod) {
                const ClusterLodView lv = view_lod_of(base, lod_offset, u);
                const bool kept = mine && lod_kept(lod, lv);
                if (mine && !kept)
                    survives = false;
                mine = kept;
                if (!__any(mine))
                    continue;  // (wave-uniform: no LOD-kept lane, no plane test, no cone test, no query)
            }
            const ClusterPlanes pl = view_planes_of(base, u);
            const uint32_t plane_count = base->plane_count[u];
            const bool query = (a.hiz_views >> u) & 1u;  // (set: only a queried view has pending candidates)
            [[maybe_unused]] ClusterEye eye;
            if constexpr (kCones)
                eye = view_eye_of(base, eye_offset, u);
            if (mine) {
                bool visible = !behind_frustum(corners, pl.planes, plane_count);
                if constexpr (kCones)
                    visible = visible && !cone_rejected(cone, eye);
                if (query && visible) {
                    const HizDevice hz = view_hiz_of(base, u);
                    const ClusterMatrix vm = view_matrix_of(base, u);
                    visible = !hiz_occluded(hz, vm.m, corners);
                }
                survives = visible;
            }
        }
        const unsigned long long word = __ballot(survives);
        if (lane == 0u) {
            s.kept[(size_t)q * 4u + wave] = word;
            wave_count[wave] = (uint32_t)__popcll(word);
        }
        __syncthreads();
        if (threadIdx.x == 0)
            s.kept_count[q] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
        __syncthreads();  // (the next pending tile rewrites the wave counts)
    }
}

__global__ __launch_bounds__(kClusterBlock) void cluster_second_test_kernel(const ClusterSecondLaunch s)
{
    cluster_second_test_tiles<false, false>(s, nullptr, 0u, nullptr, 0u);
}

__global__ __launch_bounds__(kClusterBlock) void cluster_second_write_kernel(const ClusterSecondLaunch s)
{
    const ClusterLaunch& a = s.k;
    const uint32_t total = a.totals[kClusterTotalCandidates];
    const uint32_t tiles = total / kClusterTile + (total % kClusterTile ? 1u : 0u);
    const uint32_t pending = s.totals[kSecondTotalPending];
    const uint32_t ptiles = pending / kClusterTile + (pending % kClusterTile ? 1u : 0u);
    const uint32_t blocks = a.first_block[a.views];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t q = blockIdx.x; q < ptiles; q += gridDim.x) {
        const unsigned long long* const words = s.kept + (size_t)q * 4u;
        const unsigned long long word = words[wave];
        if (!((word >> lane) & 1ull))
            continue;
        uint32_t rank = s.kept_count[q] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));  // (scanned: survivors in front of the pending tile)
        for (uint32_t w = 0; w < wave; w++)
            rank += (uint32_t)__popcll(words[w]);
        uint32_t tile, c, block, at, j;
        find_pending(s, q * kClusterTile + threadIdx.x, q, ptiles, tiles, tile, c);
        locate(a, c, tile, tiles, blocks, block, at, j);
        const uint32_t v = view_of_block(a.first_block, a.views, block);
        uint32_t position = rank;
        if (a.region) {
            const uint32_t in_view = rank - s.totals[kSecondSurvivorStart + v];
            if (in_view >= a.region)
                continue;
            position = v * a.region + in_view;
        }
        if (position >= a.capacity)
            continue;
        const ViewPick view = pick_view(a, v);
        const uint32_t k = at - view.first_block * kClusterBlock;
        const uint32_t g = a.draw_geometry[at];  // (the id K1 kept; below table_count and ranged: the draw had a tested cluster)
        const CommandGeometry geometry = a.table[g];
        const ClusterRange range = range_of(a, g);
        const float4* const cl = a.clusters + ((size_t)range.first + j) * 2u;
        const uint32_t from = first_of_draw(a, v, k);
        put_command(a, position, __float_as_uint(cl[1].w), instances_of_draw(a, v, k, *view.count, from), geometry.first + __float_as_uint(cl[0].w), from,
                    (uint32_t)geometry.vertex_offset, k);
    }
    if (a.region) {  // the all-zero padding positions C_v <= j < R of every view
        const uint64_t positions = (uint64_t)a.views * a.region;
        for (uint64_t p = (uint64_t)blockIdx.x * kClusterBlock + threadIdx.x; p < positions && p < a.capacity; p += (uint64_t)gridDim.x * kClusterBlock) {
            const uint32_t v = (uint32_t)(p / a.region), in_view = (uint32_t)(p % a.region);
            if (in_view < a.counts[v])
                continue;
            uint32_t* const to = reinterpret_cast<uint32_t*>(a.dst + (size_t)p * a.stride);
            for (uint32_t w = 0; w < a.stride / 4u; w++)
                to[w] = 0u;
        }
    }
}

// ---- the run form (gv_pool_cull_cluster_runs) ----
// The plain form's decisions, one command per RUN of adjacent surviving clusters. Six launches: cluster_count_kernel and
// cluster_scan_kernel<0> as they are, then
//
//   cluster_run_test_kernel    cluster_test_kernel's walk, which also ballots the LINK bit of every candidate (above). It leaves
//                              the survive words exactly as the plain form does, and no survivor counts.
//   cluster_run_heads_kernel   dense, one lane per TILE (four survive and four link words, 64 bytes read, 36 written): a survivor
//                              is a HEAD iff it is not linked or its predecessor did not survive, head = s & ~(l & (s << 1 | the top
//                              bit of the word before)). The head words and the tile's head count.
//   cluster_scan_kernel<1>     over the head counts and head words (a launch struct that points there): the heads in front of
//                              every tile and view, and counts[v]. A view's first candidate is a whole draw or has j = 0: never
//                              linked, so a view's heads are the bits from its first candidate on.
//   cluster_run_write_kernel   cluster_write_kernel's walk over the head bits: a head's position is its rank. The run ends at the
//                              first clear bit of link & survive behind the head — inside kClusterRunSpan / 64 + 1 words, because no
//                              cluster with j % kClusterRunSpan == 0 is linked; a whole draw, a dead lane and the next draw's
//                              cluster 0 have no link bit, so a run never leaves its draw. One more cluster load for its last cluster.
//
// Nothing waits, no atomics, integer ranks only; the second phase finds what the plain form would have left (it reads neither
// tile_count nor the survivor starts).
static_assert(offsetof(ClusterRunLaunch, k) == 0, "the per-view arguments are read at the plain form's offsets");

__global__ __launch_bounds__(kClusterBlock) void cluster_run_test_kernel(const ClusterRunLaunch r)
{
    cluster_test_tiles<true, false, false>(r.k, r.link, nullptr, 0u, nullptr, 0u);
}

__global__ __launch_bounds__(kClusterBlock) void cluster_run_heads_kernel(const ClusterRunLaunch r)
{
    const ClusterLaunch& a = r.k;
    const uint32_t total = a.totals[kClusterTotalCandidates];
    const uint32_t tiles = total / kClusterTile + (total % kClusterTile ? 1u : 0u);
    for (uint64_t tile = (uint64_t)blockIdx.x * kClusterBlock + threadIdx.x; tile < tiles; tile += (uint64_t)gridDim.x * kClusterBlock) {
        const ulonglong2* const sp = reinterpret_cast<const ulonglong2*>(a.survive + tile * 4u);
        const ulonglong2* const lp = reinterpret_cast<const ulonglong2*>(r.link + tile * 4u);
        const ulonglong2 s01 = sp[0], s23 = sp[1], l01 = lp[0], l23 = lp[1];
        const unsigned long long s[4] = {s01.x, s01.y, s23.x, s23.y}, l[4] = {l01.x, l01.y, l23.x, l23.y};
        unsigned long long before = tile ? a.survive[tile * 4u - 1u] >> 63 : 0ull;  // the candidate in front of the tile survived
        unsigned long long h[4];
        uint32_t n = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) {
            h[w] = s[w] & ~(l[w] & ((s[w] << 1) | before));
            before = s[w] >> 63;
            n += (uint32_t)__popcll(h[w]);
        }
        ulonglong2* const hp = reinterpret_cast<ulonglong2*>(r.head + tile * 4u);
        hp[0] = ulonglong2{h[0], h[1]};
        hp[1] = ulonglong2{h[2], h[3]};
        r.head_count[tile] = n;
    }
}

__global__ __launch_bounds__(kClusterBlock) void cluster_run_write_kernel(const ClusterRunLaunch r)
{
    const ClusterLaunch& a = r.k;
    const uint32_t total = a.totals[kClusterTotalCandidates];
    const uint32_t tiles = total / kClusterTile + (total % kClusterTile ? 1u : 0u);
    const uint64_t words_written = (uint64_t)tiles * 4u;  // (the words behind them were not written by this call)
    const uint32_t blocks = a.first_block[a.views];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const unsigned long long* const words = r.head + (size_t)tile * 4u;
        const unsigned long long word = words[wave];
        if (!((word >> lane) & 1ull))
            continue;
        uint32_t rank = r.head_count[tile] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));  // (scanned: heads in front of the tile)
        for (uint32_t w = 0; w < wave; w++)
            rank += (uint32_t)__popcll(words[w]);
        const uint32_t c = tile * kClusterTile + threadIdx.x;
        uint32_t block, at, j;
        locate(a, c, tile, tiles, blocks, block, at, j);
        const uint32_t v = view_of_block(a.first_block, a.views, block);
        uint32_t position = rank;  // packed: the views' commands back to back are the heads in order
        if (a.region) {
            const uint32_t in_view = rank - a.totals[kClusterSurvivorStart + v];  // (the scan over the heads left the heads here)
            if (in_view >= a.region)
                continue;
            position = v * a.region + in_view;
        }
        if (position >= a.capacity)
            continue;
        const ViewPick view = pick_view(a, v);
        const uint32_t k = at - view.first_block * kClusterBlock;
        const uint32_t g = a.draw_geometry[at];  // (below table_count: the draw has candidates)
        const CommandGeometry geometry = a.table[g];
        const ClusterRange range = range_of(a, g);
        uint32_t count = geometry.count, first = geometry.first;
        if (range.count) {
            // the run's end: the first candidate behind the head that is not linked or did not survive
            uint64_t end = (uint64_t)c + 1u;
            for (uint32_t step = 0; step <= kClusterRunSpan / 64u; step++) {
                const uint64_t w = end / 64u;
                if (w >= words_written)
                    break;
                const unsigned long long open = ~(r.link[w] & a.survive[w]) & (~0ull << (end % 64u));
                if (open) {
                    end = w * 64u + (uint32_t)__builtin_ctzll(open);
                    break;
                }
                end = (w + 1u) * 64u;
            }
            // (below the range's count by the rule: cluster 0 of the next draw, a whole draw and a dead lane have no link bit)
            const uint32_t last = min(j + (uint32_t)(end - c) - 1u, range.count - 1u);
            const float4* const table = a.clusters + (size_t)range.first * 2u;
            const uint32_t head_first = __float_as_uint(table[(size_t)j * 2u].w);
            first += head_first;
            count = __float_as_uint(table[(size_t)last * 2u].w) + __float_as_uint(table[(size_t)last * 2u + 1u].w) - head_first;
        }
        const uint32_t from = first_of_draw(a, v, k);
        put_command(a, position, count, instances_of_draw(a, v, k, *view.count, from), first, from, (uint32_t)geometry.vertex_offset, k);
    }
    if (a.region) {  // the all-zero padding positions C_v <= j < R of every view
        const uint64_t positions = (uint64_t)a.views * a.region;
        for (uint64_t p = (uint64_t)blockIdx.x * kClusterBlock + threadIdx.x; p < positions && p < a.capacity; p += (uint64_t)gridDim.x * kClusterBlock) {
            const uint32_t v = (uint32_t)(p / a.region), in_view = (uint32_t)(p % a.region);
            if (in_view < a.counts[v])
                continue;
            uint32_t* const to = reinterpret_cast<uint32_t*>(a.dst + (size_t)p * a.stride);
            for (uint32_t w = 0; w < a.stride / 4u; w++)
                to[w] = 0u;
        }
    }
}

// ---- the normal-cone form (gv_pool_cull_cluster_cones) ----
// The three test kernels above with the cone test in their conjunction; count, scans, heads and writers are the launches above as
// they are, given the wrapped struct. The wrappers' first members keep the per-view arguments at the plain form's offsets.
static_assert(offsetof(ClusterConeLaunch, k) == 0 && offsetof(ClusterConeRunLaunch, r) == 0 && offsetof(ClusterConeSecondLaunch, s) == 0,
              "the per-view arguments are read at the plain form's offsets");
static_assert(sizeof(ClusterEye) == sizeof(float[4]), "an eye is four floats of the argument block");

__global__ __launch_bounds__(kClusterBlock) void cluster_cone_test_kernel(const ClusterConeLaunch c)
{
    cluster_test_tiles<false, true, false>(c.k, nullptr, c.cone.cones, (uint32_t)(offsetof(ClusterConeLaunch, cone) + offsetof(ClusterConeArgs, eyes)), nullptr, 0u);
}

__global__ __launch_bounds__(kClusterBlock) void cluster_cone_run_test_kernel(const ClusterConeRunLaunch c)
{
    cluster_test_tiles<true, true, false>(c.r.k, c.r.link, c.cone.cones, (uint32_t)(offsetof(ClusterConeRunLaunch, cone) + offsetof(ClusterConeArgs, eyes)), nullptr,
                                          0u);
}

__global__ __launch_bounds__(kClusterBlock) void cluster_cone_second_test_kernel(const ClusterConeSecondLaunch c)
{
    cluster_second_test_tiles<true, false>(c.s, c.cone.cones, (uint32_t)(offsetof(ClusterConeSecondLaunch, cone) + offsetof(ClusterConeArgs, eyes)), nullptr,
                                           0u);
}

// ---- the level-of-detail form (gv_pool_cull_cluster_lods) ----
// The six test kernels above with the LOD cut in front of their conjunction; count, scans, heads and writers are the launches above
// as they are, given the innermost wrapped struct. The wrappers' first members keep every other argument at its form's offsets.
static_assert(offsetof(ClusterLodLaunch, k) == 0 && offsetof(ClusterLodRunLaunch, r) == 0 && offsetof(ClusterLodConeLaunch, c) == 0 &&
                  offsetof(ClusterLodConeRunLaunch, c) == 0 && offsetof(ClusterLodSecondLaunch, s) == 0 && offsetof(ClusterLodConeSecondLaunch, c) == 0,
              "the per-view arguments and the eyes are read at the wrapped form's offsets");
#define GV_LOD_VIEWS_AT(T) ((uint32_t)(offsetof(T, lod) + offsetof(ClusterLodArgs, views)))
#define GV_CONE_EYES_AT(T) ((uint32_t)(offsetof(T, cone) + offsetof(ClusterConeArgs, eyes)))

__global__ __launch_bounds__(kClusterBlock) void cluster_lod_test_kernel(const ClusterLodLaunch l)
{
    cluster_test_tiles<false, false, true>(l.k, nullptr, nullptr, 0u, l.lod.lods, GV_LOD_VIEWS_AT(ClusterLodLaunch));
}

__global__ __launch_bounds__(kClusterBlock) void cluster_lod_run_test_kernel(const ClusterLodRunLaunch l)
{
    cluster_test_tiles<true, false, true>(l.r.k, l.r.link, nullptr, 0u, l.lod.lods, GV_LOD_VIEWS_AT(ClusterLodRunLaunch));
}

__global__ __launch_bounds__(kClusterBlock) void cluster_lod_cone_test_kernel(const ClusterLodConeLaunch l)
{
    cluster_test_tiles<false, true, true>(l.c.k, nullptr, l.c.cone.cones, GV_CONE_EYES_AT(ClusterConeLaunch), l.lod.lods, GV_LOD_VIEWS_AT(ClusterLodConeLaunch));
}

__global__ __launch_bounds__(kClusterBlock) void cluster_lod_cone_run_test_kernel(const ClusterLodConeRunLaunch l)
{
    cluster_test_tiles<true, true, true>(l.c.r.k, l.c.r.link, l.c.cone.cones, GV_CONE_EYES_AT(ClusterConeRunLaunch), l.lod.lods,
                                         GV_LOD_VIEWS_AT(ClusterLodConeRunLaunch));
}

__global__ __launch_bounds__(kClusterBlock) void cluster_lod_second_test_kernel(const ClusterLodSecondLaunch l)
{
    cluster_second_test_tiles<false, true>(l.s, nullptr, 0u, l.lod.lods, GV_LOD_VIEWS_AT(ClusterLodSecondLaunch));
}

__global__ __launch_bounds__(kClusterBlock) void cluster_lod_cone_second_test_kernel(const ClusterLodConeSecondLaunch l)
{
    cluster_second_test_tiles<true, true>(l.c.s, l.c.cone.cones, GV_CONE_EYES_AT(ClusterConeSecondLaunch), l.lod.lods,
                                          GV_LOD_VIEWS_AT(ClusterLodConeSecondLaunch));
}
#undef GV_LOD_VIEWS_AT
#undef GV_CONE_EYES_AT

// the fixed grid of the test and write launches: kClusterGridPerCu workgroups per compute unit of the current device
uint32_t walk_grid()
{
    int device = 0, units = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&units, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || units <= 0)
        units = 256;
    return (uint32_t)units * kClusterGridPerCu;
}

}  // namespace

hipError_t launch_cluster_count(const ClusterLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_count_kernel, dim3(std::max(1u, launch.first_block[launch.views])), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_scan_candidates(const ClusterLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_scan_kernel<0>, dim3(1), dim3(kClusterScanBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_test(const ClusterLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_scan_survivors(const ClusterLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_scan_kernel<1>, dim3(1), dim3(kClusterScanBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_write(const ClusterLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_write_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_run_test(const ClusterRunLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_run_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_run_heads(const ClusterRunLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_run_heads_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_run_scan(const ClusterRunLaunch& launch, hipStream_t stream)
{
    ClusterLaunch heads = launch.k;  // the survivors' scan, pointed at the head counts and head words
    heads.tile_count = launch.head_count;
    heads.survive = launch.head;
    hipLaunchKernelGGL(cluster_scan_kernel<1>, dim3(1), dim3(kClusterScanBlock), 0, stream, heads);
    return hipGetLastError();
}

hipError_t launch_cluster_run_write(const ClusterRunLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_run_write_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_second_count(const ClusterSecondLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_second_count_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_second_scan_pending(const ClusterSecondLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_second_scan_kernel<0>, dim3(1), dim3(kClusterScanBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_second_test(const ClusterSecondLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_second_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_second_scan_survivors(const ClusterSecondLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_second_scan_kernel<1>, dim3(1), dim3(kClusterScanBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_second_write(const ClusterSecondLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_second_write_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_cone_test(const ClusterConeLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_cone_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_cone_run_test(const ClusterConeRunLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_cone_run_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_cone_second_test(const ClusterConeSecondLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_cone_second_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_lod_test(const ClusterLodLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_lod_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_lod_run_test(const ClusterLodRunLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_lod_run_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_lod_cone_test(const ClusterLodConeLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_lod_cone_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_lod_cone_run_test(const ClusterLodConeRunLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_lod_cone_run_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_lod_second_test(const ClusterLodSecondLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_lod_second_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_cluster_lod_cone_second_test(const ClusterLodConeSecondLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(cluster_lod_cone_second_test_kernel, dim3(walk_grid()), dim3(kClusterBlock), 0, stream, launch);
    return hipGetLastError();
}

}  // namespace gv
