// gv_group.hip — gfx950 kernels of gv_pool_group_draws: a view's records reordered by geometry key, stable (DESIGN.md §4 item 12,
// §5.15). A key launch followed by an LSD radix sort over the 8-bit digits the key table needs, two launches per digit and nothing
// between them but the kernel boundary — gv_sort.hip's policy: static tile ids, no workgroup waits for another, and no atomic
// decides a place (the only atomics add integer counts), so the order is reproducible.
//
//   group_key_kernel      a workgroup of 256 lanes owns a tile of 2048 draws, eight per lane, each wave a run of 512. Per draw: idx[k]
//                         streams in; the id gather and the size gather are issued together; with GV_GROUP_BY_LOD the record's third
//                         model row (ONE aligned 16-byte load at float 12 k + 8), the 32-byte table entry and lod_level, exactly as
//                         lod_kernel. The key min(g, K) is stored, and the tile is ranked for digit 0 on the spot (below).
//   group_rank_kernel     digits 1 and 2: reloads the tile's keys of the current order and ranks them.
//       ranking (both)    per round the lanes of the wave sharing my digit (8 ballots, or none when the wave agrees), my rank among
//                         them, the wave's running count from a wave-private LDS table (stable: rounds in order); then the waves'
//                         counts are scanned per digit: 16-bit ranks within the tile, the tile's 256 counts, and their sum into the
//                         counts of the tile's group of 32.
//   group_scatter_kernel  same-digit keys in front of the tile = whole groups + the tiles before it inside its group, the digit's
//                         total = the sum over the groups; the tile is reordered by digit in LDS and every digit's run written to
//                         its place as (key, record index) pairs. The LAST digit writes the records instead: idx and distanceSq are
//                         gathered by the record index, the 48-byte models by three lanes per record, so that a run leaves as
//                         whole contiguous rows.
//
// A workgroup beyond the device count leaves after one wave-uniform load (the grids are sized for the occupancy). A slot is below
// the occupancy the columns were checked against on the host; the LOD table is read inside [0, lod_table_count) only.
#include "gv_device.hpp"
#include "gv_group_kernels.hpp"

namespace gv {

namespace {

constexpr uint32_t kWaves = kGroupBlock / 64u;
constexpr uint32_t kRounds = kGroupTileKeys / kGroupBlock;  // keys per lane
constexpr uint32_t kWaveRun = kGroupTileKeys / kWaves;      // consecutive keys per wave
static_assert(kGroupBlock == 256u, "one thread per digit");
static_assert(kGroupTileKeys <= 65536u, "16-bit ranks");

// Ranks the tile's keys (key[r] = the key at wave_base + 64 r + lane; 0xFFFFFFFF beyond n) for digit `pass`.
__device__ __forceinline__ void rank_tile(const GroupLaunch& a, uint32_t pass, uint32_t n, uint32_t tile, const uint32_t (&key)[kRounds],
                                          uint32_t (*wcount)[256])
{
    for (uint32_t k = threadIdx.x; k < kWaves * 256u; k += kGroupBlock)
        (&wcount[0][0])[k] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t shift = pass * 8u;
    const uint32_t wave_base = tile * kGroupTileKeys + wave * kWaveRun;
    uint32_t local[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t j = wave_base + r * 64u + lane;
        const bool valid = j < n;
        const uint32_t d = (key[r] >> shift) & 255u;
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);  // lane 0 is valid whenever any lane is
        const unsigned long long peer = __ballot(valid && d != d0) != 0ull ? match_digit(d, valid) : __ballot(valid);
        const uint32_t below = (uint32_t)__popcll(peer & ((1ull << lane) - 1ull));
        const uint32_t prior = wcount[wave][d];
        wave_lds_order();
        if (valid && below == 0)
            wcount[wave][d] = prior + (uint32_t)__popcll(peer);
        wave_lds_order();
        local[r] = prior + below;  // rank among this wave's keys of digit d
    }
    __syncthreads();
    {  // one thread per digit: the waves' counts become the counts of the waves before them, their sum the tile's count
        const uint32_t d = threadIdx.x;
        uint32_t tile_count = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; w++) {
            const uint32_t c = wcount[w][d];
            wcount[w][d] = tile_count;
            tile_count += c;
        }
        a.tile_hist[(size_t)tile * 256u + d] = tile_count;
        if (tile_count)
            atomicAdd(&a.group_hist[((size_t)pass * a.groups + tile / kGroupGroupTiles) * 256u + d], tile_count);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t j = wave_base + r * 64u + lane;
        if (j < n)
            a.ranks[j] = (uint16_t)(local[r] + wcount[wave][(key[r] >> shift) & 255u]);
    }
}

template <bool BY_LOD>
__global__ __launch_bounds__(kGroupBlock) void group_key_kernel(const GroupLaunch a)
{
    __shared__ uint32_t wcount[kWaves][256];
    const uint32_t n = min(*a.count, a.capacity);
    const uint32_t tile = blockIdx.x;
    if (tile * kGroupTileKeys >= n)
        return;  // (the whole workgroup, after ONE load)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t wave_base = tile * kGroupTileKeys + wave * kWaveRun;
    uint32_t key[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t k = wave_base + r * 64u + lane;
        key[r] = 0xFFFFFFFFu;
        if (k < n) {
            const uint32_t slot = stream_load(a.idx_in + k);
            uint32_t g = a.ids ? a.ids[slot] : 0u;
            if (BY_LOD) {
                const float4 row = stream_load(reinterpret_cast<const float4*>(a.model_in) + (size_t)k * 3 + 2);  // (c2.z, c3.x, c3.y, c3.z)
                const float size = a.sizes ? __uint_as_float(a.sizes[slot]) : 1.0f;
                const float x = lod_distance_sq(row.y, row.z, row.w) * a.scale;
                uint32_t levels = 1u;
                float sw[kMaxLodLevels - 1] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                if (g < a.lod_table_count) {
                    const float4* const e = reinterpret_cast<const float4*>(a.table + g);
                    const float4 e0 = e[0], e1 = e[1];
                    levels = __float_as_uint(e0.x);
                    sw[0] = e0.y, sw[1] = e0.z, sw[2] = e0.w;
                    sw[3] = e1.x, sw[4] = e1.y, sw[5] = e1.z, sw[6] = e1.w;
                }
                g += lod_level(x, size, levels, sw);  // (wraps as the selection's b + level)
            }
            key[r] = min(g, a.key_max);
            a.keys[0][k] = key[r];
        }
    }
    rank_tile(a, 0u, n, tile, key, wcount);
}

__global__ __launch_bounds__(kGroupBlock) void group_rank_kernel(const GroupLaunch a, const uint32_t pass)
{
    __shared__ uint32_t wcount[kWaves][256];
    const uint32_t n = min(*a.count, a.capacity);
    const uint32_t tile = blockIdx.x;
    if (tile * kGroupTileKeys >= n)
        return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t wave_base = tile * kGroupTileKeys + wave * kWaveRun;
    const uint32_t* __restrict__ keys_in = a.keys[pass & 1u];
    uint32_t key[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t j = wave_base + r * 64u + lane;
        key[r] = j < n ? keys_in[j] : 0xFFFFFFFFu;
    }
    rank_tile(a, pass, n, tile, key, wcount);
}

// exclusive scan of one value per thread over the 256-lane workgroup
__device__ __forceinline__ uint32_t group_exclusive_scan(uint32_t v, uint32_t* wave_sum /* LDS [kWaves] */)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_scan(v, lane);
    __syncthreads();  // wave_sum may still be read from a previous scan
    if (lane == 63u)
        wave_sum[wave] = incl;
    __syncthreads();
    uint32_t wave_prefix = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; w++)
        wave_prefix += w < wave ? wave_sum[w] : 0u;
    return wave_prefix + incl - v;
}

template <bool LAST>
__global__ __launch_bounds__(kGroupBlock) void group_scatter_kernel(const GroupLaunch a, const uint32_t pass)
{
    __shared__ uint32_t tile_excl[256];  // exclusive scan of the tile's digit counts (tile-local sorted order)
    __shared__ uint32_t dst_base[256];   // global position of the tile's first key of each digit
    __shared__ uint32_t skey[kGroupTileKeys];  // the tile reordered by digit
    __shared__ uint32_t sval[kGroupTileKeys];
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t n = min(*a.count, a.capacity);
    const uint32_t tile = blockIdx.x;
    if (tile * kGroupTileKeys >= n)
        return;
    const uint32_t tiles = (n + kGroupTileKeys - 1u) / kGroupTileKeys;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t shift = pass * 8u;
    const uint32_t wave_base = tile * kGroupTileKeys + wave * kWaveRun;
    const uint32_t* __restrict__ keys_in = a.keys[pass & 1u];
    const uint32_t* __restrict__ vals_in = a.vals[pass & 1u];
    uint32_t key[kRounds], val[kRounds], rank[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t j = wave_base + r * 64u + lane;
        const bool valid = j < n;
        key[r] = valid ? keys_in[j] : 0xFFFFFFFFu;
        val[r] = pass == 0u ? j : (valid ? vals_in[j] : 0u);
        rank[r] = valid ? (uint32_t)a.ranks[j] : 0u;
    }
    // one thread per digit: same-digit keys in the tiles before this one = whole groups + the tiles before it in its group
    const uint32_t d = threadIdx.x;
    uint32_t before = 0, digit_total = 0;
    const uint32_t tile_count = a.tile_hist[(size_t)tile * 256u + d];
    {
        const uint32_t group = tile / kGroupGroupTiles;
        const uint32_t* __restrict__ gh = a.group_hist + (size_t)pass * a.groups * 256u + d;
        const uint32_t* __restrict__ th = a.tile_hist + d;
        const uint32_t live_groups = (tiles + kGroupGroupTiles - 1u) / kGroupGroupTiles;
#pragma unroll 8
        for (uint32_t g = 0; g < live_groups; g++) {
            const uint32_t c = gh[(size_t)g * 256u];
            digit_total += c;
            before += g < group ? c : 0u;
        }
#pragma unroll 8
        for (uint32_t u = group * kGroupGroupTiles; u < tile; u++)
            before += th[(size_t)u * 256u];
    }
    const uint32_t gbase = group_exclusive_scan(digit_total, wave_sum);  // keys of lower digits, all tiles
    const uint32_t texcl = group_exclusive_scan(tile_count, wave_sum);   // ... in this tile
    tile_excl[d] = texcl;
    dst_base[d] = gbase + before;
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t j = wave_base + r * 64u + lane;
        if (j < n) {
            const uint32_t lpos = tile_excl[(key[r] >> shift) & 255u] + rank[r];
            skey[lpos] = key[r];
            sval[lpos] = val[r];
        }
    }
    __syncthreads();
    const uint32_t live = min(kGroupTileKeys, n - tile * kGroupTileKeys);
    if (!LAST) {
        uint32_t* __restrict__ keys_out = a.keys[(pass & 1u) ^ 1u];
        uint32_t* __restrict__ vals_out = a.vals[(pass & 1u) ^ 1u];
#pragma unroll 4
        for (uint32_t t = threadIdx.x; t < live; t += kGroupBlock) {
            const uint32_t k = skey[t];
            const uint32_t dd = (k >> shift) & 255u;
            const uint32_t pos = dst_base[dd] + (t - tile_excl[dd]);
            keys_out[pos] = k;
            vals_out[pos] = sval[t];
        }
        return;
    }
    // LAST: the records go straight to their places. sval[t] = the record's index before the call.
    for (uint32_t t = threadIdx.x; t < live; t += kGroupBlock) {
        const uint32_t dd = (skey[t] >> shift) & 255u;
        const uint32_t pos = dst_base[dd] + (t - tile_excl[dd]);
        const uint32_t v = sval[t];
        a.idx_out[pos] = a.idx_in[v];
        a.dist_out[pos] = a.dist_in[v];
        skey[t] = pos;  // only this thread reads skey[t] in this loop
    }
    __syncthreads();
    const float4* __restrict__ src = reinterpret_cast<const float4*>(a.model_in);
    float4* __restrict__ dst = reinterpret_cast<float4*>(a.model_out);
#pragma unroll 4
    for (uint32_t q = threadIdx.x; q < live * 3u; q += kGroupBlock) {
        const uint32_t t = q / 3u, part = q - t * 3u;
        dst[(size_t)skey[t] * 3 + part] = src[(size_t)sval[t] * 3 + part];
    }
}

}  // namespace

hipError_t launch_group_keys(const GroupLaunch& launch, hipStream_t stream)
{
    const dim3 grid(std::max(1u, group_tile_count(launch.capacity))), block(kGroupBlock);
    if (launch.by_lod)
        hipLaunchKernelGGL(group_key_kernel<true>, grid, block, 0, stream, launch);
    else
        hipLaunchKernelGGL(group_key_kernel<false>, grid, block, 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_group_rank(const GroupLaunch& launch, uint32_t pass, hipStream_t stream)
{
    hipLaunchKernelGGL(group_rank_kernel, dim3(std::max(1u, group_tile_count(launch.capacity))), dim3(kGroupBlock), 0, stream, launch, pass);
    return hipGetLastError();
}

hipError_t launch_group_scatter(const GroupLaunch& launch, uint32_t pass, bool last, hipStream_t stream)
{
    const dim3 grid(std::max(1u, group_tile_count(launch.capacity))), block(kGroupBlock);
    if (last)
        hipLaunchKernelGGL(group_scatter_kernel<true>, grid, block, 0, stream, launch, pass);
    else
        hipLaunchKernelGGL(group_scatter_kernel<false>, grid, block, 0, stream, launch, pass);
    return hipGetLastError();
}

}  // namespace gv
