// gv_group_kernels.hpp — launch interface of gv_group.hip: gv_pool_group_draws, the stable reorder of a view's records by geometry
// key. Kept apart from gv_kernels.hpp like gv_sort_kernels.hpp (bench.py hashes that file).
#pragma once
#include "gv_kernels.hpp"

namespace gv {

constexpr uint32_t kGroupBlock = 256;       // lanes per workgroup of every grouping kernel
constexpr uint32_t kGroupTileKeys = 2048;   // keys per workgroup and launch: eight per lane, a run of 512 per wave
constexpr uint32_t kGroupGroupTiles = 32;   // tiles whose digit counts are also summed per group (as the sort's kSortGroupTiles)
constexpr uint32_t kGroupMaxDigits = 3;     // 8-bit digits of the value 65 536

// the digits a key table of K entries needs: the bytes that hold the VALUE K (the void bucket)
inline uint32_t group_digits(uint32_t table_count) { return table_count <= 255u ? 1u : table_count <= 65535u ? 2u : 3u; }
inline uint32_t group_tile_count(uint32_t capacity) { return (capacity + kGroupTileKeys - 1u) / kGroupTileKeys; }
inline uint32_t group_group_count(uint32_t capacity) { return (group_tile_count(capacity) + kGroupGroupTiles - 1u) / kGroupGroupTiles; }
// words of `hist`: [digits][groups][256] group counts (zeroed in front of every call), then [tiles][256] tile counts
inline size_t group_counter_words(uint32_t capacity) { return (size_t)kGroupMaxDigits * group_group_count(capacity) * 256u; }
inline size_t group_hist_words(uint32_t capacity) { return group_counter_words(capacity) + (size_t)group_tile_count(capacity) * 256u; }

struct GroupLaunch {
    const uint32_t* count;     // device draw count
    uint32_t capacity;         // the view's occupancy: the host's bound of *count (sizes the grid)
    uint32_t key_max;          // K: keys are min(g, K)
    const uint32_t* idx_in;    // the view's records ...
    const float* model_in;
    const float* dist_in;
    uint32_t* idx_out;         // ... and its alternate set
    float* model_out;
    float* dist_out;
    const uint32_t* ids;       // base geometry id per POOL SLOT (NULL: 0)
    const uint32_t* sizes;     // fp32 bit patterns per POOL SLOT (NULL: 1); read with by_lod only
    const LodEntry* table;     // by_lod only
    uint32_t lod_table_count;
    uint32_t by_lod;
    float scale;
    uint32_t groups;           // group_group_count(capacity)
    uint32_t* keys[2];         // (key, record index) pairs, ping-pong: pass p reads set p & 1 (pass 0: the index is the position)
    uint32_t* vals[2];
    uint16_t* ranks;           // per key of the current order: rank among its tile's keys of the same digit
    uint32_t* group_hist;      // [digits][groups][256], zero on entry
    uint32_t* tile_hist;       // [tiles][256], rewritten by each pass
};
// One call = launch_group_keys (keys + the ranks of digit 0), then per digit p: launch_group_scatter(p, p == digits - 1), and in
// front of it for p > 0 launch_group_rank(p). 2 x digits launches, fixed by the host.
hipError_t launch_group_keys(const GroupLaunch& launch, hipStream_t stream);
hipError_t launch_group_rank(const GroupLaunch& launch, uint32_t pass, hipStream_t stream);
hipError_t launch_group_scatter(const GroupLaunch& launch, uint32_t pass, bool last, hipStream_t stream);

}  // namespace gv
