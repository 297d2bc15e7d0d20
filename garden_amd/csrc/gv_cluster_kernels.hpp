// gv_cluster_kernels.hpp — launch interface of gv_clusters.hip: gv_pool_cull_clusters, one indirect command per surviving mesh
// cluster of every draw of the pool's last instance emission. Kept apart from gv_kernels.hpp like
// gv_previous_kernels.hpp.
#pragma once
#include "gv_kernels.hpp"

namespace gv {

constexpr uint32_t kClusterBlock = 256;       // draws per cluster_count_kernel workgroup; lanes of the test and write workgroups
constexpr uint32_t kClusterTile = 256;        // CANDIDATES per tile (one lane each): a draw of 65 535 clusters spreads over 256 tiles
constexpr uint32_t kClusterScanBlock = 1024;  // lanes of the one workgroup that scans a table, four entries per lane and turn
constexpr uint32_t kClusterGridPerCu = 8;     // test / write workgroups per compute unit: the fixed grid that walks the tiles
constexpr uint32_t kClusterNone = 0xFFFFFFFFu;  // draw_geometry of a draw that emits nothing
static_assert(kClusterBlock == kInstanceBlock, "view_of_block finds the view of a count workgroup");
static_assert(kClusterTile == 4 * 64, "a tile's survivors are four ballot words");

struct ClusterEntry {                         // GvCluster
    float box_min[3];
    uint32_t first;
    float box_max[3];
    uint32_t count;
};
struct ClusterRange { uint32_t first, count; };  // GvClusterRange
struct ClusterView {
    const uint32_t* count;  // device draw count
    const uint32_t* idx;    // records in delivery order: POOL slots
    const float* model;     // bakedModel, 12 floats per record
};
// words of ClusterLaunch::totals
constexpr uint32_t kClusterTotalCandidates = 0;              // T
constexpr uint32_t kClusterCandidateStart = 1;               // [views + 1]: candidates in front of view v (the last one: T)
constexpr uint32_t kClusterSurvivorStart = 1 + (kMaxInstanceViews + 1);  // [views + 1]: survivors in front of view v
constexpr uint32_t kClusterTotalWords = 1 + 2 * (kMaxInstanceViews + 1);

struct ClusterLaunch {
    ClusterView view[kMaxInstanceViews];             // the views of E, in E's order
    uint32_t first_block[kMaxInstanceViews + 1];     // cluster_count_kernel workgroups in front of view v (of its occupancy)
    uint32_t views;
    uint32_t region;                                 // R (0: packed)
    uint32_t stride, count, instance_count, first, first_instance, vertex_offset, draw;  // GvCommandLayout (kNoField: absent)
    const uint32_t* ids;                             // the geometry id mirror, one per POOL slot (NULL: every id is 0)
    const uint32_t* draw_ids;                        // behind a LOD selection: g_k of the listed views' draws, back to back (else NULL)
    const CommandGeometry* table;
    uint32_t table_count;
    const ClusterRange* ranges;
    uint32_t range_count;
    const float4* clusters;                          // two 16-byte pieces per cluster
    const uint32_t* starts;                          // E's starts[views + 1]
    const uint32_t* first_instance_of;               // E's first_instance[] (NULL after gv_pool_emit_instances)
    const uint32_t* draw_starts;                     // ... and draw_starts[views + 1]
    // scratch, sized by the host: draws = first_block[views] * kClusterBlock, tiles = ceil(bound / kClusterTile)
    uint32_t* draw_geometry;                         // [draws]: g_k, or kClusterNone for a draw that emits nothing
    uint32_t* draw_local;                            // [draws]: candidates in front of the draw inside its workgroup
    uint32_t* block_total;                           // [blocks]: candidates of a count workgroup; scanned in place into those in front
    uint32_t* block_tested;                          // [blocks]: of those, clusters (whole draws left out)
    uint32_t* totals;                                // [kClusterTotalWords]
    uint32_t* tile_count;                            // [tiles]: survivors of a tile; scanned in place into those in front
    uint32_t* tile_block;                            // [tiles]: the count workgroup that holds a tile's first candidate
    unsigned long long* survive;                     // [tiles * 4]: one ballot word per wave and tile
    uint8_t* dst;
    uint32_t capacity;                               // command positions dst holds: those at or beyond it are not written
    uint32_t* counts;                                // [2 * views]: commands per view, then clusters tested per view
    // per view, read at a wave-uniform offset from the argument block
    float planes[kMaxInstanceViews][6][4];
    uint32_t plane_count[kMaxInstanceViews];
    float vp[kMaxInstanceViews][16];
    HizDevice hiz[kMaxInstanceViews];                // all zero where the view does not query
    uint32_t hiz_views;                              // bit v: view v queries its pyramid
};
static_assert(sizeof(ClusterLaunch) <= 4096, "a launch carries 4 KB of arguments by value");

// The five launches of one call, in this order on one stream (the host reads nothing in between).
hipError_t launch_cluster_count(const ClusterLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_scan_candidates(const ClusterLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_test(const ClusterLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_scan_survivors(const ClusterLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_write(const ClusterLaunch& launch, hipStream_t stream);

}  // namespace gv
