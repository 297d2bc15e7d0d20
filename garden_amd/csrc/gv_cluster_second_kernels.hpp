// gv_cluster_second_kernels.hpp — launch interface of the second phase of the cluster cull (gv_pool_cull_clusters_second_phase,
// DESIGN.md §4 item 21, §5.24): the clusters a cluster cull K1 tested and did not keep, in the views for which it queried a pyramid,
// tested again against that pyramid as it stands now. The kernels live in gv_clusters.hip beside K1's, whose device helpers they
// share; they read what K1 left on the device and write none of it.
#pragma once
#include "gv_cluster_kernels.hpp"

namespace gv {

// words of ClusterSecondLaunch::totals
constexpr uint32_t kSecondTotalPending = 0;                                // P
constexpr uint32_t kSecondPendingStart = 1;                                // [views + 1]: pending in front of view v (the last one: P)
constexpr uint32_t kSecondSurvivorStart = 1 + (kMaxInstanceViews + 1);     // [views + 1]: second-phase survivors in front of view v
constexpr uint32_t kSecondTotalWords = 1 + 2 * (kMaxInstanceViews + 1);

struct ClusterSecondLaunch {
    // K1's own arguments, as K1 was launched, with four things replaced: hiz[] holds the pyramids as they stand NOW, and dst,
    // capacity, region and counts are this call's. First member: the per-view arguments are read from the argument block at the
    // offsets K1's kernels read them at. Everything K1 wrote (draw_geometry, draw_local, block_total, totals, tile_block, survive)
    // is only read.
    ClusterLaunch k;
    // scratch of this call, sized by the host from K1's bound B: tiles = ceil(B / kClusterTile), as K1's
    uint32_t* pending_count;     // [tiles]: pending candidates of a candidate tile; scanned in place into those in front
    uint32_t* pending_tile;      // [tiles]: per PENDING tile (kClusterTile pending each) the candidate tile that holds its first
    uint32_t* kept_count;        // [tiles]: survivors of a pending tile; scanned in place into those in front
    unsigned long long* kept;    // [tiles * 4]: one ballot word per wave and pending tile
    uint32_t* totals;            // [kSecondTotalWords]
};
static_assert(sizeof(ClusterSecondLaunch) <= 4096, "a launch carries 4 KB of arguments by value");

// The five launches of one call, in this order on one stream (the host reads nothing in between).
hipError_t launch_cluster_second_count(const ClusterSecondLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_second_scan_pending(const ClusterSecondLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_second_test(const ClusterSecondLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_second_scan_survivors(const ClusterSecondLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_second_write(const ClusterSecondLaunch& launch, hipStream_t stream);

}  // namespace gv
