// gv_cluster_run_kernels.hpp — launch interface of the run form of the cluster cull (gv_pool_cull_cluster_runs, DESIGN.md §4 item
// 22, §5.25): the decisions of gv_pool_cull_clusters, one indirect command per RUN of adjacent surviving clusters. The kernels live
// in gv_clusters.hip beside the plain form's, whose count, scans, test body and device helpers they share.
#pragma once
#include "gv_cluster_kernels.hpp"

namespace gv {

// GV_CLUSTER_RUN_SPAN: no run crosses a multiple of it inside its draw, so the writer finds a run's end in at most kClusterRunSpan /
// 64 + 1 ballot words behind the head's
constexpr uint32_t kClusterRunSpan = 256;
static_assert(kClusterRunSpan % 64u == 0, "the writer's walk is counted in ballot words");

struct ClusterRunLaunch {
    // the plain form's arguments, as the plain form takes them. First member: the per-view arguments are read from the argument
    // block at the offsets the plain form's kernels read them at. Everything the plain form leaves on the device for a second
    // phase is left here in the same buffers with the same values; k.tile_count is not written (nothing behind the call reads it),
    // and totals[kClusterSurvivorStart ...] hold the HEADS in front of every view.
    ClusterLaunch k;
    // scratch of the run form, sized by the host from the same bound B: tiles = ceil(B / kClusterTile)
    unsigned long long* link;   // [tiles * 4]: one bit per candidate, LINKED to its predecessor (static: the tables and j alone)
    unsigned long long* head;   // [tiles * 4]: one bit per candidate, a surviving cluster that opens a run or a whole draw
    uint32_t* head_count;       // [tiles]: heads of a tile; scanned in place into those in front
};
static_assert(sizeof(ClusterRunLaunch) <= 4096, "a launch carries 4 KB of arguments by value");

// The six launches of one call, in this order on one stream (the host reads nothing in between): launch_cluster_count,
// launch_cluster_scan_candidates (gv_cluster_kernels.hpp, with launch.k), then these four.
hipError_t launch_cluster_run_test(const ClusterRunLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_run_heads(const ClusterRunLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_run_scan(const ClusterRunLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_run_write(const ClusterRunLaunch& launch, hipStream_t stream);

}  // namespace gv
