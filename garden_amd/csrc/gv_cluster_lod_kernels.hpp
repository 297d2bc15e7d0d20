// gv_cluster_lod_kernels.hpp — launch interface of the level-of-detail form of the cluster cull (gv_pool_cull_cluster_lods, DESIGN.md
// §4 item 24, §5.27): a cluster survives iff it lies on the cut through the bound cluster DAG for its view (its own error is small
// enough on screen and its parent's is not), survives gv_pool_cull_clusters' test and, when eyes are given, is not cone-rejected.
// The kernels live in gv_clusters.hip: the test kernels of the plain form, the run form, the cone form and the second phase,
// instantiated with the LOD test in front of their walk's plane tests. Count, scans, heads and writers are the other forms' launches
// as they are.
#pragma once
#include "gv_cluster_cone_kernels.hpp"

namespace gv {

struct ClusterLod {   // GvClusterLod
    float self_center[3], self_radius;
    float parent_center[3], parent_radius;
    float self_error, parent_error;
    uint32_t reserved[2];
};
struct ClusterLodView {   // GvClusterLodView
    float eye[4];   // eye[3] != 0: a point P = eye[0..2]; eye[3] == 0: a parallel projection, the error does not depend on distance
    float scale;    // k: the projection factor divided by the pixel threshold; +-0 switches the test off for the view
    float near_distance;
    float reserved[2];
};
// what the LOD test adds to a launch: the LOD table, parallel to the cluster table (three 16-byte pieces per entry), and one
// ClusterLodView per view of E — read at a wave-uniform offset from the argument block, like the planes and the cone's eye
struct ClusterLodArgs {
    const float4* lods;
    ClusterLodView views[kMaxInstanceViews];
};
static_assert(sizeof(ClusterLod) == 48 && sizeof(ClusterLodView) == 32 && sizeof(ClusterLodArgs) == 264, "8 + 8 * 32 bytes of arguments");
// The wrapped struct is the first member: the per-view arguments (and the cone's eyes) are read at the wrapped form's offsets.
struct ClusterLodLaunch {
    ClusterLaunch k;
    ClusterLodArgs lod;
};
struct ClusterLodRunLaunch {
    ClusterRunLaunch r;
    ClusterLodArgs lod;
};
struct ClusterLodConeLaunch {
    ClusterConeLaunch c;
    ClusterLodArgs lod;
};
struct ClusterLodConeRunLaunch {
    ClusterConeRunLaunch c;
    ClusterLodArgs lod;
};
struct ClusterLodSecondLaunch {
    ClusterSecondLaunch s;
    ClusterLodArgs lod;
};
struct ClusterLodConeSecondLaunch {
    ClusterConeSecondLaunch c;
    ClusterLodArgs lod;
};
static_assert(sizeof(ClusterLodLaunch) <= 4096 && sizeof(ClusterLodRunLaunch) <= 4096 && sizeof(ClusterLodConeLaunch) <= 4096 &&
                  sizeof(ClusterLodConeRunLaunch) <= 4096 && sizeof(ClusterLodSecondLaunch) <= 4096 && sizeof(ClusterLodConeSecondLaunch) <= 4096,
              "a launch carries 4 KB of arguments by value");

// The test launch of each form with the LOD test in it. Everything else of a call is launched with the innermost wrapped struct.
hipError_t launch_cluster_lod_test(const ClusterLodLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_lod_run_test(const ClusterLodRunLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_lod_cone_test(const ClusterLodConeLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_lod_cone_run_test(const ClusterLodConeRunLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_lod_second_test(const ClusterLodSecondLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_lod_cone_second_test(const ClusterLodConeSecondLaunch& launch, hipStream_t stream);

}  // namespace gv
