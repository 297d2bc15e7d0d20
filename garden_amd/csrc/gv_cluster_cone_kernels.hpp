// gv_cluster_cone_kernels.hpp — launch interface of the normal-cone form of the cluster cull (gv_pool_cull_cluster_cones, DESIGN.md
// §4 item 23, §5.26): a cluster survives iff it survives gv_pool_cull_clusters' test and its normal cone does not face away from the
// view's eye. The kernels live in gv_clusters.hip: the three test kernels of the plain form, the run form and the second phase,
// instantiated with the cone test in their walk. Count, scans, heads and writers are the other forms' launches as they are.
#pragma once
#include "gv_cluster_kernels.hpp"
#include "gv_cluster_run_kernels.hpp"
#include "gv_cluster_second_kernels.hpp"

namespace gv {

struct ClusterCone {   // GvClusterCone
    float apex[3];
    float cutoff;
    float axis[3];
    uint32_t reserved;
};
// what the cone test adds to a launch: the cone table, parallel to the cluster table (two 16-byte pieces per cone), and one eye per
// view of E in the records' space — read at a wave-uniform offset from the argument block, like the planes
struct ClusterConeArgs {
    const float4* cones;
    float eyes[kMaxInstanceViews][4];   // e[3] != 0: a point eye; e[3] == 0: parallel rays along e[0..2]; all zero: no cone test
};
// The wrapped struct is the first member: the per-view arguments are read from the argument block at the plain form's offsets.
struct ClusterConeLaunch {
    ClusterLaunch k;
    ClusterConeArgs cone;
};
struct ClusterConeRunLaunch {
    ClusterRunLaunch r;
    ClusterConeArgs cone;
};
struct ClusterConeSecondLaunch {
    ClusterSecondLaunch s;
    ClusterConeArgs cone;
};
static_assert(sizeof(ClusterConeLaunch) <= 4096 && sizeof(ClusterConeRunLaunch) <= 4096 && sizeof(ClusterConeSecondLaunch) <= 4096,
              "a launch carries 4 KB of arguments by value");

// The test launch of each form with the cone test in it. Everything else of a call is launched with the wrapped struct: the plain
// form's five launches with launch_cluster_cone_test in place of launch_cluster_test, the run form's six with
// launch_cluster_cone_run_test in place of launch_cluster_run_test, the second phase's five with launch_cluster_cone_second_test in
// place of launch_cluster_second_test.
hipError_t launch_cluster_cone_test(const ClusterConeLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_cone_run_test(const ClusterConeRunLaunch& launch, hipStream_t stream);
hipError_t launch_cluster_cone_second_test(const ClusterConeSecondLaunch& launch, hipStream_t stream);

}  // namespace gv
