// gv_cluster_cones.cpp — gv_pool_bind_cluster_cones / gv_pool_cull_cluster_cones of include/garden_vis.h: the cluster cull with
// normal-cone backface rejection in its conjunction. Every check, the bound, the target and the
// bookkeeping are gv_pool_cull_clusters' own (cull_clusters, gv_clusters.cpp), which also checks the eyes and keeps them with the
// launch; this file adds the cone table and the two launch lists — the plain form's five and the run form's six, each with the test
// launch that carries the cone test. The result is the pool's cluster result: the readers of gv_clusters.cpp serve it, and a second
// phase behind it applies the same conjunction (gv_clusters_second.cpp). Kernels: gv_clusters.hip.
#include "gv_ctx.hpp"

using namespace gv;

namespace {

static_assert(sizeof(GvClusterCone) == sizeof(ClusterCone) && sizeof(GvClusterCone) == 32, "the kernels read a cone as two 16-byte pieces");
static_assert(sizeof(GvClusterEye) == sizeof(float[4]), "an eye is four floats of the argument block");
static_assert(GV_CLUSTERS_RUNS == 2u && (GV_CLUSTERS_RUNS & GV_CLUSTERS_FRUSTUM_ONLY) == 0, "two flag bits");

// the plain form's five launches, the test with the cone in it
int write_cone_survivors(GvCtx* ctx, PoolState::Clusters& K, const ClusterLaunch& launch, size_t, const GvClusterEye* eyes, const GvClusterLodView*)
{
    ClusterConeLaunch cone{};
    cone.k = launch;
    cone.cone = cluster_cone_args(K, launch.views, eyes);
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_count(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_candidates(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_cone_test(cone, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_survivors(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_write(launch, ctx->stream));
    return GV_OK;
}

// the run form's six launches likewise
int write_cone_runs(GvCtx* ctx, PoolState::Clusters& K, const ClusterLaunch& launch, size_t tiles, const GvClusterEye* eyes, const GvClusterLodView*)
{
    ClusterConeRunLaunch cone{};
    if (int rc = reserve_runs(ctx, K, launch, tiles, &cone.r))
        return rc;
    cone.cone = cluster_cone_args(K, launch.views, eyes);
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_count(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_candidates(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_cone_run_test(cone, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_heads(cone.r, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_scan(cone.r, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_write(cone.r, ctx->stream));
    return GV_OK;
}

// the second phase's test launch behind a cone result (PoolState::Clusters::second_test): the cone table and the kept eyes
int cone_second_test(GvCtx* ctx, PoolState::Clusters& K, const ClusterSecondLaunch& launch)
{
    ClusterConeSecondLaunch cone{};
    cone.s = launch;
    cone.cone = cluster_cone_args(K, kMaxInstanceViews, K.eyes);
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_cone_second_test(cone, ctx->stream));
    return GV_OK;
}

}  // namespace

extern "C" {

int gv_pool_bind_cluster_cones(GvCtx* ctx, uint32_t pool_id, const GvClusterCone* cones, uint32_t cone_count)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_cluster_cones: pool %u out of range", pool_id);
    if (!cones != !cone_count)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_cluster_cones: cones %p with %u entries (a table, or NULL and 0 to remove the binding)",
                         (const void*)cones, cone_count);
    PoolState::Clusters& K = ctx->pools[pool_id].clusters;
    if (!K.bound)
        return ctx->fail(GV_E_STATE, "gv_pool_bind_cluster_cones: pool %u has no clusters bound (gv_pool_bind_clusters)", pool_id);
    if (cones && cone_count != K.cluster_count)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_cluster_cones: %u cones for the %u clusters bound to pool %u (one each)", cone_count,
                         K.cluster_count, pool_id);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the stream may still be reading the table)
    K.views = 0;  // a result made with the cones as they were, or without them, ends
    K.second.views = 0;
    K.cones_bound = false;
    if (!cones) {
        K.d_cones.release();
        return GV_OK;
    }
    GV_HIP(ctx, K.d_cones.reserve(cone_count));
    GV_HIP(ctx, hipMemcpy(K.d_cones.ptr, cones, (size_t)cone_count * sizeof(GvClusterCone), hipMemcpyHostToDevice));
    ctx->stats.upload_bytes += (size_t)cone_count * sizeof(GvClusterCone);
    K.cones_bound = true;
    return GV_OK;
}

int gv_pool_cull_cluster_cones(GvCtx* ctx, uint32_t pool_id, uint32_t flags, const GvClusterEye* eyes, uint32_t eye_count, uint32_t region_commands,
                               void* dst_device, size_t capacity_bytes)
{
    const ClusterConeRequest request{eyes, eye_count};
    return cull_clusters(ctx, "gv_pool_cull_cluster_cones", ClusterCullForms{write_cone_survivors, write_cone_runs, cone_second_test},
                         GV_CLUSTERS_FRUSTUM_ONLY | GV_CLUSTERS_RUNS, &request, "Meshes Cluster Cull Cones", pool_id, flags, region_commands, dst_device,
                         capacity_bytes);
}

}  // extern "C"
