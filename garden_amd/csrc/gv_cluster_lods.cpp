// gv_cluster_lods.cpp — gv_pool_bind_cluster_lods / gv_pool_cull_cluster_lods of include/garden_vis.h: the cluster cull with the cut
// through a bound cluster DAG in front of its conjunction. Every check, the bound, the target and the
// bookkeeping are gv_pool_cull_clusters' own (cull_clusters, gv_clusters.cpp), which also checks the LOD views and the eyes and keeps
// them with the launch; this file adds the LOD table and the four launch lists — the plain form's five and the run form's six, each
// without and with the cone test, the test launch carrying the LOD cut. The result is the pool's cluster result: the readers of
// gv_clusters.cpp serve it, and a second phase behind it applies the same conjunction (gv_clusters_second.cpp). Kernels:
// gv_clusters.hip.
#include "gv_ctx.hpp"

using namespace gv;

namespace {

static_assert(sizeof(GvClusterLod) == sizeof(ClusterLod) && sizeof(GvClusterLod) == 48, "the kernels read a LOD entry as three 16-byte pieces");
static_assert(sizeof(GvClusterLodView) == sizeof(ClusterLodView) && sizeof(GvClusterLodView) == 32, "a LOD view is eight floats of the argument block");

ClusterLodArgs lod_args(const PoolState::Clusters& K, uint32_t views, const GvClusterLodView* lod_views)
{
    ClusterLodArgs args{};
    args.lods = reinterpret_cast<const float4*>(K.d_lods.ptr);
    memcpy(args.views, lod_views, (size_t)views * sizeof(GvClusterLodView));  // (the views behind them: scale 0, never read)
    return args;
}

// the plain form's five launches, the test with the LOD cut in it
int write_lod_survivors(GvCtx* ctx, PoolState::Clusters& K, const ClusterLaunch& launch, size_t, const GvClusterEye*, const GvClusterLodView* lod_views)
{
    ClusterLodLaunch lod{};
    lod.k = launch;
    lod.lod = lod_args(K, launch.views, lod_views);
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_count(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_candidates(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_lod_test(lod, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_survivors(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_write(launch, ctx->stream));
    return GV_OK;
}

// ... and with the cone test behind it
int write_lod_cone_survivors(GvCtx* ctx, PoolState::Clusters& K, const ClusterLaunch& launch, size_t, const GvClusterEye* eyes,
                             const GvClusterLodView* lod_views)
{
    ClusterLodConeLaunch lod{};
    lod.c.k = launch;
    lod.c.cone = cluster_cone_args(K, launch.views, eyes);
    lod.lod = lod_args(K, launch.views, lod_views);
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_count(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_candidates(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_lod_cone_test(lod, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_survivors(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_write(launch, ctx->stream));
    return GV_OK;
}

// the run form's six launches likewise
int write_lod_runs(GvCtx* ctx, PoolState::Clusters& K, const ClusterLaunch& launch, size_t tiles, const GvClusterEye*, const GvClusterLodView* lod_views)
{
    ClusterLodRunLaunch lod{};
    if (int rc = reserve_runs(ctx, K, launch, tiles, &lod.r))
        return rc;
    lod.lod = lod_args(K, launch.views, lod_views);
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_count(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_candidates(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_lod_run_test(lod, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_heads(lod.r, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_scan(lod.r, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_write(lod.r, ctx->stream));
    return GV_OK;
}

int write_lod_cone_runs(GvCtx* ctx, PoolState::Clusters& K, const ClusterLaunch& launch, size_t tiles, const GvClusterEye* eyes,
                        const GvClusterLodView* lod_views)
{
    ClusterLodConeRunLaunch lod{};
    if (int rc = reserve_runs(ctx, K, launch, tiles, &lod.c.r))
        return rc;
    lod.c.cone = cluster_cone_args(K, launch.views, eyes);
    lod.lod = lod_args(K, launch.views, lod_views);
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_count(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_candidates(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_lod_cone_run_test(lod, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_heads(lod.c.r, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_scan(lod.c.r, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_write(lod.c.r, ctx->stream));
    return GV_OK;
}

// the second phase's test launch behind a LOD result (PoolState::Clusters::second_test): the LOD table and the kept views ...
int lod_second_test(GvCtx* ctx, PoolState::Clusters& K, const ClusterSecondLaunch& launch)
{
    ClusterLodSecondLaunch lod{};
    lod.s = launch;
    lod.lod = lod_args(K, kMaxInstanceViews, K.lod_views);
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_lod_second_test(lod, ctx->stream));
    return GV_OK;
}

// ... and behind one that was given eyes, the cone table and the kept eyes too
int lod_cone_second_test(GvCtx* ctx, PoolState::Clusters& K, const ClusterSecondLaunch& launch)
{
    ClusterLodConeSecondLaunch lod{};
    lod.c.s = launch;
    lod.c.cone = cluster_cone_args(K, kMaxInstanceViews, K.eyes);
    lod.lod = lod_args(K, kMaxInstanceViews, K.lod_views);
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_lod_cone_second_test(lod, ctx->stream));
    return GV_OK;
}

}  // namespace

extern "C" {

int gv_pool_bind_cluster_lods(GvCtx* ctx, uint32_t pool_id, const GvClusterLod* lods, uint32_t lod_count)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_cluster_lods: pool %u out of range", pool_id);
    if (!lods != !lod_count)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_cluster_lods: lods %p with %u entries (a table, or NULL and 0 to remove the binding)",
                         (const void*)lods, lod_count);
    PoolState::Clusters& K = ctx->pools[pool_id].clusters;
    if (!K.bound)
        return ctx->fail(GV_E_STATE, "gv_pool_bind_cluster_lods: pool %u has no clusters bound (gv_pool_bind_clusters)", pool_id);
    if (lods && lod_count != K.cluster_count)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_cluster_lods: %u LOD entries for the %u clusters bound to pool %u (one each)", lod_count,
                         K.cluster_count, pool_id);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the stream may still be reading the table)
    K.views = 0;  // a result made with the table as it was, or without it, ends
    K.second.views = 0;
    K.lods_bound = false;
    if (!lods) {
        K.d_lods.release();
        return GV_OK;
    }
    GV_HIP(ctx, K.d_lods.reserve(lod_count));
    GV_HIP(ctx, hipMemcpy(K.d_lods.ptr, lods, (size_t)lod_count * sizeof(GvClusterLod), hipMemcpyHostToDevice));
    ctx->stats.upload_bytes += (size_t)lod_count * sizeof(GvClusterLod);
    K.lods_bound = true;
    return GV_OK;
}

int gv_pool_cull_cluster_lods(GvCtx* ctx, uint32_t pool_id, uint32_t flags, const GvClusterLodView* views, uint32_t view_count,
                              const GvClusterEye* eyes, uint32_t eye_count, uint32_t region_commands, void* dst_device, size_t capacity_bytes)
{
    if (!ctx)
        return GV_E_ARG;
    if (!eyes != !eye_count)
        return ctx->fail(GV_E_ARG, "gv_pool_cull_cluster_lods: eyes %p with %u entries (one per view of the emission, or NULL and 0 for no cone test)",
                         (const void*)eyes, eye_count);
    const ClusterLodRequest lods{views, view_count};
    const ClusterConeRequest cones{eyes, eye_count};
    const ClusterCullForms forms = eyes ? ClusterCullForms{write_lod_cone_survivors, write_lod_cone_runs, lod_cone_second_test}
                                        : ClusterCullForms{write_lod_survivors, write_lod_runs, lod_second_test};
    return cull_clusters(ctx, "gv_pool_cull_cluster_lods", forms, GV_CLUSTERS_FRUSTUM_ONLY | GV_CLUSTERS_RUNS, eyes ? &cones : nullptr,
                         "Meshes Cluster Cull Lods", pool_id, flags, region_commands, dst_device, capacity_bytes, &lods);
}

}  // extern "C"
