// gv_cluster_runs.cpp — gv_pool_cull_cluster_runs of include/garden_vis.h: the cluster cull's decisions, one indirect command per
// run of adjacent surviving clusters. Every check, the bound, the target and the bookkeeping are
// gv_pool_cull_clusters' own (cull_clusters, gv_clusters.cpp); this file adds the run form's scratch — a link and a head bit per
// candidate, the heads per tile — and its six launches. The result is the pool's cluster result: the readers of gv_clusters.cpp
// serve it, and a second phase behind it finds what the plain form would have left. Kernels: gv_clusters.hip.
#include "gv_ctx.hpp"

using namespace gv;

namespace {

static_assert(kClusterRunSpan == GV_CLUSTER_RUN_SPAN, "the writer's walk is bounded by the header's span");

int write_runs(GvCtx* ctx, PoolState::Clusters& K, const ClusterLaunch& launch, size_t tiles, const GvClusterEye*, const GvClusterLodView*)
{
    ClusterRunLaunch run{};
    if (int rc = reserve_runs(ctx, K, launch, tiles, &run))
        return rc;
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_count(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_candidates(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_test(run, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_heads(run, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_scan(run, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_run_write(run, ctx->stream));
    return GV_OK;
}

}  // namespace

namespace gv {

int reserve_runs(GvCtx* ctx, PoolState::Clusters& K, const ClusterLaunch& launch, size_t tiles, ClusterRunLaunch* run)
{
    const size_t words = std::max<size_t>(tiles, 1) * (kClusterTile / 64);
    GV_HIP(ctx, K.d_link.reserve(words));
    GV_HIP(ctx, K.d_head.reserve(words));
    GV_HIP(ctx, K.d_head_count.reserve(std::max<size_t>(tiles, 4)));
    run->k = launch;
    run->link = K.d_link.ptr;
    run->head = K.d_head.ptr;
    run->head_count = K.d_head_count.ptr;
    return GV_OK;
}

}  // namespace gv

extern "C" {

int gv_pool_cull_cluster_runs(GvCtx* ctx, uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device, size_t capacity_bytes)
{
    return cull_clusters(ctx, "gv_pool_cull_cluster_runs", ClusterCullForms{write_runs, nullptr, nullptr}, GV_CLUSTERS_FRUSTUM_ONLY, nullptr,
                         "Meshes Cluster Cull Runs", pool_id, flags, region_commands, dst_device, capacity_bytes);
}

}  // extern "C"
