// gv_clusters_second.cpp — gv_pool_cull_clusters_second_phase / gv_pool_cluster_second_commands_device /
// gv_pool_cluster_second_commands_fetch of include/garden_vis.h: the clusters the pool's cluster cull K1 tested and did not keep, in
// the views for which it queried a pyramid, tested again against that pyramid as it stands now; one indirect command per survivor
// (DESIGN.md §4 item 21, §5.24). A reader of what K1 left on the device (PoolState::clusters) with buffers of its own
// (PoolState::clusters.second): K1's commands, counts, bits and scratch are not written. Kernels: gv_clusters.hip.
#include "gv_ctx.hpp"

using namespace gv;

namespace {

constexpr uint64_t kOwnTargetMaxBytes = 1ull << 31;  // as gv_pool_cull_clusters: a library-owned target beyond this is refused

}  // namespace

extern "C" {

int gv_pool_cull_clusters_second_phase(GvCtx* ctx, uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device,
                                       size_t capacity_bytes)
{
    if (!ctx)
        return GV_E_ARG;
    const char* const fn = "gv_pool_cull_clusters_second_phase";
    if (!bound_pool(ctx, fn, pool_id))
        return GV_E_ARG;
    if (flags)
        return ctx->fail(GV_E_ARG, "gv_pool_cull_clusters_second_phase: unknown flags 0x%x (must be 0)", flags);
    if (dst_device && (uintptr_t)dst_device % 16 != 0)
        return ctx->fail(GV_E_ARG, "gv_pool_cull_clusters_second_phase: dst_device must be 16-byte aligned");
    PoolState::Clusters& K = ctx->pools[pool_id].clusters;
    PoolState::Clusters::Second& S = K.second;
    if (!K.views)
        return ctx->fail(GV_E_STATE, "gv_pool_cull_clusters_second_phase: pool %u has no cluster commands since its last gv_cull, instance "
                         "emission or gv_pool_bind_clusters (gv_pool_cull_clusters)", pool_id);
    const uint32_t m = K.views;
    if ((uint64_t)m * region_commands > UINT32_MAX)
        return ctx->fail(GV_E_ARG, "gv_pool_cull_clusters_second_phase: %u regions of %u commands are more positions than 32 bits hold", m,
                         region_commands);
    if (K.rebound)
        return ctx->fail(GV_E_STATE, "gv_pool_cull_clusters_second_phase: gv_pool_bind_geometry or gv_pool_set_command_layout was called for pool "
                         "%u since its cluster cull, whose kept ids belong to the table as it was: cull the clusters again (gv_pool_cull_clusters)",
                         pool_id);
    for (uint32_t k = 0; k < m; k++)
        if (((K.launch.hiz_views >> k) & 1u) && !ctx->pyramid_built(K.pyramid[k]))
            return ctx->fail(GV_E_STATE, "gv_pool_cull_clusters_second_phase: view %u of pool %u's cluster cull names pyramid %u, which is not "
                             "built (gv_hiz_build)", k, pool_id, K.pyramid[k]);
    const uint32_t stride = K.launch.stride;
    const uint64_t positions = region_commands ? (uint64_t)m * region_commands : K.candidate_bound;  // (the host knows no better bound of the pending)
    if (!dst_device && positions * stride > kOwnTargetMaxBytes)
        return ctx->fail(GV_E_STATE, "gv_pool_cull_clusters_second_phase: pool %u may emit %llu commands of %u bytes, more than a library-owned "
                         "target holds: pass a caller-owned target (dst_device) sized for what is drawn", pool_id, (unsigned long long)positions,
                         stride);
    ZoneScope zone("Meshes Cluster Cull Second Phase");
    if (int rc = flush_sorts(ctx))  // the call is a read
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    ClusterSecondLaunch launch{};
    launch.k = K.launch;
    for (uint32_t k = 0; k < m; k++)
        if ((K.launch.hiz_views >> k) & 1u)
            launch.k.hiz[k] = hiz_device(ctx, K.pyramid[k]);  // the pyramid as it stands now
    launch.k.region = region_commands;
    if (int rc = choose_target(ctx, dst_device, capacity_bytes, stride, positions, S.d_data, &launch.k.dst, &launch.k.capacity))
        return rc;
    const size_t tiles = (size_t)((K.candidate_bound + kClusterTile - 1) / kClusterTile);
    GV_HIP(ctx, S.d_counts.reserve(2 * GV_MAX_VIEWS));
    GV_HIP(ctx, S.d_pending_count.reserve(std::max<size_t>(tiles, 4)));
    GV_HIP(ctx, S.d_pending_tile.reserve(std::max<size_t>(tiles, 1)));
    GV_HIP(ctx, S.d_kept_count.reserve(std::max<size_t>(tiles, 4)));
    GV_HIP(ctx, S.d_kept.reserve(std::max<size_t>(tiles, 1) * (kClusterTile / 64)));
    GV_HIP(ctx, S.d_totals.reserve(kSecondTotalWords));
    launch.k.counts = S.d_counts.ptr;
    launch.pending_count = S.d_pending_count.ptr;
    launch.pending_tile = S.d_pending_tile.ptr;
    launch.kept_count = S.d_kept_count.ptr;
    launch.kept = S.d_kept.ptr;
    launch.totals = S.d_totals.ptr;
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_second_count(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_second_scan_pending(launch, ctx->stream));
    if (K.second_test) {  // behind gv_pool_cull_cluster_cones: the same conjunction, with the kept launch's eyes and the cone table
        if (int rc = K.second_test(ctx, K, launch))
            return rc;
    } else {
        GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_second_test(launch, ctx->stream));
    }
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_second_scan_survivors(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_second_write(launch, ctx->stream));
    S.target = launch.k.dst;
    S.capacity = launch.k.capacity;
    S.views = m;
    S.stride = stride;
    S.region = region_commands;
    return GV_OK;
}

int gv_pool_cluster_second_commands_device(GvCtx* ctx, uint32_t pool_id, const void** commands, const void** counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !commands || !counts)
        return ctx->fail(GV_E_ARG, "gv_pool_cluster_second_commands_device: bad argument (pool %u)", pool_id);
    const PoolState::Clusters::Second& S = ctx->pools[pool_id].clusters.second;
    if (!S.views)
        return ctx->fail(GV_E_STATE, "gv_pool_cluster_second_commands_device: pool %u has no second-phase cluster commands since its last "
                         "gv_pool_cull_clusters", pool_id);
    *commands = S.target;
    *counts = S.d_counts.ptr;
    return GV_OK;
}

int gv_pool_cluster_second_commands_fetch(GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* counts, uint32_t counts_capacity)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !counts)
        return ctx->fail(GV_E_ARG, "gv_pool_cluster_second_commands_fetch: bad argument (pool %u)", pool_id);
    PoolState::Clusters::Second& S = ctx->pools[pool_id].clusters.second;
    if (!S.views)
        return ctx->fail(GV_E_STATE, "gv_pool_cluster_second_commands_fetch: pool %u has no second-phase cluster commands since its last "
                         "gv_pool_cull_clusters", pool_id);
    if (counts_capacity < 2 * S.views)
        return ctx->fail(GV_E_ARG, "gv_pool_cluster_second_commands_fetch: room for %u counts, the cluster cull listed %u views (two counts each)",
                         counts_capacity, S.views);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_staged(ctx, S.h_counts, 2 * GV_MAX_VIEWS, S.d_counts.ptr, 2 * S.views))
        return rc;
    uint64_t positions = (uint64_t)S.views * S.region;
    if (!S.region)
        for (uint32_t k = 0; k < S.views; k++)
            positions += S.h_counts.ptr[k];
    const size_t held = (size_t)std::min<uint64_t>(positions, S.capacity);  // (a caller-owned device target may have been too small for the rest)
    if (dst_host && bytes < held * S.stride)
        return ctx->fail(GV_E_ARG, "gv_pool_cluster_second_commands_fetch: %zu bytes for %zu commands of %u bytes", bytes, held, S.stride);
    memcpy(counts, S.h_counts.ptr, 2 * S.views * sizeof(uint32_t));
    if (!dst_host || !held)
        return GV_OK;
    return fetch_staged(ctx, S.h_data, held * S.stride, S.target, held * S.stride, dst_host);
}

}  // extern "C"
