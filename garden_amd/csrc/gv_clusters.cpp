// gv_clusters.cpp — gv_pool_bind_clusters / gv_pool_cull_clusters / gv_pool_cluster_commands_device / gv_pool_cluster_commands_fetch
// of include/garden_vis.h: one indirect command per surviving mesh cluster of every draw of the pool's last instance emission, built
// on the device from the records, the emission's instance ranges and the bound cluster tables.
// Buffers of its own (PoolState::clusters): neither the cull side, the instance data nor the per-draw commands are touched. Shared
// with the other derived results (gv_ctx.hpp): the reader's checks, the target choice, the staged fetch. Kernels: gv_clusters.hip.
#include "gv_ctx.hpp"

using namespace gv;

namespace {

constexpr uint64_t kOwnTargetMaxBytes = 1ull << 31;  // a library-owned target beyond this is refused: the caller sizes one for what is drawn

// the plain form's five launches: one command per survivor
int write_survivors(GvCtx* ctx, PoolState::Clusters&, const ClusterLaunch& launch, size_t, const GvClusterEye*, const GvClusterLodView*)
{
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_count(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_candidates(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_test(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_scan_survivors(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_cluster_write(launch, ctx->stream));
    return GV_OK;
}

}  // namespace

namespace gv {

int cull_clusters(GvCtx* ctx, const char* fn, ClusterCullForms forms, uint32_t allowed_flags, const ClusterConeRequest* cones, const char* zone_name,
                  uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device, size_t capacity_bytes, const ClusterLodRequest* lods)
{
    if (!ctx)
        return GV_E_ARG;
    if (!bound_pool(ctx, fn, pool_id))
        return GV_E_ARG;
    if (flags & ~allowed_flags)
        return ctx->fail(GV_E_ARG, "%s: unknown flags 0x%x", fn, flags);
    if (cones && !cones->eyes)
        return ctx->fail(GV_E_ARG, "%s: eyes is NULL (one GvClusterEye per view of the emission)", fn);
    if (lods && !lods->views)
        return ctx->fail(GV_E_ARG, "%s: views is NULL (one GvClusterLodView per view of the emission)", fn);
    const ClusterCullLaunches enqueue = (flags & GV_CLUSTERS_RUNS) ? forms.runs : forms.survivors;
    if (dst_device && (uintptr_t)dst_device % 16 != 0)
        return ctx->fail(GV_E_ARG, "%s: dst_device must be 16-byte aligned", fn);
    PoolState& p = ctx->pools[pool_id];
    PoolState::Instances& I = p.instances;
    PoolState::Geometry& G = p.geometry;
    PoolState::Clusters& K = p.clusters;
    const GvCommandLayout L = p.commands.layout;
    if (!K.bound)
        return ctx->fail(GV_E_STATE, "%s: pool %u has no clusters bound (gv_pool_bind_clusters)", fn, pool_id);
    if (cones && !K.cones_bound)
        return ctx->fail(GV_E_STATE, "%s: pool %u has no cluster cones bound (gv_pool_bind_cluster_cones)", fn, pool_id);
    if (lods && !K.lods_bound)
        return ctx->fail(GV_E_STATE, "%s: pool %u has no cluster LOD table bound (gv_pool_bind_cluster_lods)", fn, pool_id);
    if (!L.stride)
        return ctx->fail(GV_E_STATE, "%s: pool %u has no command layout (gv_pool_set_command_layout)", fn, pool_id);
    if (!G.bound)
        return ctx->fail(GV_E_STATE, "%s: pool %u has no geometry bound (gv_pool_bind_geometry)", fn, pool_id);
    if (!I.views)
        return ctx->fail(GV_E_STATE, "%s: pool %u has no instance emission since its last gv_cull", fn, pool_id);
    const uint32_t m = I.views;
    if (cones && cones->eye_count != m)
        return ctx->fail(GV_E_ARG, "%s: %u eyes for the %u views of pool %u's emission (one each)", fn, cones->eye_count, m, pool_id);
    if (lods && lods->view_count != m)
        return ctx->fail(GV_E_ARG, "%s: %u LOD views for the %u views of pool %u's emission (one each)", fn, lods->view_count, m, pool_id);
    for (uint32_t k = 0; lods && k < m; k++)
        if (!(lods->views[k].scale >= 0.0f) || !(lods->views[k].near_distance >= 0.0f))  // (negative or NaN)
            return ctx->fail(GV_E_ARG, "%s: LOD view %u has scale %g and near_distance %g (neither negative nor NaN)", fn, k,
                             (double)lods->views[k].scale, (double)lods->views[k].near_distance);
    if ((uint64_t)m * region_commands > UINT32_MAX)
        return ctx->fail(GV_E_ARG, "%s: %u regions of %u commands are more positions than 32 bits hold", fn, m, region_commands);
    const bool frustum_only = (flags & GV_CLUSTERS_FRUSTUM_ONLY) != 0;
    uint64_t slots = 0;  // the sum of the listed views' occupancies
    for (uint32_t k = 0; k < m; k++) {
        const ViewState* vs = view_of(ctx, pool_id, I.listed[k]);
        if (!vs)
            return ctx->fail(GV_E_STATE, "%s: pool %u view %u has no results", fn, pool_id, I.listed[k]);
        if (int rc = column_covers(ctx, fn, kGeometryIds, pool_id, G.ids, G.occupancy, *vs, I.listed[k]))
            return rc;
        if (!frustum_only && vs->use_hiz && !ctx->pyramid_built(Context::pyramid_of(vs->use_hiz)))
            return ctx->fail(GV_E_STATE, "%s: view %u of pool %u names pyramid %u, which is not built (gv_hiz_build, or "
                             "GV_CLUSTERS_FRUSTUM_ONLY)", fn, I.listed[k], pool_id, Context::pyramid_of(vs->use_hiz));
        slots += vs->occupancy;
    }
    // the host's bound of the candidates: a view draws a slot at most once, a draw has at most max(1, the largest range) candidates
    const uint64_t bound = slots * std::max(1u, K.max_range);
    if (bound > UINT32_MAX)
        return ctx->fail(GV_E_STATE, "%s: %llu slots of pool %u with up to %u clusters each may be %llu candidates, more than "
                         "32 bits hold: cull fewer views per emission", fn, (unsigned long long)slots, pool_id, K.max_range, (unsigned long long)bound);
    const uint64_t positions = region_commands ? (uint64_t)m * region_commands : bound;
    if (!dst_device && positions * L.stride > kOwnTargetMaxBytes)
        return ctx->fail(GV_E_STATE, "%s: pool %u may emit %llu commands of %u bytes, more than a library-owned target holds: "
                         "pass a caller-owned target (dst_device) sized for what is drawn", fn, pool_id, (unsigned long long)positions, L.stride);
    ZoneScope zone(zone_name);
    if (int rc = flush_sorts(ctx))  // the call is a read: recorded culls and deferred sorts first (as the emissions)
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    const bool selected = p.lod.views != 0;  // behind a LOD selection the ids are the selected ones, per draw (as the command emission)
    if (int rc = selected ? GV_OK : want_column(ctx, p, G.ids, G, upload_geometry))  // marks made since the cull are seen by this call
        return rc;
    ClusterLaunch launch{};
    for (uint32_t k = 0; k < m; k++) {
        const ViewState& vs = *view_of(ctx, pool_id, I.listed[k]);
        const ViewRecords r = records_of(vs);
        launch.view[k] = ClusterView{r.count, r.idx, r.model};
        launch.first_block[k + 1] = launch.first_block[k] + (vs.occupancy + kClusterBlock - 1) / kClusterBlock;
        memcpy(launch.planes[k], vs.planes, sizeof(vs.planes));
        launch.plane_count[k] = vs.plane_count;
        memcpy(launch.vp[k], vs.view_proj, sizeof(vs.view_proj));
        if (!frustum_only && vs.use_hiz) {
            launch.hiz[k] = hiz_device(ctx, Context::pyramid_of(vs.use_hiz));  // the pyramid as it stands now
            launch.hiz_views |= 1u << k;
        }
    }
    for (uint32_t k = m; k < kMaxInstanceViews; k++)
        launch.first_block[k + 1] = launch.first_block[m];
    launch.views = m;
    launch.region = region_commands;
    launch.stride = L.stride;
    launch.count = L.count;
    launch.instance_count = L.instance_count;
    launch.first = L.first;
    launch.first_instance = L.first_instance;
    launch.vertex_offset = L.vertex_offset;
    launch.draw = L.draw;
    launch.ids = G.ids.ptr && !selected ? G.d_column.ptr : nullptr;
    launch.draw_ids = selected ? p.lod.d_draw_geometry.ptr : nullptr;
    launch.table = reinterpret_cast<const CommandGeometry*>(G.d_table.ptr);
    launch.table_count = G.table_count;
    launch.ranges = reinterpret_cast<const ClusterRange*>(K.d_ranges.ptr);
    launch.range_count = K.range_count;
    launch.clusters = reinterpret_cast<const float4*>(K.d_clusters.ptr);
    launch.starts = I.d_starts.ptr;
    launch.first_instance_of = I.draws ? I.d_first.ptr : nullptr;
    launch.draw_starts = I.draws ? I.d_draw_starts.ptr : nullptr;
    if (int rc = choose_target(ctx, dst_device, capacity_bytes, L.stride, positions, K.d_data, &launch.dst, &launch.capacity))
        return rc;
    const size_t blocks = launch.first_block[m], draws = blocks * kClusterBlock;
    const size_t tiles = (size_t)((bound + kClusterTile - 1) / kClusterTile);
    GV_HIP(ctx, K.d_counts.reserve(2 * GV_MAX_VIEWS));
    GV_HIP(ctx, K.d_draw_geometry.reserve(std::max<size_t>(draws, 1)));
    GV_HIP(ctx, K.d_draw_local.reserve(std::max<size_t>(draws, 1)));
    GV_HIP(ctx, K.d_block_total.reserve(std::max<size_t>(blocks, 4)));
    GV_HIP(ctx, K.d_block_tested.reserve(std::max<size_t>(blocks, 4)));
    GV_HIP(ctx, K.d_totals.reserve(kClusterTotalWords));
    GV_HIP(ctx, K.d_tile_count.reserve(std::max<size_t>(tiles, 4)));
    GV_HIP(ctx, K.d_tile_block.reserve(std::max<size_t>(tiles, 1)));
    GV_HIP(ctx, K.d_survive.reserve(std::max<size_t>(tiles, 1) * (kClusterTile / 64)));
    launch.draw_geometry = K.d_draw_geometry.ptr;
    launch.draw_local = K.d_draw_local.ptr;
    launch.block_total = K.d_block_total.ptr;
    launch.block_tested = K.d_block_tested.ptr;
    launch.totals = K.d_totals.ptr;
    launch.tile_count = K.d_tile_count.ptr;
    launch.tile_block = K.d_tile_block.ptr;
    launch.survive = K.d_survive.ptr;
    launch.counts = K.d_counts.ptr;
    if (int rc = enqueue(ctx, K, launch, tiles, cones ? cones->eyes : nullptr, lods ? lods->views : nullptr))
        return rc;
    K.second_test = forms.second_test;  // (cones: the second phase behind this result applies the same conjunction, with these eyes)
    if (cones)
        memcpy(K.eyes, cones->eyes, (size_t)m * sizeof(GvClusterEye));
    if (lods)
        memcpy(K.lod_views, lods->views, (size_t)m * sizeof(GvClusterLodView));
    K.second.views = 0;  // the bits and prefixes a second phase read are replaced
    K.launch = launch;   // gv_pool_cull_clusters_second_phase tests with the same arguments
    K.candidate_bound = bound;
    for (uint32_t k = 0; k < m; k++)
        K.pyramid[k] = Context::pyramid_of(view_of(ctx, pool_id, I.listed[k])->use_hiz);
    K.rebound = false;
    K.target = launch.dst;
    K.capacity = launch.capacity;
    K.views = m;
    K.stride = L.stride;
    K.region = region_commands;
    return GV_OK;
}

}  // namespace gv

extern "C" {

int gv_pool_bind_clusters(GvCtx* ctx, uint32_t pool_id, const GvClusterRange* ranges, uint32_t range_count, const GvCluster* clusters,
                          uint32_t cluster_count)
{
    static_assert(sizeof(GvCluster) == sizeof(ClusterEntry) && sizeof(GvCluster) == 32, "the kernels read a cluster as two 16-byte pieces");
    static_assert(sizeof(GvClusterRange) == sizeof(ClusterRange) && sizeof(GvClusterRange) == 8, "the kernels read the ranges as they are bound");
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_clusters: pool %u out of range", pool_id);
    const bool none = !ranges && !range_count && !clusters && !cluster_count;
    if (!none && (!ranges || !range_count || !clusters || !cluster_count))
        return ctx->fail(GV_E_ARG, "gv_pool_bind_clusters: ranges %p with %u entries, clusters %p with %u entries (both tables, or NULL and 0 for "
                         "both to remove the binding)", (const void*)ranges, range_count, (const void*)clusters, cluster_count);
    if (range_count > GV_MAX_GEOMETRIES || cluster_count > GV_MAX_CLUSTERS)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_clusters: %u ranges (at most %u) and %u clusters (at most %u)", range_count, GV_MAX_GEOMETRIES,
                         cluster_count, GV_MAX_CLUSTERS);
    uint32_t max_range = 0;
    for (uint32_t g = 0; g < range_count; g++) {
        if (ranges[g].count > GV_MAX_GEOMETRY_CLUSTERS || (uint64_t)ranges[g].first + ranges[g].count > cluster_count)
            return ctx->fail(GV_E_ARG, "gv_pool_bind_clusters: range %u = {first %u, count %u}: at most %u clusters, inside the table of %u", g,
                             ranges[g].first, ranges[g].count, GV_MAX_GEOMETRY_CLUSTERS, cluster_count);
        max_range = std::max(max_range, ranges[g].count);
    }
    PoolState::Clusters& K = ctx->pools[pool_id].clusters;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the stream may still be reading the tables)
    K.views = 0;  // a result made from the tables as they were ends
    K.second.views = 0;
    K.bound = false;
    K.range_count = K.cluster_count = K.max_range = 0;
    K.cones_bound = false;  // the cones belong to the table as it was
    K.d_cones.release();
    K.lods_bound = false;  // ... and so does the LOD table
    K.d_lods.release();
    if (none) {
        K.d_ranges.release();
        K.d_clusters.release();
        return GV_OK;
    }
    GV_HIP(ctx, K.d_ranges.reserve(range_count));
    GV_HIP(ctx, K.d_clusters.reserve(cluster_count));
    GV_HIP(ctx, hipMemcpy(K.d_ranges.ptr, ranges, (size_t)range_count * sizeof(GvClusterRange), hipMemcpyHostToDevice));
    GV_HIP(ctx, hipMemcpy(K.d_clusters.ptr, clusters, (size_t)cluster_count * sizeof(GvCluster), hipMemcpyHostToDevice));
    ctx->stats.upload_bytes += (size_t)range_count * sizeof(GvClusterRange) + (size_t)cluster_count * sizeof(GvCluster);
    K.bound = true;
    K.range_count = range_count;
    K.cluster_count = cluster_count;
    K.max_range = max_range;
    return GV_OK;
}

int gv_pool_cull_clusters(GvCtx* ctx, uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device, size_t capacity_bytes)
{
    return cull_clusters(ctx, "gv_pool_cull_clusters", ClusterCullForms{write_survivors, nullptr, nullptr}, GV_CLUSTERS_FRUSTUM_ONLY, nullptr, "Meshes Cluster Cull",
                         pool_id, flags, region_commands, dst_device, capacity_bytes);
}

int gv_pool_cluster_commands_device(GvCtx* ctx, uint32_t pool_id, const void** commands, const void** counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !commands || !counts)
        return ctx->fail(GV_E_ARG, "gv_pool_cluster_commands_device: bad argument (pool %u)", pool_id);
    const PoolState::Clusters& K = ctx->pools[pool_id].clusters;
    if (!K.views)
        return ctx->fail(GV_E_STATE, "gv_pool_cluster_commands_device: pool %u has no cluster commands since its last gv_cull, instance emission "
                         "or gv_pool_bind_clusters", pool_id);
    *commands = K.target;
    *counts = K.d_counts.ptr;
    return GV_OK;
}

int gv_pool_cluster_commands_fetch(GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* counts, uint32_t counts_capacity)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !counts)
        return ctx->fail(GV_E_ARG, "gv_pool_cluster_commands_fetch: bad argument (pool %u)", pool_id);
    PoolState::Clusters& K = ctx->pools[pool_id].clusters;
    if (!K.views)
        return ctx->fail(GV_E_STATE, "gv_pool_cluster_commands_fetch: pool %u has no cluster commands since its last gv_cull, instance emission "
                         "or gv_pool_bind_clusters", pool_id);
    if (counts_capacity < 2 * K.views)
        return ctx->fail(GV_E_ARG, "gv_pool_cluster_commands_fetch: room for %u counts, the call listed %u views (two counts each)", counts_capacity,
                         K.views);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_staged(ctx, K.h_counts, 2 * GV_MAX_VIEWS, K.d_counts.ptr, 2 * K.views))
        return rc;
    uint64_t positions = (uint64_t)K.views * K.region;
    if (!K.region)
        for (uint32_t k = 0; k < K.views; k++)
            positions += K.h_counts.ptr[k];
    const size_t held = (size_t)std::min<uint64_t>(positions, K.capacity);  // (a caller-owned device target may have been too small for the rest)
    if (dst_host && bytes < held * K.stride)
        return ctx->fail(GV_E_ARG, "gv_pool_cluster_commands_fetch: %zu bytes for %zu commands of %u bytes", bytes, held, K.stride);
    memcpy(counts, K.h_counts.ptr, 2 * K.views * sizeof(uint32_t));
    if (!dst_host || !held)
        return GV_OK;
    return fetch_staged(ctx, K.h_data, held * K.stride, K.target, held * K.stride, dst_host);
}

}  // extern "C"
