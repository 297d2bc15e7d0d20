// gv_group.cpp — gv_pool_group_draws of include/garden_vis.h: the records of one view reordered by geometry key on the device, stable
// (DESIGN.md §4 item 12). The reorder goes where gv_pool_sort's goes — into the view's alternate record set, which is then swapped in
// (sort_records_of / swap_in_sorted of gv_results.cpp) — so that every later step that defines draw k as "record k in delivery order"
// composes with it unchanged. Keys, pairs and ranks use the view's sort scratch; the digit counts are a buffer of their own
// (ViewState::group_hist). The reader's checks are those of the derived results (gv_ctx.hpp). Kernels: gv_group.hip.
#include "gv_ctx.hpp"

using namespace gv;

extern "C" {

int gv_pool_group_draws(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t flags, float view_scale)
{
    if (!ctx)
        return GV_E_ARG;
    const char* const fn = "gv_pool_group_draws";
    if (!bound_pool(ctx, fn, pool_id))
        return GV_E_ARG;
    if (flags & ~GV_GROUP_BY_LOD)
        return ctx->fail(GV_E_ARG, "gv_pool_group_draws: unknown flags 0x%x", flags);
    if (!view_of(ctx, pool_id, view_index) || !view_of(ctx, pool_id, view_index)->emitted)
        return ctx->fail(GV_E_ARG, "gv_pool_group_draws: pool %u view %u has no emitted records", pool_id, view_index);
    PoolState& p = ctx->pools[pool_id];
    PoolState::Geometry& G = p.geometry;
    PoolState::Lod& S = p.lod;
    ViewState& vs = *view_of(ctx, pool_id, view_index);
    const bool by_lod = (flags & GV_GROUP_BY_LOD) != 0;
    if (!G.bound)
        return ctx->fail(GV_E_STATE, "gv_pool_group_draws: pool %u has no geometry bound (gv_pool_bind_geometry)", pool_id);
    if (by_lod && !S.bound)
        return ctx->fail(GV_E_STATE, "gv_pool_group_draws: GV_GROUP_BY_LOD and pool %u has no LOD table bound (gv_pool_bind_lod)", pool_id);
    if (int rc = column_covers(ctx, fn, kGeometryIds, pool_id, G.ids, G.occupancy, vs, view_index))
        return rc;
    if (int rc = by_lod ? column_covers(ctx, fn, kLodSizes, pool_id, S.sizes, S.occupancy, vs, view_index) : GV_OK)
        return rc;
    if (p.instances.views)  // group first, then emit: instance data written before the reorder would no longer match its draws
        return ctx->fail(GV_E_STATE, "gv_pool_group_draws: pool %u holds an instance emission since its last gv_cull", pool_id);
    if (!G.ids.ptr && !by_lod)  // every key is 0: the stable order is the order as it stands
        return GV_OK;
    ZoneScope zone("Meshes Group");
    if (int rc = flush_sorts(ctx))  // the grouping is a read: recorded culls and deferred sorts first (as the emissions)
        return rc;
    vs.sorted_dir = 0;  // no longer the distance order (gv_merge_sorted refuses the view; a later gv_pool_sort orders it again)
    if (vs.occupancy == 0)
        return GV_OK;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = want_column(ctx, p, G.ids, G, upload_geometry))  // marks made since the cull are seen by this call (as gv_pool_select_lods)
        return rc;
    if (int rc = by_lod ? want_column(ctx, p, S.sizes, S, upload_lod) : GV_OK)
        return rc;
    const uint32_t n = vs.occupancy;  // the host's bound of the draw count: sizes the scratch and the grids
    SortRecords r{};
    if (int rc = sort_records_of(ctx, vs, r))
        return rc;
    for (int k = 0; k < 2; k++) {
        GV_HIP(ctx, vs.sort_keys[k].reserve(n));
        GV_HIP(ctx, vs.sort_vals[k].reserve(n));
    }
    GV_HIP(ctx, vs.sort_ranks.reserve(n));
    GV_HIP(ctx, vs.group_hist.reserve(group_hist_words(n)));
    GroupLaunch launch{};
    launch.count = r.count;
    launch.capacity = n;
    launch.key_max = G.table_count;
    launch.idx_in = r.idx_in, launch.model_in = r.model_in, launch.dist_in = r.dist_in;
    launch.idx_out = r.idx_out, launch.model_out = r.model_out, launch.dist_out = r.dist_out;
    launch.ids = G.ids.ptr ? G.d_column.ptr : nullptr;
    launch.sizes = by_lod && S.sizes.ptr ? S.d_column.ptr : nullptr;
    launch.table = by_lod ? reinterpret_cast<const LodEntry*>(S.d_table.ptr) : nullptr;
    launch.lod_table_count = by_lod ? S.table_count : 0u;
    launch.by_lod = by_lod ? 1u : 0u;
    launch.scale = view_scale;
    launch.groups = group_group_count(n);
    for (int k = 0; k < 2; k++) {
        launch.keys[k] = vs.sort_keys[k].ptr;
        launch.vals[k] = vs.sort_vals[k].ptr;
    }
    launch.ranks = vs.sort_ranks.ptr;
    launch.group_hist = vs.group_hist.ptr;
    launch.tile_hist = vs.group_hist.ptr + group_counter_words(n);
    const uint32_t digits = group_digits(G.table_count);  // fixed by the host: never derived from a count read back
    GV_HIP(ctx, hipMemsetAsync(launch.group_hist, 0, (size_t)digits * launch.groups * 256u * sizeof(uint32_t), ctx->stream));
    GV_LAUNCH(ctx, GV_K_SORT, launch_group_keys(launch, ctx->stream));
    for (uint32_t pass = 0; pass < digits; pass++) {
        if (pass)
            GV_LAUNCH(ctx, GV_K_SORT, launch_group_rank(launch, pass, ctx->stream));
        GV_LAUNCH(ctx, GV_K_SORT, launch_group_scatter(launch, pass, pass + 1 == digits, ctx->stream));
    }
    swap_in_sorted(vs);  // the grouped records now live in what was the alternate set
    vs.published = false, vs.records_fetched = false;  // the next fetch delivers the new order
    return GV_OK;
}

}  // extern "C"
