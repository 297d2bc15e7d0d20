// gv_lod.cpp — gv_pool_bind_lod / gv_pool_select_lods / gv_pool_lods_device / gv_pool_lods_fetch of include/garden_vis.h: the level
// of detail of every draw of the pool's last instance emission, selected on the device from the delivered records, the geometry id
// mirror and a size per pool slot. The sizes are mirrored per pool slot (gv_mirror.cpp upload_lod); buffers
// of its own (PoolState::lod): neither the cull side nor the instance data is touched. A command emission behind the selection
// takes its ids (gv_commands.cpp). Shared with the other derived results (gv_ctx.hpp): the reader's checks, the staged fetch, and
// end_derived, which says what a dropped selection ends. Kernel: gv_lod.hip.
#include "gv_ctx.hpp"

using namespace gv;

extern "C" {

int gv_pool_bind_lod(GvCtx* ctx, uint32_t pool_id, const void* sizes, uint32_t stride, uint32_t occupancy, const GvLodGeometry* table,
                     uint32_t table_count)
{
    static_assert(sizeof(GvLodGeometry) == sizeof(LodEntry) && sizeof(GvLodGeometry) == 32, "the kernel reads the table as it is bound");
    static_assert(GV_MAX_LOD_LEVELS == kMaxLodLevels, "one histogram word per level");
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_lod: pool %u out of range", pool_id);
    if (sizes && stride < 4)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_lod: sizes every %u bytes (fp32: a stride of at least 4)", stride);
    if ((!table && table_count) || (table && !table_count) || (sizes && !table) || table_count > GV_MAX_GEOMETRIES)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_lod: table %p with %u entries (1 to %u; NULL and 0 together with NULL sizes remove the binding)",
                         (const void*)table, table_count, GV_MAX_GEOMETRIES);
    if (sizes && occupancy >= kSlotNone)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_lod: occupancy %u exceeds the 28-bit slot range", occupancy);
    for (uint32_t g = 0; g < table_count; g++)
        if (table[g].levels < 1 || table[g].levels > GV_MAX_LOD_LEVELS)
            return ctx->fail(GV_E_ARG, "gv_pool_bind_lod: entry %u has %u levels (1 to %u)", g, table[g].levels, GV_MAX_LOD_LEVELS);
    PoolState::Lod& S = ctx->pools[pool_id].lod;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the stream may still be reading the table or the mirror)
    S.reset();
    S.sizes = Column{static_cast<const uint8_t*>(sizes), sizes ? stride : 0};
    S.occupancy = sizes ? occupancy : 0;
    S.table_count = table_count;
    S.bound = table != nullptr;
    if (!sizes) {  // no column: no mirror
        S.wanted = false;
        S.SlotMirror::release();
        S.staged.pending = false;
    }
    if (!table) {
        S.d_table.release();
        end_derived(ctx, ctx->pools[pool_id], Ends::SelectionDropped);  // (a selection needs its binding: a command emission goes back to the id mirror)
        return GV_OK;
    }
    GV_HIP(ctx, S.d_table.reserve(table_count));
    GV_HIP(ctx, hipMemcpy(S.d_table.ptr, table, (size_t)table_count * sizeof(GvLodGeometry), hipMemcpyHostToDevice));
    ctx->stats.upload_bytes += (size_t)table_count * sizeof(GvLodGeometry);
    return GV_OK;
}

int gv_pool_select_lods(GvCtx* ctx, uint32_t pool_id, const float* view_scale, uint32_t view_count)
{
    if (!ctx)
        return GV_E_ARG;
    const char* const fn = "gv_pool_select_lods";
    if (!bound_pool(ctx, fn, pool_id))
        return GV_E_ARG;
    PoolState& p = ctx->pools[pool_id];
    PoolState::Instances& I = p.instances;
    PoolState::Geometry& G = p.geometry;
    PoolState::Lod& S = p.lod;
    if (!view_scale && !view_count) {  // dropped: a command emission takes the id mirror again
        end_derived(ctx, p, Ends::SelectionDropped);
        return GV_OK;
    }
    if (!view_scale)
        return ctx->fail(GV_E_ARG, "gv_pool_select_lods: no view_scale for %u views", view_count);
    if (!S.bound)
        return ctx->fail(GV_E_STATE, "gv_pool_select_lods: pool %u has no LOD table bound (gv_pool_bind_lod)", pool_id);
    if (!G.bound)
        return ctx->fail(GV_E_STATE, "gv_pool_select_lods: pool %u has no geometry bound (gv_pool_bind_geometry)", pool_id);
    if (!I.views)
        return ctx->fail(GV_E_STATE, "gv_pool_select_lods: pool %u has no instance emission since its last gv_cull", pool_id);
    const uint32_t m = I.views;
    if (view_count != m)
        return ctx->fail(GV_E_ARG, "gv_pool_select_lods: %u scales, the emission of pool %u listed %u views", view_count, pool_id, m);
    for (uint32_t k = 0; k < m; k++) {
        const ViewState* vs = view_of(ctx, pool_id, I.listed[k]);
        if (!vs)
            return ctx->fail(GV_E_STATE, "gv_pool_select_lods: pool %u view %u has no results", pool_id, I.listed[k]);
        if (int rc = column_covers(ctx, fn, kGeometryIds, pool_id, G.ids, G.occupancy, *vs, I.listed[k]))
            return rc;
        if (int rc = column_covers(ctx, fn, kLodSizes, pool_id, S.sizes, S.occupancy, *vs, I.listed[k]))
            return rc;
    }
    ZoneScope zone("Meshes LODs");
    if (int rc = flush_sorts(ctx))  // the selection is a read: recorded culls and deferred sorts first (as the emissions)
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = want_column(ctx, p, G.ids, G, upload_geometry))  // marks made since the cull are seen by this selection
        return rc;
    if (int rc = want_column(ctx, p, S.sizes, S, upload_lod))
        return rc;
    LodLaunch launch{};
    uint64_t slots = 0;  // the sum of the listed views' occupancies: the host's upper bound of the draws
    for (uint32_t k = 0; k < m; k++) {
        const ViewState& vs = *view_of(ctx, pool_id, I.listed[k]);
        const ViewRecords r = records_of(vs);
        launch.view[k] = LodView{r.count, r.idx, r.model, view_scale[k]};
        launch.first_block[k + 1] = launch.first_block[k] + (vs.occupancy + kLodBlock - 1) / kLodBlock;
        slots += vs.occupancy;
    }
    launch.views = m;
    launch.ids = G.ids.ptr ? G.d_column.ptr : nullptr;
    launch.sizes = S.sizes.ptr ? S.d_column.ptr : nullptr;
    launch.table = reinterpret_cast<const LodEntry*>(S.d_table.ptr);
    launch.table_count = S.table_count;
    GV_HIP(ctx, S.d_draw_geometry.reserve(std::max<size_t>((size_t)slots, 1)));
    GV_HIP(ctx, S.d_level_counts.reserve(GV_MAX_VIEWS * GV_MAX_LOD_LEVELS));
    launch.draw_geometry = S.d_draw_geometry.ptr;
    launch.level_counts = S.d_level_counts.ptr;
    GV_HIP(ctx, hipMemsetAsync(S.d_level_counts.ptr, 0, GV_MAX_VIEWS * GV_MAX_LOD_LEVELS * sizeof(uint32_t), ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_lod(launch, ctx->stream));
    S.views = m;
    return GV_OK;
}

int gv_pool_lods_device(GvCtx* ctx, uint32_t pool_id, const void** draw_geometry, const void** level_counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !draw_geometry || !level_counts)
        return ctx->fail(GV_E_ARG, "gv_pool_lods_device: bad argument (pool %u)", pool_id);
    const PoolState::Lod& S = ctx->pools[pool_id].lod;
    if (!S.views)
        return ctx->fail(GV_E_STATE, "gv_pool_lods_device: pool %u holds no selection since its last gv_cull or instance emission", pool_id);
    *draw_geometry = S.d_draw_geometry.ptr;
    *level_counts = S.d_level_counts.ptr;
    return GV_OK;
}

int gv_pool_lods_fetch(GvCtx* ctx, uint32_t pool_id, uint32_t* draw_geometry, uint32_t capacity, uint32_t* level_counts, uint32_t counts_capacity)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !level_counts)
        return ctx->fail(GV_E_ARG, "gv_pool_lods_fetch: bad argument (pool %u)", pool_id);
    PoolState::Lod& S = ctx->pools[pool_id].lod;
    if (!S.views)
        return ctx->fail(GV_E_STATE, "gv_pool_lods_fetch: pool %u holds no selection since its last gv_cull or instance emission", pool_id);
    const uint32_t words = S.views * GV_MAX_LOD_LEVELS;
    if (counts_capacity < words)
        return ctx->fail(GV_E_ARG, "gv_pool_lods_fetch: room for %u counts, the selection holds %u views of %u levels", counts_capacity, S.views,
                         GV_MAX_LOD_LEVELS);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_staged(ctx, S.h_level_counts, GV_MAX_VIEWS * GV_MAX_LOD_LEVELS, S.d_level_counts.ptr, words))
        return rc;
    uint64_t draws = 0;  // every draw is counted at exactly one level
    for (uint32_t w = 0; w < words; w++)
        draws += S.h_level_counts.ptr[w];
    if (draw_geometry && capacity < draws)
        return ctx->fail(GV_E_ARG, "gv_pool_lods_fetch: room for %u ids, the selection holds %llu draws", capacity, (unsigned long long)draws);
    memcpy(level_counts, S.h_level_counts.ptr, words * sizeof(uint32_t));
    if (!draw_geometry || !draws)
        return GV_OK;
    return fetch_staged(ctx, S.h_draw_geometry, (size_t)draws, S.d_draw_geometry.ptr, (size_t)draws, draw_geometry);
}

}  // extern "C"
