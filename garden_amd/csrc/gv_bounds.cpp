// gv_bounds.cpp — gv_pool_view_bounds / gv_pool_view_bounds_device / gv_pool_view_bounds_fetch of include/garden_vis.h: the bounds of
// the draws a view delivered, in a basis the caller names — what fits a shadow cascade's depth range, or a
// camera's near / far, to what is actually visible. Read on the device from the delivered records, the box mirror and the slot ->
// entry table as they stand: nothing is uploaded, no mark is consumed, nothing any other call can observe changes. Buffers of its
// own (PoolState::bounds); the checks and the fetch it shares with the other derived results are gv_ctx.hpp's. Kernels: gv_bounds.hip.
#include "gv_ctx.hpp"

using namespace gv;

extern "C" {

int gv_pool_view_bounds(GvCtx* ctx, uint32_t pool_id, const uint32_t* view_indices, const float* bases, uint32_t item_count)
{
    static_assert(sizeof(GvViewBounds) == sizeof(BoundsResult) && sizeof(GvViewBounds) == 32, "the kernel stores the struct as it is fetched");
    static_assert(sizeof(BoundsPartial) == 32, "a partial row is two 16-byte stores");
    static_assert(GV_MAX_BOUNDS_ITEMS == kMaxBoundsItems, "one kernel argument per item");
    if (!ctx)
        return GV_E_ARG;
    if (!bound_pool(ctx, "gv_pool_view_bounds", pool_id))
        return GV_E_ARG;
    if (item_count == 0 || item_count > GV_MAX_BOUNDS_ITEMS || !view_indices || !bases)
        return ctx->fail(GV_E_ARG, "gv_pool_view_bounds: %u items (1 to %u) with view_indices %p and bases %p", item_count,
                         (uint32_t)GV_MAX_BOUNDS_ITEMS, (const void*)view_indices, (const void*)bases);
    PoolState& p = ctx->pools[pool_id];
    for (uint32_t i = 0; i < item_count; i++) {
        const uint32_t v = view_indices[i];
        if (v >= GV_MAX_VIEWS)
            return ctx->fail(GV_E_ARG, "gv_pool_view_bounds: view index %u is out of range", v);
        const ViewState& vs = ctx->views[pool_id][v];
        if (!vs.valid && !vs.draw_count.ptr)  // (no cull of this pool has ever had such a view)
            return ctx->fail(GV_E_ARG, "gv_pool_view_bounds: %u is not a view of pool %u", v, pool_id);
        if (!vs.valid)
            return ctx->fail(GV_E_STATE, "gv_pool_view_bounds: pool %u view %u has no results", pool_id, v);
        if (!vs.emitted)
            return ctx->fail(GV_E_STATE, "gv_pool_view_bounds: pool %u view %u was culled count-only (emit_records == 0)", pool_id, v);
    }
    ZoneScope zone("Meshes Bounds");
    if (int rc = flush_sorts(ctx))  // the call is a read: recorded culls and deferred sorts first (as gv_pool_select_lods)
        return rc;
    // every read stays inside buffers that cover the occupancy the views were culled with
    const uint32_t entries = (uint32_t)std::min<size_t>({(size_t)p.mirrored, p.d_a.cap, p.d_b.cap});
    const bool permuted = !p.inv.empty();
    const uint32_t slots = permuted ? (uint32_t)std::min<size_t>(p.inv.size(), p.d_inv.cap) : entries;
    BoundsLaunch launch{};
    for (uint32_t i = 0; i < item_count; i++) {
        const ViewState& vs = ctx->views[pool_id][view_indices[i]];
        if (entries < vs.occupancy || slots < vs.occupancy)
            return ctx->fail(GV_E_STATE, "gv_pool_view_bounds: the mirror of pool %u covers %u entries and %u slots of the %u view %u was culled with "
                             "(cull again first)", pool_id, entries, slots, vs.occupancy, view_indices[i]);
        const ViewRecords r = records_of(vs);
        BoundsItem& it = launch.item[i];
        it.count = r.count, it.idx = r.idx, it.model = r.model;
        it.capacity = vs.occupancy;
        memcpy(it.basis, bases + (size_t)12 * i, sizeof(it.basis));
        launch.first_block[i + 1] = launch.first_block[i] + (vs.occupancy + kBoundsRecords - 1) / kBoundsRecords;
    }
    for (uint32_t i = item_count; i < kMaxBoundsItems; i++)
        launch.first_block[i + 1] = launch.first_block[item_count];
    launch.items = item_count;
    launch.a = p.d_a.ptr;
    launch.b = p.d_b.ptr;
    launch.inv = permuted ? p.d_inv.ptr : nullptr;
    launch.slots = slots;
    launch.entries = entries;
    PoolState::Bounds& S = p.bounds;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_HIP(ctx, S.d_partial.reserve(std::max<size_t>(launch.first_block[item_count], 1)));
    GV_HIP(ctx, S.d_out.reserve(GV_MAX_BOUNDS_ITEMS));
    launch.partial = S.d_partial.ptr;
    launch.out = S.d_out.ptr;
    S.items = 0;  // (a failed launch leaves no result)
    GV_LAUNCH(ctx, GV_K_EMIT, launch_bounds_fold(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_bounds_finish(launch, ctx->stream));
    S.items = item_count;
    return GV_OK;
}

int gv_pool_view_bounds_device(GvCtx* ctx, uint32_t pool_id, const void** bounds, uint32_t* item_count)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !bounds || !item_count)
        return ctx->fail(GV_E_ARG, "gv_pool_view_bounds_device: bad argument (pool %u)", pool_id);
    const PoolState::Bounds& S = ctx->pools[pool_id].bounds;
    if (!S.items)
        return ctx->fail(GV_E_STATE, "gv_pool_view_bounds_device: pool %u holds no bounds since its last gv_cull", pool_id);
    *bounds = S.d_out.ptr;
    *item_count = S.items;
    return GV_OK;
}

int gv_pool_view_bounds_fetch(GvCtx* ctx, uint32_t pool_id, GvViewBounds* bounds, uint32_t capacity)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !bounds)
        return ctx->fail(GV_E_ARG, "gv_pool_view_bounds_fetch: bad argument (pool %u)", pool_id);
    PoolState::Bounds& S = ctx->pools[pool_id].bounds;
    if (!S.items)
        return ctx->fail(GV_E_STATE, "gv_pool_view_bounds_fetch: pool %u holds no bounds since its last gv_cull", pool_id);
    if (capacity < S.items)
        return ctx->fail(GV_E_ARG, "gv_pool_view_bounds_fetch: room for %u items, the pool holds %u", capacity, S.items);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    return fetch_staged(ctx, S.h_out, GV_MAX_BOUNDS_ITEMS, S.d_out.ptr, S.items, bounds);
}

}  // extern "C"
