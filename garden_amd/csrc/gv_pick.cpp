// gv_pick.cpp — gv_pick of include/garden_vis.h: the editor's click selection (MeshSelectorEditorSystem::render,
// editor/system/render/mesh-selector.cpp:67-122) over the device mirror. One pick_kernel launch per listed pool into a key per
// ray, one small copy of the keys to pinned memory; the host decodes pool, slot and distance. Nothing a cull produced is touched.
#include "gv_ctx.hpp"

using namespace gv;

extern "C" {

int gv_pick(GvCtx* ctx, const uint32_t* pool_ids, uint32_t pool_count, const uint32_t* exclude_slots, const float camera_position[4],
            const GvPickRay* rays, uint32_t ray_count, GvPickHit* hits)
{
    static_assert(GV_MAX_PICK_RAYS == kPickMaxRays, "one key per ray in the kernel");
    static_assert(GV_MAX_POOLS <= 16u, "the pool's position in the list takes the top 4 bits of the key's low word");
    if (!ctx)
        return GV_E_ARG;
    if (ctx->cull_batching)
        return ctx->fail(GV_E_STATE, "gv_pick: called between gv_cull_batch_begin and gv_cull_batch_end");
    if (!rays || !hits || !camera_position || ray_count == 0 || ray_count > GV_MAX_PICK_RAYS || pool_count > GV_MAX_POOLS ||
        (pool_count && !pool_ids))
        return ctx->fail(GV_E_ARG, "gv_pick: bad argument (%u rays, %u pools)", ray_count, pool_count);
    for (uint32_t k = 0; k < pool_count; k++) {
        if (pool_ids[k] >= GV_MAX_POOLS || !ctx->pools[pool_ids[k]].bound)
            return ctx->fail(GV_E_ARG, "gv_pick: pool %u is not bound", pool_ids[k]);
        const PoolState& p = ctx->pools[pool_ids[k]];
        if (p.occupancy > kSlotMask)
            return ctx->fail(GV_E_ARG, "gv_pick: pool %u has %u slots (2^28 at the most)", pool_ids[k], p.occupancy);
        if (p.index_map_count) {
            if (p.index_map_count < p.occupancy)
                return ctx->fail(GV_E_STATE, "gv_pick: the index map of pool %u covers %u of its %u slots", pool_ids[k], p.index_map_count,
                                 p.occupancy);
            if (p.index_map_wide)  // (counted when the map is set or updated, not here: a pick costs no pass over the table)
                return ctx->fail(GV_E_ARG, "gv_pick: the index map of pool %u names %u slots of 2^28 or more", pool_ids[k],
                                 p.index_map_wide);
        }
    }
    if (!ctx->xf.bound)
        return ctx->fail(GV_E_STATE, "gv_pick: no transforms bound");
    ZoneScope zone("Mesh Selector");
    if (int rc = sync_mirror(ctx))
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_HIP(ctx, ctx->d_pick_keys.reserve(kPickMaxRays));
    GV_HIP(ctx, ctx->h_pick_keys.reserve(kPickMaxRays));
    GV_HIP(ctx, hipMemsetAsync(ctx->d_pick_keys.ptr, 0xFF, ray_count * sizeof(unsigned long long), ctx->stream));
    PickLaunch launch{};
    for (int c = 0; c < 3; c++)
        launch.cam[c] = camera_position[c];
    for (uint32_t r = 0; r < ray_count; r++)
        for (int c = 0; c < 3; c++) {
            launch.ray[r][c] = rays[r].origin[c];
            launch.ray[r][3 + c] = rays[r].direction[c];
        }
    launch.rays = ray_count;
    launch.keys = ctx->d_pick_keys.ptr;
    const TransformMirror xf = xf_mirror(ctx);
    for (uint32_t k = 0; k < pool_count; k++) {
        const PoolState& p = ctx->pools[pool_ids[k]];
        launch.order_bits = k << 28;
        launch.exclude = exclude_slots ? exclude_slots[k] : GV_NONE;
        launch.index_map = p.index_map_count ? p.d_index_map.ptr : nullptr;
        GV_HIP(ctx, launch_pick(mesh_mirror(p), xf, launch, ctx->stream));
    }
    GV_HIP(ctx, hipMemcpyAsync(ctx->h_pick_keys.ptr, ctx->d_pick_keys.ptr, ray_count * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               ctx->stream));
    if (int rc = wait_for_stream(ctx))
        return rc;
    for (uint32_t r = 0; r < ray_count; r++) {
        const unsigned long long key = ctx->h_pick_keys.ptr[r];
        GvPickHit h{GV_NONE, GV_NONE, 0.0f, 0};
        if (key != ~0ull) {
            const uint32_t low = (uint32_t)key, bits = (uint32_t)(key >> 32);
            h.pool_id = pool_ids[low >> 28];
            h.slot = low & kSlotMask;
            memcpy(&h.distance_sq, &bits, 4);
        }
        hits[r] = h;
    }
    return GV_OK;
}

}  // extern "C"
