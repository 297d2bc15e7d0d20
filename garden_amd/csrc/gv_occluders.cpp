// gv_occluders.cpp — gv_pool_bind_occluders / gv_occluder_begin / gv_pool_draw_occluders / gv_occluder_depth_device /
// gv_occluder_depth_fetch / gv_hiz_build_from_occluders of include/garden_vis.h: a depth image drawn on the device from the occluder
// boxes of the draws a view delivered, for the Hi-Z query of a frame whose renderer has drawn no depth yet, or
// that has no renderer. The boxes are mirrored per pool slot (gv_mirror.cpp upload_occluders); the images, counts and scratch are the
// context's (Context::occluder_depth): accumulated state — end_derived has no line for them. Shared with the derived results
// (gv_ctx.hpp): the reader's checks, the column rules and the staged fetch. Kernels: gv_occluders.hip.
#include "gv_ctx.hpp"

using namespace gv;

extern "C" {

int gv_pool_bind_occluders(GvCtx* ctx, uint32_t pool_id, const void* box_min, const void* box_max, uint32_t stride, uint32_t occupancy)
{
    static_assert(sizeof(GvOccluderCounts) == sizeof(OccluderCounts) && sizeof(GvOccluderCounts) == 24, "the kernel adds into the struct as it is fetched");
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_occluders: pool %u out of range", pool_id);
    if ((box_min == nullptr) != (box_max == nullptr))
        return ctx->fail(GV_E_ARG, "gv_pool_bind_occluders: box_min %p with box_max %p (both, or both NULL to remove the binding)", box_min, box_max);
    if (box_min && stride < 12)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_occluders: boxes every %u bytes (3 fp32: a stride of at least 12)", stride);
    if (box_min && occupancy >= kSlotNone)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_occluders: occupancy %u exceeds the 28-bit slot range", occupancy);
    PoolState::Occluders& O = ctx->pools[pool_id].occluders;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the stream may still be reading the mirror)
    O.reset();
    O.elem = kOccluderRowBytes;
    O.box_min = Column{static_cast<const uint8_t*>(box_min), box_min ? stride : 0};
    O.box_max = Column{static_cast<const uint8_t*>(box_max), box_max ? stride : 0};
    O.occupancy = box_min ? occupancy : 0;
    if (!box_min) {  // no column: no mirror
        O.wanted = false;
        O.SlotMirror::release();
        O.staged.pending = false;
    }
    return GV_OK;
}

int gv_occluder_begin(GvCtx* ctx, uint32_t width, uint32_t height)
{
    if (!ctx)
        return GV_E_ARG;
    if (width == 0 || height == 0 || width > 32768 || height > 32768)
        return ctx->fail(GV_E_ARG, "gv_occluder_begin: bad image size %ux%u (1 to 32768 each)", width, height);
    Context::OccluderDepth& D = ctx->occluder_depth;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    // an image no pyramid reads: the one already in use if it is free, else the lowest free one (Context::free_image)
    const uint32_t take = ctx->free_image(D.d_image, D.current);
    const size_t texels = (size_t)width * height;
    GV_HIP(ctx, D.d_counts.reserve(1));
    // (a larger size replaces this image alone, behind whatever still reads it: hipFree waits; if that fails, the image is gone)
    if (const hipError_t e = D.d_image[take].reserve(texels); e != hipSuccess) {
        if (take == D.current)
            D.open = false, D.width = D.height = 0;
        return ctx->hip_fail(e, "gv_occluder_begin: the image");
    }
    GV_HIP(ctx, hipMemsetAsync(D.d_image[take].ptr, 0, texels * sizeof(float), ctx->stream));
    GV_HIP(ctx, hipMemsetAsync(D.d_counts.ptr, 0, sizeof(OccluderCounts), ctx->stream));
    D.current = take;
    D.width = width;
    D.height = height;
    D.open = true;
    return GV_OK;
}

int gv_pool_draw_occluders(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t min_pixels)
{
    if (!ctx)
        return GV_E_ARG;
    const char* const fn = "gv_pool_draw_occluders";
    if (!bound_pool(ctx, fn, pool_id))
        return GV_E_ARG;
    if (view_index >= GV_MAX_VIEWS)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_occluders: view index %u is out of range", view_index);
    PoolState& p = ctx->pools[pool_id];
    PoolState::Occluders& O = p.occluders;
    Context::OccluderDepth& D = ctx->occluder_depth;
    const ViewState& vs = ctx->views[pool_id][view_index];
    if (!vs.valid && !vs.draw_count.ptr)  // (no cull of this pool has ever had such a view)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_occluders: %u is not a view of pool %u", view_index, pool_id);
    if (!vs.valid)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_occluders: pool %u view %u has no results", pool_id, view_index);
    if (!vs.emitted)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_occluders: pool %u view %u was culled count-only (emit_records == 0)", pool_id, view_index);
    if (!D.open)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_occluders: no open occluder image (gv_occluder_begin)");
    if (!O.box_min.ptr)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_occluders: pool %u has no occluder boxes bound (gv_pool_bind_occluders)", pool_id);
    if (int rc = column_covers(ctx, fn, kOccluderBoxes, pool_id, O.box_min, O.occupancy, vs, view_index))
        return rc;
    ZoneScope zone("Occluders Draw");
    if (int rc = flush_sorts(ctx))  // the call is a read: recorded culls and deferred sorts first (as gv_pool_view_bounds)
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = want_column(ctx, p, O.box_min, O, upload_occluders))  // marks made since the cull are seen by this draw
        return rc;
    const ViewRecords r = records_of(vs);
    OccluderLaunch launch{};
    launch.count = r.count, launch.idx = r.idx, launch.model = r.model;
    launch.capacity = vs.occupancy;
    launch.boxes = reinterpret_cast<const float4*>(O.d_column.ptr);
    launch.slots = (uint32_t)std::min<size_t>(O.mirrored, O.d_column.cap / kOccluderRowBytes);
    memcpy(launch.view_proj, vs.view_proj, sizeof(launch.view_proj));
    launch.width = D.width, launch.height = D.height, launch.min_pixels = min_pixels;
    const size_t blocks = ((size_t)vs.occupancy + kOccluderBlock - 1) / kOccluderBlock;
    GV_HIP(ctx, D.d_local.reserve(std::max<size_t>(vs.occupancy, 1)));
    GV_HIP(ctx, D.d_base.reserve(blocks + 1));
    launch.local = D.d_local.ptr;
    launch.base = D.d_base.ptr;
    launch.counts = D.d_counts.ptr;
    launch.depth = D.d_image[D.current].ptr;
    GV_LAUNCH(ctx, GV_K_HIZ, launch_occluder_setup(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_HIZ, launch_occluder_scan(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_HIZ, launch_occluder_raster(launch, ctx->stream));
    return GV_OK;
}

int gv_occluder_depth_device(GvCtx* ctx, const void** depth, uint32_t* width, uint32_t* height, const void** counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (!depth || !width || !height || !counts)
        return ctx->fail(GV_E_ARG, "gv_occluder_depth_device: bad argument");
    const Context::OccluderDepth& D = ctx->occluder_depth;
    if (!D.width)
        return ctx->fail(GV_E_STATE, "gv_occluder_depth_device: no occluder image (gv_occluder_begin)");
    *depth = D.d_image[D.current].ptr;
    *width = D.width;
    *height = D.height;
    *counts = D.d_counts.ptr;
    return GV_OK;
}

int gv_occluder_depth_fetch(GvCtx* ctx, float* depth, size_t bytes, GvOccluderCounts* counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (!depth && !counts)
        return ctx->fail(GV_E_ARG, "gv_occluder_depth_fetch: neither an image nor counts asked for");
    Context::OccluderDepth& D = ctx->occluder_depth;
    if (!D.width)
        return ctx->fail(GV_E_STATE, "gv_occluder_depth_fetch: no occluder image (gv_occluder_begin)");
    const size_t texels = (size_t)D.width * D.height;
    if (depth && bytes < texels * sizeof(float))
        return ctx->fail(GV_E_ARG, "gv_occluder_depth_fetch: room for %zu bytes, the %ux%u image holds %zu", bytes, D.width, D.height, texels * sizeof(float));
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (counts)
        if (int rc = fetch_staged(ctx, D.h_counts, 1, D.d_counts.ptr, 1, counts))
            return rc;
    if (depth)
        return fetch_staged(ctx, D.h_image, texels, D.d_image[D.current].ptr, texels, depth);
    return GV_OK;
}

int gv_hiz_build_from_occluders(GvCtx* ctx)
{
    if (!ctx)
        return GV_E_ARG;
    Context::OccluderDepth& D = ctx->occluder_depth;
    if (!D.open)
        return ctx->fail(GV_E_STATE, "gv_hiz_build_from_occluders: no open occluder image (gv_occluder_begin)");
    // (gv_hiz_build closes an image of the context's that it adopts: the pyramid reads it from here on, the next begin takes the other)
    return gv_hiz_build(ctx, D.d_image[D.current].ptr, D.width, D.height, GV_MEM_DEVICE);
}

}  // extern "C"
