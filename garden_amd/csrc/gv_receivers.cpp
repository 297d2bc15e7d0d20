// gv_receivers.cpp — gv_receiver_begin / gv_pool_draw_receivers / gv_receiver_mask_device / gv_receiver_mask_fetch /
// gv_hiz_build_from_receivers of include/garden_vis.h: a receiver mask drawn on the device from the cull AABBs of the draws a view
// delivered, in the clip space of a matrix the caller names — what a shadow cascade's Hi-Z cull is held against
// so that casters whose shadows fall on nothing the main view sees are dropped. The boxes are the mesh mirror's, read through the slot
// -> entry table as they stand (as gv_pool_view_bounds): nothing is uploaded, there is no binding. The images and counts are the
// context's (Context::receiver_mask): accumulated state — end_derived has no line for them; a draw's scratch is the occluder draws'.
// Shared with the derived results (gv_ctx.hpp): the reader's checks and the staged fetch. Kernels: gv_receivers.hip.
#include "gv_ctx.hpp"

using namespace gv;

extern "C" {

int gv_receiver_begin(GvCtx* ctx, uint32_t width, uint32_t height)
{
    static_assert(sizeof(GvReceiverCounts) == sizeof(ReceiverCounts) && sizeof(GvReceiverCounts) == 24, "the kernel adds into the struct as it is fetched");
    if (!ctx)
        return GV_E_ARG;
    if (width == 0 || height == 0 || width > 32768 || height > 32768)
        return ctx->fail(GV_E_ARG, "gv_receiver_begin: bad image size %ux%u (1 to 32768 each)", width, height);
    Context::ReceiverMask& R = ctx->receiver_mask;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    // an image no pyramid reads: the one already in use if it is free, else the lowest free one (Context::free_image)
    const uint32_t take = ctx->free_image(R.d_image, R.current);
    const size_t texels = (size_t)width * height;
    GV_HIP(ctx, R.d_counts.reserve(1));
    // (a larger size replaces this image alone, behind whatever still reads it: hipFree waits; if that fails, the image is gone)
    if (const hipError_t e = R.d_image[take].reserve(texels); e != hipSuccess) {
        if (take == R.current)
            R.open = false, R.width = R.height = 0;
        return ctx->hip_fail(e, "gv_receiver_begin: the image");
    }
    GV_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(R.d_image[take].ptr), 0x7F800000, texels, ctx->stream));  // +inf: no receiver
    GV_HIP(ctx, hipMemsetAsync(R.d_counts.ptr, 0, sizeof(ReceiverCounts), ctx->stream));
    R.current = take;
    R.width = width;
    R.height = height;
    R.open = true;
    return GV_OK;
}

int gv_pool_draw_receivers(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, const float light_view_proj[16])
{
    if (!ctx)
        return GV_E_ARG;
    const char* const fn = "gv_pool_draw_receivers";
    if (!light_view_proj)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_receivers: light_view_proj is NULL");
    if (!bound_pool(ctx, fn, pool_id))
        return GV_E_ARG;
    if (view_index >= GV_MAX_VIEWS)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_receivers: view index %u is out of range", view_index);
    PoolState& p = ctx->pools[pool_id];
    Context::ReceiverMask& R = ctx->receiver_mask;
    Context::OccluderDepth& D = ctx->occluder_depth;  // (its scratch)
    const ViewState& vs = ctx->views[pool_id][view_index];
    if (!vs.valid && !vs.draw_count.ptr)  // (no cull of this pool has ever had such a view)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_receivers: %u is not a view of pool %u", view_index, pool_id);
    if (!vs.valid)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_receivers: pool %u view %u has no results", pool_id, view_index);
    if (!vs.emitted)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_receivers: pool %u view %u was culled count-only (emit_records == 0)", pool_id, view_index);
    if (!R.open)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_receivers: no open receiver mask (gv_receiver_begin)");
    ZoneScope zone("Receivers Draw");
    if (int rc = flush_sorts(ctx))  // the call is a read: recorded culls and deferred sorts first (as gv_pool_view_bounds)
        return rc;
    // every read stays inside buffers that cover the occupancy the view was culled with
    const uint32_t entries = (uint32_t)std::min<size_t>({(size_t)p.mirrored, p.d_a.cap, p.d_b.cap});
    const bool permuted = !p.inv.empty();
    const uint32_t slots = permuted ? (uint32_t)std::min<size_t>(p.inv.size(), p.d_inv.cap) : entries;
    if (entries < vs.occupancy || slots < vs.occupancy)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_receivers: the mirror of pool %u covers %u entries and %u slots of the %u view %u was culled with "
                         "(cull again first)", pool_id, entries, slots, vs.occupancy, view_index);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    const ViewRecords r = records_of(vs);
    ReceiverLaunch launch{};
    launch.count = r.count, launch.idx = r.idx, launch.model = r.model;
    launch.capacity = vs.occupancy;
    launch.a = p.d_a.ptr;
    launch.b = p.d_b.ptr;
    launch.inv = permuted ? p.d_inv.ptr : nullptr;
    launch.slots = slots;
    launch.entries = entries;
    memcpy(launch.light, light_view_proj, sizeof(launch.light));
    launch.width = R.width, launch.height = R.height;
    const size_t blocks = ((size_t)vs.occupancy + kReceiverBlock - 1) / kReceiverBlock;
    GV_HIP(ctx, D.d_local.reserve(std::max<size_t>(vs.occupancy, 1)));
    GV_HIP(ctx, D.d_base.reserve(blocks + 1));
    launch.local = D.d_local.ptr;
    launch.base = D.d_base.ptr;
    launch.counts = R.d_counts.ptr;
    launch.mask = R.d_image[R.current].ptr;
    OccluderLaunch scan{};  // (what occluder_scan_kernel reads: the count, its bound and base[])
    scan.count = r.count, scan.capacity = vs.occupancy, scan.base = D.d_base.ptr;
    GV_LAUNCH(ctx, GV_K_HIZ, launch_receiver_setup(launch, ctx->stream));
    GV_LAUNCH(ctx, GV_K_HIZ, launch_occluder_scan(scan, ctx->stream));
    GV_LAUNCH(ctx, GV_K_HIZ, launch_receiver_raster(launch, ctx->stream));
    return GV_OK;
}

int gv_receiver_mask_device(GvCtx* ctx, const void** mask, uint32_t* width, uint32_t* height, const void** counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (!mask || !width || !height || !counts)
        return ctx->fail(GV_E_ARG, "gv_receiver_mask_device: bad argument");
    const Context::ReceiverMask& R = ctx->receiver_mask;
    if (!R.width)
        return ctx->fail(GV_E_STATE, "gv_receiver_mask_device: no receiver mask (gv_receiver_begin)");
    *mask = R.d_image[R.current].ptr;
    *width = R.width;
    *height = R.height;
    *counts = R.d_counts.ptr;
    return GV_OK;
}

int gv_receiver_mask_fetch(GvCtx* ctx, float* mask, size_t bytes, GvReceiverCounts* counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (!mask && !counts)
        return ctx->fail(GV_E_ARG, "gv_receiver_mask_fetch: neither an image nor counts asked for");
    Context::ReceiverMask& R = ctx->receiver_mask;
    if (!R.width)
        return ctx->fail(GV_E_STATE, "gv_receiver_mask_fetch: no receiver mask (gv_receiver_begin)");
    const size_t texels = (size_t)R.width * R.height;
    if (mask && bytes < texels * sizeof(float))
        return ctx->fail(GV_E_ARG, "gv_receiver_mask_fetch: room for %zu bytes, the %ux%u image holds %zu", bytes, R.width, R.height, texels * sizeof(float));
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (counts)
        if (int rc = fetch_staged(ctx, R.h_counts, 1, R.d_counts.ptr, 1, counts))
            return rc;
    if (mask)
        return fetch_staged(ctx, R.h_image, texels, R.d_image[R.current].ptr, texels, mask);
    return GV_OK;
}

int gv_hiz_build_from_receivers(GvCtx* ctx)
{
    if (!ctx)
        return GV_E_ARG;
    Context::ReceiverMask& R = ctx->receiver_mask;
    if (!R.open)
        return ctx->fail(GV_E_STATE, "gv_hiz_build_from_receivers: no open receiver mask (gv_receiver_begin)");
    // (gv_hiz_build closes an image of the context's that it adopts: the pyramid reads it from here on, the next begin takes the other)
    return gv_hiz_build(ctx, R.d_image[R.current].ptr, R.width, R.height, GV_MEM_DEVICE);
}

}  // extern "C"
