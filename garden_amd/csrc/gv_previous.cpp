// gv_previous.cpp — gv_pool_keep_models / gv_pool_forget_models / gv_pool_emit_previous / gv_pool_previous_device /
// gv_pool_previous_fetch of include/garden_vis.h: last frame's viewProj * model per draw, the second matrix per instance that a velocity
// pass needs for objects that move. The models a view delivered are kept per POOL slot on the device
// (PoolState::models: history, like the delta baselines — end_derived has no line for it) and joined to the next frame's draws there;
// the host never reads a count, a slot or a model. The answer (PoolState::previous) is made from a view and ends with it. The checks,
// the target choice and the fetch it shares with the derived results are gv_ctx.hpp's. Kernels: gv_previous.hip.
#include "gv_ctx.hpp"

using namespace gv;

namespace {

// What the three calls that read a view check alike, in the order of the header's error list; *out: the view, delivered with records.
int delivered_view(GvCtx* ctx, const char* fn, uint32_t pool_id, uint32_t view_index, uint32_t flags, uint32_t known_flags, const ViewState** out)
{
    if (!bound_pool(ctx, fn, pool_id))
        return GV_E_ARG;
    if (view_index >= GV_MAX_VIEWS)
        return ctx->fail(GV_E_ARG, "%s: view index %u is out of range", fn, view_index);
    const ViewState& vs = ctx->views[pool_id][view_index];
    if (!vs.valid && !vs.draw_count.ptr)  // (no cull of this pool has ever had such a view)
        return ctx->fail(GV_E_ARG, "%s: %u is not a view of pool %u", fn, view_index, pool_id);
    if (flags & ~known_flags)
        return ctx->fail(GV_E_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~known_flags);
    *out = &vs;
    return GV_OK;
}
int has_records(GvCtx* ctx, const char* fn, uint32_t pool_id, uint32_t view_index, const ViewState& vs)
{
    if (!vs.valid)
        return ctx->fail(GV_E_STATE, "%s: pool %u view %u has no results", fn, pool_id, view_index);
    if (!vs.emitted)
        return ctx->fail(GV_E_STATE, "%s: pool %u view %u was culled count-only (emit_records == 0)", fn, pool_id, view_index);
    return GV_OK;
}
// every read of a record stays inside buffers that cover the occupancy the view was culled with
int records_cover(GvCtx* ctx, const char* fn, uint32_t pool_id, uint32_t view_index, const ViewState& vs)
{
    if (vs.visible_idx.cap < vs.occupancy || vs.baked_model.cap < (size_t)vs.occupancy * 12 || !vs.draw_count.ptr)
        return ctx->fail(GV_E_STATE, "%s: the records of pool %u view %u do not cover its %u slots", fn, pool_id, view_index, vs.occupancy);
    return GV_OK;
}
PreviousView previous_view(const ViewState& vs)
{
    const ViewRecords r = records_of(vs);
    return PreviousView{r.count, r.idx, r.model, vs.occupancy};
}

bool layout_fits(const GvPreviousLayout& L)
{
    if (L.stride % 16 != 0 || L.stride < kMinPreviousStride || L.stride > kMaxPreviousStride)
        return false;
    if (L.prev_mvp % 16 != 0 || L.prev_mvp > L.stride || L.stride - L.prev_mvp < 64)
        return false;
    if (L.has_history == GV_NONE)
        return true;
    if (L.has_history % 4 != 0 || L.has_history > L.stride - 4)
        return false;
    return L.has_history + 4 <= L.prev_mvp || L.has_history >= L.prev_mvp + 64;
}

}  // namespace

extern "C" {

int gv_pool_keep_models(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t flags)
{
    static_assert(sizeof(float4) * kPreviousRowPieces == kPreviousRowBytes, "a row is four 16-byte pieces");
    if (!ctx)
        return GV_E_ARG;
    const char* const fn = "gv_pool_keep_models";
    const ViewState* view = nullptr;
    if (int rc = delivered_view(ctx, fn, pool_id, view_index, flags, GV_KEEP_ADD, &view))
        return rc;
    const ViewState& vs = *view;
    if (int rc = has_records(ctx, fn, pool_id, view_index, vs))
        return rc;
    PoolState::Models& H = ctx->pools[pool_id].models;
    const bool add = (flags & GV_KEEP_ADD) != 0;
    if (add && H.epoch == 0)
        return ctx->fail(GV_E_STATE, "gv_pool_keep_models: GV_KEEP_ADD into the empty history of pool %u (keep the first view without it)", pool_id);
    if (add && (memcmp(H.view_proj, vs.view_proj, sizeof(H.view_proj)) != 0 || memcmp(H.camera_position, vs.camera_position, sizeof(H.camera_position)) != 0))
        return ctx->fail(GV_E_STATE, "gv_pool_keep_models: GV_KEEP_ADD of pool %u view %u, whose view_proj and camera_position are not the kept "
                         "ones bit for bit", pool_id, view_index);
    ZoneScope zone("Meshes Keep Models");
    if (int rc = flush_sorts(ctx))  // the call is a read: recorded culls and deferred sorts first (as gv_pool_emit_instances)
        return rc;
    if (int rc = records_cover(ctx, fn, pool_id, view_index, vs))
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (vs.occupancy > H.slots) {  // the coverage grows: old rows survive, new rows have stamp 0 (which no epoch equals)
        GV_HIP(ctx, H.d_rows.grow((size_t)vs.occupancy * kPreviousRowPieces, (size_t)H.slots * kPreviousRowPieces, ctx->stream));
        GV_HIP(ctx, hipMemsetAsync(H.d_rows.ptr + (size_t)H.slots * kPreviousRowPieces, 0, (size_t)(vs.occupancy - H.slots) * kPreviousRowBytes,
                                   ctx->stream));
        H.slots = vs.occupancy;
    }
    uint32_t epoch = H.epoch;
    if (!add) {
        if (epoch == UINT32_MAX) {  // e would wrap to 0, "empty": every stamp is cleared first and e becomes 1
            if (H.slots)
                GV_LAUNCH(ctx, GV_K_EMIT, launch_previous_forget(H.d_rows.ptr, 0, H.slots, ctx->stream));
            epoch = 0;
        }
        epoch++;
    }
    PreviousKeep launch{};
    launch.view = previous_view(vs);
    launch.rows = H.d_rows.ptr;
    launch.slots = H.slots;
    launch.epoch = epoch;
    GV_LAUNCH(ctx, GV_K_EMIT, launch_previous_keep(launch, ctx->stream));
    H.epoch = epoch;
    memcpy(H.view_proj, vs.view_proj, sizeof(H.view_proj));
    memcpy(H.camera_position, vs.camera_position, sizeof(H.camera_position));
    return GV_OK;
}

int gv_pool_forget_models(GvCtx* ctx, uint32_t pool_id, uint32_t first, uint32_t count)
{
    if (!ctx)
        return GV_E_ARG;
    if (!bound_pool(ctx, "gv_pool_forget_models", pool_id))
        return GV_E_ARG;
    PoolState::Models& H = ctx->pools[pool_id].models;
    if (count == 0) {  // the whole history (the convention of gv_pool_view_delta's drop call); the buffers stay for the next keep
        H.empty();
        return GV_OK;
    }
    const uint32_t lo = std::min(first, H.slots), hi = (uint32_t)std::min<uint64_t>((uint64_t)first + count, H.slots);
    if (hi <= lo)
        return GV_OK;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_previous_forget(H.d_rows.ptr, lo, hi - lo, ctx->stream));
    return GV_OK;
}

int gv_pool_emit_previous(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, const GvPreviousLayout* layout, const float* prev_view_proj,
                          uint32_t flags, void* dst_device, size_t capacity_bytes)
{
    static_assert(GV_NONE == kNoField, "an absent has_history is GV_NONE in the kernel's layout too");
    if (!ctx)
        return GV_E_ARG;
    const char* const fn = "gv_pool_emit_previous";
    const ViewState* view = nullptr;
    if (int rc = delivered_view(ctx, fn, pool_id, view_index, flags, GV_PREVIOUS_CUT, &view))
        return rc;
    const ViewState& vs = *view;
    const GvPreviousLayout L = layout ? *layout : GvPreviousLayout{64, 0, GV_NONE};
    if (!layout_fits(L))
        return ctx->fail(GV_E_ARG, "gv_pool_emit_previous: stride %u (a multiple of 16, %u to %u) with prev_mvp at %u (64 bytes, 16-byte aligned) "
                         "and has_history at %u (4-byte aligned, 0x%x: none): fields must lie inside the stride and be disjoint", L.stride,
                         kMinPreviousStride, kMaxPreviousStride, L.prev_mvp, L.has_history, GV_NONE);
    if (dst_device && (uintptr_t)dst_device % 16 != 0)
        return ctx->fail(GV_E_ARG, "gv_pool_emit_previous: dst_device must be 16-byte aligned");
    if (int rc = has_records(ctx, fn, pool_id, view_index, vs))
        return rc;
    PoolState& p = ctx->pools[pool_id];
    const PoolState::Models& H = p.models;
    PoolState::Previous& R = p.previous;
    ZoneScope zone("Meshes Previous");
    if (int rc = flush_sorts(ctx))  // the emission is a read: recorded culls and deferred sorts first (as gv_pool_emit_instances)
        return rc;
    if (int rc = records_cover(ctx, fn, pool_id, view_index, vs))
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    PreviousEmit launch{};
    launch.view = previous_view(vs);
    launch.report_epoch = H.epoch;
    const bool cut = (flags & GV_PREVIOUS_CUT) != 0 || H.epoch == 0;
    if (cut) {  // every draw is fresh against the view's own matrix: the bytes of gv_pool_emit_instances' mvp
        memcpy(launch.pvp, vs.view_proj, sizeof(launch.pvp));
    } else {
        memcpy(launch.pvp, prev_view_proj ? prev_view_proj : H.view_proj, sizeof(launch.pvp));
        for (int r = 0; r < 3; r++)
            launch.d[r] = vs.camera_position[r] - H.camera_position[r];
        launch.rows = H.d_rows.ptr;
        launch.slots = std::min<uint32_t>(H.slots, (uint32_t)std::min<size_t>(H.d_rows.cap / kPreviousRowPieces, UINT32_MAX));
        launch.epoch = H.epoch;
    }
    if ((!dst_device && R.d_data.cap < std::max<size_t>((size_t)vs.occupancy * L.stride, 16)) || R.d_counts.cap < 4)
        R.result = false;  // (the answer's buffers are about to be replaced: should that fail, the previous answer is gone)
    if (int rc = choose_target(ctx, dst_device, capacity_bytes, L.stride, vs.occupancy, R.d_data, &launch.dst, &launch.capacity))
        return rc;
    GV_HIP(ctx, R.d_counts.reserve(4));
    launch.stride = L.stride;
    launch.prev_mvp = L.prev_mvp;
    launch.has_history = L.has_history;
    launch.counts = R.d_counts.ptr;
    R.result = false;  // (a failed launch leaves no answer)
    GV_HIP(ctx, hipMemsetAsync(R.d_counts.ptr, 0, 4 * sizeof(uint32_t), ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_previous_emit(launch, ctx->stream));
    R.emitted = L;
    R.target = launch.dst;
    R.capacity = launch.capacity;
    R.result = true;
    return GV_OK;
}

int gv_pool_previous_device(GvCtx* ctx, uint32_t pool_id, const void** items, const void** counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (!bound_pool(ctx, "gv_pool_previous_device", pool_id))
        return GV_E_ARG;
    if (!items || !counts)
        return ctx->fail(GV_E_ARG, "gv_pool_previous_device: a NULL output (pool %u)", pool_id);
    const PoolState::Previous& R = ctx->pools[pool_id].previous;
    if (!R.result)
        return ctx->fail(GV_E_STATE, "gv_pool_previous_device: pool %u has no previous-frame data since its last gv_cull", pool_id);
    *items = R.target;
    *counts = R.d_counts.ptr;
    return GV_OK;
}

int gv_pool_previous_fetch(GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* counts4)
{
    if (!ctx)
        return GV_E_ARG;
    if (!bound_pool(ctx, "gv_pool_previous_fetch", pool_id))
        return GV_E_ARG;
    if (!counts4)
        return ctx->fail(GV_E_ARG, "gv_pool_previous_fetch: counts4 is NULL (pool %u)", pool_id);
    PoolState::Previous& R = ctx->pools[pool_id].previous;
    if (!R.result)
        return ctx->fail(GV_E_STATE, "gv_pool_previous_fetch: pool %u has no previous-frame data since its last gv_cull", pool_id);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_staged(ctx, R.h_counts, 4, R.d_counts.ptr, 4))
        return rc;
    const GvPreviousLayout L = R.emitted;
    const uint32_t written = std::min(R.h_counts.ptr[2], R.capacity);
    if (dst_host && bytes < (size_t)written * L.stride)
        return ctx->fail(GV_E_ARG, "gv_pool_previous_fetch: %zu bytes for %u items of %u bytes", bytes, written, L.stride);
    memcpy(counts4, R.h_counts.ptr, 4 * sizeof(uint32_t));
    if (!dst_host || !written)
        return GV_OK;
    // whole items into the library's pinned staging, then field by field into the caller's (pageable, never page-locked) array: the
    // bytes between the fields are the caller's and stay as they are
    if (int rc = fetch_staged(ctx, R.h_data, (size_t)written * L.stride, R.target, (size_t)written * L.stride))
        return rc;
    uint8_t* const to = static_cast<uint8_t*>(dst_host);
    const uint8_t* const from = R.h_data.ptr;
    parallel_ranges(0, written, [&](uint32_t a, uint32_t b) {
        for (uint32_t k = a; k < b; k++) {
            memcpy(to + (size_t)k * L.stride + L.prev_mvp, from + (size_t)k * L.stride + L.prev_mvp, 64);
            if (L.has_history != GV_NONE)
                memcpy(to + (size_t)k * L.stride + L.has_history, from + (size_t)k * L.stride + L.has_history, 4);
        }
    });
    return GV_OK;
}

}  // extern "C"
