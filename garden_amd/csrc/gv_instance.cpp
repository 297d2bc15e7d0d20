// gv_instance.cpp — gv_pool_set_instance_layout / gv_pool_emit_instances / gv_pool_instances_device / gv_pool_instances_fetch of
// include/garden_vis.h: the instance array the reference's draw loops fill (renderUnsorted / renderSorted, mesh.cpp:556-770, call
// drawAsync per draw, and every plugin starts with instanceData[instanceIndex].mvp = viewProj * model, sprite.cpp:107-108,122-126),
// made on the device from the records a cull left there. One instance_kernel launch per call; buffers of its own (PoolState::
// instances): the cull side is left as a read through gv_pool_results_device leaves it.
#include "gv_ctx.hpp"

using namespace gv;

namespace {

struct Field {
    uint32_t at, bytes, align;
};

// the layout's fields in the order mvp, model, slot, distance_sq; returns how many it has
uint32_t fields_of(const GvInstanceLayout& L, Field (&f)[4])
{
    uint32_t n = 0;
    f[n++] = Field{L.mvp, 64, 16};
    if (L.model != GV_NONE)
        f[n++] = Field{L.model, 48, 4};
    if (L.slot != GV_NONE)
        f[n++] = Field{L.slot, 4, 4};
    if (L.distance_sq != GV_NONE)
        f[n++] = Field{L.distance_sq, 4, 4};
    return n;
}

}  // namespace

extern "C" {

int gv_pool_set_instance_layout(GvCtx* ctx, uint32_t pool_id, const GvInstanceLayout* layout)
{
    static_assert(GV_MAX_VIEWS == kMaxInstanceViews, "one InstanceView per view of a cull");
    static_assert(GV_NONE == kNoField, "absent fields are GV_NONE in the kernel's layout too");
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_set_instance_layout: pool %u out of range", pool_id);
    GvInstanceLayout L{};
    if (layout) {
        L = *layout;
        Field f[4];
        const uint32_t n = fields_of(L, f);
        bool ok = L.stride % 16 == 0 && L.stride >= kMinInstanceStride && L.stride <= kMaxInstanceStride;
        for (uint32_t i = 0; ok && i < n; i++) {
            ok = f[i].at % f[i].align == 0 && f[i].at <= L.stride && f[i].bytes <= L.stride - f[i].at;
            for (uint32_t j = 0; ok && j < i; j++)
                ok = f[i].at + f[i].bytes <= f[j].at || f[j].at + f[j].bytes <= f[i].at;
        }
        if (!ok)
            return ctx->fail(GV_E_ARG, "gv_pool_set_instance_layout: stride %u (a multiple of 16, %u to %u) with mvp at %u (16-byte aligned) and "
                             "model / slot / distance_sq at %u / %u / %u (4-byte aligned, 0x%x: none): fields must lie inside the instance and "
                             "be disjoint", L.stride, kMinInstanceStride, kMaxInstanceStride, L.mvp, L.model, L.slot, L.distance_sq, GV_NONE);
    }
    ctx->pools[pool_id].instances.layout = L;  // read by the next emission; an emission already made keeps the layout it was made with
    return GV_OK;
}

int gv_pool_emit_instances(GvCtx* ctx, uint32_t pool_id, const uint32_t* view_indices, uint32_t view_count, void* dst_device,
                           size_t capacity_bytes)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !ctx->pools[pool_id].bound)
        return ctx->fail(GV_E_ARG, "gv_pool_emit_instances: pool %u is not bound", pool_id);
    PoolState& p = ctx->pools[pool_id];
    PoolState::Instances& I = p.instances;
    uint32_t culled = 0;
    while (culled < GV_MAX_VIEWS && ctx->views[pool_id][culled].valid)
        culled++;
    if (!view_indices || view_count == 0 || view_count > culled)
        return ctx->fail(GV_E_ARG, "gv_pool_emit_instances: %u views listed, the last gv_cull of pool %u had %u", view_count, pool_id, culled);
    if (dst_device && (uintptr_t)dst_device % 16 != 0)
        return ctx->fail(GV_E_ARG, "gv_pool_emit_instances: dst_device must be 16-byte aligned");
    uint32_t listed = 0;
    for (uint32_t k = 0; k < view_count; k++) {
        const uint32_t v = view_indices[k];
        if (v >= GV_MAX_VIEWS || ((listed >> v) & 1u))
            return ctx->fail(GV_E_ARG, "gv_pool_emit_instances: view index %u is out of range or listed twice", v);
        listed |= 1u << v;
    }
    const GvInstanceLayout L = I.layout;
    if (!L.stride)
        return ctx->fail(GV_E_STATE, "gv_pool_emit_instances: pool %u has no instance layout (gv_pool_set_instance_layout)", pool_id);
    for (uint32_t k = 0; k < view_count; k++) {
        const ViewState* vs = view_of(ctx, pool_id, view_indices[k]);
        if (!vs)
            return ctx->fail(GV_E_STATE, "gv_pool_emit_instances: pool %u view %u has no results", pool_id, view_indices[k]);
        if (!vs->emitted)
            return ctx->fail(GV_E_STATE, "gv_pool_emit_instances: pool %u view %u was culled count-only (emit_records == 0)", pool_id,
                             view_indices[k]);
        if (L.slot != GV_NONE && p.index_map_count && p.index_map_count < vs->occupancy)
            return ctx->fail(GV_E_STATE, "gv_pool_emit_instances: the index map of pool %u covers %u of its %u slots", pool_id, p.index_map_count,
                             vs->occupancy);
    }
    if (p.ready.ptr && p.ready_many_count)
        return ctx->fail(GV_E_STATE, "gv_pool_emit_instances: the ready column of pool %u holds %u live counts above 1: such a draw takes several "
                         "instances, and the instance index of draw k is k only while every draw takes one (ready counts of 0 / 1 work)",
                         pool_id, p.ready_many_count);
    ZoneScope zone("Meshes Instances");
    if (int rc = flush_sorts(ctx))  // the emission is a read: recorded culls and deferred sorts first (as gv_pool_results_device)
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    InstanceLaunch launch{};
    uint64_t bound = 0;  // the host's upper bound of the total
    for (uint32_t k = 0; k < view_count; k++) {
        const ViewState& vs = *view_of(ctx, pool_id, view_indices[k]);
        InstanceView& w = launch.view[k];
        w.count = vs.draw_count.ptr;
        w.idx = vs.visible_idx.ptr;
        w.model = vs.baked_model.ptr;
        w.dist = vs.distance_sq.ptr;
        memcpy(w.view_proj, vs.view_proj, sizeof(w.view_proj));
        launch.first_block[k + 1] = launch.first_block[k] + (vs.occupancy + kInstanceBlock - 1) / kInstanceBlock;
        bound += vs.occupancy;
    }
    launch.views = view_count;
    launch.stride = L.stride;
    launch.mvp = L.mvp;
    launch.model = L.model;
    launch.slot = L.slot;
    launch.distance_sq = L.distance_sq;
    launch.index_map = p.index_map_count ? p.d_index_map.ptr : nullptr;
    if (dst_device) {
        launch.dst = static_cast<uint8_t*>(dst_device);
        launch.capacity = (uint32_t)std::min<uint64_t>(capacity_bytes / L.stride, bound);
    } else {
        GV_HIP(ctx, I.d_data.reserve(std::max<size_t>((size_t)bound * L.stride, 16)));
        launch.dst = I.d_data.ptr;
        launch.capacity = (uint32_t)bound;
    }
    GV_HIP(ctx, I.d_starts.reserve(GV_MAX_VIEWS + 1));
    launch.starts = I.d_starts.ptr;
    GV_HIP(ctx, launch_instances(launch, ctx->stream));
    I.target = launch.dst;
    I.capacity = launch.capacity;
    I.views = view_count;
    I.emitted = L;
    return GV_OK;
}

int gv_pool_instances_device(GvCtx* ctx, uint32_t pool_id, const void** instances, const void** starts)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !instances || !starts)
        return ctx->fail(GV_E_ARG, "gv_pool_instances_device: bad argument (pool %u)", pool_id);
    const PoolState::Instances& I = ctx->pools[pool_id].instances;
    if (!I.views)
        return ctx->fail(GV_E_STATE, "gv_pool_instances_device: pool %u has no instance data since its last gv_cull", pool_id);
    *instances = I.target;
    *starts = I.d_starts.ptr;
    return GV_OK;
}

int gv_pool_instances_info(GvCtx* ctx, uint32_t pool_id, uint32_t* view_count, uint32_t* stride, uint32_t* capacity)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_instances_info: pool %u out of range", pool_id);
    const PoolState::Instances& I = ctx->pools[pool_id].instances;
    if (!I.views)
        return ctx->fail(GV_E_STATE, "gv_pool_instances_info: pool %u has no instance data since its last gv_cull", pool_id);
    if (view_count)
        *view_count = I.views;
    if (stride)
        *stride = I.emitted.stride;
    if (capacity)
        *capacity = I.capacity;
    return GV_OK;
}

int gv_pool_instances_fetch(GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* starts, uint32_t starts_capacity)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !starts)
        return ctx->fail(GV_E_ARG, "gv_pool_instances_fetch: bad argument (pool %u)", pool_id);
    PoolState::Instances& I = ctx->pools[pool_id].instances;
    if (!I.views)
        return ctx->fail(GV_E_STATE, "gv_pool_instances_fetch: pool %u has no instance data since its last gv_cull", pool_id);
    if (starts_capacity < I.views + 1)
        return ctx->fail(GV_E_ARG, "gv_pool_instances_fetch: room for %u starts, the emission listed %u views", starts_capacity, I.views);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_HIP(ctx, I.h_starts.reserve(GV_MAX_VIEWS + 1));
    GV_HIP(ctx, hipMemcpyAsync(I.h_starts.ptr, I.d_starts.ptr, (I.views + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    GV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t total = I.h_starts.ptr[I.views];
    const GvInstanceLayout L = I.emitted;
    if (dst_host && bytes < (size_t)total * L.stride)
        return ctx->fail(GV_E_ARG, "gv_pool_instances_fetch: %zu bytes for %u instances of %u bytes", bytes, total, L.stride);
    memcpy(starts, I.h_starts.ptr, (I.views + 1) * sizeof(uint32_t));
    const uint32_t held = std::min(total, I.capacity);  // (a caller-owned device target may have been too small for the rest)
    if (!dst_host || !held)
        return GV_OK;
    // whole instances into the library's pinned staging, then field by field into the caller's (pageable, never page-locked) array:
    // the bytes between the fields are the plugin's and stay as they are
    GV_HIP(ctx, I.h_data.reserve((size_t)held * L.stride));
    GV_HIP(ctx, hipMemcpyAsync(I.h_data.ptr, I.target, (size_t)held * L.stride, hipMemcpyDeviceToHost, ctx->stream));
    GV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    Field f[4];
    const uint32_t n = fields_of(L, f);
    uint8_t* const to = static_cast<uint8_t*>(dst_host);
    const uint8_t* const from = I.h_data.ptr;
    parallel_ranges(0, held, [&](uint32_t a, uint32_t b) {
        for (uint32_t k = a; k < b; k++)
            for (uint32_t i = 0; i < n; i++)
                memcpy(to + (size_t)k * L.stride + f[i].at, from + (size_t)k * L.stride + f[i].at, f[i].bytes);
    });
    return GV_OK;
}

}  // extern "C"
