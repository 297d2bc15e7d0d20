// gv_delta.cpp — gv_pool_view_delta / gv_pool_view_delta_device / gv_pool_view_delta_fetch of include/garden_vis.h: the pool slots that
// came into view and those that left it since a channel's last call — what streaming, animation and audio ask
// of visibility, and all the isVisible write-back has to touch. The current set is read on the device from the listed views' records
// (or a count-only main view's bytes) as they stand: nothing is uploaded, no mark is consumed, nothing any other call can observe
// changes. The baseline and the answer are the channel's own (PoolState::delta); the checks and the fetch it shares with the derived
// results are gv_ctx.hpp's. Kernels: gv_delta.hip.
#include "gv_ctx.hpp"

using namespace gv;

extern "C" {

int gv_pool_view_delta(GvCtx* ctx, uint32_t pool_id, uint32_t channel, const uint32_t* view_indices, uint32_t view_count, uint32_t flags)
{
    static_assert(sizeof(DeltaTotals) == 16, "a row of totals is one 16-byte load");
    if (!ctx)
        return GV_E_ARG;
    if (!bound_pool(ctx, "gv_pool_view_delta", pool_id))
        return GV_E_ARG;
    if (channel >= GV_MAX_DELTA_CHANNELS || view_count > GV_MAX_VIEWS || (flags & ~GV_DELTA_RESTART) || (view_count && !view_indices))
        return ctx->fail(GV_E_ARG, "gv_pool_view_delta: channel %u (below %u), %u views (up to %u) at %p, flags 0x%x", channel,
                         (uint32_t)GV_MAX_DELTA_CHANNELS, view_count, (uint32_t)GV_MAX_VIEWS, (const void*)view_indices, flags);
    PoolState& p = ctx->pools[pool_id];
    PoolState::Delta::Channel& ch = p.delta.channel[channel];
    if (view_count == 0) {  // the drop call (the convention of gv_pool_select_lods(NULL, 0)); the buffers stay for the next call
        ch.drop();
        return GV_OK;
    }
    uint32_t listed = 0;
    for (uint32_t i = 0; i < view_count; i++) {
        const uint32_t v = view_indices[i];
        if (v >= GV_MAX_VIEWS)
            return ctx->fail(GV_E_ARG, "gv_pool_view_delta: view index %u is out of range", v);
        if ((listed >> v) & 1u)
            return ctx->fail(GV_E_ARG, "gv_pool_view_delta: view %u is listed twice", v);
        listed |= 1u << v;
        const ViewState& vs = ctx->views[pool_id][v];
        if (!vs.valid && !vs.draw_count.ptr)  // (no cull of this pool has ever had such a view)
            return ctx->fail(GV_E_ARG, "gv_pool_view_delta: %u is not a view of pool %u", v, pool_id);
    }
    for (uint32_t i = 0; i < view_count; i++) {
        const uint32_t v = view_indices[i];
        const ViewState& vs = ctx->views[pool_id][v];
        if (!vs.valid)
            return ctx->fail(GV_E_STATE, "gv_pool_view_delta: pool %u view %u has no results", pool_id, v);
        if (!vs.emitted && !vs.main_pass)
            return ctx->fail(GV_E_STATE, "gv_pool_view_delta: pool %u view %u is a count-only shadow view: it has neither records nor isVisible bytes",
                             pool_id, v);
    }
    ZoneScope zone("Meshes Delta");
    if (int rc = flush_sorts(ctx))  // the call is a read: recorded culls and deferred sorts first (as gv_pool_select_lods)
        return rc;
    // C.slots, and every read inside buffers that cover the occupancy the view was culled with
    uint32_t current_slots = 0;
    for (uint32_t i = 0; i < view_count; i++) {
        const ViewState& vs = ctx->views[pool_id][view_indices[i]];
        current_slots = std::max(current_slots, vs.occupancy);
        if (vs.emitted ? vs.visible_idx.cap < vs.occupancy : vs.is_visible.cap < vs.occupancy)
            return ctx->fail(GV_E_STATE, "gv_pool_view_delta: the results of pool %u view %u do not cover its %u slots", pool_id, view_indices[i],
                             vs.occupancy);
        // the bytes are in mirror order; a fetch takes them through the entry -> slot table when the table matches the view (deliver_large)
        if (!vs.emitted && p.perm.size() == vs.occupancy && p.d_orig.cap < vs.occupancy)
            return ctx->fail(GV_E_STATE, "gv_pool_view_delta: the entry -> slot table of pool %u does not cover the %u slots of view %u", pool_id,
                             vs.occupancy, view_indices[i]);
    }
    const uint32_t baseline_slots = (flags & GV_DELTA_RESTART) ? 0u : ch.baseline_slots;
    const uint32_t universe = std::max(baseline_slots, current_slots);
    const size_t current_words = delta_words(current_slots);
    DeviceBuf<unsigned long long>& spare = ch.d_set[ch.held ^ 1u];
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_HIP(ctx, spare.reserve(std::max<size_t>(current_words, 1)));
    GV_HIP(ctx, p.delta.d_totals.reserve(std::max<uint32_t>(delta_groups(universe), 1)));
    if (ch.d_counts.cap < 4 || ch.d_slots.cap < std::max<uint32_t>(universe, 1))
        ch.result = false;  // (the answer's buffers are about to be replaced: should that fail, the previous answer is gone)
    GV_HIP(ctx, ch.d_counts.reserve(4));
    GV_HIP(ctx, ch.d_slots.reserve(std::max<uint32_t>(universe, 1)));
    DeltaSets sets{};
    sets.current = spare.ptr;
    sets.baseline = ch.d_set[ch.held].ptr;
    sets.current_slots = current_slots;
    sets.baseline_slots = baseline_slots;
    sets.universe = universe;
    sets.totals = p.delta.d_totals.ptr;
    sets.slots = ch.d_slots.ptr;
    sets.counts = ch.d_counts.ptr;
    if (baseline_slots && ch.d_set[ch.held].cap < delta_words(baseline_slots))  // (cannot happen: the commit below is the only writer)
        return ctx->fail(GV_E_STATE, "gv_pool_view_delta: the baseline of pool %u channel %u is not covered by its buffer", pool_id, channel);
    ch.result = false;  // (a failed launch leaves no answer; the baseline is committed behind the last one)
    if (current_words)
        GV_HIP(ctx, hipMemsetAsync(spare.ptr, 0, current_words * sizeof(unsigned long long), ctx->stream));
    for (uint32_t i = 0; i < view_count; i++) {
        const ViewState& vs = ctx->views[pool_id][view_indices[i]];
        if (vs.emitted) {
            const ViewRecords r = records_of(vs);
            GV_LAUNCH(ctx, GV_K_EMIT, launch_delta_mark_records(r.count, r.idx, vs.occupancy, current_slots, spare.ptr, ctx->stream));
        } else {
            const bool permuted = !p.perm.empty() && p.perm.size() == vs.occupancy;
            GV_LAUNCH(ctx, GV_K_EMIT, launch_delta_mark_bytes(vs.is_visible.ptr, vs.occupancy, permuted ? p.d_orig.ptr : nullptr, current_slots, spare.ptr,
                                                              ctx->stream));
        }
    }
    GV_LAUNCH(ctx, GV_K_EMIT, launch_delta_count(sets, ctx->stream));
    GV_LAUNCH(ctx, GV_K_EMIT, launch_delta_place(sets, ctx->stream));
    if (universe == 0)  // nothing to launch over: the four counts are zeros
        GV_HIP(ctx, hipMemsetAsync(ch.d_counts.ptr, 0, 4 * sizeof(uint32_t), ctx->stream));
    // the commit: C is the baseline from here on, in stream order (the next call's launches read it behind these)
    ch.held ^= 1u;
    ch.baseline_slots = current_slots;
    ch.universe = universe;
    ch.result = true;
    return GV_OK;
}

int gv_pool_view_delta_device(GvCtx* ctx, uint32_t pool_id, uint32_t channel, const void** slots, const void** counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || channel >= GV_MAX_DELTA_CHANNELS || !slots || !counts)
        return ctx->fail(GV_E_ARG, "gv_pool_view_delta_device: bad argument (pool %u, channel %u)", pool_id, channel);
    const PoolState::Delta::Channel& ch = ctx->pools[pool_id].delta.channel[channel];
    if (!ch.result)
        return ctx->fail(GV_E_STATE, "gv_pool_view_delta_device: pool %u channel %u holds no result", pool_id, channel);
    *slots = ch.d_slots.ptr;
    *counts = ch.d_counts.ptr;
    return GV_OK;
}

int gv_pool_view_delta_fetch(GvCtx* ctx, uint32_t pool_id, uint32_t channel, int write_back, GvViewDelta* out)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || channel >= GV_MAX_DELTA_CHANNELS || !out)
        return ctx->fail(GV_E_ARG, "gv_pool_view_delta_fetch: bad argument (pool %u, channel %u)", pool_id, channel);
    const PoolState& p = ctx->pools[pool_id];
    PoolState::Delta::Channel& ch = ctx->pools[pool_id].delta.channel[channel];
    if (!ch.result)
        return ctx->fail(GV_E_STATE, "gv_pool_view_delta_fetch: pool %u channel %u holds no result", pool_id, channel);
    const bool mapped = (p.result_flags & GV_RESULTS_MAP_VISIBLE) != 0;
    if (write_back && (!p.bound || (mapped ? !p.visible_base : !p.is_visible)))
        return ctx->fail(GV_E_STATE, "gv_pool_view_delta_fetch: pool %u has no isVisible target to write back into", pool_id);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_staged(ctx, ch.h_counts, 4, ch.d_counts.ptr, 4))
        return rc;
    const uint32_t* counts = ch.h_counts.ptr;
    if ((uint64_t)counts[0] + counts[1] > ch.universe)  // (two disjoint sets of at most U slots: only a broken launch gets here)
        return ctx->fail(GV_E_HIP, "gv_pool_view_delta_fetch: pool %u channel %u answers %u + %u slots of %u", pool_id, channel, counts[0], counts[1],
                         ch.universe);
    const uint32_t appeared = counts[0], total = counts[0] + counts[1];
    if (total) {
        size_t room = 1024;  // grow-only staging in powers of two: a steady stream of small answers never reallocates pinned memory
        while (room < total)
            room *= 2;
        if (int rc = fetch_staged(ctx, ch.h_slots, room, ch.d_slots.ptr, total))
            return rc;
    }
    drain_events(ctx);
    const uint32_t* slots = ch.h_slots.ptr;
    out->appeared = slots;
    out->vanished = slots ? slots + appeared : nullptr;
    out->appeared_count = appeared;
    out->vanished_count = total - appeared;
    out->visible_count = counts[2];
    out->slots = counts[3];
    if (!write_back || !total)
        return GV_OK;
    // 1 into the byte of every appeared slot, 0 into that of every vanished one, nothing else; a slot at or beyond the bound occupancy
    // has no component any more
    const uint32_t limit = p.occupancy;
    if (mapped) {
        const uint32_t* map = p.h_index_map.data();
        const uint32_t covered = (uint32_t)std::min<size_t>(p.h_index_map.size(), limit);
        uint8_t* base = p.visible_base;
        const size_t stride = p.visible_stride;
        const uint32_t world = p.visible_count;
        parallel_ranges(0, total, [&](uint32_t a, uint32_t b) {
            for (uint32_t k = a; k < b; k++)
                if (slots[k] < covered && map[slots[k]] < world)  // (GV_NONE: a hole)
                    base[(size_t)map[slots[k]] * stride] = k < appeared ? 1 : 0;
        }, kWriteBackFloor);
    } else {
        uint8_t* component_vis = p.is_visible;
        const size_t component_stride = p.is_visible_stride;
        parallel_ranges(0, total, [&](uint32_t a, uint32_t b) {
            for (uint32_t k = a; k < b; k++)
                if (slots[k] < limit)
                    component_vis[(size_t)slots[k] * component_stride] = k < appeared ? 1 : 0;
        }, kWriteBackFloor);
    }
    return GV_OK;
}

}  // extern "C"
