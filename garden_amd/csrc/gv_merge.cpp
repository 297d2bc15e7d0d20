// gv_merge.cpp — gv_merge_sorted / gv_merge_device / gv_merge_fetch of include/garden_vis.h: the shared sorted arrays of the
// reference (transSortedMeshes / uiSortedMeshes / the shadow passes' translucent arrays: every sorted system appends its records,
// mesh.cpp:247-261, one sort orders the whole array, mesh.cpp:296-326, renderSorted walks it, mesh.cpp:659-760), made on the
// device from the lists gv_pool_sort has ordered. One merge_sorted_kernel launch per call (gv_merge.hip); buffers of its own
// (Context::merges): the members' results are left as a read through gv_pool_results_device leaves them. Target choice and staged
// fetch are those of the other derived results (gv_ctx.hpp).
#include "gv_ctx.hpp"

using namespace gv;

extern "C" {

int gv_merge_sorted(GvCtx* ctx, const GvMergeGroup* groups, uint32_t group_count)
{
    static_assert(GV_MAX_MERGE_GROUPS == kMaxMergeGroups && GV_MAX_MERGE_ITEMS == kMaxMergeGroupLists, "MergeLaunch holds a call's groups");
    if (!ctx)
        return GV_E_ARG;
    if (!groups || group_count == 0 || group_count > GV_MAX_MERGE_GROUPS)
        return ctx->fail(GV_E_ARG, "gv_merge_sorted: %u groups (1 to %u)", group_count, GV_MAX_MERGE_GROUPS);
    uint32_t total_items = 0, seen_groups = 0;
    for (uint32_t k = 0; k < group_count; k++) {
        const GvMergeGroup& G = groups[k];
        if (G.group_id >= GV_MAX_MERGE_GROUPS || ((seen_groups >> G.group_id) & 1u))
            return ctx->fail(GV_E_ARG, "gv_merge_sorted: group id %u is out of range (%u result slots) or listed twice", G.group_id,
                             GV_MAX_MERGE_GROUPS);
        seen_groups |= 1u << G.group_id;
        if (G.item_count == 0 || G.item_count > GV_MAX_MERGE_ITEMS || !G.items)
            return ctx->fail(GV_E_ARG, "gv_merge_sorted: group %u lists %u items (1 to %u)", G.group_id, G.item_count, GV_MAX_MERGE_ITEMS);
        total_items += G.item_count;
        if (total_items > kMaxSortViews)
            return ctx->fail(GV_E_ARG, "gv_merge_sorted: more than %u items in one call", kMaxSortViews);
        const uint32_t stride = G.stride;
        auto inside = [&](uint32_t offset, uint32_t bytes) { return offset % 4 == 0 && offset <= stride && bytes <= stride - offset; };
        struct Span { uint32_t at, bytes; } spans[4] = {{G.component_offset, 8}, {G.baked_model, 48}, {G.distance_sq, 4}, {G.buffer_index, 4}};
        const uint32_t fields = G.buffer_index == GV_NONE ? 3 : 4;
        bool ok = stride != 0 && stride % 16 == 0 && stride <= kMaxRecordStride;
        for (uint32_t i = 0; ok && i < fields; i++) {
            ok = inside(spans[i].at, spans[i].bytes);
            for (uint32_t j = 0; ok && j < i; j++)
                ok = spans[i].at + spans[i].bytes <= spans[j].at || spans[j].at + spans[j].bytes <= spans[i].at;
        }
        if (!ok)
            return ctx->fail(GV_E_ARG, "gv_merge_sorted: group %u: stride %u (a multiple of 16, at most %u) with fields at %u/%u/%u/%u: fields "
                             "must be 4-byte aligned, inside the record and disjoint", G.group_id, stride, kMaxRecordStride, G.component_offset,
                             G.baked_model, G.distance_sq, G.buffer_index);
        if (G.dst_device && (uintptr_t)G.dst_device % 16 != 0)
            return ctx->fail(GV_E_ARG, "gv_merge_sorted: group %u: dst_device must be 16-byte aligned", G.group_id);
        for (uint32_t i = 0; i < G.item_count; i++) {
            const GvMergeItem& it = G.items[i];
            if (it.pool_id >= GV_MAX_POOLS || !ctx->pools[it.pool_id].bound)
                return ctx->fail(GV_E_ARG, "gv_merge_sorted: group %u item %u: pool %u is not bound", G.group_id, i, it.pool_id);
            const uint32_t culled = culled_views(ctx, it.pool_id);
            if (it.view_index >= culled)
                return ctx->fail(GV_E_ARG, "gv_merge_sorted: group %u item %u: view %u, the last gv_cull of pool %u had %u", G.group_id, i,
                                 it.view_index, it.pool_id, culled);
            if (it.component_stride == 0)
                return ctx->fail(GV_E_ARG, "gv_merge_sorted: group %u item %u: component_stride is 0", G.group_id, i);
            for (uint32_t j = 0; j < i; j++)
                if (G.items[j].pool_id == it.pool_id && G.items[j].view_index == it.view_index)
                    return ctx->fail(GV_E_ARG, "gv_merge_sorted: group %u lists pool %u view %u twice", G.group_id, it.pool_id, it.view_index);
        }
    }
    for (uint32_t k = 0; k < group_count; k++) {
        const GvMergeGroup& G = groups[k];
        for (uint32_t i = 0; i < G.item_count; i++) {
            const GvMergeItem& it = G.items[i];
            const ViewState& vs = ctx->views[it.pool_id][it.view_index];
            const PoolState& p = ctx->pools[it.pool_id];
            if (!vs.emitted)
                return ctx->fail(GV_E_STATE, "gv_merge_sorted: pool %u view %u was culled count-only (emit_records == 0)", it.pool_id, it.view_index);
            if (vs.sorted_dir != (G.descending ? 2 : 1))
                return ctx->fail(GV_E_STATE, "gv_merge_sorted: pool %u view %u has not been sorted %s by gv_pool_sort since its cull", it.pool_id,
                                 it.view_index, G.descending ? "descending" : "ascending");
            if ((p.result_flags & GV_RESULTS_MAP_RECORDS) && p.index_map_count < vs.occupancy)
                return ctx->fail(GV_E_STATE, "gv_merge_sorted: pool %u delivers records in world slots (gv_pool_set_result_mapping), but its index "
                                 "map covers %u of %u slots", it.pool_id, p.index_map_count, vs.occupancy);
        }
    }
    ZoneScope zone("Meshes Sort");
    if (int rc = flush_sorts(ctx))  // the merge is a read: recorded culls and deferred sorts first (as gv_pool_emit_instances)
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    MergeLaunch launch{};
    uint32_t widest = 0;
    for (uint32_t k = 0; k < group_count; k++) {
        const GvMergeGroup& G = groups[k];
        Context::MergeSlot& M = ctx->merges[G.group_id];
        M.valid = false;
        MergeGroup& g = launch.group[k];
        g.first = launch.lists;
        g.lists = G.item_count;
        g.descending = G.descending ? 1u : 0u;
        g.stride = G.stride;
        g.component_offset = G.component_offset;
        g.baked_model = G.baked_model;
        g.distance_sq = G.distance_sq;
        g.buffer_index = G.buffer_index;
        uint64_t bound = 0;  // the host's upper bound of the total
        uint32_t members = 0;
        for (uint32_t i = 0; i < G.item_count; i++) {
            const GvMergeItem& it = G.items[i];
            const ViewState& vs = ctx->views[it.pool_id][it.view_index];
            const PoolState& p = ctx->pools[it.pool_id];
            const ViewRecords r = records_of(vs);
            MergeList& l = launch.list[launch.lists];
            l.count = r.count, l.idx = r.idx, l.model = r.model, l.dist = r.dist;
            l.slot_map = (p.result_flags & GV_RESULTS_MAP_RECORDS) ? p.d_index_map.ptr : nullptr;
            l.component_stride = it.component_stride;
            l.buffer_index = it.buffer_index;
            launch.group_of[launch.lists++] = (uint8_t)k;
            bound += vs.occupancy;
            widest = std::max(widest, vs.occupancy);
            members |= 1u << it.pool_id;
        }
        // (a bound of GV_MAX_MERGE_ITEMS occupancies of 28 bits each stays below the clamp: it changes no size)
        if (int rc = choose_target(ctx, G.dst_device, G.capacity_bytes, G.stride, std::min<uint64_t>(bound, 0xFFFFFFFEu), M.d_records, &g.dst, &g.capacity))
            return rc;
        GV_HIP(ctx, M.d_counts.reserve(GV_MAX_MERGE_ITEMS + 1));
        g.counts = M.d_counts.ptr;
        M.pools = members;
        M.items = G.item_count;
        M.stride = G.stride;
        M.target = g.dst;
        M.capacity = g.capacity;
    }
    GV_LAUNCH(ctx, GV_K_SORT, launch_merge_sorted(launch, widest, ctx->stream));
    for (uint32_t k = 0; k < group_count; k++)
        ctx->merges[groups[k].group_id].valid = true;
    return GV_OK;
}

int gv_merge_device(GvCtx* ctx, uint32_t group_id, const void** records, const void** counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (group_id >= GV_MAX_MERGE_GROUPS || !records || !counts)
        return ctx->fail(GV_E_ARG, "gv_merge_device: bad argument (group %u)", group_id);
    const Context::MergeSlot& M = ctx->merges[group_id];
    if (!M.valid)
        return ctx->fail(GV_E_STATE, "gv_merge_device: group %u has no merged array since the last gv_cull of its members", group_id);
    *records = M.target;
    *counts = M.d_counts.ptr;
    return GV_OK;
}

int gv_merge_fetch(GvCtx* ctx, uint32_t group_id, void* dst_host, size_t bytes, uint32_t* counts, uint32_t counts_capacity)
{
    if (!ctx)
        return GV_E_ARG;
    if (group_id >= GV_MAX_MERGE_GROUPS || !counts)
        return ctx->fail(GV_E_ARG, "gv_merge_fetch: bad argument (group %u)", group_id);
    Context::MergeSlot& M = ctx->merges[group_id];
    if (!M.valid)
        return ctx->fail(GV_E_STATE, "gv_merge_fetch: group %u has no merged array since the last gv_cull of its members", group_id);
    if (counts_capacity < M.items + 1)
        return ctx->fail(GV_E_ARG, "gv_merge_fetch: room for %u counts, the group has %u items", counts_capacity, M.items);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_staged(ctx, M.h_counts, GV_MAX_MERGE_ITEMS + 1, M.d_counts.ptr, M.items + 1))
        return rc;
    const uint32_t total = M.h_counts.ptr[M.items];
    if (dst_host && bytes < (size_t)total * M.stride)
        return ctx->fail(GV_E_ARG, "gv_merge_fetch: %zu bytes for %u records of %u bytes", bytes, total, M.stride);
    memcpy(counts, M.h_counts.ptr, (M.items + 1) * sizeof(uint32_t));
    const uint32_t held = std::min(total, M.capacity);  // (a caller-owned device target may have been too small for the rest)
    if (!dst_host || !held)
        return GV_OK;
    // into the library's pinned staging, then into the caller's (pageable, never page-locked) array
    const size_t size = (size_t)held * M.stride;
    if (int rc = fetch_staged(ctx, M.h_records, size, M.target, size))
        return rc;
    uint8_t* const to = static_cast<uint8_t*>(dst_host);
    const uint8_t* const from = M.h_records.ptr;
    constexpr size_t kPiece = (size_t)256 << 10;  // (as copy_staged_records: 256 KB pieces over the worker threads)
    const size_t pieces = (size + kPiece - 1) / kPiece;
    const uint32_t parts = size >= ((size_t)1 << 20) ? std::min<uint32_t>((uint32_t)pieces, worker_parts((size_t)1 << 30)) : 1u;
    run_parts(parts, [&](uint32_t t) {
        for (size_t k = t; k < pieces; k += parts)
            memcpy(to + k * kPiece, from + k * kPiece, std::min(kPiece, size - k * kPiece));
    });
    return GV_OK;
}

}  // extern "C"
