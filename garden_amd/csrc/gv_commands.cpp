// gv_commands.cpp — gv_pool_bind_geometry / gv_pool_set_command_layout / gv_pool_emit_draw_commands / gv_pool_draw_commands_device /
// gv_pool_draw_commands_fetch of include/garden_vis.h: one indirect command per draw (or per run of draws of one geometry) of the
// pool's last instance emission, in the caller's command struct, built on the device from the records and the emission's instance
// ranges. The geometry ids are mirrored per pool slot (gv_mirror.cpp upload_geometry); buffers of its own
// (PoolState::commands): neither the cull side nor the instance data is touched. Shared with the other derived results (gv_ctx.hpp):
// the reader's checks, the target choice, the staged fetch. Kernels: gv_commands.hip.
#include "gv_ctx.hpp"

using namespace gv;

extern "C" {

int gv_pool_bind_geometry(GvCtx* ctx, uint32_t pool_id, const void* ids, uint32_t stride, uint32_t width, uint32_t occupancy,
                          const GvGeometry* table, uint32_t table_count)
{
    static_assert(sizeof(GvGeometry) == sizeof(CommandGeometry) && sizeof(GvGeometry) == 12, "the kernels read the table as it is bound");
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_geometry: pool %u out of range", pool_id);
    if (ids && ((width != 1 && width != 2 && width != 4) || stride < width))
        return ctx->fail(GV_E_ARG, "gv_pool_bind_geometry: ids of %u bytes every %u bytes (1, 2 or 4 bytes, a stride of at least the width)", width,
                         stride);
    if ((!table && table_count) || ((table || ids) && !table_count) || table_count > GV_MAX_GEOMETRIES)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_geometry: table %p with %u entries (1 to %u; NULL and 0 together with NULL ids remove the binding)",
                         (const void*)table, table_count, GV_MAX_GEOMETRIES);
    if (ids && occupancy >= kSlotNone)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_geometry: occupancy %u exceeds the 28-bit slot range", occupancy);
    PoolState::Geometry& G = ctx->pools[pool_id].geometry;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    GV_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the stream may still be reading the table or the mirror)
    G.reset();
    ctx->pools[pool_id].clusters.rebound = true;  // a cluster result's kept ids index the table as it was: no second phase of it
    G.ids = Column{static_cast<const uint8_t*>(ids), ids ? stride : 0};
    G.width = ids ? width : 0;
    G.occupancy = ids ? occupancy : 0;
    G.table_count = table_count;
    G.bound = table != nullptr;
    if (!ids) {  // no column: no mirror
        G.wanted = false;
        G.SlotMirror::release();
        G.staged.pending = false;
    }
    if (!table) {
        G.d_table.release();
        return GV_OK;
    }
    GV_HIP(ctx, G.d_table.reserve(table_count));
    GV_HIP(ctx, hipMemcpy(G.d_table.ptr, table, (size_t)table_count * sizeof(GvGeometry), hipMemcpyHostToDevice));
    ctx->stats.upload_bytes += (size_t)table_count * sizeof(GvGeometry);
    return GV_OK;
}

int gv_pool_set_command_layout(GvCtx* ctx, uint32_t pool_id, const GvCommandLayout* layout)
{
    static_assert(GV_NONE == kNoField, "absent fields are GV_NONE in the kernel's layout too");
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_set_command_layout: pool %u out of range", pool_id);
    GvCommandLayout L{};
    if (layout) {
        L = *layout;
        uint32_t at[6] = {L.count, L.instance_count, L.first, L.first_instance, L.vertex_offset, L.draw};
        bool ok = L.stride % 4 == 0 && L.stride >= kMinCommandStride && L.stride <= kMaxCommandStride;
        for (uint32_t i = 0; ok && i < 6; i++) {
            if (i >= 4 && at[i] == GV_NONE)
                continue;
            ok = at[i] % 4 == 0 && at[i] < L.stride;  // (4-byte aligned below a stride that is a multiple of 4: the field lies inside)
            for (uint32_t j = 0; ok && j < i; j++)
                ok = at[j] != at[i];
        }
        if (!ok)
            return ctx->fail(GV_E_ARG, "gv_pool_set_command_layout: stride %u (a multiple of 4, %u to %u) with count / instance_count / first / "
                             "first_instance at %u / %u / %u / %u and vertex_offset / draw at %u / %u (0x%x: none): fields must be 4-byte aligned, "
                             "lie inside the command and be disjoint", L.stride, kMinCommandStride, kMaxCommandStride, L.count, L.instance_count,
                             L.first, L.first_instance, L.vertex_offset, L.draw, GV_NONE);
    }
    ctx->pools[pool_id].commands.layout = L;  // read by the next command emission
    ctx->pools[pool_id].clusters.rebound = true;  // (a cluster result was written in the layout as it was: no second phase of it)
    return GV_OK;
}

int gv_pool_emit_draw_commands(GvCtx* ctx, uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device, size_t capacity_bytes)
{
    static_assert(kDrawChunk % kCommandBlock == 0, "a chunk is a whole number of command_runs_kernel workgroups");
    if (!ctx)
        return GV_E_ARG;
    const char* const fn = "gv_pool_emit_draw_commands";
    if (!bound_pool(ctx, fn, pool_id))
        return GV_E_ARG;
    if (flags & ~(uint32_t)GV_COMMANDS_MERGE_RUNS)
        return ctx->fail(GV_E_ARG, "gv_pool_emit_draw_commands: unknown flags 0x%x", flags);
    if (dst_device && (uintptr_t)dst_device % 16 != 0)
        return ctx->fail(GV_E_ARG, "gv_pool_emit_draw_commands: dst_device must be 16-byte aligned");
    PoolState& p = ctx->pools[pool_id];
    PoolState::Instances& I = p.instances;
    PoolState::Geometry& G = p.geometry;
    PoolState::Commands& M = p.commands;
    const GvCommandLayout L = M.layout;
    if (!L.stride)
        return ctx->fail(GV_E_STATE, "gv_pool_emit_draw_commands: pool %u has no command layout (gv_pool_set_command_layout)", pool_id);
    if (!G.bound)
        return ctx->fail(GV_E_STATE, "gv_pool_emit_draw_commands: pool %u has no geometry bound (gv_pool_bind_geometry)", pool_id);
    if (!I.views)
        return ctx->fail(GV_E_STATE, "gv_pool_emit_draw_commands: pool %u has no instance emission since its last gv_cull", pool_id);
    const uint32_t m = I.views;
    if ((uint64_t)m * region_commands > UINT32_MAX)
        return ctx->fail(GV_E_ARG, "gv_pool_emit_draw_commands: %u regions of %u commands are more positions than 32 bits hold", m, region_commands);
    for (uint32_t k = 0; k < m; k++) {
        const ViewState* vs = view_of(ctx, pool_id, I.listed[k]);
        if (!vs)
            return ctx->fail(GV_E_STATE, "gv_pool_emit_draw_commands: pool %u view %u has no results", pool_id, I.listed[k]);
        if (int rc = column_covers(ctx, fn, kGeometryIds, pool_id, G.ids, G.occupancy, *vs, I.listed[k]))
            return rc;
    }
    ZoneScope zone("Meshes Draw Commands");
    if (int rc = flush_sorts(ctx))  // the emission is a read: recorded culls and deferred sorts first (as the instance emissions)
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    // behind a LOD selection (gv_pool_select_lods) the ids are the selected ones, per draw: the id mirror is not read, and marks made
    // after the selection wait for the next selection, emission without one, or gv_sync
    const bool selected = p.lod.views != 0;
    if (int rc = selected ? GV_OK : want_column(ctx, p, G.ids, G, upload_geometry))  // marks made since the cull are seen by this emission
        return rc;
    CommandLaunch launch{};
    const bool merge = (flags & GV_COMMANDS_MERGE_RUNS) != 0;
    uint64_t slots = 0;  // the sum of the listed views' occupancies: the host's upper bound of the commands
    for (uint32_t k = 0; k < m; k++) {
        const ViewState& vs = *view_of(ctx, pool_id, I.listed[k]);
        launch.view[k] = CommandView{records_of(vs).count, records_of(vs).idx};
        const uint32_t blocks = (vs.occupancy + kCommandBlock - 1) / kCommandBlock;
        // (with regions only the positions below R are ever written: the workgroups of R cover them)
        launch.first_block[k + 1] = launch.first_block[k] + (region_commands ? (region_commands + kCommandBlock - 1) / kCommandBlock : blocks);
        launch.first_draw_block[k + 1] = launch.first_draw_block[k] + blocks;
        launch.first_chunk[k + 1] = launch.first_chunk[k] + (vs.occupancy + kDrawChunk - 1) / kDrawChunk;
        slots += vs.occupancy;
    }
    launch.views = m;
    launch.merge_runs = merge;
    launch.region = region_commands;
    launch.stride = L.stride;
    launch.count = L.count;
    launch.instance_count = L.instance_count;
    launch.first = L.first;
    launch.first_instance = L.first_instance;
    launch.vertex_offset = L.vertex_offset;
    launch.draw = L.draw;
    launch.ids = G.ids.ptr && !selected ? G.d_column.ptr : nullptr;
    launch.draw_ids = selected ? p.lod.d_draw_geometry.ptr : nullptr;
    launch.table = reinterpret_cast<const CommandGeometry*>(G.d_table.ptr);
    launch.table_count = G.table_count;
    launch.starts = I.d_starts.ptr;
    launch.first_instance_of = I.draws ? I.d_first.ptr : nullptr;
    launch.draw_starts = I.draws ? I.d_draw_starts.ptr : nullptr;
    const uint64_t positions = region_commands ? (uint64_t)m * region_commands : slots;
    if (int rc = choose_target(ctx, dst_device, capacity_bytes, L.stride, positions, M.d_data, &launch.dst, &launch.capacity))
        return rc;
    GV_HIP(ctx, M.d_counts.reserve(GV_MAX_VIEWS));
    launch.command_counts = M.d_counts.ptr;
    const bool scan = merge && launch.first_chunk[m] != 0;
    if (merge) {
        const size_t draws = (size_t)launch.first_draw_block[m] * kCommandBlock;
        GV_HIP(ctx, M.d_rank.reserve(std::max<size_t>(draws, 1)));
        GV_HIP(ctx, M.d_chunk_total.reserve(std::max<size_t>(launch.first_chunk[m], 1)));
        GV_HIP(ctx, M.d_draw_of.reserve(draws + m));  // (one word more per view: a view's runs begin at its draws + v)
        GV_HIP(ctx, M.d_first_of.reserve(draws + m));
        launch.rank = M.d_rank.ptr;
        launch.chunk_total = M.d_chunk_total.ptr;
        launch.draw_of = M.d_draw_of.ptr;
        launch.first_of = M.d_first_of.ptr;
    }
    if (scan) {
        GV_LAUNCH(ctx, GV_K_EMIT, launch_command_heads(launch, ctx->stream));
        GV_LAUNCH(ctx, GV_K_EMIT, launch_command_runs(launch, ctx->stream));
    }
    GV_LAUNCH(ctx, GV_K_EMIT, launch_commands(launch, ctx->stream));
    M.target = launch.dst;
    M.capacity = launch.capacity;
    M.views = m;
    M.stride = L.stride;
    M.region = region_commands;
    return GV_OK;
}

int gv_pool_draw_commands_device(GvCtx* ctx, uint32_t pool_id, const void** commands, const void** command_counts)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !commands || !command_counts)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_commands_device: bad argument (pool %u)", pool_id);
    const PoolState::Commands& M = ctx->pools[pool_id].commands;
    if (!M.views)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_commands_device: pool %u has no commands since its last gv_cull or instance emission", pool_id);
    *commands = M.target;
    *command_counts = M.d_counts.ptr;
    return GV_OK;
}

int gv_pool_draw_commands_fetch(GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* command_counts, uint32_t counts_capacity)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !command_counts)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_commands_fetch: bad argument (pool %u)", pool_id);
    PoolState::Commands& M = ctx->pools[pool_id].commands;
    if (!M.views)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_commands_fetch: pool %u has no commands since its last gv_cull or instance emission", pool_id);
    if (counts_capacity < M.views)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_commands_fetch: room for %u counts, the emission listed %u views", counts_capacity, M.views);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_staged(ctx, M.h_counts, GV_MAX_VIEWS, M.d_counts.ptr, M.views))
        return rc;
    uint64_t positions = (uint64_t)M.views * M.region;
    if (!M.region)
        for (uint32_t k = 0; k < M.views; k++)
            positions += M.h_counts.ptr[k];
    const size_t held = (size_t)std::min<uint64_t>(positions, M.capacity);  // (a caller-owned device target may have been too small for the rest)
    if (dst_host && bytes < held * M.stride)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_commands_fetch: %zu bytes for %zu commands of %u bytes", bytes, held, M.stride);
    memcpy(command_counts, M.h_counts.ptr, M.views * sizeof(uint32_t));
    if (!dst_host || !held)
        return GV_OK;
    return fetch_staged(ctx, M.h_data, held * M.stride, M.target, held * M.stride, dst_host);
}

}  // extern "C"
