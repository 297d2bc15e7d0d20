// gv_instance.cpp — gv_pool_set_instance_layout / gv_pool_emit_instances / gv_pool_instances_device / gv_pool_instances_fetch of
// include/garden_vis.h: the instance array the reference's draw loops fill (renderUnsorted / renderSorted, mesh.cpp:556-770, call
// drawAsync per draw, and every plugin starts with instanceData[instanceIndex].mvp = viewProj * model, sprite.cpp:107-108,122-126),
// made on the device from the records a cull left there. One instance_kernel launch per call; buffers of its own (PoolState::
// instances): the cull side is left as a read through gv_pool_results_device leaves it.
// gv_pool_bind_payload / gv_pool_set_payload_layout: the component bytes a plugin copies next to mvp (sprite.cpp:127-129), mirrored
// per pool slot (gv_mirror.cpp upload_payload) and written by the same launch (instance_kernel<true>).
// gv_pool_emit_draw_instances / gv_pool_set_instance_index_field / gv_pool_draw_bases_device / gv_pool_draw_bases_fetch: the same for
// draws that take several instances — the ready count of the record's slot, read on the device from a mirror of the ready column
// (gv_mirror.cpp upload_counts); two launches (draw_counts_kernel, draw_instances_kernel), the host never reads a count.
// The checks, the target choice and the fetch it shares with the other derived results are gv_ctx.hpp's.
#include "gv_ctx.hpp"

using namespace gv;

namespace {

struct Field {
    uint32_t at, bytes, align;
};

constexpr uint32_t kMaxFields = 4 + GV_MAX_PAYLOAD_FIELDS + 1;

// The fields an instance has: the layout's in the order mvp, model, slot, distance_sq (stride 0: no layout yet, none), the payload
// destinations `at` that are set, the index word (GV_NONE: none). Returns how many; room for kMaxFields.
uint32_t instance_fields(const GvInstanceLayout& L, uint32_t payload, const uint32_t* at, const uint32_t* bytes, uint32_t index_at, Field* f)
{
    uint32_t n = 0;
    if (L.stride) {
        f[n++] = Field{L.mvp, 64, 16};
        for (const Field& optional : {Field{L.model, 48, 4}, Field{L.slot, 4, 4}, Field{L.distance_sq, 4, 4}})
            if (optional.at != GV_NONE)
                f[n++] = optional;
    }
    for (uint32_t k = 0; k < payload; k++)
        if (at[k] != GV_NONE)
            f[n++] = Field{at[k], bytes[k], 4};
    if (index_at != GV_NONE)
        f[n++] = Field{index_at, 4, 4};
    return n;
}

bool overlaps_any(const Field* f, uint32_t n, uint32_t at, uint32_t bytes)
{
    for (uint32_t j = 0; j < n; j++)
        if (!(at + bytes <= f[j].at || f[j].at + f[j].bytes <= at))
            return true;
    return false;
}

// the payload destinations `at` against the instance layout (stride 0: none yet — only each other): 4-byte aligned, inside the
// stride, disjoint from one another and from the layout's fields (which are disjoint among themselves: gv_pool_set_instance_layout)
bool payload_fits(const GvInstanceLayout& L, const PoolState::Payload& P, const uint32_t* at)
{
    for (uint32_t k = 0; k < P.count; k++)
        if (at[k] != GV_NONE &&
            (at[k] % 4 != 0 || at[k] > kMaxInstanceStride || (L.stride && (at[k] > L.stride || P.bytes[k] > L.stride - at[k]))))
            return false;
    Field f[kMaxFields];
    const uint32_t n = instance_fields(L, P.count, at, P.bytes, GV_NONE, f);
    for (uint32_t i = 1; i < n; i++)
        if (overlaps_any(f, i, f[i].at, f[i].bytes))
            return false;
    return true;
}

// the "index within the draw" word of gv_pool_set_instance_index_field against the layout and the destinations `at` (stride 0: none
// yet — only the destinations): 4-byte aligned, inside the stride, disjoint from the layout's fields and the payload destinations
bool index_fits(const GvInstanceLayout& L, const PoolState::Payload& P, const uint32_t* at, uint32_t index_at)
{
    if (index_at % 4 != 0 || index_at > kMaxInstanceStride - 4 || (L.stride && index_at > L.stride - 4))
        return false;
    Field f[kMaxFields];
    return !overlaps_any(f, instance_fields(L, P.count, at, P.bytes, GV_NONE, f), index_at, 4);
}

// What gv_pool_emit_instances and gv_pool_emit_draw_instances (`fn`) check alike: the arguments, the layout, the listed views
// (results, not count-only, covered by the index map) and the payload's fit and occupancy. *with_payload: a destination is set.
int check_emission(GvCtx* ctx, const char* fn, uint32_t pool_id, const uint32_t* view_indices, uint32_t view_count, const void* dst_device,
                   bool* with_payload)
{
    if (!ctx)
        return GV_E_ARG;
    if (!bound_pool(ctx, fn, pool_id))
        return GV_E_ARG;
    PoolState& p = ctx->pools[pool_id];
    const uint32_t culled = culled_views(ctx, pool_id);
    if (!view_indices || view_count == 0 || view_count > culled)
        return ctx->fail(GV_E_ARG, "%s: %u views listed, the last gv_cull of pool %u had %u", fn, view_count, pool_id, culled);
    if (dst_device && (uintptr_t)dst_device % 16 != 0)
        return ctx->fail(GV_E_ARG, "%s: dst_device must be 16-byte aligned", fn);
    uint32_t listed = 0;
    for (uint32_t k = 0; k < view_count; k++) {
        const uint32_t v = view_indices[k];
        if (v >= GV_MAX_VIEWS || ((listed >> v) & 1u))
            return ctx->fail(GV_E_ARG, "%s: view index %u is out of range or listed twice", fn, v);
        listed |= 1u << v;
    }
    const GvInstanceLayout L = p.instances.layout;
    if (!L.stride)
        return ctx->fail(GV_E_STATE, "%s: pool %u has no instance layout (gv_pool_set_instance_layout)", fn, pool_id);
    for (uint32_t k = 0; k < view_count; k++) {
        const ViewState* vs = view_of(ctx, pool_id, view_indices[k]);
        if (!vs)
            return ctx->fail(GV_E_STATE, "%s: pool %u view %u has no results", fn, pool_id, view_indices[k]);
        if (!vs->emitted)
            return ctx->fail(GV_E_STATE, "%s: pool %u view %u was culled count-only (emit_records == 0)", fn, pool_id, view_indices[k]);
        if (L.slot != GV_NONE && p.index_map_count && p.index_map_count < vs->occupancy)
            return ctx->fail(GV_E_STATE, "%s: the index map of pool %u covers %u of its %u slots", fn, pool_id, p.index_map_count, vs->occupancy);
    }
    const PoolState::Payload& P = p.payload;
    *with_payload = P.count && P.any_destination();
    if (*with_payload) {
        if (!payload_fits(L, P, P.at))
            return ctx->fail(GV_E_ARG, "%s: the payload destinations of pool %u do not fit its instance layout (stride %u)", fn, pool_id, L.stride);
        for (uint32_t k = 0; k < view_count; k++)
            if (int rc = column_covers(ctx, fn, kPayloadRows, pool_id, P.src[0], P.occupancy, *view_of(ctx, pool_id, view_indices[k]), view_indices[k]))
                return rc;
    }
    return GV_OK;
}

// What both emissions launch with: the listed views and their workgroups, the layout, the index map, and — with_payload — where each
// word of a payload row goes. slots: the sum of the views' occupancies. Returns the bytes of an instance that the fields, the payload
// and the index word at `index_at` (GV_NONE: none) cover.
uint32_t fill_launch(GvCtx* ctx, const PoolState& p, const uint32_t* view_indices, uint32_t view_count, bool with_payload, uint32_t index_at,
                     InstanceLaunch& launch, uint64_t& slots)
{
    const uint32_t pool_id = (uint32_t)(&p - ctx->pools);
    const PoolState::Payload& P = p.payload;
    const GvInstanceLayout L = p.instances.layout;
    for (uint32_t k = 0; k < view_count; k++) {
        const ViewState& vs = *view_of(ctx, pool_id, view_indices[k]);
        const ViewRecords r = records_of(vs);
        InstanceView& w = launch.view[k];
        w.count = r.count, w.idx = r.idx, w.model = r.model, w.dist = r.dist;
        memcpy(w.view_proj, vs.view_proj, sizeof(w.view_proj));
        launch.first_block[k + 1] = launch.first_block[k] + (vs.occupancy + kInstanceBlock - 1) / kInstanceBlock;
        slots += vs.occupancy;
    }
    launch.views = view_count;
    launch.stride = L.stride;
    launch.mvp = L.mvp;
    launch.model = L.model;
    launch.slot = L.slot;
    launch.distance_sq = L.distance_sq;
    launch.index_map = p.index_map_count ? p.d_index_map.ptr : nullptr;
    Field fields[kMaxFields];
    uint32_t covered = 0;
    for (uint32_t i = 0, n = instance_fields(L, with_payload ? P.count : 0, P.at, P.bytes, index_at, fields); i < n; i++)
        covered += fields[i].bytes;
    if (with_payload) {
        // where each word of a row goes; a 16-byte piece whose four words go to one 16-byte aligned place travels whole
        launch.payload_rows = P.d_column.ptr;
        launch.payload_pitch = P.pitch;
        std::fill(launch.piece_at, launch.piece_at + 4, kNoPayloadPlace);
        std::fill(launch.word_at, launch.word_at + 16, kNoPayloadPlace);
        for (uint32_t f = 0; f < P.count; f++) {
            if (P.at[f] == GV_NONE)
                continue;
            for (uint32_t w = 0; w < P.bytes[f] / 4; w++)
                launch.word_at[P.offset[f] / 4 + w] = (uint16_t)(P.at[f] + 4 * w);
        }
        for (uint32_t j = 0; j < 4; j++) {
            uint16_t* w = launch.word_at + 4 * j;
            if (w[0] != kNoPayloadPlace && w[0] % 16 == 0 && w[1] == w[0] + 4 && w[2] == w[0] + 8 && w[3] == w[0] + 12) {
                launch.piece_at[j] = w[0];
                std::fill(w, w + 4, kNoPayloadPlace);
            }
        }
    }
    return covered;
}

// what an emission that has been launched leaves for the fetches and for gv_pool_emit_draw_commands
void note_emission(GvCtx* ctx, PoolState& p, const InstanceLaunch& launch, const uint32_t* view_indices, uint32_t view_count, bool with_payload, uint32_t index,
                   bool draws)
{
    PoolState::Instances& I = p.instances;
    I.target = launch.dst;
    I.capacity = launch.capacity;
    I.views = view_count;
    std::copy(view_indices, view_indices + view_count, I.listed);
    end_derived(ctx, p, Ends::EmissionReplaced);  // commands and selected levels belong to the emission in front of them
    I.emitted = I.layout;
    I.emitted_payload = 0;
    for (uint32_t f = 0; with_payload && f < p.payload.count; f++)
        if (p.payload.at[f] != GV_NONE) {
            I.emitted_at[I.emitted_payload] = p.payload.at[f];
            I.emitted_bytes[I.emitted_payload++] = p.payload.bytes[f];
        }
    I.emitted_index = index;
    I.draws = draws;
}

}  // namespace

extern "C" {

int gv_pool_bind_payload(GvCtx* ctx, uint32_t pool_id, const GvPayloadField* fields, uint32_t count, uint32_t occupancy)
{
    static_assert(GV_MAX_PAYLOAD_BYTES == 64 && GV_MAX_PAYLOAD_FIELDS == 4, "InstanceLaunch::piece_at / word_at describe a 64-byte row");
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !ctx->pools[pool_id].bound)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_payload: pool %u is not bound", pool_id);
    PoolState::Payload& P = ctx->pools[pool_id].payload;
    if (count == 0) {  // removed, mirror freed (the stream may still be reading it)
        GV_HIP(ctx, hipSetDevice(ctx->device));
        GV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        P.release();
        P.reset();
        P.count = P.occupancy = P.pitch = 0;
        std::fill(P.at, P.at + GV_MAX_PAYLOAD_FIELDS, GV_NONE);
        return GV_OK;
    }
    if (count > GV_MAX_PAYLOAD_FIELDS || !fields)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_payload: %u fields (1 to %u, or 0 to remove the payload)", count, GV_MAX_PAYLOAD_FIELDS);
    if (occupancy >= kSlotNone)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_payload: occupancy %u exceeds the 28-bit slot range", occupancy);
    uint32_t sum = 0;
    for (uint32_t f = 0; f < count; f++) {
        const GvPayloadField& g = fields[f];
        if (!g.data || g.bytes == 0 || g.bytes % 4 != 0 || g.bytes > 64 || g.stride < g.bytes)
            return ctx->fail(GV_E_ARG, "gv_pool_bind_payload: field %u: data %p, %u bytes (4 to 64, a multiple of 4) every %u bytes (at least its size)",
                             f, g.data, g.bytes, g.stride);
        sum += g.bytes;
    }
    if (sum > GV_MAX_PAYLOAD_BYTES)
        return ctx->fail(GV_E_ARG, "gv_pool_bind_payload: %u bytes per slot, at most %u", sum, GV_MAX_PAYLOAD_BYTES);
    bool same = P.count == count && occupancy >= P.occupancy;
    for (uint32_t f = 0; same && f < count; f++)
        same = P.bytes[f] == fields[f].bytes;
    if (!same)  // another shape or a smaller occupancy: everything is uploaded
        P.reset();
    P.count = count;
    P.occupancy = occupancy;
    P.pitch = P.elem = sum <= 16 ? 16 : (sum <= 32 ? 32 : 64);  // (the mirror's element is the row)
    for (uint32_t f = 0, offset = 0; f < GV_MAX_PAYLOAD_FIELDS; f++) {
        P.src[f] = f < count ? Column{static_cast<const uint8_t*>(fields[f].data), fields[f].stride} : Column{};
        P.bytes[f] = f < count ? fields[f].bytes : 0;
        P.offset[f] = offset;
        offset += P.bytes[f];
        P.at[f] = GV_NONE;
    }
    return GV_OK;
}

int gv_pool_set_payload_layout(GvCtx* ctx, uint32_t pool_id, const uint32_t* at, uint32_t count)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_set_payload_layout: pool %u out of range", pool_id);
    PoolState& p = ctx->pools[pool_id];
    if (!p.payload.count)
        return ctx->fail(GV_E_STATE, "gv_pool_set_payload_layout: pool %u has no payload (gv_pool_bind_payload)", pool_id);
    if (!at || count != p.payload.count)
        return ctx->fail(GV_E_ARG, "gv_pool_set_payload_layout: %u destinations for the %u fields of pool %u", count, p.payload.count, pool_id);
    if (!payload_fits(p.instances.layout, p.payload, at))
        return ctx->fail(GV_E_ARG, "gv_pool_set_payload_layout: destinations must be 4-byte aligned, lie inside the instance (stride %u) and be "
                         "disjoint from each other and from mvp / model / slot / distance_sq", p.instances.layout.stride);
    if (p.instances.index_at != GV_NONE && !index_fits(p.instances.layout, p.payload, at, p.instances.index_at))
        return ctx->fail(GV_E_ARG, "gv_pool_set_payload_layout: the destinations overlap the index field of pool %u at %u "
                         "(gv_pool_set_instance_index_field)", pool_id, p.instances.index_at);
    std::copy(at, at + count, p.payload.at);  // read by the next emission
    return GV_OK;
}

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
        Field f[kMaxFields];
        const uint32_t n = instance_fields(L, 0, nullptr, nullptr, GV_NONE, f);
        bool ok = L.stride % 16 == 0 && L.stride >= kMinInstanceStride && L.stride <= kMaxInstanceStride;
        for (uint32_t i = 0; ok && i < n; i++)
            ok = f[i].at % f[i].align == 0 && f[i].at <= L.stride && f[i].bytes <= L.stride - f[i].at && !overlaps_any(f, i, f[i].at, f[i].bytes);
        if (!ok)
            return ctx->fail(GV_E_ARG, "gv_pool_set_instance_layout: stride %u (a multiple of 16, %u to %u) with mvp at %u (16-byte aligned) and "
                             "model / slot / distance_sq at %u / %u / %u (4-byte aligned, 0x%x: none): fields must lie inside the instance and "
                             "be disjoint", L.stride, kMinInstanceStride, kMaxInstanceStride, L.mvp, L.model, L.slot, L.distance_sq, GV_NONE);
    }
    if (layout && ctx->pools[pool_id].payload.count && !payload_fits(L, ctx->pools[pool_id].payload, ctx->pools[pool_id].payload.at))
        return ctx->fail(GV_E_ARG, "gv_pool_set_instance_layout: the payload destinations of pool %u (gv_pool_set_payload_layout) do not fit "
                         "this layout: they must lie inside the stride (%u) and be disjoint from mvp / model / slot / distance_sq", pool_id, L.stride);
    if (layout && ctx->pools[pool_id].instances.index_at != GV_NONE &&
        !index_fits(L, ctx->pools[pool_id].payload, ctx->pools[pool_id].payload.at, ctx->pools[pool_id].instances.index_at))
        return ctx->fail(GV_E_ARG, "gv_pool_set_instance_layout: the index field of pool %u at %u (gv_pool_set_instance_index_field) does not fit "
                         "this layout: it must lie inside the stride (%u) and be disjoint from mvp / model / slot / distance_sq", pool_id,
                         ctx->pools[pool_id].instances.index_at, L.stride);
    ctx->pools[pool_id].instances.layout = L;  // read by the next emission; an emission already made keeps the layout it was made with
    return GV_OK;
}

int gv_pool_emit_instances(GvCtx* ctx, uint32_t pool_id, const uint32_t* view_indices, uint32_t view_count, void* dst_device,
                           size_t capacity_bytes)
{
    const char* const fn = "gv_pool_emit_instances";
    bool with_payload = false;
    if (int rc = check_emission(ctx, fn, pool_id, view_indices, view_count, dst_device, &with_payload))
        return rc;
    PoolState& p = ctx->pools[pool_id];
    PoolState::Instances& I = p.instances;
    const GvInstanceLayout L = I.layout;
    if (p.ready.ptr && p.ready_many_count)
        return ctx->fail(GV_E_STATE, "gv_pool_emit_instances: the ready column of pool %u holds %u live counts above 1: such a draw takes several "
                         "instances, and the instance index of draw k is k only while every draw takes one (ready counts of 0 / 1 work)",
                         pool_id, p.ready_many_count);
    ZoneScope zone("Meshes Instances");
    if (int rc = flush_sorts(ctx))  // the emission is a read: recorded culls and deferred sorts first (as gv_pool_results_device)
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (p.payload.count)  // marks made since the cull are seen by this emission (the reference reads the component at draw time, mesh.cpp:592)
        if (int rc = upload_payload(ctx, p))
            return rc;
    InstanceLaunch launch{};
    uint64_t bound = 0;  // the host's upper bound of the total
    const uint32_t covered = fill_launch(ctx, p, view_indices, view_count, with_payload, GV_NONE, launch, bound);
    if (int rc = choose_target(ctx, dst_device, capacity_bytes, L.stride, bound, I.d_data, &launch.dst, &launch.capacity))
        return rc;
    GV_HIP(ctx, I.d_starts.reserve(GV_MAX_VIEWS + 1));
    launch.starts = I.d_starts.ptr;
    // fields and payload are disjoint and inside the stride: together as many bytes as the stride = all of it
    launch.staged = with_payload && covered == L.stride && L.stride <= kMaxStagedInstanceStride;
    GV_HIP(ctx, launch_instances(launch, ctx->stream));
    note_emission(ctx, p, launch, view_indices, view_count, with_payload, GV_NONE, false);
    return GV_OK;
}

int gv_pool_emit_draw_instances(GvCtx* ctx, uint32_t pool_id, const uint32_t* view_indices, uint32_t view_count, void* dst_device,
                                size_t capacity_bytes)
{
    static_assert(kDrawChunk % kInstanceBlock == 0, "a chunk is a whole number of draw_instances_kernel workgroups");
    const char* const fn = "gv_pool_emit_draw_instances";
    bool with_payload = false;
    if (int rc = check_emission(ctx, fn, pool_id, view_indices, view_count, dst_device, &with_payload))
        return rc;
    PoolState& p = ctx->pools[pool_id];
    PoolState::Instances& I = p.instances;
    PoolState::Counts& K = p.counts;
    const GvInstanceLayout L = I.layout;
    if (I.index_at != GV_NONE && !index_fits(L, p.payload, p.payload.at, I.index_at))
        return ctx->fail(GV_E_ARG, "gv_pool_emit_draw_instances: the index field of pool %u (offset %u) does not fit its instance layout (stride %u) "
                         "and payload destinations", pool_id, I.index_at, L.stride);
    const bool counted = p.ready.ptr != nullptr;
    if (counted && p.result_flags)
        return ctx->fail(GV_E_STATE, "gv_pool_emit_draw_instances: pool %u has a ready column AND a result mapping (gv_pool_set_result_mapping): "
                         "not available together", pool_id);
    if (counted && p.ready_over_count)
        return ctx->fail(GV_E_STATE, "gv_pool_emit_draw_instances: the ready column of pool %u holds %u live counts above the limit of %u "
                         "instances per draw (GV_MAX_DRAW_INSTANCES)", pool_id, p.ready_over_count, GV_MAX_DRAW_INSTANCES);
    if (counted)
        for (uint32_t k = 0; k < view_count; k++)
            if (int rc = column_covers(ctx, fn, kReadyColumn, pool_id, p.ready, p.occupancy, *view_of(ctx, pool_id, view_indices[k]), view_indices[k]))
                return rc;
    ZoneScope zone("Meshes Draw Instances");
    if (int rc = flush_sorts(ctx))  // the emission is a read: recorded culls and deferred sorts first (as gv_pool_results_device)
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (p.payload.count)  // marks made since the cull are seen by this emission (mesh.cpp:592)
        if (int rc = upload_payload(ctx, p))
            return rc;
    if (counted) {  // ... and so are the counts (getInstancesAsync is read at draw time, mesh.cpp:597); the first call uploads the column
        if (int rc = want_column(ctx, p, p.ready, K, upload_counts))
            return rc;
        // a mark made since the last gv_sync may have put a count above the limit into the mirror (ready_over_count has not seen it);
        // live: a candidate as of that sync, hence possibly a draw of the cull
        uint32_t over = 0;
        for (uint32_t slot : K.over)
            over += slot < p.ready_many.size() && (p.ready_many[slot] & PoolState::kReadyLive);
        if (over)
            return ctx->fail(GV_E_STATE, "gv_pool_emit_draw_instances: the ready column of pool %u holds %u live counts above the limit of %u "
                             "instances per draw (GV_MAX_DRAW_INSTANCES), marked since the last gv_sync", pool_id, over, GV_MAX_DRAW_INSTANCES);
    }
    DrawInstanceLaunch launch{};
    uint64_t slots = 0;  // the sum of the listed views' occupancies: the host's upper bound of the DRAWS
    const uint32_t covered = fill_launch(ctx, p, view_indices, view_count, with_payload, I.index_at, launch.base, slots);
    for (uint32_t k = 0; k < view_count; k++)
        launch.first_chunk[k + 1] = launch.first_chunk[k] + (view_of(ctx, pool_id, view_indices[k])->occupancy + kDrawChunk - 1) / kDrawChunk;
    // the host's upper bound of the INSTANCES: a view draws a slot at most once
    const uint64_t bound = counted ? (uint64_t)view_count * K.sum : slots;
    if (!dst_device && bound > UINT32_MAX)
        return ctx->fail(GV_E_STATE, "gv_pool_emit_draw_instances: %u views of pool %u may take %llu instances, more than 32 bits hold: pass a "
                         "caller-owned target (dst_device) sized for what is drawn", view_count, pool_id, (unsigned long long)bound);
    if (int rc = choose_target(ctx, dst_device, capacity_bytes, L.stride, bound, I.d_data, &launch.base.dst, &launch.base.capacity))
        return rc;
    GV_HIP(ctx, I.d_starts.reserve(GV_MAX_VIEWS + 1));
    GV_HIP(ctx, I.d_draw_starts.reserve(GV_MAX_VIEWS + 1));
    GV_HIP(ctx, I.d_first.reserve((size_t)slots + 1));
    GV_HIP(ctx, I.d_local.reserve(std::max<size_t>((size_t)launch.base.first_block[view_count] * kInstanceBlock, 1)));
    GV_HIP(ctx, I.d_chunk_total.reserve(std::max<size_t>(launch.first_chunk[view_count], 1)));
    launch.base.starts = I.d_starts.ptr;
    launch.draw_starts = I.d_draw_starts.ptr;
    launch.first_instance = I.d_first.ptr;
    launch.local = I.d_local.ptr;
    launch.chunk_total = I.d_chunk_total.ptr;
    launch.counts = counted ? K.d_column.ptr : nullptr;
    launch.index_at = I.index_at;
    launch.base.staged = covered == L.stride && L.stride <= kMaxStagedInstanceStride;
    GV_HIP(ctx, launch_draw_instances(launch, ctx->stream));
    note_emission(ctx, p, launch.base, view_indices, view_count, with_payload, I.index_at, true);
    return GV_OK;
}

int gv_pool_set_instance_index_field(GvCtx* ctx, uint32_t pool_id, uint32_t offset)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS)
        return ctx->fail(GV_E_ARG, "gv_pool_set_instance_index_field: pool %u out of range", pool_id);
    PoolState& p = ctx->pools[pool_id];
    if (offset != GV_NONE && !index_fits(p.instances.layout, p.payload, p.payload.at, offset))
        return ctx->fail(GV_E_ARG, "gv_pool_set_instance_index_field: offset %u must be 4-byte aligned, lie inside the instance (stride %u) and be "
                         "disjoint from mvp / model / slot / distance_sq and the payload destinations", offset, p.instances.layout.stride);
    p.instances.index_at = offset;  // read by the next draw emission
    return GV_OK;
}

int gv_pool_draw_bases_device(GvCtx* ctx, uint32_t pool_id, const void** first_instance, const void** draw_starts)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !first_instance || !draw_starts)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_bases_device: bad argument (pool %u)", pool_id);
    const PoolState::Instances& I = ctx->pools[pool_id].instances;
    if (!I.views || !I.draws)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_bases_device: the last emission of pool %u since its last gv_cull is not a draw emission "
                         "(gv_pool_emit_draw_instances)", pool_id);
    *first_instance = I.d_first.ptr;
    *draw_starts = I.d_draw_starts.ptr;
    return GV_OK;
}

int gv_pool_draw_bases_fetch(GvCtx* ctx, uint32_t pool_id, uint32_t* first_instance, uint32_t capacity, uint32_t* draw_starts,
                             uint32_t starts_capacity)
{
    if (!ctx)
        return GV_E_ARG;
    if (pool_id >= GV_MAX_POOLS || !draw_starts)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_bases_fetch: bad argument (pool %u)", pool_id);
    PoolState::Instances& I = ctx->pools[pool_id].instances;
    if (!I.views || !I.draws)
        return ctx->fail(GV_E_STATE, "gv_pool_draw_bases_fetch: the last emission of pool %u since its last gv_cull is not a draw emission "
                         "(gv_pool_emit_draw_instances)", pool_id);
    if (starts_capacity < I.views + 1)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_bases_fetch: room for %u starts, the emission listed %u views", starts_capacity, I.views);
    GV_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_staged(ctx, I.h_starts, GV_MAX_VIEWS + 1, I.d_draw_starts.ptr, I.views + 1))
        return rc;
    const uint32_t draws = I.h_starts.ptr[I.views];
    if (first_instance && capacity < (uint64_t)draws + 1)
        return ctx->fail(GV_E_ARG, "gv_pool_draw_bases_fetch: room for %u words, %u draws and the closing total", capacity, draws);
    if (first_instance) {
        if (int rc = fetch_staged(ctx, I.h_first, (size_t)draws + 1, I.d_first.ptr, (size_t)draws + 1, first_instance))
            return rc;
    }
    memcpy(draw_starts, I.h_starts.ptr, (I.views + 1) * sizeof(uint32_t));
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
    if (int rc = fetch_staged(ctx, I.h_starts, GV_MAX_VIEWS + 1, I.d_starts.ptr, I.views + 1))
        return rc;
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
    if (int rc = fetch_staged(ctx, I.h_data, (size_t)held * L.stride, I.target, (size_t)held * L.stride))
        return rc;
    Field f[kMaxFields];  // the layout's, the payload fields the emission wrote, the index field of a draw emission
    const uint32_t n = instance_fields(L, I.emitted_payload, I.emitted_at, I.emitted_bytes, I.emitted_index, f);
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
