// gv_instance.hip — gfx950 kernel of gv_pool_emit_instances: the per-draw arithmetic the reference's plugins do at the top of
// drawAsync (sprite.cpp:107-108,122-126: instanceData[instanceIndex].mvp = viewProj * model, model completed at mesh.cpp:596),
// for every record of the listed views of one pool, written at the draw's instance index into the plugin's instance struct.
//
//   instance_kernel   one lane per record, 256-lane workgroups, ONE launch for all listed views. The grid is sized from the
//                     views' occupancies (the host's upper bound of the counts); a workgroup finds its view from first_block[],
//                     leaves after one wave-uniform load when its first record lies beyond its view's count, and otherwise
//                     adds up the device counts of the views in front of it (< 8 more loads: its base instance). Workgroup 0 also writes starts[].
//                     Per record 48 B of model as three 16-byte nontemporal loads (a lane's rows are contiguous with its
//                     neighbours': 3 KB per wave), view_proj wave-uniform (SGPRs), sixteen 4-term fma chains (DESIGN.md §4 item
//                     9). The four mvp columns go through LDS so that consecutive lanes store consecutive 16-byte pieces: with
//                     stride 64 and only mvp a wave writes 4 KB contiguous, 1 KB per store instruction (a lane storing its own
//                     64 bytes would touch 64 lines per instruction). The optional fields are stored by the record's own lane.
//
//   instance_kernel<true>   the same with the pool's payload (gv_pool_bind_payload): launched only when a payload destination is set.
//                     The lane loads the record's slot first and gathers the slot's packed row (16, 32 or 64 bytes: one sector)
//                     with 16-byte loads — the one dependent load of the kernel, issued in front of the mvp arithmetic so that the
//                     fma chains cover it. Where each 16-byte piece / each word of the row goes is a table the host made
//                     (piece_at / word_at, wave-uniform): no register is indexed dynamically. Two ways out:
//                       staged   the layout's fields and the payload cover the whole stride (the sprite struct: mvp 0, colour 64,
//                                uv 80, stride 96): every lane builds its WHOLE instance in LDS (256 x stride bytes, stride <= 128),
//                                then consecutive lanes store consecutive 16-byte pieces — the launch writes whole lines by
//                                itself, which is what makes the nontemporal stores right.
//                                Image layout: linear, piece q of the workgroup at byte 16 q, so that the way out (ds_read_b128,
//                                banks of 256 B) is conflict-free and needs no division by the piece count. On the way in
//                                (ds_write_b128: groups of 8 consecutive lanes, banks of 128 B) lanes are `stride` bytes apart:
//                                conflict-free at stride 80 and 112, 2-way at 96 (16 array cycles against the 13 the store's
//                                operand transfer takes anyway), and 8-way at 128 — there the piece index is XORed with the
//                                instance's low three bits, which makes both directions conflict-free.
//                       direct   otherwise: mvp as in instance_kernel<false>, the payload stored by the record's own lane with plain
//                                stores like the optional fields.
//
// Only the bytes of the layout's fields and of the payload destinations are written; instances at or beyond `capacity` are not
// written at all. The payload is opaque: moved as bit patterns (no arithmetic touches it), NaNs and -0 included.
//
//   draw_counts_kernel + draw_instances_kernel   gv_pool_emit_draw_instances: draw k takes count[visible_idx[k]] instances (the
//                     pool's mirrored ready column). Two launches, no atomics, no host read, no workgroup waits for another: a
//                     scan of the counts per chunk of 4096 records, then the expansion of every record's instance — built once in
//                     LDS — into its contiguous range of instances (described at the kernels, below instance_kernel).
#include "gv_device.hpp"

namespace gv {

// the row's pieces and words to where the host's tables send them; put4(offset, float4) / put1(offset, float) write into the instance
template <typename Put4, typename Put1>
__device__ __forceinline__ void place_payload(const InstanceLaunch& a, const float4 (&row)[4], Put4 put4, Put1 put1)
{
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        if (a.piece_at[j] != kNoPayloadPlace) {
            put4(a.piece_at[j], row[j]);
        } else {
            if (a.word_at[4 * j] != kNoPayloadPlace)
                put1(a.word_at[4 * j], row[j].x);
            if (a.word_at[4 * j + 1] != kNoPayloadPlace)
                put1(a.word_at[4 * j + 1], row[j].y);
            if (a.word_at[4 * j + 2] != kNoPayloadPlace)
                put1(a.word_at[4 * j + 2], row[j].z);
            if (a.word_at[4 * j + 3] != kNoPayloadPlace)
                put1(a.word_at[4 * j + 3], row[j].w);
        }
    }
}

template <bool kPayload>
__global__ __launch_bounds__(kInstanceBlock) void instance_kernel(const InstanceLaunch a)
{
    __shared__ float4 stage[kInstanceBlock * (kPayload ? kMaxStagedInstanceStride / 16 : 4)];
    // workgroup-uniform: this workgroup's view, the instances in front of it, the total
    uint32_t v = 0, base = 0;
#pragma unroll
    for (uint32_t k = 1; k < kMaxInstanceViews; k++)
        if (k < a.views && blockIdx.x >= a.first_block[k])
            v = k;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t at = 0;
        for (uint32_t k = 0; k < a.views; k++) {
            a.starts[k] = at;
            at += *a.view[k].count;
        }
        a.starts[a.views] = at;
    }
    const InstanceView& vw = a.view[v];
    const uint32_t n = *vw.count;
    const uint32_t first = (blockIdx.x - a.first_block[v]) * kInstanceBlock;
    if (first >= n)
        return;  // (the whole workgroup, after ONE load: the grid is sized for the occupancy, most of it holds no record)
    for (uint32_t k = 0; k < v; k++)
        base += *a.view[k].count;
    if (base + first >= a.capacity)
        return;  // (nothing of it fits)
    const uint32_t k = first + threadIdx.x;
    const bool live = k < n;
    float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
    [[maybe_unused]] uint32_t own_slot = 0;
    [[maybe_unused]] float4 row[4] = {r0, r0, r0, r0};
    if (live) {
        if constexpr (kPayload)
            own_slot = stream_load(vw.idx + k);
        const float4* rows = reinterpret_cast<const float4*>(vw.model) + (size_t)k * 3;
        r0 = stream_load(rows);
        r1 = stream_load(rows + 1);
        r2 = stream_load(rows + 2);
        if constexpr (kPayload) {  // (a gather: plain loads — the shadow passes' records name the same rows again)
            const float4* from = reinterpret_cast<const float4*>(a.payload_rows + (size_t)own_slot * a.payload_pitch);
            row[0] = from[0];
            if (a.payload_pitch > 16u)
                row[1] = from[1];
            if (a.payload_pitch > 32u) {
                row[2] = from[2];
                row[3] = from[3];
            }
        }
    }
    if constexpr (kPayload) {
        if (a.staged) {  // (wave-uniform) the whole instance through LDS, whole lines out
            const uint32_t rot = a.stride == 128u ? 7u : 0u;
            uint8_t* const mine = reinterpret_cast<uint8_t*>(stage) + threadIdx.x * a.stride;
            const uint32_t turn = threadIdx.x & rot;
            auto put4 = [&](uint32_t o, float4 v) { *reinterpret_cast<float4*>(mine + (((o >> 4) ^ turn) << 4)) = v; };
            auto put1 = [&](uint32_t o, float v) { *reinterpret_cast<float*>(mine + (((o >> 4) ^ turn) << 4) + (o & 15u)) = v; };
            put4(a.mvp, mvp_column(vw.view_proj, r0.x, r0.y, r0.z, 0.0f));
            put4(a.mvp + 16u, mvp_column(vw.view_proj, r0.w, r1.x, r1.y, 0.0f));
            put4(a.mvp + 32u, mvp_column(vw.view_proj, r1.z, r1.w, r2.x, 0.0f));
            put4(a.mvp + 48u, mvp_column(vw.view_proj, r2.y, r2.z, r2.w, 1.0f));
            if (a.model != kNoField) {
                if ((a.model & 15u) == 0) {
                    put4(a.model, r0);
                    put4(a.model + 16u, r1);
                    put4(a.model + 32u, r2);
                } else {
                    put1(a.model, r0.x); put1(a.model + 4u, r0.y); put1(a.model + 8u, r0.z); put1(a.model + 12u, r0.w);
                    put1(a.model + 16u, r1.x); put1(a.model + 20u, r1.y); put1(a.model + 24u, r1.z); put1(a.model + 28u, r1.w);
                    put1(a.model + 32u, r2.x); put1(a.model + 36u, r2.y); put1(a.model + 40u, r2.z); put1(a.model + 44u, r2.w);
                }
            }
            if (a.slot != kNoField)
                put1(a.slot, __uint_as_float(live && a.index_map ? a.index_map[own_slot] : own_slot));
            if (a.distance_sq != kNoField)
                put1(a.distance_sq, live ? __uint_as_float(stream_load(reinterpret_cast<const uint32_t*>(vw.dist) + k)) : 0.0f);
            place_payload(a, row, put4, put1);
            __syncthreads();
            const uint32_t pieces = a.stride >> 4;  // per instance: 5 .. 8
            const uint32_t room = min(min(kInstanceBlock, n - first), a.capacity - (base + first)) * pieces;
            float4* const out = reinterpret_cast<float4*>(a.dst + (size_t)(base + first) * a.stride);
#pragma unroll
            for (uint32_t j = 0; j < kMaxStagedInstanceStride / 16; j++) {
                const uint32_t q = j * kInstanceBlock + threadIdx.x;
                if (q < room)
                    stream_store(out + q, stage[q ^ ((q >> 3) & rot)]);
            }
            return;
        }
    }
    // bakedModel: c0 = (r0.x r0.y r0.z), c1 = (r0.w r1.x r1.y), c2 = (r1.z r1.w r2.x), c3 = (r2.y r2.z r2.w); bottom row 0 0 0 1
    stage[stage_slot(threadIdx.x, 0)] = mvp_column(vw.view_proj, r0.x, r0.y, r0.z, 0.0f);
    stage[stage_slot(threadIdx.x, 1)] = mvp_column(vw.view_proj, r0.w, r1.x, r1.y, 0.0f);
    stage[stage_slot(threadIdx.x, 2)] = mvp_column(vw.view_proj, r1.z, r1.w, r2.x, 0.0f);
    stage[stage_slot(threadIdx.x, 3)] = mvp_column(vw.view_proj, r2.y, r2.z, r2.w, 1.0f);
    __syncthreads();
    // Nontemporal stores only where the launch writes whole lines by itself (stride 64, mvp alone): with other fields or a wider
    // stride a line is completed by several store instructions, which the L2 merges when they are plain stores — as streaming
    // stores they left as partial writes (10^7 entities, 128-byte layout with all fields: 318 us against 53 us for the bare one)
    const bool whole_lines = a.stride == 64u && a.model == kNoField && a.slot == kNoField && a.distance_sq == kNoField;
    const uint32_t live_here = min(kInstanceBlock, n - first);
    const uint32_t room_here = min(live_here, a.capacity - (base + first));
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t q = j * kInstanceBlock + threadIdx.x, i = q >> 2, c = q & 3u;
        if (i < room_here) {
            float4* to = reinterpret_cast<float4*>(a.dst + (size_t)(base + first + i) * a.stride + a.mvp) + c;
            if (whole_lines)
                stream_store(to, stage[stage_slot(i, c)]);
            else
                *to = stage[stage_slot(i, c)];
        }
    }
    if (threadIdx.x >= room_here)
        return;
    uint8_t* inst = a.dst + (size_t)(base + k) * a.stride;
    if (a.model != kNoField) {
        if ((a.model & 15u) == 0) {  // (wave-uniform)
            float4* to = reinterpret_cast<float4*>(inst + a.model);
            to[0] = r0;
            to[1] = r1;
            to[2] = r2;
        } else {
            float* to = reinterpret_cast<float*>(inst + a.model);
            to[0] = r0.x; to[1] = r0.y; to[2] = r0.z; to[3] = r0.w;
            to[4] = r1.x; to[5] = r1.y; to[6] = r1.z; to[7] = r1.w;
            to[8] = r2.x; to[9] = r2.y; to[10] = r2.z; to[11] = r2.w;
        }
    }
    if constexpr (kPayload) {
        auto put4 = [&](uint32_t o, float4 v) { *reinterpret_cast<float4*>(inst + o) = v; };
        auto put1 = [&](uint32_t o, float v) { *reinterpret_cast<float*>(inst + o) = v; };
        place_payload(a, row, put4, put1);
    }
    if (a.slot != kNoField) {
        uint32_t slot = kPayload ? own_slot : stream_load(vw.idx + k);
        if (a.index_map)
            slot = a.index_map[slot];
        *reinterpret_cast<uint32_t*>(inst + a.slot) = slot;
    }
    if (a.distance_sq != kNoField)
        *reinterpret_cast<uint32_t*>(inst + a.distance_sq) = stream_load(reinterpret_cast<const uint32_t*>(vw.dist) + k);
}

hipError_t launch_instances(const InstanceLaunch& launch, hipStream_t stream)
{
    const dim3 grid(std::max(1u, launch.first_block[launch.views])), block(kInstanceBlock);  // (no record at all: starts[] still)
    if (launch.payload_rows)  // (set only when a payload destination is: everything else runs the kernel it always ran)
        hipLaunchKernelGGL(instance_kernel<true>, grid, block, 0, stream, launch);
    else
        hipLaunchKernelGGL(instance_kernel<false>, grid, block, 0, stream, launch);
    return hipGetLastError();
}

// ---- gv_pool_emit_draw_instances: draw k takes count[visible_idx[k]] instances -----------------------------------------------

// One workgroup per chunk of kDrawChunk records, 16 rounds of 256 consecutive records: the counts are gathered first (idx -> count,
// the one dependent load), every round is scanned inside its wave, the 64 (round, wave) totals by wave 0: two barriers in all.
__global__ __launch_bounds__(kInstanceBlock) void draw_counts_kernel(const DrawInstanceLaunch a)
{
    constexpr uint32_t kRounds = kDrawChunk / kInstanceBlock;
    static_assert(kRounds * (kInstanceBlock / 64u) == 64u, "wave 0 scans one (round, wave) total per lane");
    __shared__ uint32_t part[64];
    const uint32_t v = view_of_block(a.first_chunk, a.base.views, blockIdx.x);
    const InstanceView& vw = a.base.view[v];
    const uint32_t n = *vw.count;
    const uint32_t first = (blockIdx.x - a.first_chunk[v]) * kDrawChunk;
    if (first >= n) {  // (the whole workgroup, after ONE load) nothing here: the flat prefix over the table skips it
        if (threadIdx.x == 0)
            a.chunk_total[blockIdx.x] = 0;
        return;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t slot[kRounds], c[kRounds], inc[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t k = first + r * kInstanceBlock + threadIdx.x;
        slot[r] = k < n ? stream_load(vw.idx + k) : kNoField;
    }
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++)
        c[r] = slot[r] == kNoField ? 0u : (a.counts ? a.counts[slot[r]] : 1u);
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        inc[r] = wave_inclusive_scan(c[r], lane);
        if (lane == 63u)
            part[r * (kInstanceBlock / 64u) + wave] = inc[r];
    }
    const uint32_t chunk_sum = chunk_scan_tail(part, lane, wave);
    uint32_t* const local = a.local + (size_t)a.base.first_block[v] * kInstanceBlock;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t k = first + r * kInstanceBlock + threadIdx.x;
        if (k < n)
            local[k] = part[r * (kInstanceBlock / 64u) + wave] + inc[r] - c[r];
    }
    if (threadIdx.x == 0)
        a.chunk_total[blockIdx.x] = chunk_sum;
}

// the record that owns instance g: the last r of [0, 256) with pre[r] <= g (pre ascending, pre[0] <= g < pre[256]); records
// that take no instance share their successor's pre and are skipped by construction. 8 steps.
__device__ __forceinline__ uint32_t owner_of(const uint32_t* pre, uint32_t g)
{
    uint32_t r = 0;
#pragma unroll
    for (uint32_t step = kInstanceBlock / 2; step >= 1u; step >>= 1)
        if (pre[r + step] <= g)
            r += step;
    return r;
}

// The staged image: record t at byte t * stride, its 16-byte pieces XORed with image_turn so that the eight lanes of a
// ds_write_b128 group (128-byte bank rows) land on eight different slots: lanes are one stride apart, which is conflict-free as it is
// at stride 80 and 112 and 2-way at 96; at 128 the eight lanes would share a slot (t & 7 spreads them), at 64 every second pair
// would ((t >> 1) & 3 spreads the four pairs). The way out reads whole records' pieces in order, whatever their permutation.
__device__ __forceinline__ uint32_t image_turn(uint32_t stride, uint32_t t)
{
    return stride == 128u ? (t & 7u) : (stride == 64u ? ((t >> 1) & 3u) : 0u);
}

__device__ __forceinline__ float4 with_word(float4 v, uint32_t word, uint32_t value)
{
    const float f = __uint_as_float(value);
    if (word == 0) v.x = f;
    if (word == 1) v.y = f;
    if (word == 2) v.z = f;
    if (word == 3) v.w = f;
    return v;
}

// One workgroup per 256 records. The record's lane builds the instance ONCE in LDS (image) next to the 257-entry prefix of the
// workgroup's first instances (pre); then the workgroup walks its contiguous output range [pre[0], pre[256]) in strides of its size,
// every lane finding the owning record of its output instance in pre.
//   staged   the image is the instance itself (record t at t * stride, its pieces XORed with image_turn: instance_kernel<true>'s
//            image, and at stride 64 rotated per pair of records — conflict-free on the way in); consecutive lanes copy consecutive 16-byte pieces of consecutive instances,
//            nontemporal: whole lines. The index word is patched into its piece per instance.
//   direct   the image is piece-major (piece p of record t at p * 256 + t: conflict-free both ways): mvp 0-3, model 4-6,
//            (slot, distance_sq) 7, payload row 8-11. mvp goes out as (instance, column) pairs, the rest by one lane per instance with
//            plain stores.
__global__ __launch_bounds__(kInstanceBlock) void draw_instances_kernel(const DrawInstanceLaunch a)
{
    static_assert((kInstanceBlock + 1 + kInstanceBlock / 64u + 1) * 4u <= kDrawLdsTail && kDrawLdsTail % 16u == 0, "pre and scratch behind the image");
    extern __shared__ __attribute__((aligned(16))) uint8_t draw_lds[];  // (all of the LDS: the dynamic base stays 16-byte aligned)
    const InstanceLaunch& L = a.base;
    float4* const image = reinterpret_cast<float4*>(draw_lds);
    uint32_t* const pre = reinterpret_cast<uint32_t*>(draw_lds + draw_image_bytes(L.staged, L.stride));
    uint32_t* const scratch = pre + kInstanceBlock + 1;
    const uint32_t v = view_of_block(L.first_block, L.views, blockIdx.x);
    const InstanceView& vw = L.view[v];
    const uint32_t n = *vw.count;
    const uint32_t first = (blockIdx.x - L.first_block[v]) * kInstanceBlock;
    const bool opens = blockIdx.x == L.first_block[v], closes = blockIdx.x == gridDim.x - 1u;
    if (first >= n && !opens && !closes)
        return;  // (the whole workgroup, after ONE load)
    const uint32_t chunk = a.first_chunk[v] + first / kDrawChunk;
    const uint32_t base = block_sum_of(a.chunk_total, 0, chunk, scratch);  // instances in front of this workgroup's chunk
    uint32_t draws_before = 0;
    for (uint32_t k = 0; k < v; k++)
        draws_before += *L.view[k].count;
    if (opens && threadIdx.x == 0) {  // (first == 0: base is where the view begins) also for views in front that have no workgroup
        for (uint32_t k = 0; k <= v; k++)
            if (L.first_block[k] == blockIdx.x) {
                L.starts[k] = base;
                a.draw_starts[k] = draws_before;
            }
    }
    if (closes) {  // the closing totals, and the views behind that have no workgroup
        const uint32_t total = base + block_sum_of(a.chunk_total, chunk, a.first_chunk[L.views], scratch);
        if (threadIdx.x == 0) {
            uint32_t draws = draws_before;
            for (uint32_t k = v; k < L.views; k++) {
                draws += *L.view[k].count;
                L.starts[k + 1] = total;
                a.draw_starts[k + 1] = draws;
            }
            a.first_instance[draws] = total;
        }
    }
    if (first >= n)
        return;
    const uint32_t k = first + threadIdx.x;
    const bool live = k < n;
    const uint32_t live_here = min(kInstanceBlock, n - first);
    float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
    float4 row[4] = {r0, r0, r0, r0};
    uint32_t own_slot = 0, mine = 0, take = 0;
    if (live) {
        own_slot = stream_load(vw.idx + k);
        const float4* rows = reinterpret_cast<const float4*>(vw.model) + (size_t)k * 3;
        r0 = stream_load(rows);
        r1 = stream_load(rows + 1);
        r2 = stream_load(rows + 2);
        mine = base + stream_load(a.local + (size_t)L.first_block[v] * kInstanceBlock + k);
        if (threadIdx.x == live_here - 1u)  // (the one lane that closes the prefix)
            take = a.counts ? a.counts[own_slot] : 1u;
        if (L.payload_rows) {  // (a gather, issued in front of the fma chains)
            const float4* from = reinterpret_cast<const float4*>(L.payload_rows + (size_t)own_slot * L.payload_pitch);
            row[0] = from[0];
            if (L.payload_pitch > 16u)
                row[1] = from[1];
            if (L.payload_pitch > 32u) {
                row[2] = from[2];
                row[3] = from[3];
            }
        }
        a.first_instance[draws_before + k] = mine;
        pre[threadIdx.x] = mine;
        if (threadIdx.x == live_here - 1u)
            scratch[kInstanceBlock / 64u] = mine + take;
    }
    __syncthreads();
    const uint32_t begin = pre[0], end = scratch[kInstanceBlock / 64u];
    if (!live)
        pre[threadIdx.x] = end;
    if (threadIdx.x == 0)
        pre[kInstanceBlock] = end;
    const uint32_t room_end = min(end, L.capacity);  // instances at or beyond the capacity are not written
    if (begin >= room_end)
        return;  // (workgroup-uniform) only draws without an instance, or nothing of it fits
    // every draw of the workgroup takes ONE instance (the common case): instance i belongs to record i, nothing is searched
    const bool ones = __syncthreads_and(!live || mine == begin + threadIdx.x) && end == begin + live_here;
    const float4 c0 = mvp_column(vw.view_proj, r0.x, r0.y, r0.z, 0.0f), c1 = mvp_column(vw.view_proj, r0.w, r1.x, r1.y, 0.0f);
    const float4 c2 = mvp_column(vw.view_proj, r1.z, r1.w, r2.x, 0.0f), c3 = mvp_column(vw.view_proj, r2.y, r2.z, r2.w, 1.0f);
    const uint32_t slot_out = live && L.slot != kNoField && L.index_map ? L.index_map[own_slot] : own_slot;
    const uint32_t dist = live && (L.distance_sq != kNoField) ? stream_load(reinterpret_cast<const uint32_t*>(vw.dist) + k) : 0u;
    if (L.staged) {  // (wave-uniform)
        if (live) {
            uint8_t* const at = reinterpret_cast<uint8_t*>(image) + threadIdx.x * L.stride;
            const uint32_t turn = image_turn(L.stride, threadIdx.x);
            auto put4 = [&](uint32_t o, float4 x) { *reinterpret_cast<float4*>(at + (((o >> 4) ^ turn) << 4)) = x; };
            auto put1 = [&](uint32_t o, float x) { *reinterpret_cast<float*>(at + (((o >> 4) ^ turn) << 4) + (o & 15u)) = x; };
            put4(L.mvp, c0);
            put4(L.mvp + 16u, c1);
            put4(L.mvp + 32u, c2);
            put4(L.mvp + 48u, c3);
            if (L.model != kNoField) {
                if ((L.model & 15u) == 0) {
                    put4(L.model, r0);
                    put4(L.model + 16u, r1);
                    put4(L.model + 32u, r2);
                } else {
                    put1(L.model, r0.x); put1(L.model + 4u, r0.y); put1(L.model + 8u, r0.z); put1(L.model + 12u, r0.w);
                    put1(L.model + 16u, r1.x); put1(L.model + 20u, r1.y); put1(L.model + 24u, r1.z); put1(L.model + 28u, r1.w);
                    put1(L.model + 32u, r2.x); put1(L.model + 36u, r2.y); put1(L.model + 40u, r2.z); put1(L.model + 44u, r2.w);
                }
            }
            if (L.slot != kNoField)
                put1(L.slot, __uint_as_float(slot_out));
            if (L.distance_sq != kNoField)
                put1(L.distance_sq, __uint_as_float(dist));
            if (L.payload_rows)
                place_payload(L, row, put4, put1);
        }
        __syncthreads();
        const uint32_t pieces = L.stride >> 4;  // per instance: 4 .. 8
        const uint32_t index_piece = a.index_at == kNoField ? kNoField : a.index_at >> 4, index_word = (a.index_at >> 2) & 3u;
        // in spans of 2^24 instances, so that the piece index stays a 32-bit number whatever the counts are (one span unless a
        // workgroup's draws take more: the host refuses counts above GV_MAX_DRAW_INSTANCES, the kernel does not rely on it)
        constexpr uint32_t kSpan = 1u << 24;
        for (uint32_t from = begin; from < room_end; from += min(kSpan, room_end - from)) {
            const uint32_t room = min(kSpan, room_end - from) * pieces;
            float4* const out = reinterpret_cast<float4*>(L.dst + (size_t)from * L.stride);
            for (uint32_t q = threadIdx.x; q < room; q += kInstanceBlock) {
                // (divisions by constants: the piece count is wave-uniform)
                const uint32_t i = pieces == 8u ? q >> 3 : (pieces == 4u ? q >> 2 : (pieces == 6u ? q / 6u : (pieces == 5u ? q / 5u : q / 7u)));
                const uint32_t j = q - i * pieces, g = from + i;
                const uint32_t r = ones ? g - begin : owner_of(pre, g);
                float4 x = *reinterpret_cast<const float4*>(reinterpret_cast<const uint8_t*>(image) + r * L.stride +
                                                            ((j ^ image_turn(L.stride, r)) << 4));
                if (j == index_piece)
                    x = with_word(x, index_word, ones ? 0u : g - pre[r]);
                stream_store(out + q, x);
            }
        }
        return;
    }
    if (live) {
        image[0 * kInstanceBlock + threadIdx.x] = c0;
        image[1 * kInstanceBlock + threadIdx.x] = c1;
        image[2 * kInstanceBlock + threadIdx.x] = c2;
        image[3 * kInstanceBlock + threadIdx.x] = c3;
        image[4 * kInstanceBlock + threadIdx.x] = r0;
        image[5 * kInstanceBlock + threadIdx.x] = r1;
        image[6 * kInstanceBlock + threadIdx.x] = r2;
        image[7 * kInstanceBlock + threadIdx.x] = make_float4(__uint_as_float(slot_out), __uint_as_float(dist), 0.0f, 0.0f);
        image[8 * kInstanceBlock + threadIdx.x] = row[0];
        image[9 * kInstanceBlock + threadIdx.x] = row[1];
        image[10 * kInstanceBlock + threadIdx.x] = row[2];
        image[11 * kInstanceBlock + threadIdx.x] = row[3];
    }
    __syncthreads();
    const uint32_t room = room_end - begin;
    // (64-bit loop counters: no count, however large, makes a 32-bit one wrap in front of `room`)
    for (uint64_t q = threadIdx.x; q < (uint64_t)room * 4u; q += kInstanceBlock) {  // (instance, column) pairs
        const uint32_t g = begin + (uint32_t)(q >> 2), c = (uint32_t)q & 3u;
        const uint32_t r = ones ? (uint32_t)(q >> 2) : owner_of(pre, g);
        *(reinterpret_cast<float4*>(L.dst + (size_t)g * L.stride + L.mvp) + c) = image[c * kInstanceBlock + r];
    }
    const bool rest = L.model != kNoField || L.slot != kNoField || L.distance_sq != kNoField || L.payload_rows || a.index_at != kNoField;
    if (!rest)
        return;
    for (uint64_t at = threadIdx.x; at < room; at += kInstanceBlock) {
        const uint32_t i = (uint32_t)at, g = begin + i;
        const uint32_t r = ones ? i : owner_of(pre, g);
        uint8_t* const inst = L.dst + (size_t)g * L.stride;
        if (L.model != kNoField) {
            const float4 m0 = image[4 * kInstanceBlock + r], m1 = image[5 * kInstanceBlock + r], m2 = image[6 * kInstanceBlock + r];
            if ((L.model & 15u) == 0) {  // (wave-uniform)
                float4* to = reinterpret_cast<float4*>(inst + L.model);
                to[0] = m0;
                to[1] = m1;
                to[2] = m2;
            } else {
                float* to = reinterpret_cast<float*>(inst + L.model);
                to[0] = m0.x; to[1] = m0.y; to[2] = m0.z; to[3] = m0.w;
                to[4] = m1.x; to[5] = m1.y; to[6] = m1.z; to[7] = m1.w;
                to[8] = m2.x; to[9] = m2.y; to[10] = m2.z; to[11] = m2.w;
            }
        }
        if (L.payload_rows) {
            const float4 held[4] = {image[8 * kInstanceBlock + r], image[9 * kInstanceBlock + r], image[10 * kInstanceBlock + r],
                                    image[11 * kInstanceBlock + r]};
            auto put4 = [&](uint32_t o, float4 x) { *reinterpret_cast<float4*>(inst + o) = x; };
            auto put1 = [&](uint32_t o, float x) { *reinterpret_cast<float*>(inst + o) = x; };
            place_payload(L, held, put4, put1);
        }
        if (L.slot != kNoField || L.distance_sq != kNoField) {
            const float4 sd = image[7 * kInstanceBlock + r];
            if (L.slot != kNoField)
                *reinterpret_cast<float*>(inst + L.slot) = sd.x;
            if (L.distance_sq != kNoField)
                *reinterpret_cast<float*>(inst + L.distance_sq) = sd.y;
        }
        if (a.index_at != kNoField)
            *reinterpret_cast<uint32_t*>(inst + a.index_at) = ones ? 0u : g - pre[r];
    }
}

hipError_t launch_draw_instances(const DrawInstanceLaunch& launch, hipStream_t stream)
{
    const dim3 block(kInstanceBlock);
    if (launch.first_chunk[launch.base.views])
        hipLaunchKernelGGL(draw_counts_kernel, dim3(launch.first_chunk[launch.base.views]), block, 0, stream, launch);
    hipLaunchKernelGGL(draw_instances_kernel, dim3(std::max(1u, launch.base.first_block[launch.base.views])), block,
                       draw_image_bytes(launch.base.staged, launch.base.stride) + kDrawLdsTail, stream, launch);
    return hipGetLastError();
}

}  // namespace gv
