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
#include "gv_device.hpp"

namespace gv {

// 16-byte slot of column c of the workgroup's instance i in the stage: rotated by i / 4 so that the 16 lanes of a store group
// (4 instances x 4 columns on the way out, 16 instances x 1 column on the way in) cover the 16 slots of a bank row
__device__ __forceinline__ uint32_t stage_slot(uint32_t i, uint32_t c) { return i * 4u + ((c + (i >> 2)) & 3u); }

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

}  // namespace gv
