// gv_previous.hip — gfx950 kernels of gv_pool_keep_models / gv_pool_forget_models / gv_pool_emit_previous: last frame's
// viewProj * model per draw, the second matrix a velocity pass needs, the rule in gv_device_math.hpp
// (previous_*). The history is one 64-byte row per POOL slot: the model a view delivered for the slot (words 0-11, verbatim), the
// epoch it was kept at (word 12), zeros (13-15) — one aligned 64-byte access both ways.
//
//   previous_keep_kernel     one lane per record. In: the slot and the three 16-byte stream loads of the model (a lane's rows are
//                            contiguous with its neighbours'). The row is built in LDS (stage_slot, as instance_kernel's mvp) so that
//                            four consecutive lanes store the four 16-byte pieces of ONE row: 16 whole rows per store instruction,
//                            where a lane storing its own row would touch 64 lines. A slot occurs at most once in a view: no two
//                            lanes write one row. Plain stores: a 128-byte line holds two rows, completed by whoever keeps the
//                            neighbour. 52 B in, 64 B out per record.
//   previous_emit_kernel     one lane per record. The slot, the model, then the slot's row — the one dependent load, four plain
//                            16-byte loads issued in front of the fma chains. Kept or fresh selects the OPERANDS of the sixteen
//                            chains (v_cndmask), nothing branches around them. prev_mvp leaves through the same stage as instance_kernel's mvp:
//                            nontemporal where the launch writes whole lines by itself (stride 64, no flag), plain stores
//                            otherwise (the rule above whole_lines in gv_instance.hip). A workgroup takes kPreviousEmitTiles
//                            tiles of 256 records one after the other. Kept draws: one ballot per wave and tile, summed in
//                            registers and LDS, ONE integer atomic add per workgroup. 52 + 64 B in, 64 B out per record.
//   previous_forget_kernel   one lane per slot of the range: the stamp word becomes 0.
// The grids are sized from the occupancy the view was culled with; a workgroup whose first record lies beyond the device count
// leaves after one wave-uniform load. Nothing waits for another workgroup; no scratch.
#include "gv_device.hpp"
#include "gv_previous_kernels.hpp"

namespace gv {

namespace {

__global__ __launch_bounds__(kPreviousBlock) void previous_keep_kernel(const PreviousKeep a)
{
    __shared__ float4 stage[kPreviousBlock * kPreviousRowPieces];
    __shared__ uint32_t slot_of[kPreviousBlock];
    const uint32_t n = min(*a.view.count, a.view.capacity);
    const uint32_t first = blockIdx.x * kPreviousBlock;
    if (first >= n)
        return;  // (the whole workgroup, after ONE load)
    const uint32_t k = first + threadIdx.x;
    uint32_t slot = kNoField;  // (at or beyond every coverage: a lane without a record stores nothing)
    float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
    if (k < n) {
        slot = stream_load(a.view.idx + k);
        const float4* rows = reinterpret_cast<const float4*>(a.view.model) + (size_t)k * 3;
        r0 = stream_load(rows);
        r1 = stream_load(rows + 1);
        r2 = stream_load(rows + 2);
    }
    stage[stage_slot(threadIdx.x, 0)] = r0;
    stage[stage_slot(threadIdx.x, 1)] = r1;
    stage[stage_slot(threadIdx.x, 2)] = r2;
    stage[stage_slot(threadIdx.x, 3)] = make_float4(__uint_as_float(a.epoch), 0.0f, 0.0f, 0.0f);
    slot_of[threadIdx.x] = slot;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kPreviousRowPieces; j++) {
        const uint32_t q = j * kPreviousBlock + threadIdx.x, i = q >> 2, c = q & 3u;
        const uint32_t s = slot_of[i];  // (four lanes read one word: a broadcast)
        if (s < a.slots)
            a.rows[(size_t)s * kPreviousRowPieces + c] = stage[stage_slot(i, c)];
    }
}

__global__ __launch_bounds__(kPreviousBlock) void previous_emit_kernel(const PreviousEmit a)
{
    __shared__ float4 stage[kPreviousBlock * 4];
    __shared__ uint32_t kept_of_wave[kPreviousBlock / 64u];
    const uint32_t n = min(*a.view.count, a.view.capacity);
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (counts[1] is added into: zeroed in front of the launch)
        a.counts[0] = n;
        a.counts[2] = min(n, a.capacity);
        a.counts[3] = a.report_epoch;
    }
    const bool whole_lines = a.stride == 64u && a.has_history == kNoField;  // (the rule above whole_lines in gv_instance.hip)
    uint32_t kept_here = 0;  // (wave-uniform) this wave's kept draws over the workgroup's tiles
    for (uint32_t t = 0; t < kPreviousEmitTiles; t++) {
        const uint32_t first = (blockIdx.x * kPreviousEmitTiles + t) * kPreviousBlock;
        if (first >= n)
            break;  // (the whole workgroup, after ONE load at its first tile: the grid is sized for the occupancy)
        const uint32_t k = first + threadIdx.x;
        const bool live = k < n;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0, h0 = r0, h1 = r0, h2 = r0, h3 = r0;
        bool kept = false;
        if (live) {
            const uint32_t slot = stream_load(a.view.idx + k);
            const float4* rows = reinterpret_cast<const float4*>(a.view.model) + (size_t)k * 3;
            r0 = stream_load(rows);
            r1 = stream_load(rows + 1);
            r2 = stream_load(rows + 2);
            const bool covered = a.epoch != 0u && slot < a.slots;  // (epoch 0 is wave-uniform: a cut or an empty history reads no row)
            if (covered) {  // (a gather: plain loads — next frame's keep writes the same lines)
                const float4* from = a.rows + (size_t)slot * kPreviousRowPieces;
                h0 = from[0];
                h1 = from[1];
                h2 = from[2];
                h3 = from[3];
            }
            kept = covered && __float_as_uint(h3.x) == a.epoch;
        }
        // fresh: the draw is taken as static in the world — its model relative to the kept camera (one add per component of c3)
        const float4 f2 = make_float4(r2.x, r2.y + a.d[0], r2.z + a.d[1], r2.w + a.d[2]);
        const float4 p0 = kept ? h0 : r0, p1 = kept ? h1 : r1, p2 = kept ? h2 : f2;
        // bakedModel: c0 = (p0.x p0.y p0.z), c1 = (p0.w p1.x p1.y), c2 = (p1.z p1.w p2.x), c3 = (p2.y p2.z p2.w); bottom row 0 0 0 1
        stage[stage_slot(threadIdx.x, 0)] = mvp_column(a.pvp, p0.x, p0.y, p0.z, 0.0f);
        stage[stage_slot(threadIdx.x, 1)] = mvp_column(a.pvp, p0.w, p1.x, p1.y, 0.0f);
        stage[stage_slot(threadIdx.x, 2)] = mvp_column(a.pvp, p1.z, p1.w, p2.x, 0.0f);
        stage[stage_slot(threadIdx.x, 3)] = mvp_column(a.pvp, p2.y, p2.z, p2.w, 1.0f);
        kept_here += (uint32_t)__popcll(__ballot(kept));
        __syncthreads();
        const uint32_t live_here = min(kPreviousBlock, n - first);
        const uint32_t room_here = a.capacity > first ? min(live_here, a.capacity - first) : 0u;  // items at or beyond the capacity are not written
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t q = j * kPreviousBlock + threadIdx.x, i = q >> 2, c = q & 3u;
            if (i < room_here) {
                float4* to = reinterpret_cast<float4*>(a.dst + (size_t)(first + i) * a.stride + a.prev_mvp) + c;
                if (whole_lines)
                    stream_store(to, stage[stage_slot(i, c)]);
                else
                    *to = stage[stage_slot(i, c)];
            }
        }
        if (a.has_history != kNoField && threadIdx.x < room_here)
            *reinterpret_cast<uint32_t*>(a.dst + (size_t)k * a.stride + a.has_history) = kept ? 1u : 0u;
        __syncthreads();  // (the next tile rewrites the stage)
    }
    // ONE integer atomic per workgroup: every add goes to one word, and same-address atomics are served one after the other (about
    // 10 ns each, measured: an add per wave, 33 000 of them at 2.1 M draws, took 340 us beside 50 us of streaming)
    if ((threadIdx.x & 63u) == 0)
        kept_of_wave[threadIdx.x >> 6] = kept_here;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < kPreviousBlock / 64u; w++)
            sum += kept_of_wave[w];
        if (sum)  // (integer sums do not depend on order)
            atomicAdd(a.counts + 1, sum);
    }
}

__global__ __launch_bounds__(kPreviousBlock) void previous_forget_kernel(float4* rows, uint32_t first, uint32_t count)
{
    const uint32_t i = blockIdx.x * kPreviousBlock + threadIdx.x;
    if (i < count)
        reinterpret_cast<uint32_t*>(rows)[((size_t)first + i) * (kPreviousRowBytes / 4) + kPreviousStampWord] = 0u;
}

uint32_t blocks_for(uint32_t items) { return std::max(1u, (uint32_t)(((size_t)items + kPreviousBlock - 1) / kPreviousBlock)); }

}  // namespace

hipError_t launch_previous_keep(const PreviousKeep& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(previous_keep_kernel, dim3(blocks_for(launch.view.capacity)), dim3(kPreviousBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_previous_emit(const PreviousEmit& launch, hipStream_t stream)
{
    const uint32_t groups = (uint32_t)(((size_t)launch.view.capacity + kPreviousEmitTiles * kPreviousBlock - 1) / (kPreviousEmitTiles * kPreviousBlock));
    hipLaunchKernelGGL(previous_emit_kernel, dim3(std::max(1u, groups)), dim3(kPreviousBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_previous_forget(float4* rows, uint32_t first, uint32_t count, hipStream_t stream)
{
    hipLaunchKernelGGL(previous_forget_kernel, dim3(blocks_for(count)), dim3(kPreviousBlock), 0, stream, rows, first, count);
    return hipGetLastError();
}

}  // namespace gv
