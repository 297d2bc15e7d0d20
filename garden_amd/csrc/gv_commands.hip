// gv_commands.hip — gfx950 kernels of gv_pool_emit_draw_commands: one indirect command per draw of the pool's last emission (or per
// run of consecutive draws of one geometry id), in the caller's command struct, built on the device.
// The rule holds no arithmetic: a command is the geometry table's entry of the draw's id beside the instance range the emission
// gave the draw.
//
//   command_kernel        one lane per command POSITION, 256 per workgroup, serves both modes. Per lane: draw_of[j] -> idx -> id (the
//                         one dependent gather) -> the 12-byte table entry (at most 768 KB: cache-resident); first_of[j] and
//                         first_of[j + 1] give the instance range. In per-draw mode draw_of is the identity and first_of the
//                         emission's first_instance[] (or starts[v] + k): ONE launch, no scan. The workgroup builds its 256
//                         commands in LDS (256 x stride <= 16 KB), every byte of the stride, then consecutive lanes store
//                         consecutive 16-byte pieces (where the workgroup's byte range is 16-byte aligned) or dwords: a 20-byte
//                         stride leaves as 5 120 contiguous bytes per workgroup, not as five 4-byte stores 20 bytes apart per lane.
//                         With regions the same launch writes the all-zero padding commands. Workgroup 0 writes command_counts[].
//   command_heads_kernel  run mode. One workgroup per chunk of kDrawChunk draws, 16 rounds of 256: idx -> id, head flag from
//                         id[k] != id[k - 1] (a wave's first lane takes its predecessor's id from LDS, the chunk's first lane gathers
//                         it), chunk-local exclusive head rank by ballot + popcount and a scan of the 64 (round, wave) totals by
//                         wave 0, as draw_counts_kernel scans. One head total per chunk, 0 beyond the view's count.
//   command_runs_kernel   run mode. One workgroup per 256 draws: adds up its view's chunk totals in front of its chunk; every head
//                         writes draw_of[rank] = k and first_of[rank] = first_k.
//
// Behind a LOD selection (gv_pool_select_lods, CommandLaunch::draw_ids) command_kernel<true> and command_heads_kernel<true> take the
// id of draw k of view v from draw_ids[D_v + k] (D_v: at most 7 count loads) instead of the slot gather — a coalesced stream; the
// <false> instantiations are the kernels as they were (same registers, same occupancy: DESIGN.md §5.14).
//
// No atomics, no workgroup waits for another, no host read; grids sized from the views' occupancies, workgroups beyond a view's
// device count leave after one wave-uniform load. Whatever an id holds, the table is read inside [0, table_count) only.
#include "gv_device.hpp"

namespace gv {

namespace {

__device__ __forceinline__ uint32_t geometry_id(const CommandLaunch& a, uint32_t slot) { return a.ids ? a.ids[slot] : 0u; }

// behind a LOD selection (the kLod instantiations): where the selected ids of view v begin, D_v draws into draw_ids
__device__ __forceinline__ const uint32_t* draw_ids_of(const CommandLaunch& a, uint32_t v)
{
    uint32_t at = 0;
    for (uint32_t u = 0; u < v; u++)
        at += *a.view[u].count;
    return a.draw_ids + at;
}

// draw k of view v: the first instance the emission gave it
__device__ __forceinline__ uint32_t first_of_draw(const CommandLaunch& a, uint32_t v, uint32_t k)
{
    return a.first_instance_of ? a.first_instance_of[a.draw_starts[v] + k] : a.starts[v] + k;
}

template <bool kLod>
__global__ __launch_bounds__(kCommandBlock) void command_heads_kernel(const CommandLaunch a)
{
    constexpr uint32_t kRounds = kDrawChunk / kCommandBlock, kWaves = kCommandBlock / 64u;
    static_assert(kRounds * kWaves == 64u, "wave 0 scans one (round, wave) total per lane");
    __shared__ uint32_t tail[64];  // the id of every (round, wave)'s last lane
    __shared__ uint32_t part[64];
    const uint32_t v = view_of_block(a.first_chunk, a.views, blockIdx.x);
    const CommandView& vw = a.view[v];
    const uint32_t n = *vw.count;
    const uint32_t first = (blockIdx.x - a.first_chunk[v]) * kDrawChunk;
    if (first >= n) {  // (the whole workgroup, after ONE load) nothing here: the prefix over the table skips it
        if (threadIdx.x == 0)
            a.chunk_total[blockIdx.x] = 0;
        return;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t id[kRounds];
    uint32_t before = 0;  // the id of the draw in front of the chunk
    if constexpr (kLod) {  // the selected ids, draw-indexed: no gather
        const uint32_t* const ids = draw_ids_of(a, v);
#pragma unroll
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint32_t k = first + r * kCommandBlock + threadIdx.x;
            id[r] = k < n ? stream_load(ids + k) : 0u;
        }
        if (threadIdx.x == 0 && first > 0)
            before = ids[first - 1];
    } else {
#pragma unroll
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint32_t k = first + r * kCommandBlock + threadIdx.x;
            id[r] = k < n ? stream_load(vw.idx + k) : kNoField;  // (the slot, for now)
        }
        if (threadIdx.x == 0 && first > 0)
            before = geometry_id(a, vw.idx[first - 1]);
    }
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        if constexpr (!kLod)
            id[r] = id[r] == kNoField ? 0u : geometry_id(a, id[r]);
        if (lane == 63u)
            tail[r * kWaves + wave] = id[r];
    }
    __syncthreads();
    uint32_t heads = 0, below[kRounds];  // bit r: draw (r, lane) opens a run; heads in front of it inside its wave
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t k = first + r * kCommandBlock + threadIdx.x, q = r * kWaves + wave;
        uint32_t prev = __shfl_up(id[r], 1, 64);
        if (lane == 0)
            prev = q ? tail[q - 1] : before;
        const bool head = k < n && (k == 0 || id[r] != prev);
        const unsigned long long m = __ballot(head);
        below[r] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        heads |= head ? 1u << r : 0u;
        if (lane == 0)
            part[q] = (uint32_t)__popcll(m);
    }
    const uint32_t chunk_sum = chunk_scan_tail(part, lane, wave);
    uint32_t* const rank = a.rank + (size_t)a.first_draw_block[v] * kCommandBlock;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t k = first + r * kCommandBlock + threadIdx.x;
        if (k < n)
            rank[k] = (part[r * kWaves + wave] + below[r]) | (((heads >> r) & 1u) ? kCommandHead : 0u);
    }
    if (threadIdx.x == 0)
        a.chunk_total[blockIdx.x] = chunk_sum;
}

__global__ __launch_bounds__(kCommandBlock) void command_runs_kernel(const CommandLaunch a)
{
    __shared__ uint32_t scratch[kCommandBlock / 64u];
    const uint32_t v = view_of_block(a.first_draw_block, a.views, blockIdx.x);
    const uint32_t n = *a.view[v].count;
    const uint32_t first = (blockIdx.x - a.first_draw_block[v]) * kCommandBlock;
    if (first >= n)
        return;  // (the whole workgroup, after ONE load)
    const uint32_t base = block_sum_of(a.chunk_total, a.first_chunk[v], a.first_chunk[v] + first / kDrawChunk, scratch);  // runs of the view in front
    const uint32_t k = first + threadIdx.x;
    if (k >= n)
        return;
    const size_t at = (size_t)a.first_draw_block[v] * kCommandBlock;
    const uint32_t w = stream_load(a.rank + at + k);
    if (w & kCommandHead) {
        const size_t run = at + v + base + (w & ~kCommandHead);
        a.draw_of[run] = k;
        a.first_of[run] = first_of_draw(a, v, k);
    }
}

template <bool kLod>
__global__ __launch_bounds__(kCommandBlock) void command_kernel(const CommandLaunch a)
{
    __shared__ __attribute__((aligned(16))) uint32_t image[kCommandBlock * kMaxCommandStride / 4u];
    __shared__ uint32_t scratch[kCommandBlock / 64u];
    if (blockIdx.x == 0) {  // command_counts[]: the true counts, whatever fits
        for (uint32_t u = 0; u < a.views; u++) {
            const uint32_t c = a.merge_runs ? block_sum_of(a.chunk_total, a.first_chunk[u], a.first_chunk[u + 1], scratch) : *a.view[u].count;
            if (threadIdx.x == 0)
                a.command_counts[u] = c;
        }
    }
    const uint32_t v = view_of_block(a.first_block, a.views, blockIdx.x);
    const uint32_t first = (blockIdx.x - a.first_block[v]) * kCommandBlock;
    const uint32_t region = a.region;
    if (region && first >= region)
        return;
    const uint32_t n = *a.view[v].count;
    if (!region && first >= n)
        return;  // (the whole workgroup, after ONE load: the grid is sized for the occupancy)
    const uint32_t commands = a.merge_runs ? block_sum_of(a.chunk_total, a.first_chunk[v], a.first_chunk[v + 1], scratch) : n;  // C_v
    if (!region && first >= commands)
        return;
    // where the workgroup's positions begin and how many it writes
    uint32_t at = v * region;
    if (!region) {
        if (a.merge_runs) {
            at = block_sum_of(a.chunk_total, 0, a.first_chunk[v], scratch);
        } else {
            for (uint32_t u = 0; u < v; u++)
                at += *a.view[u].count;
        }
    }
    at += first;
    if (at >= a.capacity)
        return;  // (nothing of it fits)
    const uint32_t here = min(min(kCommandBlock, (region ? region : commands) - first), a.capacity - at);
    const uint32_t words = a.stride / 4u;
    [[maybe_unused]] const uint32_t* ids_of_view = nullptr;
    if constexpr (kLod)
        ids_of_view = draw_ids_of(a, v);
    if (threadIdx.x < here) {
        uint32_t* const mine = image + threadIdx.x * words;
        for (uint32_t w = 0; w < words; w++)
            mine[w] = 0u;  // (every byte of the stride; a padding position stays all zero)
        const uint32_t j = first + threadIdx.x;
        if (j < commands) {
            uint32_t k = j, from, next;
            if (a.merge_runs) {
                const size_t run = (size_t)a.first_draw_block[v] * kCommandBlock + v + j;
                k = a.draw_of[run];
                from = a.first_of[run];
                next = j + 1u < commands ? a.first_of[run + 1] : a.starts[v + 1];
            } else {
                from = first_of_draw(a, v, k);
                next = k + 1u < n ? first_of_draw(a, v, k + 1u) : a.starts[v + 1];
            }
            uint32_t id;
            if constexpr (kLod)
                id = ids_of_view[k];
            else
                id = geometry_id(a, a.view[v].idx[k]);
            const bool known = id < a.table_count;
            CommandGeometry g{0u, 0u, 0};
            if (known)
                g = a.table[id];
            mine[a.count / 4u] = g.count;
            mine[a.instance_count / 4u] = known ? next - from : 0u;
            mine[a.first / 4u] = g.first;
            mine[a.first_instance / 4u] = from;
            if (a.vertex_offset != kNoField)
                mine[a.vertex_offset / 4u] = (uint32_t)g.vertex_offset;
            if (a.draw != kNoField)
                mine[a.draw / 4u] = k;
        }
    }
    __syncthreads();
    // out: the workgroup's positions are one contiguous byte range
    const size_t byte_at = (size_t)at * a.stride;
    const uint32_t total = here * words;
    uint32_t done = 0;
    if ((byte_at & 15u) == 0) {
        float4* const to = reinterpret_cast<float4*>(a.dst + byte_at);
        const float4* const from = reinterpret_cast<const float4*>(image);
        for (uint32_t q = threadIdx.x; q < total / 4u; q += kCommandBlock)
            to[q] = from[q];
        done = total & ~3u;
    }
    uint32_t* const to = reinterpret_cast<uint32_t*>(a.dst + byte_at);
    for (uint32_t w = done + threadIdx.x; w < total; w += kCommandBlock)
        to[w] = image[w];
}

}  // namespace

hipError_t launch_command_heads(const CommandLaunch& launch, hipStream_t stream)
{
    if (launch.draw_ids)
        hipLaunchKernelGGL(command_heads_kernel<true>, dim3(launch.first_chunk[launch.views]), dim3(kCommandBlock), 0, stream, launch);
    else
        hipLaunchKernelGGL(command_heads_kernel<false>, dim3(launch.first_chunk[launch.views]), dim3(kCommandBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_command_runs(const CommandLaunch& launch, hipStream_t stream)
{
    hipLaunchKernelGGL(command_runs_kernel, dim3(launch.first_draw_block[launch.views]), dim3(kCommandBlock), 0, stream, launch);
    return hipGetLastError();
}

hipError_t launch_commands(const CommandLaunch& launch, hipStream_t stream)
{
    const dim3 grid(std::max(1u, launch.first_block[launch.views]));
    if (launch.draw_ids)
        hipLaunchKernelGGL(command_kernel<true>, grid, dim3(kCommandBlock), 0, stream, launch);
    else
        hipLaunchKernelGGL(command_kernel<false>, grid, dim3(kCommandBlock), 0, stream, launch);
    return hipGetLastError();
}

}  // namespace gv
