// gv_delta.hip — gfx950 (CDNA4, wave64) kernels of gv_pool_view_delta: the difference between the set of pool slots the listed views
// hold now (C) and the set a channel kept from its last call (P). A set is one bit per POOL slot.
//
//   delta_mark_records_kernel   an emitted view's RECORDS -> bits of C (second_seen_kernel's shape, without the slot -> entry table).
//   delta_mark_bytes_kernel     a count-only main view's isVisible bytes (mirror order) -> bits of C, through the entry -> slot table
//                               or, for a mirror in slot order, as one ballot word per wave.
//   delta_count_kernel          per workgroup of kDeltaGroupSlots slots: |C \ P|, |P \ C| and |C| of its words.
//   delta_place_kernel          each workgroup sums the totals in front of it and writes its slots in ascending order; workgroup 0
//                               writes the four counts.
//
// Policy as gv_cull.hip / gv_second.hip: static work assignment, no workgroup waits for another, atomics only OR integers and never
// decide a place. Every output word is a function of the two sets alone.
#include "gv_delta_kernels.hpp"

namespace gv {

// One lane per record. The device count is one wave-uniform load; lanes beyond it leave at once. ORs commute: the set is the same
// whatever the arrival order. (second_seen_kernel measured that such a launch is bound by its device-scope atomics and that several
// records per lane did not help: profiles/r24_second_phase.md; the shape is kept.)
__global__ __launch_bounds__(kDeltaBlock) void delta_mark_records_kernel(const uint32_t* __restrict__ count, const uint32_t* __restrict__ idx,
                                                                          uint32_t capacity, uint32_t slots, unsigned long long* __restrict__ current)
{
    const uint32_t k = blockIdx.x * kDeltaBlock + threadIdx.x;
    const uint32_t n = min(*count, capacity);
    if (k >= n)
        return;
    const uint32_t slot = idx[k];
    if (slot < slots)
        atomicOr(&current[slot >> 6], 1ull << (slot & 63u));
}

// One lane per mirror entry: a wave reads 64 consecutive bytes. PERMUTED: only the lanes whose byte is set load their slot and issue
// an OR. Otherwise entry == slot and the wave's ballot IS word (entry >> 6) of the set: lane 0 ORs it in, if it holds anything.
template <bool PERMUTED>
__global__ __launch_bounds__(kDeltaBlock) void delta_mark_bytes_kernel(const uint8_t* __restrict__ is_visible, uint32_t entries,
                                                                        const uint32_t* __restrict__ orig, uint32_t slots,
                                                                        unsigned long long* __restrict__ current)
{
    const uint32_t e = blockIdx.x * kDeltaBlock + threadIdx.x;
    const bool set = e < entries && is_visible[e] != 0;
    if (PERMUTED) {
        if (!set)
            return;
        const uint32_t slot = orig[e];
        if (slot < slots)
            atomicOr(&current[slot >> 6], 1ull << (slot & 63u));
    } else {
        const unsigned long long word = __ballot(set && e < slots);
        if ((threadIdx.x & 63u) == 0 && word)  // (a set lane has e < slots: the word lies inside the set)
            atomicOr(&current[e >> 6], word);
    }
}

// word w of C and of P as the difference sees them: past a set's coverage a word reads as 0
__device__ __forceinline__ void delta_words_at(const DeltaSets& s, uint32_t w, uint32_t current_words, uint32_t baseline_words,
                                               unsigned long long& c, unsigned long long& p)
{
    c = w < current_words ? s.current[w] : 0ull;
    p = w < baseline_words ? s.baseline[w] : 0ull;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1)
        x += __shfl_xor(x, d);
    return x;
}

// Lane t of workgroup g owns word g * kDeltaBlock + t. Popcounts, a wave sum, one row per workgroup.
__global__ __launch_bounds__(kDeltaBlock) void delta_count_kernel(const DeltaSets s, uint32_t current_words, uint32_t baseline_words)
{
    __shared__ uint32_t part[3][kDeltaBlock / 64];
    const uint32_t tid = threadIdx.x, w = blockIdx.x * kDeltaBlock + tid;
    unsigned long long c, p;
    delta_words_at(s, w, current_words, baseline_words, c, p);
    const uint32_t a = wave_sum((uint32_t)__popcll(c & ~p)), v = wave_sum((uint32_t)__popcll(p & ~c)), n = wave_sum((uint32_t)__popcll(c));
    if ((tid & 63u) == 0)
        part[0][tid >> 6] = a, part[1][tid >> 6] = v, part[2][tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        DeltaTotals t{0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < kDeltaBlock / 64; k++)
            t.appeared += part[0][k], t.vanished += part[1][k], t.current += part[2][k];
        s.totals[blockIdx.x] = t;
    }
}

// The bits of `word` as slot numbers, ascending, from out[at] on (at + popcount <= limit by construction; the guard keeps a wrong
// total from ever becoming a store outside the buffer).
__device__ __forceinline__ void delta_write(unsigned long long word, uint32_t first_slot, uint32_t* __restrict__ out, uint32_t at, uint32_t limit)
{
    while (word) {
        const uint32_t bit = (uint32_t)__ffsll((long long)word) - 1u;
        if (at < limit)
            out[at] = first_slot + bit;
        at++;
        word &= word - 1ull;
    }
}

// Workgroup g: the totals of the workgroups in front of it give its two bases (every workgroup sums them itself: nobody waits for
// anybody, and groups rows are a few KB of L2 hits), a scan over its own 256 words the lane's places. A workgroup whose own row is
// (0, 0) — in the sparse regime almost all of them — leaves after one load, workgroup 0 excepted, which also writes the counts.
__global__ __launch_bounds__(kDeltaBlock) void delta_place_kernel(const DeltaSets s, uint32_t current_words, uint32_t baseline_words, uint32_t groups)
{
    __shared__ uint32_t sum[5][kDeltaBlock / 64];
    __shared__ uint32_t wave_base[kDeltaBlock / 64];
    const uint32_t tid = threadIdx.x, g = blockIdx.x, lane = tid & 63u, wave = tid >> 6;
    const DeltaTotals own = s.totals[g];
    if (g != 0 && own.appeared == 0 && own.vanished == 0)  // workgroup-uniform
        return;
    // a_front, v_front: in front of g; a_all, v_all, c_all: of every workgroup (the vanished list starts behind ALL that appeared)
    uint32_t a_front = 0, v_front = 0, a_all = 0, v_all = 0, c_all = 0;
    for (uint32_t j = tid; j < groups; j += kDeltaBlock) {
        const DeltaTotals t = s.totals[j];
        a_all += t.appeared, v_all += t.vanished, c_all += t.current;
        if (j < g)
            a_front += t.appeared, v_front += t.vanished;
    }
    a_front = wave_sum(a_front), v_front = wave_sum(v_front), a_all = wave_sum(a_all);
    if (g == 0)
        v_all = wave_sum(v_all), c_all = wave_sum(c_all);
    if (lane == 0) {
        sum[0][wave] = a_front, sum[1][wave] = v_front, sum[2][wave] = a_all;
        sum[3][wave] = v_all, sum[4][wave] = c_all;  // (whole sums in workgroup 0 only, which alone reads them)
    }
    // the lane's own word and its place among the workgroup's: both counts in one scan, 16 bits each (kDeltaGroupSlots < 65536)
    const uint32_t w = g * kDeltaBlock + tid;
    unsigned long long c, p;
    delta_words_at(s, w, current_words, baseline_words, c, p);
    const unsigned long long appeared = c & ~p, vanished = p & ~c;
    const uint32_t mine = (uint32_t)__popcll(appeared) | ((uint32_t)__popcll(vanished) << 16);
    uint32_t incl = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d)
            incl += up;
    }
    if (lane == 63)
        wave_base[wave] = incl;
    __syncthreads();
    uint32_t a_base = 0, v_base = 0, a_total = 0, v_total = 0, c_total = 0, before = 0;
#pragma unroll
    for (uint32_t k = 0; k < kDeltaBlock / 64; k++) {
        a_base += sum[0][k], v_base += sum[1][k], a_total += sum[2][k], v_total += sum[3][k], c_total += sum[4][k];
        if (k < wave)
            before += wave_base[k];
    }
    if (g == 0 && tid == 0) {
        s.counts[0] = a_total;
        s.counts[1] = v_total;
        s.counts[2] = c_total;
        s.counts[3] = s.universe;
    }
    if (!(appeared | vanished))
        return;
    const uint32_t excl = before + incl - mine;
    delta_write(appeared, w * kDeltaWordSlots, s.slots, a_base + (excl & 0xFFFFu), s.universe);
    delta_write(vanished, w * kDeltaWordSlots, s.slots, a_total + v_base + (excl >> 16), s.universe);
}

hipError_t launch_delta_mark_records(const uint32_t* count, const uint32_t* idx, uint32_t capacity, uint32_t slots, unsigned long long* current,
                                     hipStream_t stream)
{
    if (capacity == 0 || slots == 0)
        return hipSuccess;
    hipLaunchKernelGGL(delta_mark_records_kernel, dim3((capacity + kDeltaBlock - 1) / kDeltaBlock), dim3(kDeltaBlock), 0, stream, count, idx, capacity,
                       slots, current);
    return hipGetLastError();
}

hipError_t launch_delta_mark_bytes(const uint8_t* is_visible, uint32_t entries, const uint32_t* orig, uint32_t slots, unsigned long long* current,
                                   hipStream_t stream)
{
    if (entries == 0 || slots == 0)
        return hipSuccess;
    const dim3 grid((entries + kDeltaBlock - 1) / kDeltaBlock), block(kDeltaBlock);
    if (orig)
        hipLaunchKernelGGL(delta_mark_bytes_kernel<true>, grid, block, 0, stream, is_visible, entries, orig, slots, current);
    else
        hipLaunchKernelGGL(delta_mark_bytes_kernel<false>, grid, block, 0, stream, is_visible, entries, orig, slots, current);
    return hipGetLastError();
}

hipError_t launch_delta_count(const DeltaSets& sets, hipStream_t stream)
{
    const uint32_t groups = delta_groups(sets.universe);
    if (groups == 0)
        return hipSuccess;
    hipLaunchKernelGGL(delta_count_kernel, dim3(groups), dim3(kDeltaBlock), 0, stream, sets, (uint32_t)delta_words(sets.current_slots),
                       (uint32_t)delta_words(sets.baseline_slots));
    return hipGetLastError();
}

hipError_t launch_delta_place(const DeltaSets& sets, hipStream_t stream)
{
    const uint32_t groups = delta_groups(sets.universe);
    if (groups == 0)
        return hipSuccess;
    hipLaunchKernelGGL(delta_place_kernel, dim3(groups), dim3(kDeltaBlock), 0, stream, sets, (uint32_t)delta_words(sets.current_slots),
                       (uint32_t)delta_words(sets.baseline_slots), groups);
    return hipGetLastError();
}

}  // namespace gv
