// gv_dense_rounds.hpp — a super-tile's corner candidates settled in dense rounds (cull_hot_kernel<true, K>, gv_cull.hip; the same text
// runs under tests/dense_rounds_probe.hip). A super-tile is K 256-entry tiles of one 256-lane workgroup, lane tid holding entries
// k * 256 + tid. Few of them are candidates (the bench's frame: 25 of a wave's 64 where there is any), and the per-candidate decision is
// long, so the workgroup lists its candidates in LDS and decides them 256 at a time with every lane busy, whichever lane and tile they
// came from. Every decision is per entry and the results are ORed bits and one integer sum, so the outputs do not depend on the order of
// the list: ballot word (tile k, wave w) bit l is entry k * 256 + w * 64 + l, as where each wave decides its own lanes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gv {

constexpr uint32_t kDenseWaves = 4;                 // waves of the workgroup: 256 lanes
constexpr uint32_t kDenseLanes = kDenseWaves * 64;
constexpr uint32_t kDenseUndecided = 0x8000u;       // list entry: k * 256 + tid, | this bit for an undecided (not an inside) entry

template <uint32_t K>
struct DenseRoundsLds {
    unsigned long long words[K * kDenseWaves];  // the ballot words, (tile k, wave w) at k * 4 + w
    uint32_t counts[K * kDenseWaves];           // candidates of (tile k, wave w)
    uint16_t list[K * kDenseLanes];
};

// where the super-tile's results go (read when they are written, not before: a kernel hands them out of freshly loaded arguments)
struct DenseOutputs {
    unsigned long long* mask;  // ballot words of the whole array, 4 per tile
    uint32_t* chunk_count;     // one total per `tiles_per_chunk` tiles
    uint8_t* is_visible;       // one byte per entry, or null: not written
    uint32_t nblocks;          // tiles of the array: words of tiles from here on are not stored
    uint32_t count;            // entries of the array: bytes from here on are not stored
    uint32_t tiles_per_chunk;
};

// `where`: the lane's K classes, entry k in bits 2k, 2k + 1; 0 = outside (not a candidate, not visible), `undecided_class` and every other
// non-zero class = candidate. decide(slot, undecided) -> visible, for slot = k * 256 + tid of a candidate; outputs() -> DenseOutputs.
// Called by all 256 lanes of a workgroup whose first tile `first` lies inside the array; three barriers, one when there is no candidate.
template <uint32_t K, typename Decide, typename Outputs>
__device__ __forceinline__ void dense_rounds(DenseRoundsLds<K>& lds, uint32_t where, uint32_t undecided_class, uint32_t first, Decide&& decide,
                                             Outputs&& outputs)
{
    static_assert(K >= 1 && K * kDenseWaves <= 64 && K * kDenseLanes <= kDenseUndecided, "the words fit one wave, a slot fits 15 bits");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // 1. count
    unsigned long long cand[K];
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        cand[k] = __ballot(((where >> (2u * k)) & 3u) != 0u);
        if (lane == 0)
            lds.counts[k * kDenseWaves + wave] = (uint32_t)__popcll(cand[k]);
    }
    if (tid < K * kDenseWaves)
        lds.words[tid] = 0ull;
    __syncthreads();
    // 2. the super-tile's total (the same LDS words in every lane: uniform over the workgroup) and where each (tile, wave) starts
    uint32_t total = 0, start[K];
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        start[k] = total;  // behind all of the tiles before k, and the waves before this one in tile k
#pragma unroll
        for (uint32_t w = 0; w < kDenseWaves; w++) {
            const uint32_t c = lds.counts[k * kDenseWaves + w];
            if (w < wave)
                start[k] += c;
            total += c;
        }
    }
    if (total == 0) {
        const DenseOutputs out = outputs();
        if (tid < K * kDenseWaves && first + tid / kDenseWaves < out.nblocks)
            out.mask[(size_t)first * kDenseWaves + tid] = 0ull;
        if (out.is_visible)
#pragma unroll
            for (uint32_t k = 0; k < K; k++) {
                const uint32_t i = (first + k) * kDenseLanes + tid;
                if (i < out.count)
                    out.is_visible[i] = 0;
            }
        return;
    }
    // 3. list
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t wk = (where >> (2u * k)) & 3u;
        if (wk != 0u)
            lds.list[start[k] + (uint32_t)__popcll(cand[k] & ((1ull << lane) - 1ull))] =
                (uint16_t)(k * kDenseLanes + tid + (wk == undecided_class ? kDenseUndecided : 0u));
    }
    __syncthreads();
    // 4. dense rounds (no barrier inside: the list is only read, the words only take ORs)
#pragma unroll 1
    for (uint32_t r0 = 0; r0 < total; r0 += kDenseLanes) {
        if (r0 + tid < total) {
            const uint32_t e = lds.list[r0 + tid], slot = e & (kDenseUndecided - 1u);
            if (decide(slot, (e & kDenseUndecided) != 0u))
                atomicOr(&lds.words[slot >> 6], 1ull << (slot & 63u));
        }
    }
    __syncthreads();
    // 5. output: the 4K words as one contiguous store, the super-tile's count as one atomic, the bytes out of the words
    const DenseOutputs out = outputs();
    if (tid < K * kDenseWaves && first + tid / kDenseWaves < out.nblocks)
        out.mask[(size_t)first * kDenseWaves + tid] = lds.words[tid];
    if (tid == 0) {
        uint32_t visible = 0;
#pragma unroll
        for (uint32_t j = 0; j < K * kDenseWaves; j++)
            visible += (uint32_t)__popcll(lds.words[j]);
        if (visible)  // integer adds commute: the sum is deterministic whatever the arrival order
            atomicAdd(&out.chunk_count[first / out.tiles_per_chunk], visible);
    }
    if (out.is_visible)
#pragma unroll
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t i = (first + k) * kDenseLanes + tid;
            if (i < out.count)
                out.is_visible[i] = (uint8_t)((lds.words[k * kDenseWaves + wave] >> lane) & 1ull);
        }
}

}  // namespace gv
