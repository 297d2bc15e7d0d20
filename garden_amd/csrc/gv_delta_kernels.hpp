// gv_delta_kernels.hpp — launch interface of gv_delta.hip: gv_pool_view_delta, what came into view and what left it since a channel's
// last call. Kept apart from gv_kernels.hpp like gv_second_kernels.hpp and gv_bounds_kernels.hpp.
#pragma once
#include "gv_kernels.hpp"

namespace gv {

constexpr uint32_t kDeltaBlock = 256;      // lanes per workgroup of all four launches
constexpr uint32_t kDeltaWordSlots = 64;   // pool slots per word of a set (unsigned long long, as the second phase's seen set)
constexpr uint32_t kDeltaWaveSlots = 4096;   // delta_count / delta_place: a lane owns one word, a wave 64 of them
constexpr uint32_t kDeltaGroupSlots = 16384; // ... and a workgroup kDeltaBlock (literals: the tests read them from this text)
static_assert(kDeltaWaveSlots == 64 * kDeltaWordSlots && kDeltaGroupSlots == kDeltaBlock * kDeltaWordSlots, "one word per lane");
static_assert(kDeltaBlock % 64 == 0, "a wave of delta_mark_bytes_kernel owns one whole word of entries");
// (a lane's two counts travel through the workgroup's scan packed into one word: 16 bits each)
static_assert(kDeltaGroupSlots < 65536, "a workgroup's appeared / vanished count fits 16 bits");

inline size_t delta_words(uint32_t slots) { return ((size_t)slots + kDeltaWordSlots - 1) / kDeltaWordSlots; }
inline uint32_t delta_groups(uint32_t slots) { return (uint32_t)(((size_t)slots + kDeltaGroupSlots - 1) / kDeltaGroupSlots); }

struct DeltaTotals {  // one row per delta_count_kernel workgroup
    uint32_t appeared, vanished, current, pad;
};
struct DeltaSets {
    const unsigned long long* current;   // C: [delta_words(current_slots)], bits at or beyond current_slots clear
    const unsigned long long* baseline;  // P: [delta_words(baseline_slots)], likewise (baseline_slots 0: empty, never read)
    uint32_t current_slots, baseline_slots;
    uint32_t universe;                   // U = max of the two: words past a set's coverage read as 0
    DeltaTotals* totals;                 // [delta_groups(universe)]
    uint32_t* slots;                     // [universe]: appeared at [0, a), vanished at [a, a + v), ascending each
    uint32_t* counts;                    // {a, v, |C|, U}
};

// C |= the slots of a view's records: visible_idx[0 .. min(*count, capacity)), a slot at or beyond `slots` is ignored
hipError_t launch_delta_mark_records(const uint32_t* count, const uint32_t* idx, uint32_t capacity, uint32_t slots, unsigned long long* current,
                                     hipStream_t stream);
// C |= the slots whose isVisible byte is set: `entries` bytes in mirror order, orig[entry] = the pool slot (NULL: entry == slot,
// one OR of a whole word per wave)
hipError_t launch_delta_mark_bytes(const uint8_t* is_visible, uint32_t entries, const uint32_t* orig, uint32_t slots, unsigned long long* current,
                                   hipStream_t stream);
hipError_t launch_delta_count(const DeltaSets& sets, hipStream_t stream);
hipError_t launch_delta_place(const DeltaSets& sets, hipStream_t stream);

}  // namespace gv
