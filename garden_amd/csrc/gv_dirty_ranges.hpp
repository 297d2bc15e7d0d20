// gv_dirty_ranges.hpp — itemised dirty slot ranges of a bound pool (host-only, no HIP: unit-tested on the CPU tier under
// ASan / UBSan, tests/cpp/dirty_ranges_test.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace gv {

// Itemised dirty marks of a pool (setPosition on scattered entities, transform.hpp:74-104): kept as disjoint
// ranges instead of one covering range, so a handful of moved entities at opposite ends of a 10 M pool re-mirror a
// handful of slots, not everything in between. Overlapping and adjacent ranges are merged; beyond kMax ranges, ranges
// closer than a growing `gap` are merged too until they fit.
struct DirtyRanges {
    struct R {
        uint32_t lo, hi;
    };
    std::vector<R> items;
    static constexpr size_t kMax = 16384;
    bool any() const { return !items.empty(); }
    void clear() { items.clear(); }
    void add(uint32_t first, uint32_t count)
    {
        if (count == 0)
            return;
        const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)first + count, UINT32_MAX);  // saturating, see DirtyRange
        if (!items.empty() && first <= items.back().hi && hi >= items.back().lo) {  // extends / overlaps the last mark
            items.back().lo = std::min(items.back().lo, first);
            items.back().hi = std::max(items.back().hi, hi);
            return;
        }
        items.push_back({first, hi});
        if (items.size() > 4 * kMax)
            normalise(UINT32_MAX, 0);
    }
    // sorted, clamped to [0, limit), merged
    void normalise(uint32_t limit, uint32_t gap)
    {
        for (auto& r : items)
            r.hi = std::min(r.hi, limit);
        items.erase(std::remove_if(items.begin(), items.end(), [](const R& r) { return r.lo >= r.hi; }), items.end());
        std::sort(items.begin(), items.end(), [](const R& a, const R& b) { return a.lo < b.lo; });
        for (;;) {
            std::vector<R> merged;
            for (const R& r : items) {
                if (!merged.empty() && (uint64_t)r.lo <= (uint64_t)merged.back().hi + gap)
                    merged.back().hi = std::max(merged.back().hi, r.hi);
                else
                    merged.push_back(r);
            }
            items.swap(merged);
            if (items.size() <= kMax || gap >= (1u << 30))
                break;
            gap = gap ? gap * 2 : 1;
        }
    }
    uint64_t total() const
    {
        uint64_t t = 0;
        for (const R& r : items)
            t += r.hi - r.lo;
        return t;
    }
};

// ---- the rules of the mirror sync (gv_mirror.cpp: sync_mirror and its steps), each written once -----------------------------
// Pure functions of counts, tabulated on both sides of every threshold by tests/cpp/dirty_ranges_test.cpp. The callers add
// their own terms (need_full, spatial order, link changes, whether a pool records at all); only the shared arithmetic is here.

// Too much of a pool sits in the unsorted tail (slots appended since the mirror was last in spatial order, `appended` of them
// already mirrored and occupancy - mirrored about to be): more than 1/8 of a pool of at least 1024 slots goes back into order.
inline bool tail_due_for_reorder(uint32_t occupancy, uint32_t mirrored, uint32_t appended)
{
    return occupancy > mirrored && ((uint64_t)appended + (occupancy - mirrored)) * 8 > occupancy && occupancy >= 1024;
}

// So few entries changed that flagging their blocks (of a pool of `nblocks` cull blocks) beats rebuilding the pool's block
// bounds / emit seeds once it is at rest: 1/16 of the blocks, with 64 entries free.
inline bool few_enough_to_patch_blocks(uint64_t total, uint64_t nblocks) { return total * 16 <= nblocks + 16 * 64; }

// Most of the pool changed: one dense pass over all of it is cheaper than itemised uploads.
inline bool most_of_pool(uint64_t total, uint32_t occupancy) { return total * 2 > occupancy; }

// A dirty range of an AoS pool from this many slots up travels raw and is gathered on the device (upload_*_device).
constexpr uint32_t kDeviceGatherMinSlots = 2048;

// How the candidates of a mesh pool pair with transform entries: `own` of them sit at their transform's index. The values are
// MeshMapping's (gv_kernels.hpp, which this header does not include; gv_mirror.cpp asserts that they agree).
constexpr uint32_t kPairedGeneral = 0, kPairedSpeculate = 1, kPairedExact = 2;
inline uint32_t mesh_mapping_of(size_t own, size_t candidates)
{
    return own == candidates ? kPairedExact : (own * 10 >= candidates * 9 ? kPairedSpeculate : kPairedGeneral);
}

}  // namespace gv
