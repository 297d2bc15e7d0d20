// dirty_ranges_test.cpp — gv::DirtyRanges (garden_amd/csrc/gv_dirty_ranges.hpp) against a bitmap model: random marks
// (overlapping, adjacent, empty, wrapping first + count), normalise with and without a gap, the kMax collapse. The
// invariant the mirror relies on: after normalise(limit, gap) the ranges are sorted, disjoint, inside [0, limit), cover
// EVERY marked slot below the limit, and with gap == 0 cover nothing else. Built with -fsanitize=address,undefined.
// In front of that, the rules of the mirror sync from the same header as a table (mirror_rules_table; `rules` as the first
// argument runs the table alone).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/gv_dirty_ranges.hpp"

static uint32_t rnd(uint64_t& s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

// The rules by which sync_mirror (gv_mirror.cpp) chooses its steps, on both sides of every threshold, against literals worked
// out by hand from their statements:
//   tail due for re-order: more than 1/8 of a pool of at least 1024 slots is appended-and-unsorted or about to be appended;
//   few enough to patch blocks: 16 * total <= blocks + 1024;   most of the pool: 2 * total > occupancy;
//   device gather from 2048 slots;   mapping: all own -> exact (2), at least 9 in 10 -> speculate (1), else general (0).
static bool mirror_rules_table()
{
    struct Tail { uint32_t occupancy, mirrored, appended; bool due; };
    const Tail tails[] = {
        {1024, 896, 0, false},     // 128 * 8 = 1024 is not greater than 1024
        {1024, 895, 0, true},      // 129 * 8 = 1032
        {1024, 1023, 127, false},  // (127 + 1) * 8 = 1024: what was appended before counts with what is about to be
        {1024, 1023, 128, true},   // (128 + 1) * 8 = 1032
        {1024, 1024, 1024, false}, // nothing new to mirror: the rule never fires on the appended count alone
        {1024, 1025, 0, false},    // a pool that shrank
        {1023, 0, 0, false}, {1023, 0, 1023, false}, {1023, 1022, 4000000000u, false},  // below 1024 slots: never
        {1025, 896, 0, true},      // 129 * 8 = 1032 > 1025
        {1025, 897, 0, false},     // 128 * 8 = 1024
        {8192, 7168, 0, false},    // 1024 * 8 = 8192
        {8192, 7167, 0, true},
        {4000000000u, 3500000000u, 0, false},           // 5e8 * 8 = 4e9 (64-bit arithmetic: no wrap)
        {4000000000u, 3499999999u, 0, true},
        {4294967295u, 4294967294u, 4294967295u, true},  // the sum passes 2^32 and must not wrap to 0
    };
    for (const Tail& t : tails)
        if (gv::tail_due_for_reorder(t.occupancy, t.mirrored, t.appended) != t.due) {
            printf("{\"ok\": false, \"why\": \"tail_due_for_reorder(%u, %u, %u) is not %d\"}\n", t.occupancy, t.mirrored, t.appended, t.due);
            return false;
        }
    struct Few { uint64_t total, nblocks; bool few; };
    const Few fews[] = {
        {126, 1000, true},   // 2016 <= 2024
        {127, 1000, false},  // 2032
        {64, 0, true},       // 1024 <= 1024: 64 entries are free whatever the pool
        {65, 0, false}, {65, 15, false},
        {65, 16, true},      // 1040 <= 1040
        {0, 0, true},
        {2505, 39063, true},   // a 10 M pool (39 063 blocks): 40 080 <= 40 087
        {2506, 39063, false},  // 40 096
        {1ull << 40, 16777216, false},
    };
    for (const Few& f : fews)
        if (gv::few_enough_to_patch_blocks(f.total, f.nblocks) != f.few) {
            printf("{\"ok\": false, \"why\": \"few_enough_to_patch_blocks(%llu, %llu) is not %d\"}\n", (unsigned long long)f.total, (unsigned long long)f.nblocks, f.few);
            return false;
        }
    struct Most { uint64_t total; uint32_t occupancy; bool most; };
    const Most mosts[] = {{512, 1024, false}, {513, 1024, true}, {512, 1025, false}, {513, 1025, true}, {0, 0, false}, {1, 0, true}, {1, 1, true}, {1, 2, false},
                          {2147483647u, 4294967295u, false}, {2147483648u, 4294967295u, true}};
    for (const Most& m : mosts)
        if (gv::most_of_pool(m.total, m.occupancy) != m.most) {
            printf("{\"ok\": false, \"why\": \"most_of_pool(%llu, %u) is not %d\"}\n", (unsigned long long)m.total, m.occupancy, m.most);
            return false;
        }
    struct Map { size_t own, candidates; uint32_t mapping; };
    const Map maps[] = {{0, 0, 2}, {10, 10, 2}, {9, 10, 1}, {8, 10, 0}, {90, 100, 1}, {89, 100, 0}, {99, 100, 1}, {100, 100, 2}, {0, 1, 0}, {1, 1, 2},
                        {9000000, 10000000, 1}, {8999999, 10000000, 0}};
    for (const Map& m : maps)
        if (gv::mesh_mapping_of(m.own, m.candidates) != m.mapping) {
            printf("{\"ok\": false, \"why\": \"mesh_mapping_of(%zu, %zu) is not %u\"}\n", m.own, m.candidates, m.mapping);
            return false;
        }
    static_assert(gv::kDeviceGatherMinSlots == 2048 && gv::kPairedGeneral == 0 && gv::kPairedSpeculate == 1 && gv::kPairedExact == 2, "as stated above");
    printf("mirror rules table: 16 tails, 10 few, 10 most, 12 mappings as worked out by hand: ok\n");
    return true;
}

int main(int argc, char** argv)
{
    if (!mirror_rules_table())
        return 1;
    if (argc > 1 && std::string(argv[1]) == "rules") {
        printf("{\"ok\": true}\n");
        return 0;
    }
    uint64_t seed = 12345;
    for (int round = 0; round < 400; round++) {
        const uint32_t limit = 1000 + rnd(seed) % 60000;
        std::vector<uint8_t> marked(limit, 0);
        gv::DirtyRanges d;
        const int marks = 1 + (int)(rnd(seed) % (round % 7 == 0 ? 40000 : 300));
        for (int k = 0; k < marks; k++) {
            uint32_t first = rnd(seed) % (limit + 50), count = rnd(seed) % 40;
            if (rnd(seed) % 50 == 0)
                count = 0xFFFFFFFFu - (rnd(seed) % 3);  // first + count wraps: must saturate, not vanish
            if (rnd(seed) % 5 == 0 && !d.items.empty())
                first = d.items.back().hi;  // adjacent to the previous mark
            d.add(first, count);
            for (uint64_t i = first; i < (uint64_t)first + count && i < limit; i++)
                marked[i] = 1;
        }
        const uint32_t gap = round % 3 == 0 ? 0u : rnd(seed) % 64;
        d.normalise(limit, gap);
        if (d.items.size() > gv::DirtyRanges::kMax) {
            printf("{\"ok\": false, \"why\": \"%zu ranges after normalise\"}\n", d.items.size());
            return 1;
        }
        std::vector<uint8_t> covered(limit, 0);
        uint32_t prev_hi = 0;
        bool first_range = true;
        uint64_t total = 0;
        for (const auto& r : d.items) {
            if (r.lo >= r.hi || r.hi > limit || (!first_range && r.lo <= prev_hi && gap == 0 && r.lo < prev_hi)) {
                printf("{\"ok\": false, \"why\": \"bad range [%u, %u) limit %u\"}\n", r.lo, r.hi, limit);
                return 1;
            }
            if (!first_range && r.lo < prev_hi) {
                printf("{\"ok\": false, \"why\": \"ranges overlap\"}\n");
                return 1;
            }
            for (uint32_t i = r.lo; i < r.hi; i++)
                covered[i] = 1;
            total += r.hi - r.lo;
            prev_hi = r.hi;
            first_range = false;
        }
        if (total != d.total()) {
            printf("{\"ok\": false, \"why\": \"total()\"}\n");
            return 1;
        }
        const bool exact = gap == 0 && (size_t)marks <= gv::DirtyRanges::kMax;  // (a collapse beyond kMax may widen ranges)
        for (uint32_t i = 0; i < limit; i++)
            if ((marked[i] && !covered[i]) || (exact && covered[i] && !marked[i])) {
                printf("{\"ok\": false, \"why\": \"slot %u marked %d covered %d (round %d)\"}\n", i, marked[i], covered[i], round);
                return 1;
            }
    }
    printf("{\"ok\": true}\n");
    return 0;
}
