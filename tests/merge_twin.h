/* merge_twin.h — plain C99 restatement of gv_merge_sorted's order (include/garden_vis.h): a stable k-way merge of lists that are
 * already sorted in the sort's own key order, T(u) = u ^ ((u >> 31) ? 0xFFFFFFFF : 0x80000000) on the float's bits. Ties go to the
 * list in front, then to the list's own order — what std::inplace_merge of the runs, taken in list order, produces. TEST-ONLY. */
#ifndef MERGE_TWIN_H
#define MERGE_TWIN_H
#include <stdint.h>

static uint32_t merge_twin_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }

/* keys[l][0 .. counts[l]): the float bits of list l, sorted (descending != 0: T falling). Entry k of the merged order is record
 * out_index[k] of list out_list[k]; returns the total. */
static uint32_t merge_twin_order(const uint32_t* const* keys, const uint32_t* counts, uint32_t lists, int descending, uint32_t* out_list,
                                 uint32_t* out_index)
{
    uint32_t head[64];
    uint32_t total = 0, l, k;
    if (lists > 64u)
        return 0;
    for (l = 0; l < lists; l++) {
        head[l] = 0;
        total += counts[l];
    }
    for (k = 0; k < total; k++) {
        uint32_t best = lists, best_key = 0;
        for (l = 0; l < lists; l++) {
            uint32_t t;
            if (head[l] == counts[l])
                continue;
            t = merge_twin_key(keys[l][head[l]]);
            if (best == lists || (descending ? t > best_key : t < best_key)) { /* strict: a tie stays with the list in front */
                best = l;
                best_key = t;
            }
        }
        out_list[k] = best;
        out_index[k] = head[best]++;
    }
    return total;
}
#endif
