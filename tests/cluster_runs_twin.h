/* cluster_runs_twin.h — the rule of gv_pool_cull_cluster_runs (include/garden_vis.h) restated in C. Which
 * cluster survives is decided by cluster_twin_survives of cluster_twin.h, that is by the ORACLE's gvo_is_behind_frustum and
 * gvo_hiz_occluded; this file restates only what the run form adds — linked, head, run, the run's command — and counts what the
 * census (tests/test_cluster_runs_census.py) holds the case table to. TEST INFRASTRUCTURE ONLY: nothing here comes from the
 * product's kernels, and the product never includes it. */
#ifndef CLUSTER_RUNS_TWIN_H
#define CLUSTER_RUNS_TWIN_H

#include "cluster_twin.h"

#define CLUSTER_RUNS_TWIN_SPAN 256u /* GV_CLUSTER_RUN_SPAN, restated */

/* what the census counts of one view (every word is a sum over the view; longest is a maximum) */
typedef struct ClusterRunsCensus {
    uint32_t candidates;       /* clusters of clustered draws + whole draws: the view's share of the candidate numbering */
    uint32_t survivors;        /* surviving clusters (whole draws left out) */
    uint32_t runs;             /* runs (whole draws left out) */
    uint32_t whole;            /* commands of draws drawn whole */
    uint32_t longest;          /* clusters of the longest run */
    uint32_t break_nonsurvivor; /* heads at j > 0 whose predecessor did not survive */
    uint32_t break_gap;        /* heads whose predecessor survived and whose index range does not follow it (or would wrap) */
    uint32_t break_span;       /* heads whose predecessor survived and is followed in the index buffer: j % SPAN == 0 alone broke */
    uint32_t cross_word;       /* runs whose first and last candidate lie in different 64-candidate words */
    uint32_t cross_tile;       /* ... in different 256-candidate tiles */
} ClusterRunsCensus;

/* the index interval of cluster j follows that of cluster j - 1 and does not pass 2^32 - 1 */
static int cluster_runs_twin_follows(const ClusterTwinCluster* cl, uint32_t j)
{
    return (uint64_t)cl[j - 1].first + cl[j - 1].count == (uint64_t)cl[j].first && (uint64_t)cl[j].first + cl[j].count <= 0xFFFFFFFFull;
}
/* LINKED: static, of the tables and j alone (cl: the draw's range) */
static int cluster_runs_twin_linked(const ClusterTwinCluster* cl, uint32_t j)
{
    return j > 0 && j % CLUSTER_RUNS_TWIN_SPAN != 0 && cluster_runs_twin_follows(cl, j);
}

/* the census of a finished run over candidates from .. to */
static void cluster_runs_twin_close(ClusterRunsCensus* sum, uint64_t from, uint64_t to)
{
    const uint32_t length = (uint32_t)(to - from) + 1;
    if (length > sum->longest)
        sum->longest = length;
    sum->cross_word += from / 64u != to / 64u;
    sum->cross_tile += from / 256u != to / 256u;
}

/* The commands of ONE view in the rule's order: draw k ascending, head j ascending. Arguments as cluster_twin_view; candidate_base:
 * the candidates in front of the view (of the views listed before it), for the census's word and tile edges. out: room for every
 * candidate. Returns the number of commands; *tested = clusters tested; *census (may be NULL) is overwritten. */
static uint32_t cluster_runs_twin_view(const float* models, const uint32_t* g, const uint32_t* first, uint32_t n, const ClusterTwinGeometry* table,
                                       uint32_t table_count, const ClusterTwinRange* ranges, uint32_t range_count, const ClusterTwinCluster* clusters,
                                       const float view_proj[16], const GvoHiz* hiz, uint64_t candidate_base, ClusterTwinCommand* out,
                                       uint32_t* tested, ClusterRunsCensus* census)
{
    GvoFrustum frustum;
    ClusterRunsCensus sum;
    uint32_t commands = 0;
    uint64_t c = candidate_base;
    gvo_frustum_from_view_proj(view_proj, &frustum);
    memset(&sum, 0, sizeof(sum));
    *tested = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t instances = first[k + 1] - first[k];
        if (g[k] >= table_count || instances == 0)
            continue; /* the void geometry, or no instance: nothing, and no candidate */
        const ClusterTwinGeometry geometry = table[g[k]];
        ClusterTwinRange range = {0, 0};
        if (g[k] < range_count)
            range = ranges[g[k]];
        if (range.count == 0) { /* drawn whole, untested, never merged */
            ClusterTwinCommand whole = {geometry.count, instances, geometry.first, first[k], geometry.vertex_offset, k};
            out[commands++] = whole;
            sum.whole++;
            c++;
            continue;
        }
        const ClusterTwinCluster* cl = &clusters[range.first];
        int before = 0;        /* cluster j - 1 survived */
        int open = 0;          /* out[commands - 1] is a run that cluster j may still join */
        uint32_t head = 0;
        for (uint32_t j = 0; j < range.count; j++) {
            const int survives = cluster_twin_survives(models + (size_t)k * 12, view_proj, &frustum, hiz, &cl[j]);
            (*tested)++;
            if (survives) {
                sum.survivors++;
                if (open && before && cluster_runs_twin_linked(cl, j)) {
                    ClusterTwinCommand* run = &out[commands - 1];
                    run->count = cl[j].first + cl[j].count - cl[head].first;
                } else { /* a HEAD: not linked, or cluster j - 1 did not survive */
                    ClusterTwinCommand run = {cl[j].count, instances, geometry.first + cl[j].first, first[k], geometry.vertex_offset, k};
                    if (open) /* the run before ends at j - 1 */
                        cluster_runs_twin_close(&sum, c + head, c + j - 1);
                    if (j > 0) {
                        if (!before)
                            sum.break_nonsurvivor++;
                        else if (cluster_runs_twin_follows(cl, j))
                            sum.break_span++;
                        else
                            sum.break_gap++;
                    }
                    out[commands++] = run;
                    sum.runs++;
                    head = j;
                    open = 1;
                }
            }
            if (open && (!survives || j + 1 == range.count)) { /* the open run ends: at j - 1, or at the draw's last cluster */
                cluster_runs_twin_close(&sum, c + head, c + (survives ? j : j - 1));
                open = 0;
            }
            before = survives;
        }
        c += range.count;
    }
    sum.candidates = (uint32_t)(c - candidate_base);
    if (census)
        *census = sum;
    return commands;
}

#endif
