/* cluster_second_twin.h — the rule of gv_pool_cull_clusters_second_phase (include/garden_vis.h) restated in C
 * over tests/cluster_twin.h, which decides every cluster with the ORACLE's gvo_is_behind_frustum and gvo_hiz_occluded. This file
 * adds only what the rule adds: for a view the cluster cull K1 queried, a cluster is PENDING iff K1's test (hiz1, the pyramid in
 * force at K1) does not keep it, and it SURVIVES iff the same test against hiz2 (the pyramid in force at the second phase) keeps it;
 * the command fields are cluster_twin_view's. TEST INFRASTRUCTURE ONLY: nothing here comes from the product's kernels. */
#ifndef CLUSTER_SECOND_TWIN_H
#define CLUSTER_SECOND_TWIN_H

#include "cluster_twin.h"

typedef struct ClusterSecondTwinStats {
    uint32_t pending;           /* clusters K1 tested and did not keep */
    uint32_t frustum_rejects;   /* of those, rejected by the frustum test alone */
    uint32_t rejected_in_view;  /* pending clusters that pass the frustum test and that the second phase rejects */
    uint32_t both_phases;       /* draws with a command in K1 and a command in the second phase */
} ClusterSecondTwinStats;

/* The second-phase commands of ONE view that K1 queried (hiz1 and hiz2 non-NULL), in the rule's order: draw k ascending, cluster j
 * ascending. Arguments as cluster_twin_view; out has room for every cluster. Returns the number of commands. */
static uint32_t cluster_second_twin_view(const float* models, const uint32_t* g, const uint32_t* first, uint32_t n, const ClusterTwinGeometry* table,
                                         uint32_t table_count, const ClusterTwinRange* ranges, uint32_t range_count,
                                         const ClusterTwinCluster* clusters, const float view_proj[16], const GvoHiz* hiz1, const GvoHiz* hiz2,
                                         ClusterTwinCommand* out, ClusterSecondTwinStats* stats)
{
    GvoFrustum frustum;
    uint32_t commands = 0;
    gvo_frustum_from_view_proj(view_proj, &frustum);
    memset(stats, 0, sizeof(*stats));
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t instances = first[k + 1] - first[k];
        if (g[k] >= table_count || instances == 0)
            continue; /* a void draw: no candidate, never pending */
        if (g[k] >= range_count || ranges[g[k]].count == 0)
            continue; /* a whole draw: kept untested by K1, never pending */
        const ClusterTwinGeometry geometry = table[g[k]];
        const ClusterTwinRange range = ranges[g[k]];
        uint32_t kept_first = 0, kept_second = 0;
        for (uint32_t j = 0; j < range.count; j++) {
            const ClusterTwinCluster* cl = &clusters[range.first + j];
            const float* model = models + (size_t)k * 12;
            if (cluster_twin_survives(model, view_proj, &frustum, hiz1, cl)) {
                kept_first++;
                continue; /* a survivor of K1 */
            }
            stats->pending++;
            const int in_view = cluster_twin_survives(model, view_proj, &frustum, NULL, cl);
            if (!in_view)
                stats->frustum_rejects++;
            if (!cluster_twin_survives(model, view_proj, &frustum, hiz2, cl)) {
                if (in_view)
                    stats->rejected_in_view++;
                continue;
            }
            ClusterTwinCommand c = {cl->count, instances, geometry.first + cl->first, first[k], geometry.vertex_offset, k};
            out[commands++] = c;
            kept_second++;
        }
        if (kept_first && kept_second)
            stats->both_phases++;
    }
    return commands;
}

#endif
