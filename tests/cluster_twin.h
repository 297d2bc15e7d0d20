/* cluster_twin.h — the rule of gv_pool_cull_clusters (include/garden_vis.h) restated in C over the ORACLE's
 * two tests: gvo_is_behind_frustum and gvo_hiz_occluded of oracle/gv_oracle.h decide every cluster; this file adds only what the
 * rule adds — which draws have candidates, their order, whole draws, the command's fields. TEST INFRASTRUCTURE ONLY: nothing here
 * comes from the product's kernels, and the product never includes it. Placement (regions, capacity, the caller's layout) is
 * restated in tests/clusters_support.py. */
#ifndef CLUSTER_TWIN_H
#define CLUSTER_TWIN_H

#include <stdint.h>
#include <string.h>

#include "../oracle/gv_oracle.h"

typedef struct ClusterTwinGeometry { uint32_t count, first; int32_t vertex_offset; } ClusterTwinGeometry;
typedef struct ClusterTwinRange { uint32_t first, count; } ClusterTwinRange;
typedef struct ClusterTwinCluster { float box_min[3]; uint32_t first; float box_max[3]; uint32_t count; } ClusterTwinCluster;
typedef struct ClusterTwinCommand { uint32_t count, instance_count, first, first_instance; int32_t vertex_offset; uint32_t draw; } ClusterTwinCommand;

/* M_k: the record's 12 floats (c0.xyz c1.xyz c2.xyz c3.xyz) completed with the row (0, 0, 0, 1) */
static void cluster_twin_model(const float* model12, float out[16])
{
    for (int c = 0; c < 4; c++) {
        out[c * 4 + 0] = model12[c * 3 + 0];
        out[c * 4 + 1] = model12[c * 3 + 1];
        out[c * 4 + 2] = model12[c * 3 + 2];
        out[c * 4 + 3] = c == 3 ? 1.0f : 0.0f;
    }
}

/* 1: the cluster survives. hiz NULL: the frustum test alone. */
static int cluster_twin_survives(const float* model12, const float view_proj[16], const GvoFrustum* frustum, const GvoHiz* hiz,
                                 const ClusterTwinCluster* cl)
{
    float model[16];
    cluster_twin_model(model12, model);
    if (gvo_is_behind_frustum(frustum, cl->box_min, cl->box_max, model))
        return 0;
    if (hiz && gvo_hiz_occluded(hiz, view_proj, cl->box_min, cl->box_max, model))
        return 0;
    return 1;
}

/* The commands of ONE view in the rule's order: draw k ascending, cluster j ascending. models: 12 floats per draw as fetched;
 * g[k]: the draw's geometry id; first[0 .. n]: first_k with the closing word starts[v + 1] behind the last draw. out: room for
 * every candidate (the caller sizes it: sum of max(1, range count)); survivors_without_hiz (may be NULL): how many clusters the
 * frustum test alone keeps; partial (may be NULL): draws that keep some but not all of their clusters. Returns the number of
 * commands; *tested = clusters tested. */
static uint32_t cluster_twin_view(const float* models, const uint32_t* g, const uint32_t* first, uint32_t n, const ClusterTwinGeometry* table,
                                  uint32_t table_count, const ClusterTwinRange* ranges, uint32_t range_count, const ClusterTwinCluster* clusters,
                                  const float view_proj[16], const GvoHiz* hiz, ClusterTwinCommand* out, uint32_t* tested,
                                  uint32_t* survivors_without_hiz, uint32_t* partial)
{
    GvoFrustum frustum;
    uint32_t commands = 0;
    gvo_frustum_from_view_proj(view_proj, &frustum);
    *tested = 0;
    if (survivors_without_hiz)
        *survivors_without_hiz = 0;
    if (partial)
        *partial = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t instances = first[k + 1] - first[k];
        if (g[k] >= table_count || instances == 0)
            continue; /* the void geometry, or no instance: nothing */
        const ClusterTwinGeometry geometry = table[g[k]];
        ClusterTwinRange range = {0, 0};
        if (g[k] < range_count)
            range = ranges[g[k]];
        if (range.count == 0) { /* drawn whole, untested */
            ClusterTwinCommand c = {geometry.count, instances, geometry.first, first[k], geometry.vertex_offset, k};
            out[commands++] = c;
            continue;
        }
        uint32_t kept = 0;
        for (uint32_t j = 0; j < range.count; j++) {
            const ClusterTwinCluster* cl = &clusters[range.first + j];
            (*tested)++;
            if (survivors_without_hiz && cluster_twin_survives(models + (size_t)k * 12, view_proj, &frustum, NULL, cl))
                (*survivors_without_hiz)++;
            if (!cluster_twin_survives(models + (size_t)k * 12, view_proj, &frustum, hiz, cl))
                continue;
            ClusterTwinCommand c = {cl->count, instances, geometry.first + cl->first, first[k], geometry.vertex_offset, k};
            out[commands++] = c;
            kept++;
        }
        if (partial && kept != 0 && kept != range.count)
            (*partial)++;
    }
    return commands;
}

#endif
