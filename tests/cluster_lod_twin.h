/* cluster_lod_twin.h — the rule of gv_pool_cull_cluster_lods (include/garden_vis.h) restated in C99. Which
 * cluster passes the frustum and the pyramid is decided by cluster_twin_survives of cluster_twin.h, that is by the ORACLE's
 * gvo_is_behind_frustum and gvo_hiz_occluded; which one the cone rejects by cluster_cone_twin_rejected of cluster_cone_twin.h;
 * whether a cluster follows its predecessor in the index buffer by cluster_runs_twin_linked of cluster_runs_twin.h. This file
 * restates what the LOD form adds — the cut in fp32 with fmaf in the header's order, the conjunction, the second phase's pending
 * set under it — walks the draws in the rule's order and counts what the census (tests/test_cluster_lods_census.py) holds the case
 * table to. TEST INFRASTRUCTURE ONLY: nothing here comes from the product's kernels, and the product never includes it. Build
 * with -ffp-contract=off -fno-fast-math. */
#ifndef CLUSTER_LOD_TWIN_H
#define CLUSTER_LOD_TWIN_H

#include <math.h>

#include "cluster_cone_twin.h"

typedef struct ClusterLodTwinLod {
    float self_center[3], self_radius;
    float parent_center[3], parent_radius;
    float self_error, parent_error;
    uint32_t reserved[2];
} ClusterLodTwinLod;
typedef struct ClusterLodTwinView { float eye[4]; float scale; float near_distance; float reserved[2]; } ClusterLodTwinView;

/* what the census counts of one view (sums over the view's tested clusters) */
typedef struct ClusterLodCensus {
    uint32_t tested;        /* clusters of clustered draws */
    uint32_t lod_kept;      /* ... on the cut */
    uint32_t lod_frustum;   /* ... on the cut that the frustum rejects */
    uint32_t lod_hiz;       /* ... on the cut that the frustum keeps and the pyramid rejects */
    uint32_t lod_cone;      /* ... on the cut that the unchanged test keeps and the cone rejects */
    uint32_t base_kept;     /* ... that the unchanged test keeps, on the cut or not */
    uint32_t survivors;     /* ... that survive the conjunction */
    uint32_t eyes_disagree; /* ... on which the view's eye taken as a point and taken as parallel decide differently */
} ClusterLodCensus;

/* verdict bits of one tested cluster, in the order the clusters are tested: CLUSTER_CONE_TWIN_FRUSTUM, _BASE, _CONE, _PENDING and
 * _SECOND with their meanings, and */
#define CLUSTER_LOD_TWIN_KEPT 32u /* the cluster is on the cut */

/* s2: the largest squared column norm of the record's 12 floats f (a_rc = f[3c + r]) */
static float cluster_lod_twin_scale2(const float* f)
{
    float s2 = 0.0f;
    for (int c = 0; c < 3; c++) {
        const float n = fmaf(f[3 * c + 2], f[3 * c + 2], fmaf(f[3 * c + 1], f[3 * c + 1], f[3 * c + 0] * f[3 * c + 0]));
        s2 = n > s2 ? n : s2;
    }
    return s2;
}

/* EXCEEDS of one triple (c, r, e); point: the eye is a point */
static int cluster_lod_twin_exceeds(const float* f, const float c[3], float r, float e, float s2, const ClusterLodTwinView* view, int point)
{
    float C[3];
    for (int i = 0; i < 3; i++)
        C[i] = fmaf(f[0 + i], c[0], fmaf(f[3 + i], c[1], fmaf(f[6 + i], c[2], f[9 + i])));
    const float u0 = C[0] - view->eye[0], u1 = C[1] - view->eye[1], u2 = C[2] - view->eye[2];
    const float D = fmaf(u2, u2, fmaf(u1, u1, u0 * u0));
    const float q = e * view->scale;
    const float a = q + r;
    const float A = (a * a) * s2;
    const float Q = (q * q) * s2;
    const float N = view->near_distance * view->near_distance;
    if (point)
        return Q > N && A > D;
    return Q > N;
}

/* 1: the cluster is LOD-KEPT. `point`: -1 reads the view's eye[3]; 0 / 1 force a parallel / a point eye (the census). */
static int cluster_lod_twin_kept_as(const float* f, const ClusterLodTwinLod* lod, const ClusterLodTwinView* view, int point)
{
    if (view->scale == 0.0f)
        return 1;
    if (point < 0)
        point = view->eye[3] != 0.0f;
    const float s2 = cluster_lod_twin_scale2(f);
    return !cluster_lod_twin_exceeds(f, lod->self_center, lod->self_radius, lod->self_error, s2, view, point) &&
           cluster_lod_twin_exceeds(f, lod->parent_center, lod->parent_radius, lod->parent_error, s2, view, point);
}
static int cluster_lod_twin_kept(const float* f, const ClusterLodTwinLod* lod, const ClusterLodTwinView* view)
{
    return cluster_lod_twin_kept_as(f, lod, view, -1);
}

/* The commands of ONE view in the rule's order. Arguments as cluster_cone_twin_view; lods: parallel to clusters; lod_view: the
 * view's; cones and eye: NULL for a call without eyes (no cone test). mode: CLUSTER_CONE_TWIN_PLAIN, _RUNS or _SECOND_PHASE. */
static uint32_t cluster_lod_twin_view(const float* models, const uint32_t* g, const uint32_t* first, uint32_t n, const ClusterTwinGeometry* table,
                                      uint32_t table_count, const ClusterTwinRange* ranges, uint32_t range_count, const ClusterTwinCluster* clusters,
                                      const ClusterLodTwinLod* lods, const ClusterLodTwinView* lod_view, const ClusterConeTwinCone* cones,
                                      const float* eye, const float view_proj[16], const GvoHiz* hiz, const GvoHiz* hiz2, int mode,
                                      ClusterTwinCommand* out, uint32_t* tested, uint8_t* verdict, ClusterLodCensus* census)
{
    GvoFrustum frustum;
    ClusterLodCensus sum;
    uint32_t commands = 0;
    size_t at = 0;
    gvo_frustum_from_view_proj(view_proj, &frustum);
    memset(&sum, 0, sizeof(sum));
    *tested = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t instances = first[k + 1] - first[k];
        if (g[k] >= table_count || instances == 0)
            continue; /* the void geometry, or no instance: nothing */
        const ClusterTwinGeometry geometry = table[g[k]];
        ClusterTwinRange range = {0, 0};
        if (g[k] < range_count)
            range = ranges[g[k]];
        if (range.count == 0) { /* drawn whole, untested, never merged, never pending */
            if (mode != CLUSTER_CONE_TWIN_SECOND_PHASE) {
                ClusterTwinCommand whole = {geometry.count, instances, geometry.first, first[k], geometry.vertex_offset, k};
                out[commands++] = whole;
            }
            continue;
        }
        const ClusterTwinCluster* cl = &clusters[range.first];
        const float* model = models + (size_t)k * 12;
        uint32_t head = 0;
        int before = 0; /* cluster j - 1 survived */
        for (uint32_t j = 0; j < range.count; j++) {
            const int in_frustum = cluster_twin_survives(model, view_proj, &frustum, NULL, &cl[j]);
            const int base = cluster_twin_survives(model, view_proj, &frustum, hiz, &cl[j]);
            const int rejected = cones && eye ? cluster_cone_twin_rejected(model, &cones[range.first + j], eye) : 0;
            const int kept = cluster_lod_twin_kept(model, &lods[range.first + j], lod_view);
            const int survives = kept && base && !rejected; /* the conjunction */
            uint8_t bits = (uint8_t)((in_frustum ? CLUSTER_CONE_TWIN_FRUSTUM : 0u) | (base ? CLUSTER_CONE_TWIN_BASE : 0u) |
                                     (rejected ? CLUSTER_CONE_TWIN_CONE : 0u) | (kept ? CLUSTER_LOD_TWIN_KEPT : 0u));
            sum.tested++;
            sum.lod_kept += kept;
            sum.lod_frustum += kept && !in_frustum;
            sum.lod_hiz += kept && in_frustum && !base;
            sum.lod_cone += kept && base && rejected;
            sum.base_kept += base;
            sum.survivors += survives;
            sum.eyes_disagree += cluster_lod_twin_kept_as(model, &lods[range.first + j], lod_view, 0) !=
                                 cluster_lod_twin_kept_as(model, &lods[range.first + j], lod_view, 1);
            if (mode == CLUSTER_CONE_TWIN_SECOND_PHASE) {
                if (!survives) { /* PENDING: K1 tested it and did not keep it — the LOD-rejected clusters among them */
                    bits |= CLUSTER_CONE_TWIN_PENDING;
                    (*tested)++;
                    if (kept && cluster_twin_survives(model, view_proj, &frustum, hiz2, &cl[j]) && !rejected) {
                        ClusterTwinCommand c = {cl[j].count, instances, geometry.first + cl[j].first, first[k], geometry.vertex_offset, k};
                        out[commands++] = c;
                        bits |= CLUSTER_CONE_TWIN_SECOND;
                    }
                }
            } else {
                (*tested)++;
                if (survives) {
                    if (mode == CLUSTER_CONE_TWIN_RUNS && before && cluster_runs_twin_linked(cl, j)) {
                        out[commands - 1].count = cl[j].first + cl[j].count - cl[head].first; /* joins the run its predecessor is in */
                    } else { /* a survivor of the plain form; a HEAD of the run form */
                        ClusterTwinCommand c = {cl[j].count, instances, geometry.first + cl[j].first, first[k], geometry.vertex_offset, k};
                        out[commands++] = c;
                        head = j;
                    }
                }
                before = survives;
            }
            if (verdict)
                verdict[at] = bits;
            at++;
        }
    }
    if (census)
        *census = sum;
    return commands;
}

#endif
