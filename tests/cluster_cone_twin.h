/* cluster_cone_twin.h — the rule of gv_pool_cull_cluster_cones (include/garden_vis.h) restated in C99. Which
 * cluster passes the frustum and the pyramid is decided by cluster_twin_survives of cluster_twin.h, that is by the ORACLE's
 * gvo_is_behind_frustum and gvo_hiz_occluded; whether a cluster follows its predecessor in the index buffer by
 * cluster_runs_twin_linked of cluster_runs_twin.h. This file restates what the cone form adds — the cone test in fp32 with fmaf in
 * the header's order, the conjunction, the second phase's pending set under it — walks the draws in the rule's order and counts
 * what the census (tests/test_cluster_cones_census.py) holds the case table to. TEST INFRASTRUCTURE ONLY: nothing here comes from
 * the product's kernels, and the product never includes it. Build with -ffp-contract=off -fno-fast-math. */
#ifndef CLUSTER_CONE_TWIN_H
#define CLUSTER_CONE_TWIN_H

#include <math.h>

#include "cluster_twin.h"
#include "cluster_runs_twin.h"

typedef struct ClusterConeTwinCone { float apex[3]; float cutoff; float axis[3]; uint32_t reserved; } ClusterConeTwinCone;

/* what the census counts of one view (sums over the view's tested clusters and its draws) */
typedef struct ClusterConeCensus {
    uint32_t tested;         /* clusters of clustered draws */
    uint32_t frustum_kept;   /* ... that the frustum test keeps */
    uint32_t base_kept;      /* ... that the unchanged test (frustum and, where queried, the pyramid) keeps */
    uint32_t cone_rejected;  /* ... that the cone rejects, whatever the unchanged test says */
    uint32_t cone_only;      /* ... that the cone rejects and the unchanged test keeps */
    uint32_t hiz_only;       /* ... that the frustum keeps, the pyramid rejects and the cone keeps */
    uint32_t survivors;      /* ... that survive the conjunction */
    uint32_t partial;        /* draws of which the cone rejects some clusters and not all */
} ClusterConeCensus;

/* verdict bits of one tested cluster (cluster_cone_twin_view's `verdict`, in the order the clusters are tested) */
#define CLUSTER_CONE_TWIN_FRUSTUM 1u  /* the frustum keeps it */
#define CLUSTER_CONE_TWIN_BASE 2u     /* the unchanged test keeps it */
#define CLUSTER_CONE_TWIN_CONE 4u     /* the cone rejects it */
#define CLUSTER_CONE_TWIN_PENDING 8u  /* second phase: K1 did not keep it */
#define CLUSTER_CONE_TWIN_SECOND 16u  /* second phase: it survives */

/* a_rc * ... - ...: one adjugate entry, p * q - r * s as fmaf(p, q, -(r * s)) */
static float cluster_cone_twin_cross(float p, float q, float r, float s) { return fmaf(p, q, -(r * s)); }

/* 1: the cluster is CONE-REJECTED. model12: the record's 12 floats, column-major (a_rc = f[3c + r], t_r = f[9 + r]). */
static int cluster_cone_twin_rejected(const float* f, const ClusterConeTwinCone* cone, const float eye[4])
{
    const float a00 = f[0], a10 = f[1], a20 = f[2], a01 = f[3], a11 = f[4], a21 = f[5], a02 = f[6], a12 = f[7], a22 = f[8];
    float j[3][3], w[3];
    j[0][0] = cluster_cone_twin_cross(a11, a22, a12, a21), j[0][1] = cluster_cone_twin_cross(a02, a21, a01, a22);
    j[0][2] = cluster_cone_twin_cross(a01, a12, a02, a11);
    j[1][0] = cluster_cone_twin_cross(a12, a20, a10, a22), j[1][1] = cluster_cone_twin_cross(a00, a22, a02, a20);
    j[1][2] = cluster_cone_twin_cross(a02, a10, a00, a12);
    j[2][0] = cluster_cone_twin_cross(a10, a21, a11, a20), j[2][1] = cluster_cone_twin_cross(a01, a20, a00, a21);
    j[2][2] = cluster_cone_twin_cross(a00, a11, a01, a10);
    const float det = fmaf(a00, j[0][0], fmaf(a01, j[1][0], a02 * j[2][0]));
    const int facing = det > 0.0f && det < INFINITY;
    if (eye[3] != 0.0f) { /* a point eye */
        const float u0 = eye[0] - f[9], u1 = eye[1] - f[10], u2 = eye[2] - f[11];
        for (int r = 0; r < 3; r++)
            w[r] = fmaf(det, cone->apex[r], -fmaf(j[r][0], u0, fmaf(j[r][1], u1, j[r][2] * u2)));
    } else { /* parallel rays along eye[0..2] */
        for (int r = 0; r < 3; r++)
            w[r] = fmaf(j[r][0], eye[0], fmaf(j[r][1], eye[1], j[r][2] * eye[2]));
    }
    const float s = fmaf(w[0], cone->axis[0], fmaf(w[1], cone->axis[1], w[2] * cone->axis[2]));
    const float ww = fmaf(w[0], w[0], fmaf(w[1], w[1], w[2] * w[2]));
    const float q = s * s;
    const float r = (cone->cutoff * cone->cutoff) * ww;
    return facing && s > 0.0f && q > 0.0f && q < INFINITY && q >= r;
}

#define CLUSTER_CONE_TWIN_PLAIN 0  /* one command per survivor */
#define CLUSTER_CONE_TWIN_RUNS 1   /* one command per run of adjacent survivors (the rule of cluster_runs_twin.h over these decisions) */
#define CLUSTER_CONE_TWIN_SECOND_PHASE 2 /* the second phase behind a cone result: hiz is K1's pyramid (non-NULL), hiz2 the one in force now */

/* The commands of ONE view in the rule's order: draw k ascending, cluster (or head) j ascending. models, g, first, n, the tables,
 * view_proj, hiz, out: as cluster_twin_view; cones: parallel to clusters; eye: the view's. *tested = clusters tested (second phase:
 * the pending clusters). verdict (may be NULL): one byte per cluster of a clustered draw, in order. census (may be NULL) is
 * overwritten. Returns the number of commands. */
static uint32_t cluster_cone_twin_view(const float* models, const uint32_t* g, const uint32_t* first, uint32_t n, const ClusterTwinGeometry* table,
                                       uint32_t table_count, const ClusterTwinRange* ranges, uint32_t range_count, const ClusterTwinCluster* clusters,
                                       const ClusterConeTwinCone* cones, const float eye[4], const float view_proj[16], const GvoHiz* hiz,
                                       const GvoHiz* hiz2, int mode, ClusterTwinCommand* out, uint32_t* tested, uint8_t* verdict,
                                       ClusterConeCensus* census)
{
    GvoFrustum frustum;
    ClusterConeCensus sum;
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
        uint32_t rejected_here = 0, head = 0;
        int before = 0; /* cluster j - 1 survived */
        for (uint32_t j = 0; j < range.count; j++) {
            const int in_frustum = cluster_twin_survives(model, view_proj, &frustum, NULL, &cl[j]);
            const int base = cluster_twin_survives(model, view_proj, &frustum, hiz, &cl[j]);
            const int rejected = cluster_cone_twin_rejected(model, &cones[range.first + j], eye);
            const int survives = base && !rejected; /* the conjunction */
            uint8_t bits = (uint8_t)((in_frustum ? CLUSTER_CONE_TWIN_FRUSTUM : 0u) | (base ? CLUSTER_CONE_TWIN_BASE : 0u) |
                                     (rejected ? CLUSTER_CONE_TWIN_CONE : 0u));
            sum.tested++;
            sum.frustum_kept += in_frustum;
            sum.base_kept += base;
            sum.cone_rejected += rejected;
            sum.cone_only += base && rejected;
            sum.hiz_only += in_frustum && !base && !rejected;
            sum.survivors += survives;
            rejected_here += rejected;
            if (mode == CLUSTER_CONE_TWIN_SECOND_PHASE) {
                if (!survives) { /* PENDING: K1 tested it and did not keep it — the cone-rejected clusters among them */
                    bits |= CLUSTER_CONE_TWIN_PENDING;
                    (*tested)++;
                    if (cluster_twin_survives(model, view_proj, &frustum, hiz2, &cl[j]) && !rejected) {
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
                    } else { /* a survivor of the plain form; a HEAD of the run form: not linked, or cluster j - 1 did not survive */
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
        if (rejected_here != 0 && rejected_here != range.count)
            sum.partial++;
    }
    if (census)
        *census = sum;
    return commands;
}

#endif
