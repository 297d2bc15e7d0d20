/* occluder_twin.h — TEST ONLY: plain-C99 restatement of the occluder-depth rule of DESIGN.md §4 item 16 (gv_device_math.hpp
 * occluder_*; kernels gv_occluders.hip), the check gv_pool_draw_occluders is compared against word for word. Compile with
 * -ffp-contract=off -fno-fast-math: every multiply that feeds an add is written as fmaf. One corner, one occluder, one pixel and
 * one pixel corner at a time — none of the kernel's packing, tiles, worst-corner shortcuts or atomics.
 *
 * THE RULE (the same text stands in DESIGN.md §4 item 16 and gv_device_math.hpp). For draw k of a view: slot s_k, record model M_k,
 * the slot's occluder box (omin, omax) in model space, VP = the view's view_proj, the image W x H, the call's min_pixels.
 *  1. Has a box <=> omin.x < omax.x && omin.y < omax.y && omin.z < omax.z (a NaN fails). Otherwise: not an occluder, counted no_box.
 *  2. Corners p_c = aabb_corners(M_k, omin, omax) (item 5: bit0 -> x, bit1 -> y, bit2 -> z selects max; every row
 *     fma(c0, x, fma(c1, y, fma(c2, z, c3)))). Clip: cl_r = fma(VP[r], p.x, fma(VP[4 + r], p.y, fma(VP[8 + r], p.z, VP[12 + r]))) for
 *     r = x, y, z, w; rcp = 1.0f / cl_w (IEEE); u = fma(cl_x * rcp, .5, .5), v = fma(cl_y * rcp, .5, .5), z = cl_z * rcp: the words of
 *     the Hi-Z query (hiz_occluded), restated.
 *  3. Any corner with !(cl_w > 0): skipped, counted behind.
 *  4. d = minNum(minNum over the 8 corners of z, 1.0f); !(d > 0): skipped, counted behind. (Reversed Z: d is the box's farthest depth.)
 *  5. fx = floorf(u * (float)(16 W)), fy = floorf(v * (float)(16 H)): four sub-pixel bits. Any !(|f| < 4194304.0f): skipped, counted
 *     range (a NaN or an infinity lands here). Otherwise X_c, Y_c are int32.
 *  6. Faces as corner cycles: -x (0,4,6,2), +x (1,3,7,5), -y (0,1,5,4), +y (2,6,7,3), -z (0,2,3,1), +z (4,5,7,6).
 *     A_f = sum over the cycle's edges p -> q of (X_p Y_q - X_q Y_p) in int64; a face is positive <=> A_f > 0. Each of the 12 box edges
 *     belongs to two faces: it is active <=> exactly one of them is positive, directed a -> b as in the positive face's cycle.
 *     No positive face: skipped, counted flat. (Positive faces may be the front or the back set; both bound the same silhouette.)
 *  7. Pixel (px, py) is covered <=> for every active edge and each pixel corner cx in {px, px + 1}, cy in {py, py + 1}:
 *     ex (16 cy - Y_a) - ey (16 cx - X_a) >= 2 (|ex| + |ey|), ex = X_b - X_a, ey = Y_b - Y_a, all int64. The margin 2 pays for the
 *     snapping (under one unit per axis) and the fp32 rounding in front of it (about one more).
 *  8. x0 = max(min X >> 4, 0), x1 = min(max X >> 4, W - 1) (arithmetic shifts), y likewise. An empty range, or a width or height in
 *     pixels below min_pixels: skipped, counted small. Otherwise the occluder is counted drawn (whether or not it covers a pixel).
 *  9. depth[py W + px] = max(0.0f, max over the covering occluders of d), taken on the floats' bits as uint32: every value is >= 0,
 *     so that order is the float order, and the maximum does not depend on any order of evaluation.
 */
#ifndef GV_OCCLUDER_TWIN_H
#define GV_OCCLUDER_TWIN_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define OCCLUDER_TWIN_MARGIN 2

typedef struct OccluderTwinCounts { /* GvOccluderCounts */
    uint32_t drawn, no_box, behind, range, flat, small;
} OccluderTwinCounts;

enum { OCCLUDER_TWIN_DRAWN = 0, OCCLUDER_TWIN_NO_BOX, OCCLUDER_TWIN_BEHIND, OCCLUDER_TWIN_RANGE, OCCLUDER_TWIN_FLAT, OCCLUDER_TWIN_SMALL };

typedef struct OccluderTwinSetup {
    int32_t X[8], Y[8];
    float u[8], v[8], z[8]; /* the words of item 2 (what the Hi-Z query of the same box computes) */
    float d;
    int64_t area[6];
    int positive[6];
    int active_count;
    int edge_a[12], edge_b[12]; /* the active edges, directed */
    int32_t x0, x1, y0, y1;
} OccluderTwinSetup;

static const int occluder_twin_face[6][4] = {{0, 4, 6, 2}, {1, 3, 7, 5}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 2, 3, 1}, {4, 5, 7, 6}};

static inline float occluder_twin_row(const float m[12], int r, float x, float y, float z)
{
    return fmaf(m[r], x, fmaf(m[3 + r], y, fmaf(m[6 + r], z, m[9 + r])));
}
static inline float occluder_twin_clip(const float vp[16], int r, float x, float y, float z)
{
    return fmaf(vp[r], x, fmaf(vp[4 + r], y, fmaf(vp[8 + r], z, vp[12 + r])));
}

/* items 1 - 6 and 8 for one occluder: its class (OCCLUDER_TWIN_*), *s filled as far as the rule got.
 * model: 12 floats c0.xyz c1.xyz c2.xyz c3.xyz; box: (min.xyz, max.xyz). */
static inline int occluder_twin_setup(const float model[12], const float box[6], const float vp[16], uint32_t W, uint32_t H, uint32_t min_pixels,
                                      OccluderTwinSetup* s)
{
    int c, f, j, any = 0;
    int behind = 0, range = 0;
    float zmin = 0.0f;
    int32_t xmin, xmax, ymin, ymax;
    memset(s, 0, sizeof(*s));
    if (!(box[0] < box[3] && box[1] < box[4] && box[2] < box[5]))
        return OCCLUDER_TWIN_NO_BOX;
    for (c = 0; c < 8; c++) {
        const float x = box[(c & 1) ? 3 : 0], y = box[(c & 2) ? 4 : 1], z = box[(c & 4) ? 5 : 2];
        const float px = occluder_twin_row(model, 0, x, y, z), py = occluder_twin_row(model, 1, x, y, z), pz = occluder_twin_row(model, 2, x, y, z);
        const float clx = occluder_twin_clip(vp, 0, px, py, pz), cly = occluder_twin_clip(vp, 1, px, py, pz);
        const float clz = occluder_twin_clip(vp, 2, px, py, pz), clw = occluder_twin_clip(vp, 3, px, py, pz);
        const float rcp = 1.0f / clw;
        if (!(clw > 0.0f))
            behind = 1;
        s->u[c] = fmaf(clx * rcp, 0.5f, 0.5f);
        s->v[c] = fmaf(cly * rcp, 0.5f, 0.5f);
        s->z[c] = clz * rcp;
        zmin = c ? fminf(zmin, s->z[c]) : s->z[c];
    }
    if (behind)
        return OCCLUDER_TWIN_BEHIND;
    s->d = fminf(zmin, 1.0f);
    if (!(s->d > 0.0f))
        return OCCLUDER_TWIN_BEHIND;
    for (c = 0; c < 8; c++) {
        const float fx = floorf(s->u[c] * (float)(16u * W)), fy = floorf(s->v[c] * (float)(16u * H));
        if (!(fabsf(fx) < 4194304.0f) || !(fabsf(fy) < 4194304.0f)) {
            range = 1;
            continue;
        }
        s->X[c] = (int32_t)fx;
        s->Y[c] = (int32_t)fy;
    }
    if (range)
        return OCCLUDER_TWIN_RANGE;
    for (f = 0; f < 6; f++) {
        int64_t a = 0;
        for (j = 0; j < 4; j++) {
            const int p = occluder_twin_face[f][j], q = occluder_twin_face[f][(j + 1) & 3];
            a += (int64_t)s->X[p] * s->Y[q] - (int64_t)s->X[q] * s->Y[p];
        }
        s->area[f] = a;
        s->positive[f] = a > 0;
        any |= s->positive[f];
    }
    if (!any)
        return OCCLUDER_TWIN_FLAT;
    /* an edge p -> q of a positive face is active when the face that holds q -> p is not positive */
    for (f = 0; f < 6; f++)
        for (j = 0; j < 4 && s->positive[f]; j++) {
            const int p = occluder_twin_face[f][j], q = occluder_twin_face[f][(j + 1) & 3];
            int g, i, other = -1;
            for (g = 0; g < 6; g++)
                for (i = 0; i < 4; i++)
                    if (occluder_twin_face[g][i] == q && occluder_twin_face[g][(i + 1) & 3] == p)
                        other = g;
            if (!s->positive[other]) {
                s->edge_a[s->active_count] = p;
                s->edge_b[s->active_count] = q;
                s->active_count++;
            }
        }
    xmin = xmax = s->X[0], ymin = ymax = s->Y[0];
    for (c = 1; c < 8; c++) {
        xmin = s->X[c] < xmin ? s->X[c] : xmin, xmax = s->X[c] > xmax ? s->X[c] : xmax;
        ymin = s->Y[c] < ymin ? s->Y[c] : ymin, ymax = s->Y[c] > ymax ? s->Y[c] : ymax;
    }
    s->x0 = (xmin >> 4) > 0 ? (xmin >> 4) : 0;
    s->x1 = (xmax >> 4) < (int32_t)W - 1 ? (xmax >> 4) : (int32_t)W - 1;
    s->y0 = (ymin >> 4) > 0 ? (ymin >> 4) : 0;
    s->y1 = (ymax >> 4) < (int32_t)H - 1 ? (ymax >> 4) : (int32_t)H - 1;
    if (s->x0 > s->x1 || s->y0 > s->y1 || (uint32_t)(s->x1 - s->x0 + 1) < min_pixels || (uint32_t)(s->y1 - s->y0 + 1) < min_pixels)
        return OCCLUDER_TWIN_SMALL;
    return OCCLUDER_TWIN_DRAWN;
}

/* item 7 for one pixel, with the margin as a parameter (the rule's is OCCLUDER_TWIN_MARGIN; the census also runs 0) */
static inline int occluder_twin_covered(const OccluderTwinSetup* s, int32_t px, int32_t py, int64_t margin)
{
    int e, k;
    for (e = 0; e < s->active_count; e++) {
        const int a = s->edge_a[e], b = s->edge_b[e];
        const int64_t ex = (int64_t)s->X[b] - s->X[a], ey = (int64_t)s->Y[b] - s->Y[a];
        const int64_t need = margin * ((ex < 0 ? -ex : ex) + (ey < 0 ? -ey : ey));
        for (k = 0; k < 4; k++) {
            const int64_t cx = px + (k & 1), cy = py + (k >> 1);
            if (ex * (16 * cy - s->Y[a]) - ey * (16 * cx - s->X[a]) < need)
                return 0;
        }
    }
    return 1;
}

/* item 9 for one drawn occluder; returns the pixels it covers */
static inline uint32_t occluder_twin_raster(const OccluderTwinSetup* s, float* depth, uint32_t W, int64_t margin)
{
    int32_t px, py;
    uint32_t covered = 0, bits, held;
    memcpy(&bits, &s->d, 4);
    for (py = s->y0; py <= s->y1; py++)
        for (px = s->x0; px <= s->x1; px++)
            if (occluder_twin_covered(s, px, py, margin)) {
                float* at = depth + (size_t)py * W + px;
                memcpy(&held, at, 4);
                if (held < bits)
                    memcpy(at, &bits, 4);
                covered++;
            }
    return covered;
}

/* n records into `depth` (W x H, accumulated: clear it for a new image): models[12 k], boxes[6 k] (the occluder box of the record's
 * slot, already looked up). The counts are added to. */
static inline void occluder_twin_draw(const float* models, const float* boxes, uint32_t n, const float vp[16], uint32_t W, uint32_t H,
                                      uint32_t min_pixels, float* depth, OccluderTwinCounts* counts)
{
    uint32_t k;
    OccluderTwinSetup s;
    for (k = 0; k < n; k++) {
        const int cls = occluder_twin_setup(models + 12 * (size_t)k, boxes + 6 * (size_t)k, vp, W, H, min_pixels, &s);
        (&counts->drawn)[cls]++;
        if (cls == OCCLUDER_TWIN_DRAWN)
            occluder_twin_raster(&s, depth, W, OCCLUDER_TWIN_MARGIN);
    }
}

/* Which of the kernel's three tile paths the tiles of a drawn occluder take, T x T pixels a tile on the image's grid, each tile
 * clipped to the occluder's pixel range: paths[0] wholly inside all edges, [1] mixed, [2] wholly outside some edge. Stated on the
 * pixel corners the clipped tile spans: E is linear, so "every corner of the rectangle passes" is "every pixel corner passes". */
static inline void occluder_twin_tile_paths(const OccluderTwinSetup* s, uint32_t T, uint32_t paths[3])
{
    int32_t tx, ty;
    int e, k;
    for (ty = s->y0 / (int32_t)T; ty <= s->y1 / (int32_t)T; ty++)
        for (tx = s->x0 / (int32_t)T; tx <= s->x1 / (int32_t)T; tx++) {
            const int32_t rx0 = tx * (int32_t)T > s->x0 ? tx * (int32_t)T : s->x0, ry0 = ty * (int32_t)T > s->y0 ? ty * (int32_t)T : s->y0;
            const int32_t rx1 = (tx + 1) * (int32_t)T - 1 < s->x1 ? (tx + 1) * (int32_t)T - 1 : s->x1;
            const int32_t ry1 = (ty + 1) * (int32_t)T - 1 < s->y1 ? (ty + 1) * (int32_t)T - 1 : s->y1;
            int inside = 1, outside = 0;
            for (e = 0; e < s->active_count; e++) {
                const int a = s->edge_a[e], b = s->edge_b[e];
                const int64_t ex = (int64_t)s->X[b] - s->X[a], ey = (int64_t)s->Y[b] - s->Y[a];
                const int64_t need = OCCLUDER_TWIN_MARGIN * ((ex < 0 ? -ex : ex) + (ey < 0 ? -ey : ey));
                int pass = 0;
                for (k = 0; k < 4; k++) {
                    const int64_t cx = (k & 1) ? rx1 + 1 : rx0, cy = (k >> 1) ? ry1 + 1 : ry0;
                    pass += ex * (16 * cy - s->Y[a]) - ey * (16 * cx - s->X[a]) >= need;
                }
                inside &= pass == 4;
                outside |= pass == 0;
            }
            paths[outside ? 2 : (inside ? 0 : 1)]++;
        }
}

#endif
