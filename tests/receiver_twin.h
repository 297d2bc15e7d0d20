/* receiver_twin.h — TEST ONLY: plain-C99 restatement of the receiver-mask rule of DESIGN.md §4 item 17 (gv_device_math.hpp receiver_*;
 * kernels gv_receivers.hip), the check gv_pool_draw_receivers is compared against word for word. Compile with -ffp-contract=off
 * -fno-fast-math: every multiply that feeds an add is written as fmaf. One corner, one record, one pixel and one pixel corner at a
 * time — none of the kernel's packing, tiles, small-range shortcut or atomics. Of occluder_twin.h it takes the row and clip chains
 * (step 1) and the face cycles (step 6).
 *
 * THE RECEIVER RULE (the same text stands in DESIGN.md §4 item 17 and gv_device_math.hpp). For draw k of the source view: slot s_k,
 * record model M_k, the slot's cull AABB (amin, amax) as the mesh mirror holds it, L = the call's light_view_proj, the mask W x H.
 *  1. Corners p_c = aabb_corners(M_k, amin, amax) and clip coordinates exactly as item 16 step 2 with L in place of VP: cl_r = fma(L[r],
 *     p.x, fma(L[4 + r], p.y, fma(L[8 + r], p.z, L[12 + r]))), rcp = 1.0f / cl_w (IEEE), u = fma(cl_x * rcp, .5, .5), v likewise,
 *     z = cl_z * rcp: a caster that is also a receiver gets the words its own Hi-Z query computes against L.
 *  2. Any corner with !(cl_w > 0): counted behind, and +0.0f goes into EVERY pixel of the mask (a receiver that cannot be bounded keeps
 *     every caster; it is never skipped).
 *  3. m = minNum over the 8 corners of z; d = (m > 0.0f) ? m : +0.0f (a NaN gives +0.0f; -0.0f, whose bits are the largest unsigned
 *     word, never appears). No upper clamp: a receiver in front of the near plane keeps its d > 1.
 *  4. fx = floorf(u * (float)(16 W)), fy = floorf(v * (float)(16 H)). Any !(|f| < 4194304.0f): counted range, and d goes into every
 *     pixel of the mask. Otherwise X_c, Y_c are int32.
 *  5. x0 = max((min X - 2) >> 4, 0), x1 = min((max X + 2) >> 4, W - 1) (arithmetic shifts; the 2 is item 16's margin), y likewise. An
 *     empty range: counted outside, nothing written.
 *  6. Faces, areas (int64) and active directed edges as item 16 step 6. No positive face: counted flat, and d goes into every pixel of
 *     the range (an edge-on sprite, a sub-pixel box).
 *  7. Otherwise counted drawn. Pixel (px, py) of the range is touched <=> for EVERY active edge a -> b SOME pixel corner cx in {px, px + 1},
 *     cy in {py, py + 1} passes ex (16 cy - Y_a) - ey (16 cx - X_a) >= -2 (|ex| + |ey|), ex = X_b - X_a, ey = Y_b - Y_a, all int64: item
 *     16's half-plane test at the corner that lies MOST inside, with the margin on the other side. d goes into every touched pixel.
 *  8. mask[py W + px] = min(+inf, min over the receivers that write the pixel of their word), taken on the floats' bits as uint32: every
 *     word is a non-negative float or +inf, so that order is the float order, and the result depends on no order of evaluation.
 */
#ifndef GV_RECEIVER_TWIN_H
#define GV_RECEIVER_TWIN_H
#include "occluder_twin.h"

#define RECEIVER_TWIN_MARGIN 2

typedef struct ReceiverTwinCounts { /* GvReceiverCounts */
    uint32_t drawn, flat, behind, range, outside, reserved;
} ReceiverTwinCounts;

enum { RECEIVER_TWIN_DRAWN = 0, RECEIVER_TWIN_FLAT, RECEIVER_TWIN_BEHIND, RECEIVER_TWIN_RANGE, RECEIVER_TWIN_OUTSIDE };

typedef struct ReceiverTwinSetup {
    int32_t X[8], Y[8];
    float u[8], v[8], z[8]; /* the words of step 1 (what the Hi-Z query of the same box computes against L) */
    float d;                /* the word the record writes: step 3's, or +0.0f of a record behind L */
    int64_t area[6];
    int positive[6];
    int active_count;
    int edge_a[12], edge_b[12]; /* the active edges, directed */
    int32_t x0, x1, y0, y1;     /* the pixels it may write: step 5's range, or the whole mask (behind, range) */
} ReceiverTwinSetup;

/* steps 1 - 6 for one record: its class (RECEIVER_TWIN_*), *s filled as far as the rule got.
 * model: 12 floats c0.xyz c1.xyz c2.xyz c3.xyz; box: (amin.xyz, amax.xyz). */
static inline int receiver_twin_setup(const float model[12], const float box[6], const float light[16], uint32_t W, uint32_t H, ReceiverTwinSetup* s)
{
    int c, f, j, any = 0;
    int behind = 0, range = 0;
    float m = 0.0f;
    int32_t xmin, xmax, ymin, ymax;
    memset(s, 0, sizeof(*s));
    s->x0 = 0, s->x1 = (int32_t)W - 1, s->y0 = 0, s->y1 = (int32_t)H - 1;
    for (c = 0; c < 8; c++) {
        const float x = box[(c & 1) ? 3 : 0], y = box[(c & 2) ? 4 : 1], z = box[(c & 4) ? 5 : 2];
        const float px = occluder_twin_row(model, 0, x, y, z), py = occluder_twin_row(model, 1, x, y, z), pz = occluder_twin_row(model, 2, x, y, z);
        const float clx = occluder_twin_clip(light, 0, px, py, pz), cly = occluder_twin_clip(light, 1, px, py, pz);
        const float clz = occluder_twin_clip(light, 2, px, py, pz), clw = occluder_twin_clip(light, 3, px, py, pz);
        const float rcp = 1.0f / clw;
        if (!(clw > 0.0f))
            behind = 1;
        s->u[c] = fmaf(clx * rcp, 0.5f, 0.5f);
        s->v[c] = fmaf(cly * rcp, 0.5f, 0.5f);
        s->z[c] = clz * rcp;
        m = c ? fminf(m, s->z[c]) : s->z[c];
    }
    if (behind) {
        s->d = 0.0f;
        return RECEIVER_TWIN_BEHIND;
    }
    s->d = (m > 0.0f) ? m : 0.0f;
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
        return RECEIVER_TWIN_RANGE;
    xmin = xmax = s->X[0], ymin = ymax = s->Y[0];
    for (c = 1; c < 8; c++) {
        xmin = s->X[c] < xmin ? s->X[c] : xmin, xmax = s->X[c] > xmax ? s->X[c] : xmax;
        ymin = s->Y[c] < ymin ? s->Y[c] : ymin, ymax = s->Y[c] > ymax ? s->Y[c] : ymax;
    }
    s->x0 = ((xmin - RECEIVER_TWIN_MARGIN) >> 4) > 0 ? ((xmin - RECEIVER_TWIN_MARGIN) >> 4) : 0;
    s->x1 = ((xmax + RECEIVER_TWIN_MARGIN) >> 4) < (int32_t)W - 1 ? ((xmax + RECEIVER_TWIN_MARGIN) >> 4) : (int32_t)W - 1;
    s->y0 = ((ymin - RECEIVER_TWIN_MARGIN) >> 4) > 0 ? ((ymin - RECEIVER_TWIN_MARGIN) >> 4) : 0;
    s->y1 = ((ymax + RECEIVER_TWIN_MARGIN) >> 4) < (int32_t)H - 1 ? ((ymax + RECEIVER_TWIN_MARGIN) >> 4) : (int32_t)H - 1;
    if (s->x0 > s->x1 || s->y0 > s->y1)
        return RECEIVER_TWIN_OUTSIDE;
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
        return RECEIVER_TWIN_FLAT;
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
    return RECEIVER_TWIN_DRAWN;
}

/* step 7 for one pixel of a drawn record, with the margin as a parameter (the rule's is RECEIVER_TWIN_MARGIN) */
static inline int receiver_twin_touched(const ReceiverTwinSetup* s, int32_t px, int32_t py, int64_t margin)
{
    int e, k;
    for (e = 0; e < s->active_count; e++) {
        const int a = s->edge_a[e], b = s->edge_b[e];
        const int64_t ex = (int64_t)s->X[b] - s->X[a], ey = (int64_t)s->Y[b] - s->Y[a];
        const int64_t least = -margin * ((ex < 0 ? -ex : ex) + (ey < 0 ? -ey : ey));
        int some = 0;
        for (k = 0; k < 4; k++) {
            const int64_t cx = px + (k & 1), cy = py + (k >> 1);
            if (ex * (16 * cy - s->Y[a]) - ey * (16 * cx - s->X[a]) >= least)
                some = 1;
        }
        if (!some)
            return 0;
    }
    return 1;
}

/* step 8 for one record of class cls (not outside); returns the pixels it writes */
static inline uint32_t receiver_twin_raster(const ReceiverTwinSetup* s, int cls, float* mask, uint32_t W)
{
    int32_t px, py;
    uint32_t written = 0, bits, held;
    memcpy(&bits, &s->d, 4);
    for (py = s->y0; py <= s->y1; py++)
        for (px = s->x0; px <= s->x1; px++)
            if (cls != RECEIVER_TWIN_DRAWN || receiver_twin_touched(s, px, py, RECEIVER_TWIN_MARGIN)) {
                float* at = mask + (size_t)py * W + px;
                memcpy(&held, at, 4);
                if (held > bits)
                    memcpy(at, &bits, 4);
                written++;
            }
    return written;
}

/* every word of a new mask: +inf */
static inline void receiver_twin_clear(float* mask, uint32_t W, uint32_t H)
{
    const uint32_t inf = 0x7F800000u;
    size_t i;
    for (i = 0; i < (size_t)W * H; i++)
        memcpy(mask + i, &inf, 4);
}

/* n records into `mask` (W x H, accumulated: receiver_twin_clear it for a new one): models[12 k], boxes[6 k] (the cull AABB of the
 * record's slot, already looked up). The counts are added to. */
static inline void receiver_twin_draw(const float* models, const float* boxes, uint32_t n, const float light[16], uint32_t W, uint32_t H, float* mask,
                                      ReceiverTwinCounts* counts)
{
    uint32_t k;
    ReceiverTwinSetup s;
    for (k = 0; k < n; k++) {
        const int cls = receiver_twin_setup(models + 12 * (size_t)k, boxes + 6 * (size_t)k, light, W, H, &s);
        (&counts->drawn)[cls]++;
        if (cls != RECEIVER_TWIN_OUTSIDE)
            receiver_twin_raster(&s, cls, mask, W);
    }
}

#endif
