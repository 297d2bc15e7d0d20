/* bounds_twin.h — TEST ONLY: plain-C99 restatement of the view-bounds rule of DESIGN.md §4 item 14 (gv_device_math.hpp bounds_key /
 * bounds_project over aabb_corners), the check gv_pool_view_bounds' kernels are compared against word for word. Compile with
 * -ffp-contract=off -fno-fast-math: every multiply that feeds an add is written as fmaf. One corner at a time, one record after the
 * other, comparisons on the key — none of the kernel's packing, lanes or partial rows. model / basis: 12 floats in float4x3 order
 * (c0.xyz c1.xyz c2.xyz c3.xyz); box: (min.xyz, max.xyz). */
#ifndef GV_BOUNDS_TWIN_H
#define GV_BOUNDS_TWIN_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

typedef struct BoundsTwin { /* GvViewBounds */
    float lo[3];
    uint32_t draw_count;
    float hi[3];
    uint32_t nan_records;
} BoundsTwin;

/* the order of the fold: -0 below +0, the infinities at the ends */
static inline uint32_t bounds_twin_key(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

/* row r of an affine 3x4 applied to (x, y, z, 1): fma(c0[r], x, fma(c1[r], y, fma(c2[r], z, c3[r]))) */
static inline float bounds_twin_row(const float m[12], int r, float x, float y, float z)
{
    return fmaf(m[r], x, fmaf(m[3 + r], y, fmaf(m[6 + r], z, m[9 + r])));
}

/* n records: models[12 k], boxes[6 k] (the box of the record's slot, already looked up). Returns the item's answer. */
static inline BoundsTwin bounds_twin(const float* models, const float* boxes, uint32_t n, const float basis[12])
{
    BoundsTwin out;
    uint32_t k;
    int r, c, have_lo[3] = {0, 0, 0}, have_hi[3] = {0, 0, 0};
    out.draw_count = n;
    out.nan_records = 0;
    for (r = 0; r < 3; r++) {
        out.lo[r] = INFINITY;
        out.hi[r] = -INFINITY;
    }
    for (k = 0; k < n; k++) {
        const float* m = models + 12 * (size_t)k;
        const float* box = boxes + 6 * (size_t)k;
        int nan = 0;
        for (c = 0; c < 8; c++) { /* bit0 -> x, bit1 -> y, bit2 -> z selects max */
            const float x = box[(c & 1) ? 3 : 0], y = box[(c & 2) ? 4 : 1], z = box[(c & 4) ? 5 : 2];
            const float px = bounds_twin_row(m, 0, x, y, z), py = bounds_twin_row(m, 1, x, y, z), pz = bounds_twin_row(m, 2, x, y, z);
            for (r = 0; r < 3; r++) {
                const float q = bounds_twin_row(basis, r, px, py, pz);
                if (q != q) {
                    nan = 1;
                    continue;
                }
                if (!have_lo[r] || bounds_twin_key(q) < bounds_twin_key(out.lo[r])) {
                    out.lo[r] = q;
                    have_lo[r] = 1;
                }
                if (!have_hi[r] || bounds_twin_key(q) > bounds_twin_key(out.hi[r])) {
                    out.hi[r] = q;
                    have_hi[r] = 1;
                }
            }
        }
        out.nan_records += (uint32_t)nan;
    }
    return out;
}

#endif
