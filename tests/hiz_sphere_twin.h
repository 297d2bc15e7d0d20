/* hiz_sphere_twin.h — TEST ONLY: plain-C99 restatement of hiz_sphere_occluded (garden_amd/csrc/gv_device.hpp), the occlusion
 * proof the sphere-stream cull takes from an entry's 16-byte sphere entry alone, and of the two values it is fed with (sphere_radius,
 * sphere_reach). Same operations in the same order: the kernel's verdicts are compared with this bit for bit, and the census
 * (tests/test_hiz_sphere_census.py) runs this over whole scenes against the oracle. Compile with -ffp-contract=off: every fused
 * multiply-add is written as fmaf, every other product and sum must stay unfused.
 * The pyramid is the oracle's (oracle/gv_oracle.h GvoHiz): level k >= 1 as (min, max) float pairs at mips + 2 * mip_offset[k]; an
 * RG16F pyramid holds its binary16 values as floats there, which is what the device decodes. */
#ifndef GV_HIZ_SPHERE_TWIN_H
#define GV_HIZ_SPHERE_TWIN_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define HIZ_SPHERE_TWIN_STEP 2u /* kHizSphereStep */

typedef struct {
    const float* mips;          /* (min, max) pairs, levels >= 1 */
    const uint64_t* mip_offset; /* in texels */
    uint32_t width, height, mip_count;
    uint32_t nested;
} HizSphereTwinPyramid;

/* NaN-propagating maximum (max_nan) */
static inline float hiz_sphere_twin_max_nan(float a, float b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }

/* sphere_radius: world = 12 floats in float4x3 order (c0.xyz c1.xyz c2.xyz c3.xyz), box = (min.xyz, max.xyz) */
static inline float hiz_sphere_twin_radius(const float world[12], const float box[6])
{
    const float ax = hiz_sphere_twin_max_nan(fabsf(box[0]), fabsf(box[3])), ay = hiz_sphere_twin_max_nan(fabsf(box[1]), fabsf(box[4])),
                az = hiz_sphere_twin_max_nan(fabsf(box[2]), fabsf(box[5]));
    const float n0 = fabsf(world[0]) + fabsf(world[1]) + fabsf(world[2]);
    const float n1 = fabsf(world[3]) + fabsf(world[4]) + fabsf(world[5]);
    const float n2 = fabsf(world[6]) + fabsf(world[7]) + fabsf(world[8]);
    return fmaf(n0, ax, fmaf(n1, ay, n2 * az));
}

/* sphere_reach */
static inline float hiz_sphere_twin_reach(float r, float tx, float ty, float tz)
{
    const float mag = hiz_sphere_twin_max_nan(hiz_sphere_twin_max_nan(fabsf(tx), fabsf(ty)), fabsf(tz)) + r;
    return fmaf(4e-5f, mag, r) + 0.01f;
}

static inline float hiz_sphere_twin_clamp01(float a) { return a > 0.0f ? (a < 1.0f ? a : 1.0f) : 0.0f; }

static inline uint32_t hiz_sphere_twin_axis_level(int i0, int i1)
{
    const int n = i1 - i0;
    uint32_t l;
    if (n <= 1)
        return 0u;
    l = 31u - (uint32_t)__builtin_clz((unsigned)n);
    return ((i1 >> l) - (i0 >> l)) <= 1 ? l : l + 1u;
}

/* hiz_sphere_occluded with the texels taken `step` levels above the smallest level at which the widened rect touches <= 2 x 2 of
 * them (the device: kHizSphereStep; other steps are for the census only): 1 = proven occluded, 0 = declined */
static inline int hiz_sphere_twin_at(const HizSphereTwinPyramid* hz, const float vp[16], float tx, float ty, float tz, float reach,
                                     uint32_t step)
{
    float cx, cy, cz, cw, ex, ey, ez, ew, wlo, whi, rlo, rhi, xlo, xhi, ylo, yhi, zhi, nx0, nx1, ny0, ny1, znear, probe;
    float umin, umax, vmin, vmax, t00, t10, t01, t11;
    int W, H, ix0, ix1, iy0, iy1, lw, lh, x0, x1, y0, y1;
    uint32_t level, cl;
    const float* texels;
    if (!hz->nested)
        return 0;
    cx = fmaf(vp[0], tx, fmaf(vp[4], ty, fmaf(vp[8], tz, vp[12])));
    cy = fmaf(vp[1], tx, fmaf(vp[5], ty, fmaf(vp[9], tz, vp[13])));
    cz = fmaf(vp[2], tx, fmaf(vp[6], ty, fmaf(vp[10], tz, vp[14])));
    cw = fmaf(vp[3], tx, fmaf(vp[7], ty, fmaf(vp[11], tz, vp[15])));
    ex = reach * (fabsf(vp[0]) + fabsf(vp[4]) + fabsf(vp[8]));
    ey = reach * (fabsf(vp[1]) + fabsf(vp[5]) + fabsf(vp[9]));
    ez = reach * (fabsf(vp[2]) + fabsf(vp[6]) + fabsf(vp[10]));
    ew = reach * (fabsf(vp[3]) + fabsf(vp[7]) + fabsf(vp[11]));
    wlo = cw - ew;
    whi = cw + ew;
    if (!(wlo > 0.0f))
        return 0;
    rlo = 1.0f / wlo;
    rhi = 1.0f / whi;
    xlo = cx - ex; xhi = cx + ex;
    ylo = cy - ey; yhi = cy + ey;
    zhi = cz + ez;
    nx0 = xlo * (xlo >= 0.0f ? rhi : rlo);
    nx1 = xhi * (xhi >= 0.0f ? rlo : rhi);
    ny0 = ylo * (ylo >= 0.0f ? rhi : rlo);
    ny1 = yhi * (yhi >= 0.0f ? rlo : rhi);
    znear = zhi * (zhi >= 0.0f ? rlo : rhi);
    probe = fabsf(nx0) + fabsf(nx1) + fabsf(ny0) + fabsf(ny1) + fabsf(znear) + whi;
    if (!(probe < INFINITY))
        return 0;
    znear = fmaf(fabsf(znear), 2e-6f, znear);
    W = (int)hz->width;
    H = (int)hz->height;
    umin = hiz_sphere_twin_clamp01(fmaf(nx0, 0.5f, 0.5f));
    umax = hiz_sphere_twin_clamp01(fmaf(nx1, 0.5f, 0.5f));
    vmin = hiz_sphere_twin_clamp01(fmaf(ny0, 0.5f, 0.5f));
    vmax = hiz_sphere_twin_clamp01(fmaf(ny1, 0.5f, 0.5f));
    ix0 = (int)(umin * (float)W) - 1; if (ix0 < 0) ix0 = 0;
    ix1 = (int)(umax * (float)W) + 1; if (ix1 > W - 1) ix1 = W - 1;
    iy0 = (int)(vmin * (float)H) - 1; if (iy0 < 0) iy0 = 0;
    iy1 = (int)(vmax * (float)H) + 1; if (iy1 > H - 1) iy1 = H - 1;
    level = hiz_sphere_twin_axis_level(ix0, ix1);
    cl = hiz_sphere_twin_axis_level(iy0, iy1);
    if (cl > level)
        level = cl;
    cl = level + step;
    if (cl > hz->mip_count - 1u)
        cl = hz->mip_count - 1u;
    if (cl < 2u)
        return 0;
    lw = (int)(hz->width >> cl); if (lw < 1) lw = 1;
    lh = (int)(hz->height >> cl); if (lh < 1) lh = 1;
    x0 = ix0 >> cl; if (x0 > lw - 1) x0 = lw - 1;
    x1 = ix1 >> cl; if (x1 > lw - 1) x1 = lw - 1;
    y0 = iy0 >> cl; if (y0 > lh - 1) y0 = lh - 1;
    y1 = iy1 >> cl; if (y1 > lh - 1) y1 = lh - 1;
    texels = hz->mips + 2u * (size_t)hz->mip_offset[cl];
    t00 = texels[2u * ((size_t)y0 * (size_t)lw + (size_t)x0)];
    t10 = texels[2u * ((size_t)y0 * (size_t)lw + (size_t)x1)];
    t01 = texels[2u * ((size_t)y1 * (size_t)lw + (size_t)x0)];
    t11 = texels[2u * ((size_t)y1 * (size_t)lw + (size_t)x1)];
    return (znear < t00) && (znear < t10) && (znear < t01) && (znear < t11);
}

static inline int hiz_sphere_twin(const HizSphereTwinPyramid* hz, const float vp[16], float tx, float ty, float tz, float reach)
{
    return hiz_sphere_twin_at(hz, vp, tx, ty, tz, reach, HIZ_SPHERE_TWIN_STEP);
}

/* the verdict of one sphere-stream entry hot = (pos.xyz, r) for a camera at cam: 0 for a dropped entry (r < 0) */
static inline int hiz_sphere_twin_entry(const HizSphereTwinPyramid* hz, const float vp[16], const float cam[3], const float hot[4])
{
    float tx, ty, tz;
    if (hot[3] < 0.0f)
        return 0;
    tx = hot[0] - cam[0];
    ty = hot[1] - cam[1];
    tz = hot[2] - cam[2];
    return hiz_sphere_twin(hz, vp, tx, ty, tz, hiz_sphere_twin_reach(hot[3], tx, ty, tz));
}

#endif
