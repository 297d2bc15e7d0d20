// gv_device.hpp — device-side helpers shared by the kernel files: stream loads / stores, the transform record and its
// parent-chain model (transform.hpp:197-214), the per-entity filter chain + frustum test of the cull
// (mesh.cpp:140-157, render/mesh.hpp:142-146) and the build-defined Hi-Z occlusion query.
#pragma once
#include "gv_kernels.hpp"

#include <algorithm>

#include "gv_device_math.hpp"
#include "gv_tile_order.hpp"

namespace gv {


// ------------------------------------------------------------------------------------------------
// shared device helpers
// ------------------------------------------------------------------------------------------------
// The mirror streams are read once per frame: nontemporal loads (no L2/MALL allocation priority) measured
// +20 % on this access pattern (round-1 probe tools/kbench.hip, in the history: 6.1 -> 7.1 TB/s). Ancestor re-reads use plain loads.
typedef float f32x4n __attribute__((ext_vector_type(4)));
typedef float f32x2n __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 stream_load(const float4* p)
{
    const f32x4n v = __builtin_nontemporal_load(reinterpret_cast<const f32x4n*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float2 stream_load(const float2* p)
{
    const f32x2n v = __builtin_nontemporal_load(reinterpret_cast<const f32x2n*>(p));
    return make_float2(v.x, v.y);
}
__device__ __forceinline__ uint32_t stream_load(const uint32_t* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void stream_store(float4* p, float4 v)
{
    __builtin_nontemporal_store(f32x4n{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4n*>(p));
}
__device__ __forceinline__ void stream_store(float* p, float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ uint32_t stream_load(const uint8_t* p) { return __builtin_nontemporal_load(p); }

// one transform entry: TRS + flag bits
struct XfRecord {
    float4 a, b;
    float2 c;
    uint32_t flags;
};
__device__ __forceinline__ XfRecord load_xf(const TransformMirror& xf, uint32_t s)
{
    XfRecord r;
    r.a = xf.ab[s].a;
    r.b = xf.ab[s].b;
    r.c = xf.c[s];
    r.flags = xf.flags[s];
    return r;
}
__device__ __forceinline__ XfRecord gather_xf(const TransformMirror& xf, uint32_t s, bool with_flags)
{
    XfRecord r;
    r.a = xf.ab[s].a;
    r.b = xf.ab[s].b;
    r.c = xf.c[s];
    r.flags = with_flags ? xf.flags[s] : 0u;
    return r;
}
__device__ __forceinline__ XfRecord stream_xf(const TransformMirror& xf, uint32_t s)  // the once-per-frame read
{
    XfRecord r;
    r.a = stream_load(&xf.ab[s].a);
    r.b = stream_load(&xf.ab[s].b);
    r.c = stream_load(&xf.c[s]);
    r.flags = stream_load(&xf.flags[s]);
    return r;
}
__device__ __forceinline__ Mat34 local_model(const XfRecord& r)
{
    return calc_model(r.a.x, r.a.y, r.a.z, r.b.x, r.b.y, r.b.z, r.b.w, r.a.w, r.c.x, r.c.y);
}

// A model as three float4 rows in float4x3 order (12 floats: c0.xyz, c1.xyz, c2.xyz, c3.xyz) — the layout of a record's bakedModel
// and of the resident world matrices — and back.
__device__ __forceinline__ void model_rows(const Mat34& m, float4& w0, float4& w1, float4& w2)
{
    w0 = make_float4(m.c0x, m.c0y, m.c0z, m.c1x);
    w1 = make_float4(m.c1y, m.c1z, m.c2x, m.c2y);
    w2 = make_float4(m.c2z, m.c3x, m.c3y, m.c3z);
}
__device__ __forceinline__ Mat34 rows_model(const float4 w0, const float4 w1, const float4 w2)
{
    Mat34 m;
    m.c0x = w0.x; m.c0y = w0.y; m.c0z = w0.z;
    m.c1x = w0.w; m.c1y = w1.x; m.c1z = w1.y;
    m.c2x = w1.z; m.c2y = w1.w; m.c2z = w2.x;
    m.c3x = w2.y; m.c3y = w2.z; m.c3z = w2.w;
    return m;
}

// transform.hpp:197-214: model = calcModel(self); while (parent) model = calcModel(parent) * model.
// `m` is the already-built self model of entry `s`; the parent stream is only touched when the pool has chains.
__device__ __forceinline__ Mat34 chain_model(const TransformMirror& xf, Mat34 m, uint32_t s, uint32_t flags)
{
    if (xf.max_depth != 0 && (flags & kXfWithAncestors)) {
        uint32_t p = xf.parent[s];
        for (uint32_t d = 0; d < xf.max_depth && p != kSlotNone; d++) {
            const XfRecord pr = load_xf(xf, p);
            m = mul_affine(local_model(pr), m);
            p = xf.parent[p];
        }
    }
    return m;
}

// Workgroup -> slot range is linear. An XCD-contiguous remap (each XCD's L2 owning one eighth of the slot
// range) was measured with flat and hierarchical scenes, random and Morton slot order: no effect (the streams
// have no inter-workgroup reuse and ancestor lines are shared through the Infinity Cache anyway).
__device__ __forceinline__ float hiz_min_texel(const HizDevice& hz, uint32_t level, uint32_t lw, uint32_t x, uint32_t y)
{
    if (level == 0)
        return hz.depth[(size_t)y * hz.width + x];
    if (level == 1 && hz.level1_virtual) {
        // Level 1 is the biggest level to write (half of all pyramid bytes) and the least read: with even sizes its
        // texel is just the 2x2 reduction of the depth image, in the build's own order (hiz.frag:29-33, MIN_DEPTH).
        const float2* row0 = reinterpret_cast<const float2*>(hz.depth + (size_t)(2 * y) * hz.width + 2 * x);
        const float2* row1 = reinterpret_cast<const float2*>(hz.depth + (size_t)(2 * y + 1) * hz.width + 2 * x);
        const float2 a = *row0, b = *row1;
        float m = a.x;
        m = a.y < m ? a.y : m;
        m = b.x < m ? b.x : m;
        m = b.y < m ? b.y : m;
        return hz.rg16f ? half_to_float(half_directed(m, false)) : m;  // what the stored texel would hold
    }
    const uint64_t at = hz.mip_offset[level] + (uint64_t)y * lw + x;
    if (hz.rg16f)  // uniform
        return half_to_float(reinterpret_cast<const uint32_t*>(hz.mips)[at] & 0xFFFFu);
    return hz.mips[at].x;
}
__device__ __forceinline__ float2 hiz_pair(const HizDevice& hz, uint64_t at)
{
    if (hz.rg16f)  // uniform
        return unpack_rg16f(reinterpret_cast<const uint32_t*>(hz.mips)[at]);
    return hz.mips[at];
}

__device__ __forceinline__ float clamp01(float a)
{
    return a > 0.0f ? (a < 1.0f ? a : 1.0f) : 0.0f;
}

constexpr uint32_t kHizCoarseStep = 4;  // early-accept level = query level + 4 (+3..+5 measured equal, +1/+2 slower)

// Build-defined occlusion query (SURVEY.md §8a-7'; the reference has none). Returns true if occluded.
__device__ __forceinline__ bool hiz_occluded(const HizDevice& hz, const float (&vp)[16], const Corners& c)
{
    float u[8], v[8], zc[8];
    bool bounded = true;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const v2f clx = pk_fma(splat(vp[0]), c.x[j], pk_fma(splat(vp[4]), c.y[j], pk_fma(splat(vp[8]), c.z[j], splat(vp[12]))));
        const v2f cly = pk_fma(splat(vp[1]), c.x[j], pk_fma(splat(vp[5]), c.y[j], pk_fma(splat(vp[9]), c.z[j], splat(vp[13]))));
        const v2f clz = pk_fma(splat(vp[2]), c.x[j], pk_fma(splat(vp[6]), c.y[j], pk_fma(splat(vp[10]), c.z[j], splat(vp[14]))));
        const v2f clw = pk_fma(splat(vp[3]), c.x[j], pk_fma(splat(vp[7]), c.y[j], pk_fma(splat(vp[11]), c.z[j], splat(vp[15]))));
        bounded = bounded && (clw.x > 0.0f) && (clw.y > 0.0f);
        // IEEE-correct division (-fhip-fp32-correctly-rounded-divide-sqrt), one per corner
        const v2f rcp = {1.0f / clw.x, 1.0f / clw.y};
        const v2f uu = pk_fma(clx * rcp, splat(0.5f), splat(0.5f));
        const v2f vv = pk_fma(cly * rcp, splat(0.5f), splat(0.5f));
        const v2f zz = clz * rcp;
        u[2 * j] = uu.x; u[2 * j + 1] = uu.y;
        v[2 * j] = vv.x; v[2 * j + 1] = vv.y;
        zc[2 * j] = zz.x; zc[2 * j + 1] = zz.y;
    }
    if (!bounded)
        return false;
    // IEEE minNum/maxNum reductions (v_min3_f32 / v_max3_f32), as the oracle's fminf/fmaxf
    const float umin0 = fminf(fminf(fminf(u[0], u[1]), fminf(u[2], u[3])), fminf(fminf(u[4], u[5]), fminf(u[6], u[7])));
    const float umax0 = fmaxf(fmaxf(fmaxf(u[0], u[1]), fmaxf(u[2], u[3])), fmaxf(fmaxf(u[4], u[5]), fmaxf(u[6], u[7])));
    const float vmin0 = fminf(fminf(fminf(v[0], v[1]), fminf(v[2], v[3])), fminf(fminf(v[4], v[5]), fminf(v[6], v[7])));
    const float vmax0 = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
    const float znear = fmaxf(fmaxf(fmaxf(zc[0], zc[1]), fmaxf(zc[2], zc[3])), fmaxf(fmaxf(zc[4], zc[5]), fmaxf(zc[6], zc[7])));
    float umin = umin0, umax = umax0, vmin = vmin0, vmax = vmax0;
    umin = clamp01(umin);
    umax = clamp01(umax);
    vmin = clamp01(vmin);
    vmax = clamp01(vmax);
    const int W = (int)hz.width, H = (int)hz.height;
    int ix0 = (int)(umin * (float)W), ix1 = (int)(umax * (float)W);
    int iy0 = (int)(vmin * (float)H), iy1 = (int)(vmax * (float)H);
    ix0 = min(ix0, W - 1);
    ix1 = min(ix1, W - 1);
    iy0 = min(iy0, H - 1);
    iy1 = min(iy1, H - 1);
    // Smallest level at which the pixel rect touches <= 2x2 texels. The oracle walks levels upward; per axis
    // the condition (i1 >> L) - (i0 >> L) <= 1 is monotone in L and first holds at floor(log2(n)) or one above
    // (n = i1 - i0 >= 2), so the level is max over the axes of that closed form.
    auto axis_level = [](int i0, int i1) -> uint32_t {
        const int n = i1 - i0;
        if (n <= 1)
            return 0u;
        const uint32_t l = 31u - (uint32_t)__clz(n);
        return ((i1 >> l) - (i0 >> l)) <= 1 ? l : l + 1u;
    };
    const uint32_t level = min(max(axis_level(ix0, ix1), axis_level(iy0, iy1)), hz.mip_count - 1u);
    // Exact early decisions from a coarse, cache-resident level (nested pyramids only; the answer is unchanged either
    // way). Its <= 4 texels cover a superset of the fine footprint, so their min is <= zFar and their max is >= every
    // fine texel, zFar included:
    //   zNear <  min(coarse)  =>  zNear < zFar   : occluded  — most occluded boxes end here,
    //   zNear >= max(coarse)  =>  zNear >= zFar  : visible   — boxes in front of everything around them end here,
    // and neither touches the 64 MB / 32 MB levels 0 / 1. (A NaN zNear fails both compares and takes the fine path.)
    if (hz.nested && level + kHizCoarseStep < hz.mip_count) {
        const uint32_t cl = level + kHizCoarseStep;  // >= 4: always a (min, max) level
        const int cw = max((int)(hz.width >> cl), 1), ch = max((int)(hz.height >> cl), 1);
        const int cx0 = min(ix0 >> cl, cw - 1), cx1 = min(ix1 >> cl, cw - 1);
        const int cy0 = min(iy0 >> cl, ch - 1), cy1 = min(iy1 >> cl, ch - 1);
        const uint64_t coarse = hz.mip_offset[cl];
        float2 t = hiz_pair(hz, coarse + (uint64_t)cy0 * cw + cx0);
        float cmin = t.x, cmax = t.y;
        if (cx1 != cx0) {
            t = hiz_pair(hz, coarse + (uint64_t)cy0 * cw + cx1);
            cmin = fminf(cmin, t.x);
            cmax = fmaxf(cmax, t.y);
        }
        if (cy1 != cy0) {
            t = hiz_pair(hz, coarse + (uint64_t)cy1 * cw + cx0);
            cmin = fminf(cmin, t.x);
            cmax = fmaxf(cmax, t.y);
            if (cx1 != cx0) {
                t = hiz_pair(hz, coarse + (uint64_t)cy1 * cw + cx1);
                cmin = fminf(cmin, t.x);
                cmax = fmaxf(cmax, t.y);
            }
        }
        if (znear < cmin)
            return true;
        if (znear >= cmax)
            return false;
    }
    const int lw = max((int)(hz.width >> level), 1), lh = max((int)(hz.height >> level), 1);
    const int tx0 = min(ix0 >> level, lw - 1), tx1 = min(ix1 >> level, lw - 1);
    const int ty0 = min(iy0 >> level, lh - 1), ty1 = min(iy1 >> level, lh - 1);
    float zfar = hiz_min_texel(hz, level, lw, tx0, ty0);
    float a = hiz_min_texel(hz, level, lw, tx1, ty0);
    zfar = a < zfar ? a : zfar;
    a = hiz_min_texel(hz, level, lw, tx0, ty1);
    zfar = a < zfar ? a : zfar;
    a = hiz_min_texel(hz, level, lw, tx1, ty1);
    zfar = a < zfar ? a : zfar;
    return znear < zfar;
}

// Occlusion proven from an entry's sphere alone (the sphere-stream cull, gv_cull.hip): true only when hiz_occluded would return
// true for the entity's corners, whatever its TRS and box are; false = not proven (the entry takes the exact path). (tx, ty, tz) is
// the camera-relative centre, reach = sphere_reach: the argument of block_window for ONE entity, its box the cube C of half-side
// reach around the centre.
//   * Every corner of the entity lies within r (L1 column norms, sphere_radius) of the centre in every coordinate; reach adds
//     0.01 + 4e-5 * magnitude to r, 30x the fp32 rounding of the corner generation (classify_sphere's slack), so C holds every
//     corner AS COMPUTED, with that much to spare.
//   * Each clip coordinate is affine in the point: over C it stays within c +- e, c its value at the centre and e = reach * (L1
//     norm of the row of vp). The three fmas of c and the product e round by <= 4 * 2^-24 of (row norm * magnitude); the spare
//     4e-5 * magnitude of reach, times the same row norm, is 160x that and covers the rounding of c, e, c +- e here and of
//     hiz_occluded's own clip coordinates. So every computed clw of the entity is >= wlo: wlo > 0 means hiz_occluded takes no
//     "cannot bound" exit, and a cube that reaches w <= 0 is never tested.
//   * With w in [wlo, whi], wlo > 0, a ratio p / w over C is largest at p's upper end over wlo (over whi when that end is
//     negative) and smallest at p's lower end the other way round: [nx0, nx1] x [ny0, ny1] holds every corner's x/w, y/w, and
//     znear0 >= every corner's z/w = zNear_e. The divisions and products round by 2^-23 relative: znear is widened by 2e-6
//     relative (16x), the pixel rect by one pixel each way (the u, v roundings are < 1e-3 pixel at 16 K pixels), so the rect R
//     contains the entity's R_e.
//   * The smallest level L at which R touches <= 2x2 texels is >= the entity's L_e (the condition is monotone in the rect), and so
//     is any level above it. In a NESTED pyramid every level-L_e texel that touches R_e lies inside a level-cl texel that touches
//     R, cl >= L, and a texel's min bounds everything under it (RG16F mins are rounded down): min over the <= 2x2 level-cl texels
//     <= zFar_e.
//   So znear < every one of those texels  =>  zNear_e <= znear < zFar_e: hiz_occluded returns true. A NaN texel, centre, reach or
//   any non-finite intermediate fails a comparison and declines. cl = L + kHizSphereStep: two levels up the texels come from
//   the cache-resident 2 MB of level 3 and above, never from the depth image, and still prove 95 % of what L itself would on the
//   walls image (census of tests/test_hiz_sphere_census.py: L 97.9 %, L + 2 95.5 %, L + 4 83.4 % of the occluded frustum
//   survivors; profiles/r12_hiz_sphere.md). tests/hiz_sphere_twin.h restates this in C, operation for operation.
constexpr uint32_t kHizSphereStep = 2;
// The query in two halves, so that a lane with several entries has the texel loads of all of them in flight together
// (cull_hot_kernel). hiz_sphere_query is straight-line code: a declined entry leaves with znear = NaN, which fails every
// comparison, and with texel indices that are in bounds like any other's (clamp01 maps a NaN to 0; the level and the coordinates
// are clamped to the pyramid). Both halves want hiz_sphere_usable(hz): then level mip_count - 1 >= 2 is a stored level.
struct HizSphereQuery {
    float znear;     // widened by its rounding allowance; NaN: declined
    uint32_t at[4];  // the <= 2x2 texels of level cl, as indices into HizDevice::mips (a repeated texel is repeated)
};
__device__ __forceinline__ bool hiz_sphere_usable(const HizDevice& hz)  // uniform
{
    return hz.nested && hz.mip_count > 2u;  // (a pyramid of one or two levels stores nothing a query could read)
}
__device__ __forceinline__ HizSphereQuery hiz_sphere_query(const HizDevice& hz, const float (&vp)[16], float tx, float ty, float tz, float reach)
{
    const float cx = fmaf(vp[0], tx, fmaf(vp[4], ty, fmaf(vp[8], tz, vp[12])));
    const float cy = fmaf(vp[1], tx, fmaf(vp[5], ty, fmaf(vp[9], tz, vp[13])));
    const float cz = fmaf(vp[2], tx, fmaf(vp[6], ty, fmaf(vp[10], tz, vp[14])));
    const float cw = fmaf(vp[3], tx, fmaf(vp[7], ty, fmaf(vp[11], tz, vp[15])));
    const float ex = reach * (fabsf(vp[0]) + fabsf(vp[4]) + fabsf(vp[8]));  // (the row norms are wave-uniform: scalar)
    const float ey = reach * (fabsf(vp[1]) + fabsf(vp[5]) + fabsf(vp[9]));
    const float ez = reach * (fabsf(vp[2]) + fabsf(vp[6]) + fabsf(vp[10]));
    const float ew = reach * (fabsf(vp[3]) + fabsf(vp[7]) + fabsf(vp[11]));
    const float wlo = cw - ew, whi = cw + ew;
    const float rlo = 1.0f / wlo, rhi = 1.0f / whi;  // IEEE divisions, as the twin's
    const float xlo = cx - ex, xhi = cx + ex, ylo = cy - ey, yhi = cy + ey, zhi = cz + ez;
    const float nx0 = xlo * (xlo >= 0.0f ? rhi : rlo), nx1 = xhi * (xhi >= 0.0f ? rlo : rhi);
    const float ny0 = ylo * (ylo >= 0.0f ? rhi : rlo), ny1 = yhi * (yhi >= 0.0f ? rlo : rhi);
    const float znear0 = zhi * (zhi >= 0.0f ? rlo : rhi);
    const float probe = fabsf(nx0) + fabsf(nx1) + fabsf(ny0) + fabsf(ny1) + fabsf(znear0) + whi;
    // the cube reaches w <= 0, or a NaN or an infinity anywhere above: declined
    const bool bounded = (wlo > 0.0f) & (probe < __builtin_huge_valf());
    HizSphereQuery q;
    q.znear = bounded ? fmaf(fabsf(znear0), 2e-6f, znear0) : __builtin_nanf("");
    const int W = (int)hz.width, H = (int)hz.height;
    const float umin = clamp01(fmaf(nx0, 0.5f, 0.5f)), umax = clamp01(fmaf(nx1, 0.5f, 0.5f));
    const float vmin = clamp01(fmaf(ny0, 0.5f, 0.5f)), vmax = clamp01(fmaf(ny1, 0.5f, 0.5f));
    const int ix0 = max((int)(umin * (float)W) - 1, 0), ix1 = min((int)(umax * (float)W) + 1, W - 1);
    const int iy0 = max((int)(vmin * (float)H) - 1, 0), iy1 = min((int)(vmax * (float)H) + 1, H - 1);
    auto axis_level = [](int i0, int i1) -> uint32_t {  // as in hiz_occluded
        const int n = i1 - i0;
        if (n <= 1)
            return 0u;
        const uint32_t l = 31u - (uint32_t)__clz(n);
        return ((i1 >> l) - (i0 >> l)) <= 1 ? l : l + 1u;
    };
    const uint32_t cl = min(max(axis_level(ix0, ix1), axis_level(iy0, iy1)) + kHizSphereStep, hz.mip_count - 1u);  // >= 2
    const int lw = max((int)(hz.width >> cl), 1), lh = max((int)(hz.height >> cl), 1);
    const int x0 = min(ix0 >> cl, lw - 1), x1 = min(ix1 >> cl, lw - 1);
    const int y0 = min(iy0 >> cl, lh - 1), y1 = min(iy1 >> cl, lh - 1);
    // 32-bit texel indices: the levels >= 1 of a pyramid hold a third of its depth image's texels, 2^32 are out of reach
    const uint32_t first = (uint32_t)hz.mip_offset[cl];
    q.at[0] = first + (uint32_t)(y0 * lw + x0);
    q.at[1] = first + (uint32_t)(y0 * lw + x1);
    q.at[2] = first + (uint32_t)(y1 * lw + x0);
    q.at[3] = first + (uint32_t)(y1 * lw + x1);
    return q;
}
__device__ __forceinline__ float hiz_stored_min(const HizDevice& hz, uint32_t at)  // a stored texel's min (levels >= 2; >= 1 when level 1 is stored)
{
    // one load either way: the texel's first 32-bit word is its fp32 min, or its binary16 (min, max) pair
    const uint32_t word = reinterpret_cast<const uint32_t*>(hz.mips)[hz.rg16f ? at : 2u * at];
    return hz.rg16f ? half_to_float(word & 0xFFFFu) : __uint_as_float(word);
}
// four loads whatever the rect touches: no branch between them
__device__ __forceinline__ void hiz_sphere_fetch(const HizDevice& hz, const HizSphereQuery& q, float (&t)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++)
        t[j] = hiz_stored_min(hz, q.at[j]);
}
__device__ __forceinline__ bool hiz_sphere_proven(const HizSphereQuery& q, const float (&t)[4])
{
    return (q.znear < t[0]) & (q.znear < t[1]) & (q.znear < t[2]) & (q.znear < t[3]);  // (a NaN texel fails its comparison)
}
__device__ __forceinline__ bool hiz_sphere_occluded(const HizDevice& hz, const float (&vp)[16], float tx, float ty, float tz, float reach)
{
    if (!hiz_sphere_usable(hz))
        return false;
    const HizSphereQuery q = hiz_sphere_query(hz, vp, tx, ty, tz, reach);
    float t[4];
    hiz_sphere_fetch(hz, q, t);
    return hiz_sphere_proven(q, t);
}

// ------------------------------------------------------------------------------------------------
// K1: cull — one lane per mesh slot
// ------------------------------------------------------------------------------------------------
// Workgroups are handed out round-robin over the 8 XCDs, so with the identity mapping every XCD (own L2, own TLBs)
// touches every 8th 256-entry tile of each stream. With run = R > 0, XCD x takes R consecutive tiles at a time —
// tiles (8q + x)R .. (8q + x + 1)R - 1 for its q-th run — so it streams contiguous stretches (R * 8 KB of the
// 32-byte transform stream), while runs still alternate between the XCDs often enough that the expensive part of
// the pool (the entries inside the frustum are contiguous in the spatial order) stays spread over all of them.
// Measured at 10 M entities, same box A/B: frustum-only cull 110-112 -> 102-104 us (R = 32) -> 99 us (R = 256); the
// Hi-Z variant does not move (R = 32) or loses (R = 256: +4 us; one run per XCD: 134-140 us, the queries pile up on
// two XCDs), the block-bounds variant loses (78 -> 82 -> 89 us), the fused sweep + cull is flat: only the
// frustum-only scan uses it (profiles/r01b_kbench.txt).
// A Hi-Z view keeps the identity. In the mirror's spatial order its launch runs as two phases, one after the other: the
// frustum's entries (sphere queries, exact walks: VALU and dependent loads) all lie in the first half of the dispatch
// order at the bench camera, and the rest is a bare 16-byte stream. Mixing the two over the whole dispatch, so that they
// overlap, was measured and is slower, the more so the coarser the stripes (sphere-stream cull at 10 M, 63 us: 64 stripes
// 90 us, 256 stripes 87 us, 1024 stripes 75 us, a modular stride 76 us; the same at 1 M and 2 M, on a harder depth image
// and with the camera turned round), with the same FETCH_SIZE: the heavy workgroups first and the light ones last is
// already the order with the shortest tail, and neighbours in the order share what they look up. What the two phases do
// respond to is the super-tile: hot_tiles_per_workgroup_hiz (profiles/r33_cull_order.md).
// (the mapping itself and its grid size: gv_tile_order.hpp)

struct CullArgs {
    MeshMirror mesh;
    TransformMirror xf;
    HizDevice hiz;
    ViewParams view;
    ViewBuffers out;
    uint32_t nblocks;
    uint32_t xcd_run;    // tile_of_workgroup() (gv_tile_order.hpp); 0 = workgroup b takes tile b
};

// The filter chain's verdict on one mesh entry: mesh.cpp:140-142 skips free slots and disabled meshes (`candidate`) and
// all(size <= 0) boxes, mesh.cpp:150 inactive transforms (transform.hpp:110).
__device__ __forceinline__ bool mesh_entry_dropped(bool candidate, const float4& a, const float2& b, uint32_t xf_flags)
{
    const bool empty = (a.w - a.x <= 0.0f) && (b.x - a.y <= 0.0f) && (b.y - a.z <= 0.0f);
    return !candidate || empty || !(xf_flags & kXfActive);
}

// One mesh entry through the reference's filter chain (mesh.cpp:140-157): candidate / empty-AABB / transform /
// isActive checks, parent-chain model, camera translate, 8 corners. Returns false when the entry is filtered out;
// otherwise `m` holds the camera-relative model (bakedModel) and `c` its corners. Nothing here depends on the
// frustum, so shadow passes that share cameraPosition with the main pass (mesh.cpp:809-843) share this work.
// MAP (MeshMapping) only changes which streams are read and when; the result is the same for any mapping.
// the mesh's model-space AABB (render/mesh.hpp:54) as it sits in the mirror: a = (min.xyz, max.x), b = (max.y, max.z)
template <uint32_t MAP>
__device__ __forceinline__ bool prepare_model(const MeshMirror& mesh, const TransformMirror& xf, const float (&cam)[3],
                                              uint32_t i, Mat34& m, float4& ma, float2& mb)
{
    ma = stream_load(&mesh.a[i]);
    mb = stream_load(&mesh.b[i]);
    uint32_t slot = i;
    bool candidate = true;  // kMapExact: non-candidates carry an empty box and fall out below
    XfRecord r = {};
    if (MAP == kMapGeneral) {
        const uint32_t link = stream_load(&mesh.link[i]);
        slot = link & kSlotMask;
        candidate = (link & kMeshCandidate) && slot != kSlotNone;
        if (candidate)
            r = load_xf(xf, slot);
    } else {
        // the transform loads are issued beside the mesh loads instead of one HBM round trip later
        const bool own = i < xf.count;
        if (own) {
            if (MAP == kMapExact && xf.max_depth == 0) {
                // flat + exactly paired: only the active bit matters (no chain, so modelWithAncestors is moot) and
                // the 64 bits of this wave sit in one word
                r.a = stream_load(&xf.ab[i].a);
                r.b = stream_load(&xf.ab[i].b);
                r.c = stream_load(&xf.c[i]);
                r.flags = (uint32_t)((xf.active_bits[i >> 6] >> (i & 63u)) & 1ull) * kXfActive;
            } else {
                r = stream_xf(xf, i);
            }
        }
        if (MAP == kMapSpeculate) {
            const uint32_t link = stream_load(&mesh.link[i]);
            slot = link & kSlotMask;
            candidate = (link & kMeshCandidate) && slot != kSlotNone;
            if (candidate && !(own && slot == i))
                r = load_xf(xf, slot);  // mis-speculated: this entry maps elsewhere
        } else {
            candidate = own;
        }
    }
    if (mesh_entry_dropped(candidate, ma, mb, r.flags))
        return false;
    const Mat34 world = chain_model(xf, local_model(r), slot, r.flags);
    // math::translate(-cameraPosition, model)  transform.hpp:211,213
    m = translated(world, cam[0], cam[1], cam[2]);
    return true;
}

__device__ __forceinline__ void aabb_corners(const Mat34& m, const float4 a, const float2 b, Corners& c)
{
    aabb_corners(m, a.x, a.y, a.z, a.w, b.x, b.y, c);
}

// Sphere pre-test for the default predicate: decides most entries without generating a corner, and agrees with the
// exact 8-corner test whenever it decides. Every corner M*(x,y,z) + t lies within
//   r = |c0|_1 ax + |c1|_1 ay + |c2|_1 az   (a = max(|min|, |max|) per axis; L1 column norms bound the L2 norms)
// of the translation t. With d = n.t + w for a unit-normal plane:
//   d < -(r + slack)  =>  every corner's COMPUTED distance is < 0          -> behind this plane, as the exact test says
//   d >  (r + slack)  =>  every corner's computed distance is > 0          -> this plane cannot reject
// where slack covers the fp32 rounding of both evaluations: <= ~20 roundings of relative size 2^-24 on magnitudes
// <= |t|_inf + r + |w| (corner generation, the three fmas of a distance; both use the same matrix bits, so the chain
// depth does not enter), i.e. <= 1.2e-6 * magnitude; the slack is 0.01 + 4e-5 * magnitude, 30x that. Anything else
// — a plane within the band, non-finite values (every comparison false) — is "undecided" and takes the exact test.
// At 10 M entities 0.2-0.5 % of the entries are undecided; 230 -> ~170 VALU instructions per wave with Hi-Z.
enum : uint32_t { kSphereOutside = 0, kSphereInside = 1, kSphereUndecided = 2 };
// r alone: depends on the model's columns c0..c2 and the box, not on the camera (the sphere stream stores it; the one copy of it)
__device__ __forceinline__ float sphere_radius(const Mat34& m, const float4 a, const float2 b)
{
    // NaN-propagating maxima: a NaN anywhere must reach the comparisons (fmaxf would drop it and decide for the exact test)
    const float ax = max_nan(fabsf(a.x), fabsf(a.w)), ay = max_nan(fabsf(a.y), fabsf(b.x)), az = max_nan(fabsf(a.z), fabsf(b.y));
    return fmaf(fabsf(m.c0x) + fabsf(m.c0y) + fabsf(m.c0z), ax,
                fmaf(fabsf(m.c1x) + fabsf(m.c1y) + fabsf(m.c1z), ay, (fabsf(m.c2x) + fabsf(m.c2y) + fabsf(m.c2z)) * az));
}
// r + the magnitude-proportional part of the slack, with (tx, ty, tz) the camera-relative translation c3
__device__ __forceinline__ float sphere_reach(float r, float tx, float ty, float tz)
{
    const float mag = max_nan(max_nan(fabsf(tx), fabsf(ty)), fabsf(tz)) + r;
    return fmaf(4e-5f, mag, r) + 0.01f;
}
// (view independent: shadow passes that share the camera share it)
__device__ __forceinline__ float sphere_reach(const Mat34& m, const float4 a, const float2 b)
{
    return sphere_reach(sphere_radius(m, a, b), m.c3x, m.c3y, m.c3z);
}
__device__ __forceinline__ uint32_t classify_sphere(float tx, float ty, float tz, float reach, const float (&planes)[6][4], uint32_t plane_count)
{
    bool outside = false, decided = true;
#pragma unroll
    for (uint32_t p = 0; p < 6; p++)
        if (p < plane_count) {  // wave-uniform: the coefficients stay in SGPRs
            const float bound = fmaf(4e-5f, fabsf(planes[p][3]), reach);
            const float d = fmaf(planes[p][0], tx, fmaf(planes[p][1], ty, fmaf(planes[p][2], tz, planes[p][3])));
            outside = outside | (d < -bound);  // no short circuit: straight-line code, the masks live in SGPR pairs
            decided = decided & ((d > bound) | (d < -bound));
        }
    return outside ? kSphereOutside : (decided ? kSphereInside : kSphereUndecided);
}
__device__ __forceinline__ uint32_t classify_sphere(const Mat34& m, float reach, const float (&planes)[6][4], uint32_t plane_count)
{
    return classify_sphere(m.c3x, m.c3y, m.c3z, reach, planes, plane_count);
}
__device__ __forceinline__ uint32_t classify_sphere(const Mat34& m, const float4 a, const float2 b, const float (&planes)[6][4],
                                                    uint32_t plane_count)
{
    return classify_sphere(m, sphere_reach(m, a, b), planes, plane_count);
}

// The sphere-stream entry of mirror entry i of a flat, exactly paired pool (MeshMirror::hot): the filter chain and model of
// prepare_model with a zero camera — translated(world, 0, 0, 0) leaves c3 = pos bit for bit, and the cull subtracts the camera
// from it with the same operation translated() uses — and r from sphere_radius. A dropped entry gets r = kHotDropped.
__device__ __forceinline__ float4 hot_entry(const MeshMirror& mesh, const TransformMirror& xf, uint32_t i)
{
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    Mat34 m;
    float4 a;
    float2 b;
    if (!prepare_model<kMapExact>(mesh, xf, zero, i, m, a, b))
        return make_float4(0.0f, 0.0f, 0.0f, kHotDropped);
    return make_float4(m.c3x, m.c3y, m.c3z, sphere_radius(m, a, b));
}

// default getReadyMeshesAsync predicate (render/mesh.hpp:142-146). Fully unrolled with a wave-uniform guard so
// the plane coefficients stay in SGPRs (a runtime-indexed kernarg array would be copied to LDS/scratch).
__device__ __forceinline__ bool behind_frustum(const Corners& c, const float (&planes)[6][4], uint32_t plane_count)
{
    bool behind = false;
#pragma unroll
    for (uint32_t p = 0; p < 6; p++)
        if (p < plane_count)
            behind = behind || all_behind_plane(c, planes[p][0], planes[p][1], planes[p][2], planes[p][3]);
    return behind;
}

// The default predicate's frustum decision for one view, given the sphere class `where` of the camera-relative model m with
// box (a, b): the exact 8-corner test settles what the sphere could not (near a plane, or non-finite; rare, skipped wave-wide
// otherwise). The corners are left in `c` whenever they were needed — undecided, or inside with HIZ (the caller's Hi-Z query of
// the survivors reads them).
template <bool HIZ>
__device__ __forceinline__ bool settle(uint32_t where, const Mat34& m, const float4 a, const float2 b, const float (&planes)[6][4],
                                       uint32_t plane_count, Corners& c)
{
    bool visible = where == kSphereInside;
    if (where == kSphereUndecided) {
        aabb_corners(m, a, b, c);
        visible = !behind_frustum(c, planes, plane_count);
    } else if (HIZ && visible) {
        aabb_corners(m, a, b, c);
    }
    return visible;
}
// The same decision for one of several views of an entity: `have_corners` says the corners are in `c` already, so that they are
// generated once, by the first view that needs them; `hiz`: this view runs the Hi-Z query.
__device__ __forceinline__ bool settle(uint32_t where, bool hiz, const Mat34& m, const float4 a, const float2 b,
                                       const float (&planes)[6][4], uint32_t plane_count, Corners& c, bool& have_corners)
{
    bool visible = where == kSphereInside;
    if (where == kSphereUndecided || (hiz && visible)) {
        if (!have_corners) {
            aabb_corners(m, a, b, c);
            have_corners = true;
        }
        if (where == kSphereUndecided)
            visible = !behind_frustum(c, planes, plane_count);
    }
    return visible;
}

// ------------------------------------------------------------------------------------------------
// records (mesh.cpp:169-173)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float record_distance(const ViewParams& view, const Mat34& m)
{
    const float tx = m.c3x + view.cam_offset[0];
    const float ty = m.c3y + view.cam_offset[1];
    const float tz = m.c3z + view.cam_offset[2];
    return view.distance_2d ? m.c3z + 1.0f : fmaf(tz, tz, fmaf(ty, ty, tx * tx));
}
// The record of a visible entry at output `rank`: pool slot and distance go straight out, the 48-byte model is staged at `row`
// (three float4 in LDS) for copy_rows.
__device__ __forceinline__ void put_record(const ViewParams& view, const ViewBuffers& out, size_t rank, uint32_t slot, const Mat34& m,
                                           float4* row)
{
    out.visible_idx[rank] = slot;  // componentOffset = slot * componentSize  mesh.cpp:170
    out.distance_sq[rank] = record_distance(view, m);
    model_rows(m, row[0], row[1], row[2]);
}
// ... and a round's staged models leave as whole rows: thread k of the 256 stores float4 k, k + 256, k + 512 ... of `quads`.
__device__ __forceinline__ void copy_rows(const float4* stage, float4* dst, uint32_t quads)
{
    for (uint32_t q = threadIdx.x; q < quads; q += 256)
        dst[q] = stage[q];
}

// ---- shared by the instance and command emissions (gv_instance.hip, gv_commands.hip): 256-lane workgroups over several views ----
// this workgroup's view: the last one whose workgroups (chunks) begin at or in front of it
__device__ __forceinline__ uint32_t view_of_block(const uint32_t (&first)[kMaxInstanceViews + 1], uint32_t views, uint32_t block)
{
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 1; k < kMaxInstanceViews; k++)
        if (k < views && block >= first[k])
            v = k;
    return v;
}

// 16-byte slot of column c of the workgroup's instance i in the stage: rotated by i / 4 so that the 16 lanes of a store group
// (4 instances x 4 columns on the way out, 16 instances x 1 column on the way in) cover the 16 slots of a bank row
// (instance_kernel's mvp; the rows and the prev_mvp of gv_previous.hip)
__device__ __forceinline__ uint32_t stage_slot(uint32_t i, uint32_t c) { return i * 4u + ((c + (i >> 2)) & 3u); }

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d)
            x += y;
    }
    return x;
}

// The tail of a chunk scan: `part` holds the 64 (round, wave) totals of a 256-lane workgroup; wave 0 scans them into the totals in
// front of each, in place. Two barriers. Returns the chunk's sum.
__device__ __forceinline__ uint32_t chunk_scan_tail(uint32_t* part, uint32_t lane, uint32_t wave)
{
    __shared__ uint32_t chunk_sum;
    __syncthreads();
    if (wave == 0) {
        const uint32_t own = part[lane], upto = wave_inclusive_scan(own, lane);
        part[lane] = upto - own;
        if (lane == 63u)
            chunk_sum = upto;
    }
    __syncthreads();
    return chunk_sum;
}

// sum of t[lo, hi) by the whole workgroup (every lane gets it); scratch: one word per wave
__device__ __forceinline__ uint32_t block_sum_of(const uint32_t* t, uint32_t lo, uint32_t hi, uint32_t* scratch)
{
    uint32_t x = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kInstanceBlock)
        x += t[i];
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1)
        x += __shfl_xor(x, d, 64);
    __syncthreads();  // (scratch may still be read from the call before)
    if ((threadIdx.x & 63u) == 0)
        scratch[threadIdx.x >> 6] = x;
    __syncthreads();
    return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

// ---- shared by the radix sorts (gv_sort.hip, gv_group.hip) ----
// lanes of the wave whose `digit` equals this lane's (among `valid` lanes): 8 ballots
__device__ __forceinline__ unsigned long long match_digit(uint32_t digit, bool valid)
{
    // per bit: t = 0 / ~0 from the lane's bit, m = the lanes whose bit is set; the lanes that agree with this one are
    // ~(m ^ t) — six VALU operations per bit (sign-extending bit extract, compare, two xnor, two and) where the select form
    // of the same thing compiled to nine
    const unsigned long long all = __ballot(valid);
    uint32_t lo = (uint32_t)all, hi = (uint32_t)(all >> 32);
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
        const uint32_t t = (uint32_t)((int32_t)(digit << (31u - b)) >> 31);
        const unsigned long long m = __ballot(t != 0u);
        lo &= ~((uint32_t)m ^ t);
        hi &= ~((uint32_t)(m >> 32) ^ t);
    }
    return ((unsigned long long)hi << 32) | lo;
}

// LDS operations of one wave execute in issue order; the fences keep the compiler from reordering them
__device__ __forceinline__ void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace gv
