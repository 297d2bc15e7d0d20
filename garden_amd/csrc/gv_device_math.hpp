// gv_device_math.hpp — gfx950 device-side arithmetic of the visibility pass.
//
// The reference's math library (cfnptr/math) is an empty submodule in the checkout, so the
// operation order is fixed here and in DESIGN.md §4 "Canonical arithmetic": every multiply that feeds
// an add is an explicit fma, the 4x4 product is a k = 0..3 fma chain from +0 (the order a
// v_mfma_f32_4x4x1_16b_f32 chain with a zero C operand produces), and nothing uses rcp/rsq
// approximations. Compile with -ffp-contract=off -fno-fast-math.
//
// The cull kernel is VALU-issue-bound when written with scalar v_fma_f32 (one wave64 instruction per
// ~4 cycles per SIMD, profiles/r01a_*), so the corner / plane / product arithmetic is written on
// 2-wide vectors: hipcc lowers __builtin_elementwise_fma on float2 to v_pk_fma_f32 (two IEEE fmas per
// lane per instruction, SGPR operands broadcast through op_sel). Each element sees exactly the scalar
// sequence of the oracle, so the bits do not change.
//
// Call sites being replaced (reference paths):
//   math::calcModel        include/garden/system/transform.hpp:199,207,224
//   f32x4x4 operator*      include/garden/system/transform.hpp:209
//   math::translate        include/garden/system/transform.hpp:211,213
//   isBehindFrustum        include/garden/system/render/mesh.hpp:145
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gv {

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f splat(float a) { return v2f{a, a}; }
// NaN-propagating maximum (v_maximum3_f32): "all d < 0" == "maximum(d...) < 0" including the NaN case
// (a NaN distance makes the comparison false, exactly like the oracle's !(d < 0)).
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }

// Affine 3x4 part of a column-major f32x4x4 whose bottom row is (0,0,0,1): columns c0..c3, rows x,y,z.
struct Mat34 {
    float c0x, c0y, c0z;
    float c1x, c1y, c1z;
    float c2x, c2y, c2z;
    float c3x, c3y, c3z;
};

// T * R * S from position, unit quaternion (xyzw) and scale.
__device__ __forceinline__ Mat34 calc_model(float px, float py, float pz, float qx, float qy, float qz,
                                            float qw, float sx, float sy, float sz)
{
    const float x2 = qx + qx, y2 = qy + qy, z2 = qz + qz;
    const float zz = qz * z2, yy = qy * y2;
    const float wx = qw * x2, wy = qw * y2, wz = qw * z2;
    const float r00 = 1.0f - fmaf(qy, y2, zz);
    const float r11 = 1.0f - fmaf(qx, x2, zz);
    const float r22 = 1.0f - fmaf(qx, x2, yy);
    // (r10, r01) = fma(x, y2, (+wz, -wz)) etc.: one packed fma per off-diagonal pair
    const v2f p_xy = pk_fma(splat(qx), splat(y2), v2f{wz, -wz});
    const v2f p_xz = pk_fma(splat(qx), splat(z2), v2f{-wy, wy});
    const v2f p_yz = pk_fma(splat(qy), splat(z2), v2f{wx, -wx});
    const float r10 = p_xy.x, r01 = p_xy.y;
    const float r20 = p_xz.x, r02 = p_xz.y;
    const float r21 = p_yz.x, r12 = p_yz.y;
    Mat34 m;
    m.c0x = r00 * sx; m.c0y = r10 * sx; m.c0z = r20 * sx;
    m.c1x = r01 * sy; m.c1y = r11 * sy; m.c1z = r21 * sy;
    m.c2x = r02 * sz; m.c2y = r12 * sz; m.c2z = r22 * sz;
    m.c3x = px; m.c3y = py; m.c3z = pz;
    return m;
}

// One output column of a * b, rows x,y as a packed pair and row z scalar: per element the fma chain
// over k = 0..3 from +0; b3 is the bottom-row element of b's column (0 for c0..c2, 1 for c3).
__device__ __forceinline__ void mul_column(const Mat34& a, float b0, float b1, float b2, float b3, float& ox, float& oy,
                                           float& oz)
{
    v2f acc = pk_fma(v2f{a.c0x, a.c0y}, splat(b0), splat(0.0f));
    acc = pk_fma(v2f{a.c1x, a.c1y}, splat(b1), acc);
    acc = pk_fma(v2f{a.c2x, a.c2y}, splat(b2), acc);
    acc = pk_fma(v2f{a.c3x, a.c3y}, splat(b3), acc);
    float z = fmaf(a.c0z, b0, 0.0f);
    z = fmaf(a.c1z, b1, z);
    z = fmaf(a.c2z, b2, z);
    z = fmaf(a.c3z, b3, z);
    ox = acc.x;
    oy = acc.y;
    oz = z;
}

// parentModel * model, rows 0..2 (row 3 of both operands is exactly (0,0,0,1) and stays so).
__device__ __forceinline__ Mat34 mul_affine(const Mat34& a, const Mat34& b)
{
    Mat34 r;
    mul_column(a, b.c0x, b.c0y, b.c0z, 0.0f, r.c0x, r.c0y, r.c0z);
    mul_column(a, b.c1x, b.c1y, b.c1z, 0.0f, r.c1x, r.c1y, r.c1z);
    mul_column(a, b.c2x, b.c2y, b.c2z, 0.0f, r.c2x, r.c2y, r.c2z);
    mul_column(a, b.c3x, b.c3y, b.c3z, 1.0f, r.c3x, r.c3y, r.c3z);
    return r;
}

// math::translate(-cameraPosition, model): c3.xyz - cam (transform.hpp:211,213). Returns a fresh value so the
// matrix never lives in memory (in-place field updates made LLVM keep c3 in scratch/LDS).
__device__ __forceinline__ Mat34 translated(const Mat34& a, float cx, float cy, float cz)
{
    Mat34 r;
    r.c0x = a.c0x; r.c0y = a.c0y; r.c0z = a.c0z;
    r.c1x = a.c1x; r.c1y = a.c1y; r.c1z = a.c1z;
    r.c2x = a.c2x; r.c2y = a.c2y; r.c2z = a.c2z;
    r.c3x = a.c3x - cx;
    r.c3y = a.c3y - cy;
    r.c3z = a.c3z - cz;
    return r;
}

// The 8 local corners (bit0 -> x, bit1 -> y, bit2 -> z selects max) through the model, as 4 packed pairs
// per coordinate: pair j holds corners (2j, 2j+1), i.e. (x = min, x = max) for one (y, z) choice.
// Per row: t_z = fma(c2, z, c3); t_yz = fma(c1, y, t_z); p = fma(c0, x, t_yz) — the same bits as
// evaluating each corner on its own.
struct Corners {
    v2f x[4], y[4], z[4];
};
__device__ __forceinline__ void corner_row(float c0, float c1, float c2, float c3, v2f xs, v2f ys, v2f zs, v2f (&out)[4])
{
    const v2f tz = pk_fma(splat(c2), zs, splat(c3));          // (z = min, z = max)
    const v2f ty0 = pk_fma(splat(c1), ys, splat(tz.x));        // z = min: (y = min, y = max)
    const v2f ty1 = pk_fma(splat(c1), ys, splat(tz.y));        // z = max
    out[0] = pk_fma(splat(c0), xs, splat(ty0.x));              // corners 0,1: y min, z min
    out[1] = pk_fma(splat(c0), xs, splat(ty0.y));              // corners 2,3: y max, z min
    out[2] = pk_fma(splat(c0), xs, splat(ty1.x));              // corners 4,5: y min, z max
    out[3] = pk_fma(splat(c0), xs, splat(ty1.y));              // corners 6,7: y max, z max
}
__device__ __forceinline__ void aabb_corners(const Mat34& m, float mnx, float mny, float mnz, float mxx, float mxy,
                                             float mxz, Corners& c)
{
    const v2f xs = {mnx, mxx}, ys = {mny, mxy}, zs = {mnz, mxz};
    corner_row(m.c0x, m.c1x, m.c2x, m.c3x, xs, ys, zs, c.x);
    corner_row(m.c0y, m.c1y, m.c2y, m.c3y, xs, ys, zs, c.y);
    corner_row(m.c0z, m.c1z, m.c2z, m.c3z, xs, ys, zs, c.z);
}

// isBehindFrustum for one plane: all 8 signed distances d = fma(nx,px, fma(ny,py, fma(nz,pz, nw))) < 0.
__device__ __forceinline__ bool all_behind_plane(const Corners& c, float nx, float ny, float nz, float nw)
{
    v2f d[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
        d[j] = pk_fma(splat(nx), c.x[j], pk_fma(splat(ny), c.y[j], pk_fma(splat(nz), c.z[j], splat(nw))));
    const float m = max_nan(max_nan(max_nan(d[0].x, d[0].y), max_nan(d[1].x, d[1].y)),
                            max_nan(max_nan(d[2].x, d[2].y), max_nan(d[3].x, d[3].y)));
    return m < 0.0f;
}

// RG16F pyramid texels (GV_CONFIG_HIZ_RG16F; HizRenderSystem::bufferFormat, render/hiz.hpp:41): binary16 with the min rounded
// toward -inf and the max toward +inf, so a stored pair still bounds every depth it covers. Same function as the oracle's
// gvo_half_directed (checked against every binary16 value; tests/test_gpu_cull.py compares the two on every half and its
// float neighbours). NaN stays NaN (quiet), +-0 keep their sign, overflow goes to +-inf or +-65504 by direction.
__device__ __forceinline__ uint32_t half_directed(float f, bool up)
{
    // nearest-even by the hardware conversion (v_cvt_f16_f32; subnormal halfs included), then one step in the wanted
    // direction when nearest went the other way. A step is +-1 on the encoding: away from zero when the direction grows the
    // magnitude (0x7BFF + 1 = inf), toward zero otherwise (inf - 1 = 65504; -0 steps to the smallest negative half).
    const uint32_t sign = __float_as_uint(f) >> 31;
    if (f != f)
        return (sign << 15) | 0x7E00u;
    uint32_t h = (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)f);
    const float back = (float)__builtin_bit_cast(_Float16, (unsigned short)h);
    const bool grow = up != (sign != 0u);
    if (up ? back < f : back > f)
        h = grow ? h + 1u : h - 1u;
    return h;
}
// exact (binary16 is a subset of binary32; subnormals included: v_cvt_f32_f16 with the kernels' default denormal mode)
__device__ __forceinline__ float half_to_float(uint32_t half_bits)
{
    return (float)__builtin_bit_cast(_Float16, (unsigned short)half_bits);
}
// (min, max) -> one RG16F texel (min in the low half) and back
__device__ __forceinline__ uint32_t pack_rg16f(float2 mm)
{
    return half_directed(mm.x, false) | (half_directed(mm.y, true) << 16);
}
__device__ __forceinline__ float2 unpack_rg16f(uint32_t texel)
{
    return make_float2(half_to_float(texel & 0xFFFFu), half_to_float(texel >> 16));
}

// ------------------------------------------------------------------------------------------------
// picking: inverse4x4, Ray, raycast2 and isIntersected of the editor's selector
// (editor/system/render/mesh-selector.cpp:102-107) for an affine model [A | t]
// ------------------------------------------------------------------------------------------------
// A^-1 = adj(A) * (1 / det A), each adjugate entry one fma (p*q - r*s = fma(p, q, -(r*s))), det the first-row cofactor sum nested
// in fmas. valid = false when det is 0 or not finite: such a model has nothing to hit. Row-major: inv[r][c].
struct Inv33 {
    float m[3][3];
    bool valid;
};
__device__ __forceinline__ float cross_term(float p, float q, float r, float s) { return fmaf(p, q, -(r * s)); }
__device__ __forceinline__ Inv33 affine_inverse(const Mat34& a)
{
    // a_rc: row r, column c
    const float a00 = a.c0x, a10 = a.c0y, a20 = a.c0z;
    const float a01 = a.c1x, a11 = a.c1y, a21 = a.c1z;
    const float a02 = a.c2x, a12 = a.c2y, a22 = a.c2z;
    const float j00 = cross_term(a11, a22, a12, a21), j01 = cross_term(a02, a21, a01, a22), j02 = cross_term(a01, a12, a02, a11);
    const float j10 = cross_term(a12, a20, a10, a22), j11 = cross_term(a00, a22, a02, a20), j12 = cross_term(a02, a10, a00, a12);
    const float j20 = cross_term(a10, a21, a11, a20), j21 = cross_term(a01, a20, a00, a21), j22 = cross_term(a00, a11, a01, a10);
    const float det = fmaf(a00, j00, fmaf(a01, j10, a02 * j20));
    const float rdet = 1.0f / det;
    Inv33 r;
    r.valid = det != 0.0f && fabsf(det) < __builtin_inff();  // (NaN fails the second test)
    r.m[0][0] = j00 * rdet; r.m[0][1] = j01 * rdet; r.m[0][2] = j02 * rdet;
    r.m[1][0] = j10 * rdet; r.m[1][1] = j11 * rdet; r.m[1][2] = j12 * rdet;
    r.m[2][0] = j20 * rdet; r.m[2][1] = j21 * rdet; r.m[2][2] = j22 * rdet;
    return r;
}
// adj(A) and det A, by exactly the expressions of affine_inverse above and without its reciprocal: what the normal-cone test of the
// cluster cull carries an eye into model space with. Row-major: j[r][c].
struct Adj33 {
    float j[3][3];
    float det;
};
__device__ __forceinline__ Adj33 affine_adjugate(const Mat34& a)
{
    const float a00 = a.c0x, a10 = a.c0y, a20 = a.c0z;
    const float a01 = a.c1x, a11 = a.c1y, a21 = a.c1z;
    const float a02 = a.c2x, a12 = a.c2y, a22 = a.c2z;
    Adj33 r;
    r.j[0][0] = cross_term(a11, a22, a12, a21); r.j[0][1] = cross_term(a02, a21, a01, a22); r.j[0][2] = cross_term(a01, a12, a02, a11);
    r.j[1][0] = cross_term(a12, a20, a10, a22); r.j[1][1] = cross_term(a00, a22, a02, a20); r.j[1][2] = cross_term(a02, a10, a00, a12);
    r.j[2][0] = cross_term(a10, a21, a11, a20); r.j[2][1] = cross_term(a01, a20, a00, a21); r.j[2][2] = cross_term(a00, a11, a01, a10);
    r.det = fmaf(a00, r.j[0][0], fmaf(a01, r.j[1][0], a02 * r.j[2][0]));
    return r;
}
__device__ __forceinline__ float row_dot(const float (&r)[3], float x, float y, float z) { return fmaf(r[0], x, fmaf(r[1], y, r[2] * z)); }

// The level-of-detail cut of the cluster cull (include/garden_vis.h), fp32, every step as written.
// Per draw, with a_rc = f[3c + r] of the 12 bakedModel floats: n_c = fmaf(a_2c, a_2c, fmaf(a_1c, a_1c, a_0c * a_0c)) for c = 0, 1,
// 2; s2 = 0.0f; s2 = n_0 > s2 ? n_0 : s2; then the same for n_1 and n_2 — the largest squared column norm.
__device__ __forceinline__ float lod_scale2(const Mat34& a)
{
    const float n0 = fmaf(a.c0z, a.c0z, fmaf(a.c0y, a.c0y, a.c0x * a.c0x));
    const float n1 = fmaf(a.c1z, a.c1z, fmaf(a.c1y, a.c1y, a.c1x * a.c1x));
    const float n2 = fmaf(a.c2z, a.c2z, fmaf(a.c2y, a.c2y, a.c2x * a.c2x));
    float s2 = 0.0f;
    s2 = n0 > s2 ? n0 : s2;
    s2 = n1 > s2 ? n1 : s2;
    s2 = n2 > s2 ? n2 : s2;
    return s2;
}
// Per triple (c, r, e): C_r = fmaf(a_r0, c_0, fmaf(a_r1, c_1, fmaf(a_r2, c_2, t_r))) — item 5's nesting.
__device__ __forceinline__ void lod_carry(const Mat34& a, float c0, float c1, float c2, float (&C)[3])
{
    C[0] = fmaf(a.c0x, c0, fmaf(a.c1x, c1, fmaf(a.c2x, c2, a.c3x)));
    C[1] = fmaf(a.c0y, c0, fmaf(a.c1y, c1, fmaf(a.c2y, c2, a.c3y)));
    C[2] = fmaf(a.c0z, c0, fmaf(a.c1z, c1, fmaf(a.c2z, c2, a.c3z)));
}
// u_r = C_r - P_r; D = fmaf(u_2, u_2, fmaf(u_1, u_1, u_0 * u_0)) (item 7's nesting); q = e * k; a = q + r; A = (a * a) * s2;
// Q = (q * q) * s2; N = near_distance * near_distance. Point eye: EXCEEDS iff Q > N && A > D. Parallel eye: EXCEEDS iff Q > N.
// A comparison with a NaN is false. `point` is eye[3] != 0.
__device__ __forceinline__ bool lod_exceeds(const float (&C)[3], float r, float e, float s2, const float (&P)[4], bool point, float k, float near_distance)
{
    const float q = e * k;
    const float a = q + r;
    const float A = (a * a) * s2;
    const float Q = (q * q) * s2;
    const float N = near_distance * near_distance;
    if (!point)
        return Q > N;
    const float u0 = C[0] - P[0], u1 = C[1] - P[1], u2 = C[2] - P[2];
    const float D = fmaf(u2, u2, fmaf(u1, u1, u0 * u0));
    return Q > N && A > D;
}

// One slab of raycast2: the axis interval [lo, hi] of the ray parameter, or for d == 0 the whole line when lo_box <= o <= hi_box
// (ok = false otherwise). A NaN plane parameter also clears ok: every comparison with a NaN is false.
__device__ __forceinline__ void slab(float o, float d, float lo_box, float hi_box, float& t_near, float& t_far, bool& ok)
{
    const float inv = 1.0f / d;
    const float t1 = (lo_box - o) * inv, t2 = (hi_box - o) * inv;
    const bool moving = d != 0.0f;
    const float lo = t1 < t2 ? t1 : t2, hi = t1 < t2 ? t2 : t1;
    const bool axis_ok = moving ? (t1 == t1 && t2 == t2) : (lo_box <= o && o <= hi_box);
    ok = ok && axis_ok;
    if (moving) {
        t_near = lo > t_near ? lo : t_near;
        t_far = hi < t_far ? hi : t_far;
    }
}

// The selector's test of one entry against one ray (origin o, direction d, camera-relative): the 64-bit key of the hit,
// (bits(distSq) << 32) | (order << 28) | slot, or ~0 for a miss. t = (tx, ty, tz): the model's translation; box in model space.
__device__ __forceinline__ unsigned long long pick_key(const Inv33& inv, float tx, float ty, float tz, const float4 a, const float2 b,
                                                       float ox, float oy, float oz, float dx, float dy, float dz, uint32_t order_slot)
{
    const float ux = ox - tx, uy = oy - ty, uz = oz - tz;  // o - t
    const float lox = row_dot(inv.m[0], ux, uy, uz), loy = row_dot(inv.m[1], ux, uy, uz), loz = row_dot(inv.m[2], ux, uy, uz);
    const float ldx = row_dot(inv.m[0], dx, dy, dz), ldy = row_dot(inv.m[1], dx, dy, dz), ldz = row_dot(inv.m[2], dx, dy, dz);
    float t_near = -__builtin_inff(), t_far = __builtin_inff();
    bool ok = inv.valid;
    slab(lox, ldx, a.x, a.w, t_near, t_far, ok);
    slab(loy, ldy, a.y, b.x, t_near, t_far, ok);
    slab(loz, ldz, a.z, b.y, t_near, t_far, ok);
    const float dist_sq = fmaf(uz, uz, fmaf(uy, uy, ux * ux));
    const bool hit = ok && t_near >= 0.0f && t_near <= t_far && dist_sq < 3.40282347e+38f;
    return hit ? ((unsigned long long)__float_as_uint(dist_sq) << 32) | order_slot : ~0ull;
}

// ------------------------------------------------------------------------------------------------
// instance data: mvp = viewProj * f32x4x4(bakedModel, (0,0,0,1)), the first thing every plugin's drawAsync
// computes (sprite.cpp:107-108, model completed at mesh.cpp:596)
// ------------------------------------------------------------------------------------------------
// One column of the 4x4 product of item 2, all four rows: a = view_proj (column-major, a[4 k + i] = a.c_k[i]), (b0, b1, b2, b3) a
// column of the completed model. The four-term nesting is kept although b3 is 0 or 1: dropping the term changes the sign of a
// zero and what a non-finite view_proj produces.
__device__ __forceinline__ float4 mvp_column(const float (&a)[16], float b0, float b1, float b2, float b3)
{
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
        o[i] = fmaf(a[12 + i], b3, fmaf(a[8 + i], b2, fmaf(a[4 + i], b1, fmaf(a[i], b0, 0.0f))));
    return make_float4(o[0], o[1], o[2], o[3]);
}

// ------------------------------------------------------------------------------------------------
// last frame's mvp per draw (the reference fills its velocity attachment from the camera alone,
// shaders/velocity.frag, and has no per-object velocity: the rule is this build's). Test twin: tests/previous_twin.h. Kernels:
// gv_previous.hip — the selection is two compares and three selects in front of mvp_column above, which IS step 4.
//
// THE PREVIOUS RULE (the same text stands in DESIGN.md §4 item 18, include/garden_vis.h and tests/previous_twin.h). For draw k of a
// view: slot s_k, record model M_k, VP = the view's view_proj, the pool's history H (per slot 12 floats and a stamp; an epoch e, 0 =
// empty; a coverage H.slots; the kept view's view_proj KVP and camera position KC), PVP = prev_view_proj, or KVP when it is NULL,
// d_r = view.camera_position[r] - KC[r] (one fp32 subtraction per component, done on the host).
//  1. Cut: GV_PREVIOUS_CUT, or e == 0: every draw is fresh, with PVP = VP and d = (0, 0, 0).
//  2. Kept <=> no cut && s_k < H.slots && stamp[s_k] == e: P_k = the row's 12 floats.
//  3. Fresh otherwise: the draw is taken as static in the world. P_k = M_k with c3[r] = M_k.c3[r] + d_r (one fp32 add per component);
//     the other nine floats verbatim.
//  4. prev_mvp_k = PVP * P_k exactly as item 9: element i of column j = fma(PVP[12 + i], b3, fma(PVP[8 + i], b2, fma(PVP[4 + i], b1,
//     fma(PVP[i], b0, +0)))) with (b0, b1, b2) = column j of P_k and b3 = 0, or 1 for j = 3. has_history_k = 1 when kept, 0 when fresh.
// ------------------------------------------------------------------------------------------------

// ------------------------------------------------------------------------------------------------
// level of detail of a draw (the reference carries ModelRenderComponent::lods, model.hpp:29-41, and no rule
// that picks among them, so the rule is this build's). Test twin: tests/lod_twin.h.
//   t          the translation of the record's bakedModel as delivered (floats 9, 10, 11): the pivot relative to camera_position
//   d2         fmaf(tz, tz, fmaf(ty, ty, tx * tx))
//   x          d2 * view_scale, one multiply
//   q_i        (size * switch_at[i])^2, two multiplies, for i = 0 .. levels - 2
//   level      the NUMBER of i with x > q_i: a count, so unsorted thresholds are defined; a comparison with a NaN is false, so a NaN
//              size, distance or scale gives level 0; an infinite x gives levels - 1 over finite thresholds; a tie keeps the finer level
// sw: the entry's seven switch_at words, all of them (those at or beyond levels - 1 are masked, never indexed dynamically).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lod_distance_sq(float tx, float ty, float tz) { return fmaf(tz, tz, fmaf(ty, ty, tx * tx)); }

__device__ __forceinline__ uint32_t lod_level(float x, float size, uint32_t levels, const float (&sw)[7])
{
    uint32_t level = 0;
#pragma unroll
    for (uint32_t i = 0; i < 7u; i++) {
        const float y = size * sw[i];
        const float q = y * y;
        level += (i + 1u < levels && x > q) ? 1u : 0u;
    }
    return level;
}

// ------------------------------------------------------------------------------------------------
// bounds of a view's visible draws in a caller's basis (the reference fits a cascade to its frustum slice and
// stretches the depth range by zCoeff because it does not know where the casters are, csm.cpp:294-295). Test twin: tests/bounds_twin.h.
//   p_c        the record's eight corners, exactly item 5's: aabb_corners over the record's own bakedModel and the box of its entry
//   q_{c,r}    fmaf(B.c0[r], p.x, fmaf(B.c1[r], p.y, fmaf(B.c2[r], p.z, B.c3[r]))) for r = 0, 1, 2: B an affine 3x4 like bakedModel
//   lo / hi    the minimum / maximum of q_{c,r} over all records and corners in the order of the key
//              T(u) = u ^ ((u >> 31) ? 0xFFFFFFFF : 0x80000000) on the float's bits: -0 below +0, +-inf take part, a NaN takes no part
//              (in that coordinate only); nothing taking part gives lo = +inf, hi = -inf
// Minimum and maximum of unsigned keys are associative and commutative, and every q is computed from one record alone: no order of
// evaluation — lanes, waves, workgroups, partial rows — can change any output bit. The same holds for the count of records with a NaN.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bounds_key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float bounds_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }

// row r of B over the corner pairs of `c`: four packed fma chains, each element the scalar chain above
__device__ __forceinline__ void bounds_project(const Corners& c, float b0, float b1, float b2, float b3, v2f (&q)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++)
        q[j] = pk_fma(splat(b0), c.x[j], pk_fma(splat(b1), c.y[j], pk_fma(splat(b2), c.z[j], splat(b3))));
}

// ------------------------------------------------------------------------------------------------
// occluder depth (the reference's Hi-Z reads its renderer's depth buffer, hiz.cpp:146, and nothing in this
// library draws one). Test twin: tests/occluder_twin.h. Kernels: gv_occluders.hip.
//
// THE RULE (the same text stands in DESIGN.md §4 item 16 and tests/occluder_twin.h). For draw k of a view: slot s_k, record model M_k,
// the slot's occluder box (omin, omax) in model space, VP = the view's view_proj, the image W x H, the call's min_pixels.
//  1. Has a box <=> omin.x < omax.x && omin.y < omax.y && omin.z < omax.z (a NaN fails). Otherwise: not an occluder, counted no_box.
//  2. Corners p_c = aabb_corners(M_k, omin, omax) (item 5: bit0 -> x, bit1 -> y, bit2 -> z selects max; every row
//     fma(c0, x, fma(c1, y, fma(c2, z, c3)))). Clip: cl_r = fma(VP[r], p.x, fma(VP[4 + r], p.y, fma(VP[8 + r], p.z, VP[12 + r]))) for
//     r = x, y, z, w; rcp = 1.0f / cl_w (IEEE); u = fma(cl_x * rcp, .5, .5), v = fma(cl_y * rcp, .5, .5), z = cl_z * rcp: the words of
//     the Hi-Z query (hiz_occluded), restated.
//  3. Any corner with !(cl_w > 0): skipped, counted behind.
//  4. d = minNum(minNum over the 8 corners of z, 1.0f); !(d > 0): skipped, counted behind. (Reversed Z: d is the box's farthest depth.)
//  5. fx = floorf(u * (float)(16 W)), fy = floorf(v * (float)(16 H)): four sub-pixel bits. Any !(|f| < 4194304.0f): skipped, counted
//     range (a NaN or an infinity lands here). Otherwise X_c, Y_c are int32.
//  6. Faces as corner cycles: -x (0,4,6,2), +x (1,3,7,5), -y (0,1,5,4), +y (2,6,7,3), -z (0,2,3,1), +z (4,5,7,6).
//     A_f = sum over the cycle's edges p -> q of (X_p Y_q - X_q Y_p) in int64; a face is positive <=> A_f > 0. Each of the 12 box edges
//     belongs to two faces: it is active <=> exactly one of them is positive, directed a -> b as in the positive face's cycle.
//     No positive face: skipped, counted flat. (Positive faces may be the front or the back set; both bound the same silhouette.)
//  7. Pixel (px, py) is covered <=> for every active edge and each pixel corner cx in {px, px + 1}, cy in {py, py + 1}:
//     ex (16 cy - Y_a) - ey (16 cx - X_a) >= 2 (|ex| + |ey|), ex = X_b - X_a, ey = Y_b - Y_a, all int64. The margin 2 pays for the
//     snapping (under one unit per axis) and the fp32 rounding in front of it (about one more).
//  8. x0 = max(min X >> 4, 0), x1 = min(max X >> 4, W - 1) (arithmetic shifts), y likewise. An empty range, or a width or height in
//     pixels below min_pixels: skipped, counted small. Otherwise the occluder is counted drawn (whether or not it covers a pixel).
//  9. depth[py W + px] = max(0.0f, max over the covering occluders of d), taken on the floats' bits as uint32: every value is >= 0,
//     so that order is the float order, and the maximum does not depend on any order of evaluation.
// ------------------------------------------------------------------------------------------------
// Item 2, the expressions of hiz_occluded (gv_device.hpp) restated — not shared: the hot kernels' code stays as it is. Returns item 3's
// "every corner in front of the camera plane".
__device__ __forceinline__ bool occluder_clip(const float (&vp)[16], const Corners& c, float (&u)[8], float (&v)[8], float (&z)[8])
{
    bool in_front = true;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const v2f clx = pk_fma(splat(vp[0]), c.x[j], pk_fma(splat(vp[4]), c.y[j], pk_fma(splat(vp[8]), c.z[j], splat(vp[12]))));
        const v2f cly = pk_fma(splat(vp[1]), c.x[j], pk_fma(splat(vp[5]), c.y[j], pk_fma(splat(vp[9]), c.z[j], splat(vp[13]))));
        const v2f clz = pk_fma(splat(vp[2]), c.x[j], pk_fma(splat(vp[6]), c.y[j], pk_fma(splat(vp[10]), c.z[j], splat(vp[14]))));
        const v2f clw = pk_fma(splat(vp[3]), c.x[j], pk_fma(splat(vp[7]), c.y[j], pk_fma(splat(vp[11]), c.z[j], splat(vp[15]))));
        in_front = in_front && (clw.x > 0.0f) && (clw.y > 0.0f);
        const v2f rcp = {1.0f / clw.x, 1.0f / clw.y};  // IEEE-correct division, one per corner
        const v2f uu = pk_fma(clx * rcp, splat(0.5f), splat(0.5f));
        const v2f vv = pk_fma(cly * rcp, splat(0.5f), splat(0.5f));
        const v2f zz = clz * rcp;
        u[2 * j] = uu.x; u[2 * j + 1] = uu.y;
        v[2 * j] = vv.x; v[2 * j + 1] = vv.y;
        z[2 * j] = zz.x; z[2 * j + 1] = zz.y;
    }
    return in_front;
}
// Item 4 (IEEE minNum: v_min_f32, as the twin's fminf; the nesting cannot change a value that passes d > 0)
__device__ __forceinline__ float occluder_depth(const float (&z)[8])
{
    return fminf(fminf(fminf(fminf(z[0], z[1]), fminf(z[2], z[3])), fminf(fminf(z[4], z[5]), fminf(z[6], z[7]))), 1.0f);
}
// Item 5 for one coordinate: false when it is out of range (NaN and infinities included)
__device__ __forceinline__ bool occluder_snap(float t, float scale16, int32_t& out)
{
    const float f = floorf(t * scale16);
    const bool ok = fabsf(f) < 4194304.0f;
    out = ok ? (int32_t)f : 0;
    return ok;
}
// Item 6. The 12 box edges a -> b with the face P whose cycle holds a -> b and the face Q whose cycle holds b -> a (faces numbered
// -x +x -y +y -z +z). A cross term is shared by the edge's two faces with opposite signs, so the six areas take 12 terms.
// Returns bits 0-11: the edge is active; bits 12-23: its direction is b -> a (Q is the positive face); 0: no positive face.
constexpr int kOccluderEdgeA[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3};
constexpr int kOccluderEdgeB[12] = {1, 3, 5, 7, 2, 3, 6, 7, 4, 5, 6, 7};
constexpr int kOccluderEdgeP[12] = {2, 4, 5, 3, 4, 1, 0, 5, 0, 2, 3, 1};
constexpr int kOccluderEdgeQ[12] = {4, 3, 2, 5, 0, 4, 5, 1, 2, 1, 0, 3};
__device__ __forceinline__ uint32_t occluder_edges(const int32_t (&X)[8], const int32_t (&Y)[8])
{
    long long area[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 12; e++) {
        const int a = kOccluderEdgeA[e], b = kOccluderEdgeB[e];
        const long long t = (long long)X[a] * Y[b] - (long long)X[b] * Y[a];
        area[kOccluderEdgeP[e]] += t;
        area[kOccluderEdgeQ[e]] -= t;
    }
    uint32_t edges = 0;
#pragma unroll
    for (int e = 0; e < 12; e++) {
        const bool p = area[kOccluderEdgeP[e]] > 0, q = area[kOccluderEdgeQ[e]] > 0;
        edges |= (p != q ? 1u : 0u) << e;
        edges |= (p != q && q ? 1u : 0u) << (12 + e);
    }
    return edges;
}
// Item 7 for one edge over a rectangle of pixel corners [cx0, cx1] x [cy0, cy1]: E = ex (16 cy - Ya) - ey (16 cx - Xa) - 2 (|ex| + |ey|)
// at the corner where it is smallest / largest. E is linear, so "lo >= 0" is "every pixel corner inside passes" and "hi < 0" is
// "none does". A pixel is the rectangle [px, px + 1] x [py, py + 1].
struct OccluderEdge {
    long long ex, ey, at;  // at = ex * (-Ya) + ey * Xa - margin: E = 16 (ex cy - ey cx) + at
};
__device__ __forceinline__ OccluderEdge occluder_edge(int32_t xa, int32_t ya, int32_t xb, int32_t yb)
{
    OccluderEdge g;
    g.ex = (long long)xb - xa;
    g.ey = (long long)yb - ya;
    g.at = g.ey * xa - g.ex * ya - 2 * ((g.ex < 0 ? -g.ex : g.ex) + (g.ey < 0 ? -g.ey : g.ey));
    return g;
}
__device__ __forceinline__ long long occluder_edge_lo(const OccluderEdge& g, long long cx0, long long cx1, long long cy0, long long cy1)
{
    return 16 * (g.ex * (g.ex > 0 ? cy0 : cy1) - g.ey * (g.ey > 0 ? cx1 : cx0)) + g.at;
}
__device__ __forceinline__ long long occluder_edge_hi(const OccluderEdge& g, long long cx0, long long cx1, long long cy0, long long cy1)
{
    return 16 * (g.ex * (g.ex > 0 ? cy1 : cy0) - g.ey * (g.ey > 0 ? cx0 : cx1)) + g.at;
}

// ------------------------------------------------------------------------------------------------
// receiver mask (shadow-caster culling by a receiver mask, Bittner et al. 2011: the reference culls every shadow
// pass as a plain frustum cull, mesh.cpp:795-847). The mirror image of item 16: an OUTER rasteriser that keeps the MINIMUM of the boxes'
// farthest depths, projected with a matrix the caller names. Test twin: tests/receiver_twin.h. Kernels: gv_receivers.hip.
//
// THE RECEIVER RULE (the same text stands in DESIGN.md §4 item 17 and tests/receiver_twin.h). For draw k of the source view: slot s_k,
// record model M_k, the slot's cull AABB (amin, amax) as the mesh mirror holds it, L = the call's light_view_proj, the mask W x H.
//  1. Corners p_c = aabb_corners(M_k, amin, amax) and clip coordinates exactly as item 16 step 2 with L in place of VP: cl_r = fma(L[r],
//     p.x, fma(L[4 + r], p.y, fma(L[8 + r], p.z, L[12 + r]))), rcp = 1.0f / cl_w (IEEE), u = fma(cl_x * rcp, .5, .5), v likewise,
//     z = cl_z * rcp: a caster that is also a receiver gets the words its own Hi-Z query computes against L.
//  2. Any corner with !(cl_w > 0): counted behind, and +0.0f goes into EVERY pixel of the mask (a receiver that cannot be bounded keeps
//     every caster; it is never skipped).
//  3. m = minNum over the 8 corners of z; d = (m > 0.0f) ? m : +0.0f (a NaN gives +0.0f; -0.0f, whose bits are the largest unsigned
//     word, never appears). No upper clamp: a receiver in front of the near plane keeps its d > 1.
//  4. fx = floorf(u * (float)(16 W)), fy = floorf(v * (float)(16 H)). Any !(|f| < 4194304.0f): counted range, and d goes into every
//     pixel of the mask. Otherwise X_c, Y_c are int32.
//  5. x0 = max((min X - 2) >> 4, 0), x1 = min((max X + 2) >> 4, W - 1) (arithmetic shifts; the 2 is item 16's margin), y likewise. An
//     empty range: counted outside, nothing written.
//  6. Faces, areas (int64) and active directed edges as item 16 step 6. No positive face: counted flat, and d goes into every pixel of
//     the range (an edge-on sprite, a sub-pixel box).
//  7. Otherwise counted drawn. Pixel (px, py) of the range is touched <=> for EVERY active edge a -> b SOME pixel corner cx in {px, px + 1},
//     cy in {py, py + 1} passes ex (16 cy - Y_a) - ey (16 cx - X_a) >= -2 (|ex| + |ey|), ex = X_b - X_a, ey = Y_b - Y_a, all int64: item
//     16's half-plane test at the corner that lies MOST inside, with the margin on the other side. d goes into every touched pixel.
//  8. mask[py W + px] = min(+inf, min over the receivers that write the pixel of their word), taken on the floats' bits as uint32: every
//     word is a non-negative float or +inf, so that order is the float order, and the result depends on no order of evaluation.
// ------------------------------------------------------------------------------------------------
// Steps 1, 4 and 6 are occluder_clip, occluder_snap and occluder_edges: the same words.
// Step 3 (IEEE minNum; the nesting cannot change a value that passes m > 0, and everything else becomes +0.0f)
__device__ __forceinline__ float receiver_depth(const float (&z)[8])
{
    const float m = fminf(fminf(fminf(z[0], z[1]), fminf(z[2], z[3])), fminf(fminf(z[4], z[5]), fminf(z[6], z[7])));
    return m > 0.0f ? m : 0.0f;
}
// Step 7 for one edge: E = ex (16 cy - Ya) - ey (16 cx - Xa) + 2 (|ex| + |ey|) = 16 (ex cy - ey cx) + at. A pixel passes the edge when
// E >= 0 at its best corner: occluder_edge_hi over [px, px + 1] x [py, py + 1].
__device__ __forceinline__ OccluderEdge receiver_edge(int32_t xa, int32_t ya, int32_t xb, int32_t yb)
{
    OccluderEdge g;
    g.ex = (long long)xb - xa;
    g.ey = (long long)yb - ya;
    g.at = g.ey * xa - g.ex * ya + 2 * ((g.ex < 0 ? -g.ex : g.ex) + (g.ey < 0 ? -g.ey : g.ey));
    return g;
}
__device__ __forceinline__ long long receiver_edge_at(const OccluderEdge& g, long long px, long long py)
{
    return occluder_edge_hi(g, px, px + 1, py, py + 1);
}
// ... over the PIXELS [px0, px1] x [py0, py1]: the best corner's E of the pixel where it is smallest ("lo >= 0": every pixel passes the
// edge) and largest ("hi < 0": none does). The best corner's E is linear in (px, py) too.
__device__ __forceinline__ long long receiver_edge_lo(const OccluderEdge& g, long long px0, long long px1, long long py0, long long py1)
{
    return receiver_edge_at(g, g.ey > 0 ? px1 : px0, g.ex > 0 ? py0 : py1);
}
__device__ __forceinline__ long long receiver_edge_hi(const OccluderEdge& g, long long px0, long long px1, long long py0, long long py1)
{
    return receiver_edge_at(g, g.ey > 0 ? px0 : px1, g.ex > 0 ? py1 : py0);
}

}  // namespace gv
