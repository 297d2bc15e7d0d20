/* pick_twin.h — TEST ONLY: plain-C99 restatement of the picking arithmetic of DESIGN.md §4 item 8 (gv_device_math.hpp
 * affine_inverse / slab / pick_key), the check gv_pick's kernel is compared against bit for bit. Compile with -ffp-contract=off:
 * every fused multiply-add is written as fmaf, every other product and sum must stay unfused. Models are camera-relative 3x4
 * matrices in float4x3 order (c0.xyz c1.xyz c2.xyz c3.xyz: a record's bakedModel), boxes (min.xyz, max.xyz) in model space. */
#ifndef GV_PICK_TWIN_H
#define GV_PICK_TWIN_H
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#define PICK_TWIN_MISS UINT64_MAX

static inline float pick_twin_cross(float p, float q, float r, float s) { return fmaf(p, q, -(r * s)); }

/* inv[r][c] of the upper 3x3 of `model`; returns 0 when det is 0 or not finite (nothing to hit) */
static inline int pick_twin_inverse(const float model[12], float inv[3][3])
{
    const float a00 = model[0], a10 = model[1], a20 = model[2];
    const float a01 = model[3], a11 = model[4], a21 = model[5];
    const float a02 = model[6], a12 = model[7], a22 = model[8];
    const float j00 = pick_twin_cross(a11, a22, a12, a21), j01 = pick_twin_cross(a02, a21, a01, a22), j02 = pick_twin_cross(a01, a12, a02, a11);
    const float j10 = pick_twin_cross(a12, a20, a10, a22), j11 = pick_twin_cross(a00, a22, a02, a20), j12 = pick_twin_cross(a02, a10, a00, a12);
    const float j20 = pick_twin_cross(a10, a21, a11, a20), j21 = pick_twin_cross(a01, a20, a00, a21), j22 = pick_twin_cross(a00, a11, a01, a10);
    const float det = fmaf(a00, j00, fmaf(a01, j10, a02 * j20));
    const float rdet = 1.0f / det;
    inv[0][0] = j00 * rdet; inv[0][1] = j01 * rdet; inv[0][2] = j02 * rdet;
    inv[1][0] = j10 * rdet; inv[1][1] = j11 * rdet; inv[1][2] = j12 * rdet;
    inv[2][0] = j20 * rdet; inv[2][1] = j21 * rdet; inv[2][2] = j22 * rdet;
    return det != 0.0f && fabsf(det) < INFINITY;
}

static inline float pick_twin_row(const float r[3], float x, float y, float z) { return fmaf(r[0], x, fmaf(r[1], y, r[2] * z)); }

static inline void pick_twin_slab(float o, float d, float lo_box, float hi_box, float* t_near, float* t_far, int* ok)
{
    if (d != 0.0f) {
        const float inv = 1.0f / d;
        const float t1 = (lo_box - o) * inv, t2 = (hi_box - o) * inv;
        const float lo = t1 < t2 ? t1 : t2, hi = t1 < t2 ? t2 : t1;
        if (t1 != t1 || t2 != t2)
            *ok = 0;
        if (lo > *t_near)
            *t_near = lo;
        if (hi < *t_far)
            *t_far = hi;
    } else if (!(lo_box <= o && o <= hi_box)) {
        *ok = 0;
    }
}

/* (bits(distSq) << 32) | order_slot of a hit, PICK_TWIN_MISS otherwise. ray = origin xyz, direction xyz. valid: the inverse's. */
static inline uint64_t pick_twin_key_inv(float inv[3][3], int valid, const float model[12], const float box[6], const float ray[6],
                                         uint32_t order_slot)
{
    const float ux = ray[0] - model[9], uy = ray[1] - model[10], uz = ray[2] - model[11];
    const float ox = pick_twin_row(inv[0], ux, uy, uz), oy = pick_twin_row(inv[1], ux, uy, uz), oz = pick_twin_row(inv[2], ux, uy, uz);
    const float dx = pick_twin_row(inv[0], ray[3], ray[4], ray[5]), dy = pick_twin_row(inv[1], ray[3], ray[4], ray[5]),
                dz = pick_twin_row(inv[2], ray[3], ray[4], ray[5]);
    float t_near = -INFINITY, t_far = INFINITY, dist_sq;
    int ok = valid;
    uint32_t bits;
    pick_twin_slab(ox, dx, box[0], box[3], &t_near, &t_far, &ok);
    pick_twin_slab(oy, dy, box[1], box[4], &t_near, &t_far, &ok);
    pick_twin_slab(oz, dz, box[2], box[5], &t_near, &t_far, &ok);
    dist_sq = fmaf(uz, uz, fmaf(uy, uy, ux * ux));
    if (!(ok && t_near >= 0.0f && t_near <= t_far && dist_sq < FLT_MAX))
        return PICK_TWIN_MISS;
    memcpy(&bits, &dist_sq, 4);
    return ((uint64_t)bits << 32) | order_slot;
}

static inline uint64_t pick_twin_key(const float model[12], const float box[6], const float ray[6], uint32_t order_slot)
{
    float inv[3][3];
    const int valid = pick_twin_inverse(model, inv);
    return pick_twin_key_inv(inv, valid, model, box, ray, order_slot);
}

/* keys[r] = min(keys[r], key of every entry k of one pool against ray r): n entries (models[12 k], boxes[6 k], slots[k]) at
 * position `order` of the call's pool list, `exclude` (UINT32_MAX: none) never picked */
static inline void pick_twin_min(uint32_t n, const float* models, const float* boxes, const uint32_t* slots, uint32_t order, uint32_t exclude,
                                 const float* rays, uint32_t ray_count, uint64_t* keys)
{
    uint32_t k, r;
    for (k = 0; k < n; k++) {
        float inv[3][3];
        int valid;
        if (slots[k] == exclude || slots[k] == UINT32_MAX)
            continue;
        valid = pick_twin_inverse(models + 12 * (size_t)k, inv);
        if (!valid)
            continue;
        for (r = 0; r < ray_count; r++) {
            const uint64_t key = pick_twin_key_inv(inv, valid, models + 12 * (size_t)k, boxes + 6 * (size_t)k, rays + 6 * r,
                                                   (order << 28) | slots[k]);
            if (key < keys[r])
                keys[r] = key;
        }
    }
}

#endif
