/* lod_twin.h — TEST ONLY: plain-C99 restatement of the level-of-detail rule of DESIGN.md §4 item 11 (gv_device_math.hpp lod_level),
 * the check gv_pool_select_lods' kernel is compared against word for word. Compile with -ffp-contract=off: the one fused
 * multiply-add chain is written as fmaf, every other product is a plain fp32 multiply. model is a record's bakedModel, 12 floats in
 * float4x3 order (c0.xyz c1.xyz c2.xyz c3.xyz): the translation is floats 9, 10, 11. A table entry is 8 words: levels, then seven
 * fp32 switch_at (GvLodGeometry). */
#ifndef GV_LOD_TWIN_H
#define GV_LOD_TWIN_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define LOD_TWIN_MAX_LEVELS 8u

/* the level of one draw: the NUMBER of thresholds i < levels - 1 with d2 * scale > (size * switch_at[i])^2 */
static inline uint32_t lod_twin_level(const float model[12], float size, float scale, uint32_t levels, const float* switch_at)
{
    const float tx = model[9], ty = model[10], tz = model[11];
    const float d2 = fmaf(tz, tz, fmaf(ty, ty, tx * tx));
    const float x = d2 * scale;
    uint32_t i, level = 0;
    for (i = 0; i + 1 < levels; i++) {
        const float y = size * switch_at[i];
        const float q = y * y;
        if (x > q) /* (false for a NaN on either side) */
            level++;
    }
    return level;
}

/* g = base + level as a uint32 add (wraps) */
static inline uint32_t lod_twin_effective(uint32_t base, uint32_t level) { return (uint32_t)(base + level); }

/* n draws of one view: base[k] = id of the draw's slot, size[k] = size of the draw's slot; table: table_count entries of 8 words.
 * out[k] = base + level (uint32 add); hist[0 .. 7] += draws per level */
static inline void lod_twin_many(const float* models, const uint32_t* base, const float* size, uint32_t n, float scale, const uint32_t* table,
                                 uint32_t table_count, uint32_t* out, uint32_t* hist)
{
    uint32_t k;
    for (k = 0; k < n; k++) {
        uint32_t levels = 1, level;
        float switch_at[LOD_TWIN_MAX_LEVELS - 1] = {0};
        if (base[k] < table_count) {
            levels = table[8 * (size_t)base[k]];
            memcpy(switch_at, table + 8 * (size_t)base[k] + 1, sizeof(switch_at));
        }
        level = lod_twin_level(models + 12 * (size_t)k, size[k], scale, levels, switch_at);
        out[k] = lod_twin_effective(base[k], level);
        hist[level]++;
    }
}

#endif
