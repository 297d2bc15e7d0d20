/* instance_twin.h — TEST ONLY: plain-C99 restatement of the instance arithmetic of DESIGN.md §4 item 9 (gv_device_math.hpp
 * mvp_column), the check gv_pool_emit_instances' kernel is compared against bit for bit. Compile with -ffp-contract=off: every
 * fused multiply-add is written as fmaf. view_proj and mvp are column-major 4x4 matrices (element [4 j + i] = row i of column j);
 * model is a record's bakedModel, 12 floats in float4x3 order (c0.xyz c1.xyz c2.xyz c3.xyz), completed with the bottom row
 * (0, 0, 0, 1) as mesh.cpp:596 does. */
#ifndef GV_INSTANCE_TWIN_H
#define GV_INSTANCE_TWIN_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* mvp = view_proj * model: the 4x4 product of §4 item 2, literally — four nested fmas per element from +0, the last one with
 * the bottom-row element of the model's column (0 or 1), which is kept: it decides the sign of a zero and what a non-finite
 * view_proj gives */
static inline void instance_twin_mvp(const float view_proj[16], const float model[12], float mvp[16])
{
    int i, j;
    for (j = 0; j < 4; j++) {
        const float b0 = model[3 * j], b1 = model[3 * j + 1], b2 = model[3 * j + 2], b3 = j == 3 ? 1.0f : 0.0f;
        for (i = 0; i < 4; i++)
            mvp[4 * j + i] = fmaf(view_proj[12 + i], b3, fmaf(view_proj[8 + i], b2, fmaf(view_proj[4 + i], b1, fmaf(view_proj[i], b0, 0.0f))));
    }
}

/* n records of one view */
static inline void instance_twin_many(const float view_proj[16], const float* models, uint32_t n, float* mvps)
{
    uint32_t k;
    for (k = 0; k < n; k++)
        instance_twin_mvp(view_proj, models + 12 * (size_t)k, mvps + 16 * (size_t)k);
}

#endif
