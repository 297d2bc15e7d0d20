// gv_bounds_kernels.hpp — launch interface of gv_bounds.hip: gv_pool_view_bounds, the bounds of a view's visible draws in a caller's
// basis. Kept apart from gv_kernels.hpp like gv_group_kernels.hpp and gv_second_kernels.hpp.
#pragma once
#include "gv_kernels.hpp"

namespace gv {

constexpr uint32_t kBoundsBlock = 256;      // lanes per workgroup of both launches
constexpr uint32_t kBoundsRecords = 1024;   // R: records per workgroup of bounds_fold_kernel, kBoundsRecords / kBoundsBlock per lane
constexpr uint32_t kMaxBoundsItems = 8;     // GV_MAX_BOUNDS_ITEMS
static_assert(kMaxBoundsItems == kMaxInstanceViews, "view_of_block finds the item of a workgroup");
static_assert(kBoundsRecords % kBoundsBlock == 0, "every lane takes the same number of records");

// The order of the fold: the float's bits as an unsigned key, T(u) = u ^ ((u >> 31) ? 0xFFFFFFFF : 0x80000000) (the sort's and the
// merge's key): -0 below +0, the infinities at the ends of the numbers. A NaN takes no part: its place is taken by the identity
// of the side it is folded into, which is the key of +inf for a minimum and of -inf for a maximum — exactly what an empty fold
// answers, and no participant can be moved by it.
constexpr uint32_t kBoundsLoIdentity = 0xFF800000u;  // T(+inf)
constexpr uint32_t kBoundsHiIdentity = 0x007FFFFFu;  // T(-inf)

struct BoundsItem {
    const uint32_t* count;  // device draw count of the item's view
    const uint32_t* idx;    // its records in delivery order: POOL slots
    const float* model;     // ... and their bakedModel, 12 floats each
    uint32_t capacity;      // the occupancy the view was culled with: the host's bound of *count
    float basis[12];        // B: c0.xyz c1.xyz c2.xyz c3.xyz
};
struct BoundsResult {       // GvViewBounds
    float lo[3];
    uint32_t draw_count;
    float hi[3];
    uint32_t nan_records;
};
struct BoundsPartial {      // one row per bounds_fold_kernel workgroup: keys, not floats
    uint32_t lo[3], nan_records;
    uint32_t hi[3], pad;
};
struct BoundsLaunch {
    BoundsItem item[kMaxBoundsItems];
    uint32_t first_block[kMaxBoundsItems + 1];  // bounds_fold_kernel workgroups in front of item i
    uint32_t items;
    const float4* a;        // MeshMirror::a / b: the boxes by mirror entry
    const float2* b;
    const uint32_t* inv;    // pool slot -> mirror entry (NULL: the mirror is in pool order)
    uint32_t slots;         // slots inv covers / entries a and b cover: a record outside either takes the empty box and reads nothing
    uint32_t entries;
    BoundsPartial* partial; // [first_block[items]]
    BoundsResult* out;      // [items]
};
hipError_t launch_bounds_fold(const BoundsLaunch& launch, hipStream_t stream);
hipError_t launch_bounds_finish(const BoundsLaunch& launch, hipStream_t stream);

}  // namespace gv
