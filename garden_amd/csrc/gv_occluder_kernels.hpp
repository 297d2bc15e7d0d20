// gv_occluder_kernels.hpp — launch interface of gv_occluders.hip: gv_pool_draw_occluders, the occluder boxes of a view's draws
// rasterised into a depth image. Kept apart from gv_kernels.hpp like gv_bounds_kernels.hpp.
#pragma once
#include "gv_kernels.hpp"

namespace gv {

constexpr uint32_t kOccluderBlock = 256;         // lanes per workgroup of all three launches; records per workgroup of the setup launch
constexpr uint32_t kOccluderTile = 32;           // T: a work item of the raster launch is one occluder's T x T pixels on the image's tile grid
constexpr uint32_t kOccluderRasterGroups = 1024; // the raster launch's fixed grid: every wave walks its share of the items
constexpr uint32_t kOccluderRowBytes = 32;       // a slot's row of the box mirror: min in words 0-2, max in words 4-6
static_assert(kOccluderTile == 32, "a wave's step is two rows of 32 pixels: two 128-byte segments per atomic instruction");

struct OccluderCounts {     // GvOccluderCounts
    uint32_t drawn, no_box, behind, range, flat, small;
};
// What the raster launch needs of a drawn occluder: kept in registers, computed by occluder_setup (gv_occluders.hip) in both launches.
struct OccluderRow {
    int32_t X[8], Y[8];     // item 5's snapped corners
    uint32_t depth_bits;    // d
    uint32_t edges;         // occluder_edges: bits 0-11 active, 12-23 reversed
    uint32_t xr, yr;        // x0 | x1 << 16, y0 | y1 << 16: the pixel range of item 8
};

struct OccluderLaunch {
    const uint32_t* count;  // device draw count of the view
    const uint32_t* idx;    // its records in delivery order: POOL slots
    const float* model;     // ... and their bakedModel, 12 floats each
    uint32_t capacity;      // the occupancy the view was culled with: the host's bound of *count
    const float4* boxes;    // the box mirror: two float4 per POOL slot
    uint32_t slots;         // slots it covers: a record outside takes no box
    float view_proj[16];
    uint32_t width, height, min_pixels;
    uint32_t* local;                // [capacity]: tiles of the drawn occluders in front of record k inside its workgroup
    unsigned long long* base;       // [blocks + 1] block tile totals (setup) -> items in front of the block, then the total (scan)
    OccluderCounts* counts;         // added to
    float* depth;                   // the image
};
hipError_t launch_occluder_setup(const OccluderLaunch& launch, hipStream_t stream);
hipError_t launch_occluder_scan(const OccluderLaunch& launch, hipStream_t stream);
hipError_t launch_occluder_raster(const OccluderLaunch& launch, hipStream_t stream);

}  // namespace gv
