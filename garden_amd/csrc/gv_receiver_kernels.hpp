// gv_receiver_kernels.hpp — launch interface of gv_receivers.hip: gv_pool_draw_receivers, the cull AABBs of a view's draws rasterised
// outwards into a receiver mask in a light's clip space. Kept apart from gv_kernels.hpp like
// gv_occluder_kernels.hpp, whose tile, workgroup size, raster grid and scan launch it shares.
#pragma once
#include "gv_occluder_kernels.hpp"

namespace gv {

constexpr uint32_t kReceiverBlock = kOccluderBlock;   // lanes per workgroup of both launches; records per workgroup of the setup launch
constexpr uint32_t kReceiverTile = kOccluderTile;     // T: a work item of the raster launch is one receiver's T x T pixels on the mask's tile grid
constexpr uint32_t kReceiverRasterGroups = kOccluderRasterGroups;
constexpr uint32_t kReceiverSmallPixels = 16;         // a receiver whose pixel range holds at most this many pixels is written by the setup launch itself
static_assert(kReceiverBlock == kOccluderBlock, "the scan between the two launches is launch_occluder_scan: one base[] entry per kOccluderBlock records");
static_assert(kReceiverSmallPixels <= 32, "the setup lane keeps one bit per pixel of a small range");

struct ReceiverCounts {     // GvReceiverCounts
    uint32_t drawn, flat, behind, range, outside, reserved;
};
// What writing a receiver needs: kept in registers, computed by receiver_setup (gv_receivers.hip) in both launches.
struct ReceiverRow {
    int32_t X[8], Y[8];     // step 4's snapped corners (read only where `edges` is not 0)
    uint32_t depth_bits;    // the word it writes: d, or +0.0f of a record behind L
    uint32_t edges;         // occluder_edges: bits 0-11 active, 12-23 reversed; 0: every pixel of the range is written (flat, behind, range)
    uint32_t xr, yr;        // x0 | x1 << 16, y0 | y1 << 16: the pixel range of step 5, or the whole mask
};

struct ReceiverLaunch {
    const uint32_t* count;  // device draw count of the source view
    const uint32_t* idx;    // its records in delivery order: POOL slots
    const float* model;     // ... and their bakedModel, 12 floats each
    uint32_t capacity;      // the occupancy the view was culled with: the host's bound of *count
    const float4* a;        // MeshMirror::a / b: the cull boxes by mirror entry
    const float2* b;
    const uint32_t* inv;    // pool slot -> mirror entry (NULL: the mirror is in pool order)
    uint32_t slots;         // slots inv covers / entries a and b cover: a record outside either takes the empty box and reads nothing
    uint32_t entries;
    float light[16];        // L
    uint32_t width, height;
    uint32_t* local;                // [capacity]: tiles of the listed receivers in front of record k inside its workgroup
    unsigned long long* base;       // [blocks + 1] block tile totals (setup) -> items in front of the block, then the total (scan)
    ReceiverCounts* counts;         // added to
    float* mask;                    // the image
};
hipError_t launch_receiver_setup(const ReceiverLaunch& launch, hipStream_t stream);
hipError_t launch_receiver_raster(const ReceiverLaunch& launch, hipStream_t stream);

}  // namespace gv
