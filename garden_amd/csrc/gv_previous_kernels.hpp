// gv_previous_kernels.hpp — launch interface of gv_previous.hip: gv_pool_keep_models / gv_pool_forget_models / gv_pool_emit_previous,
// last frame's mvp per draw for motion vectors. Kept apart from gv_kernels.hpp like gv_delta_kernels.hpp.
#pragma once
#include "gv_kernels.hpp"

namespace gv {

constexpr uint32_t kPreviousBlock = 256;      // lanes per workgroup of all three launches (literals: the tests read them from this text)
constexpr uint32_t kPreviousEmitTiles = 4;    // tiles of kPreviousBlock records a previous_emit_kernel workgroup takes: one atomic per 1024 records
constexpr uint32_t kPreviousRowBytes = 64;    // a history row: one aligned 64-byte access both ways
constexpr uint32_t kPreviousRowPieces = 4;    // ... as 16-byte pieces: model words 0-11 in pieces 0-2, piece 3 = {stamp, 0, 0, 0}
constexpr uint32_t kPreviousStampWord = 12;   // the row's stamp; words 13-15 are 0
constexpr uint32_t kMinPreviousStride = 64;   // GvPreviousLayout::stride: a multiple of 16 in [64, 256]
constexpr uint32_t kMaxPreviousStride = 256;
static_assert(kPreviousRowBytes == 16 * kPreviousRowPieces && kPreviousStampWord * 4 == 48, "three pieces of model, one of stamp");
static_assert(kPreviousBlock % 64 == 0, "whole waves");

// The records of a view as delivered, and the pool's history (PoolState::Models). Every read of a record stays below
// min(*count, capacity); every access of a row below `slots`.
struct PreviousView {
    const uint32_t* count;   // the device draw count n
    const uint32_t* idx;     // s_k
    const float* model;      // M_k, 12 floats each
    uint32_t capacity;       // the occupancy the view was culled with: the bound of n and of the grid
};
struct PreviousKeep {
    PreviousView view;
    float4* rows;            // [slots * 4]
    uint32_t slots;          // H.slots: a record slot at or beyond it is not kept (cannot happen: the host grows the coverage first)
    uint32_t epoch;          // the stamp written
};
struct PreviousEmit {
    PreviousView view;
    const float4* rows;      // NULL with slots == 0
    uint32_t slots;
    uint32_t epoch;          // a row is kept <=> slot < slots && stamp == epoch && epoch > 0 (0: every draw is fresh — a cut, an empty history)
    uint32_t report_epoch;   // counts[3]: the history's e whatever the flags
    float pvp[16];           // PVP: prev_view_proj, the kept view_proj, or the view's own under a cut
    float d[3];              // added to c3 of a fresh draw's model (zeros under a cut)
    uint8_t* dst;
    uint32_t capacity;       // items the target holds: items at or beyond it are not written
    uint32_t stride, prev_mvp, has_history;  // has_history kNoField: none
    uint32_t* counts;        // {n, kept draws, items written, e}; zeroed in front of the launch (kept is added into)
};

hipError_t launch_previous_keep(const PreviousKeep& launch, hipStream_t stream);
hipError_t launch_previous_emit(const PreviousEmit& launch, hipStream_t stream);
// stamps of rows [first, first + count) = 0 (the caller has clamped the range to the coverage; count > 0)
hipError_t launch_previous_forget(float4* rows, uint32_t first, uint32_t count, hipStream_t stream);

}  // namespace gv
