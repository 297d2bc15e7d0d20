// Which work unit a workgroup of the linear-scan cull takes: the dispatch order. A unit is a 256-entry tile (cull_kernel) or a
// super-tile of K tiles (cull_hot_kernel). No HIP dependency: the kernels, launch_cull and tests/test_tile_order.py (a ctypes twin
// built with gcc) read this same text.
//
// One 32-bit word (CullArgs::xcd_run) names the order:
//   0        identity: workgroup b takes unit b (Hi-Z views, small pools);
//   R > 0    XCD runs of R units (frustum-only views): workgroups go round-robin over the 8 XCDs, and XCD x takes units
//            (8q + x)R .. (8q + x + 1)R - 1 for its q-th run, so each XCD streams contiguous stretches.
// Either is a bijection of [0, grid_for_tiles()) onto itself: each unit below S is taken exactly once, a workgroup whose unit is
// >= S leaves, and there are fewer than tile_order_surplus_bound() of those.
// (A third order, which spread a Hi-Z view's frustum over the whole dispatch - P stripes, workgroup b takes unit
// (b mod P) * ceil(S / P) + b / P, or b * s mod S - was measured and lost 10-30 us at 10 M entries: profiles/r33_cull_order.md.)
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define GV_TILE_ORDER_FN __host__ __device__ __forceinline__
#else
#define GV_TILE_ORDER_FN static inline
#endif

// run length for a pool of `tiles` tiles: every XCD gets at least 8 runs (no surplus workgroups to speak of)
GV_TILE_ORDER_FN uint32_t xcd_run_for_tiles(uint32_t tiles)
{
    return tiles >= 8u * 256u * 8u ? 256u : (tiles >= 8u * 32u * 8u ? 32u : 0u);
}

GV_TILE_ORDER_FN uint32_t tile_of_workgroup(uint32_t b, uint32_t run)
{
    if (run == 0)
        return b;
    const uint32_t xcd = b & 7u, k = b >> 3;
    return ((k / run) * 8u + xcd) * run + k % run;
}

// grid size for `units` units under that mapping: whole groups of 8 runs (surplus workgroups exit at once)
GV_TILE_ORDER_FN uint32_t grid_for_tiles(uint32_t units, uint32_t run)
{
    const uint32_t group = run * 8u;
    return run ? (units + group - 1u) / group * group : units;
}

// grid_for_tiles(units, run) - units is below this
GV_TILE_ORDER_FN uint32_t tile_order_surplus_bound(uint32_t run)
{
    return run ? run * 8u : 1u;
}
