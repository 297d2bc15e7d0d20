// gv_ctx.hpp — the context behind the opaque GvCtx of include/garden_vis.h and the small host-side utilities shared
// by gv_mirror.cpp (AoS/columns -> device mirror) and gv_context.cpp (the C-ABI, per-frame dispatch, results).
#pragma once
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/garden_vis.h"
#include "gv_kernels.hpp"
#include "gv_group_kernels.hpp"
#include "gv_second_kernels.hpp"
#include "gv_bounds_kernels.hpp"
#include "gv_delta_kernels.hpp"
#include "gv_occluder_kernels.hpp"
#include "gv_receiver_kernels.hpp"
#include "gv_previous_kernels.hpp"
#include "gv_cluster_kernels.hpp"
#include "gv_cluster_second_kernels.hpp"
#include "gv_cluster_run_kernels.hpp"
#include "gv_cluster_cone_kernels.hpp"
#include "gv_cluster_lod_kernels.hpp"
#include "gv_workers.hpp"
#include "gv_dirty_ranges.hpp"


namespace gv {

template <typename T>
struct DeviceBuf {  // grow-only device allocation (scratch vectors grow, never shrink: mesh.cpp:377-395)
    T* ptr = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t n)
    {
        if (n <= cap)
            return hipSuccess;
        if (ptr)
            (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T));
        if (e == hipSuccess) {
            cap = n;
            // GV_DEBUG_POISON: fresh device memory is filled with a pattern instead of whatever (often zeros) the allocator hands
            // out, so that a kernel that reads what nobody wrote fails every time, not once in a long session
            static const bool poison = getenv("GV_DEBUG_POISON") != nullptr;
            if (poison) {  // (the fill must have landed before any stream touches the buffer: hipMemset alone may still be in flight)
                e = hipMemset(ptr, 0xCD, n * sizeof(T));
                if (e == hipSuccess)
                    e = hipDeviceSynchronize();
            }
        }
        return e;
    }
    // like reserve, but the first `keep` elements survive (pool growth: the mirror is appended to, not rebuilt);
    // capacity grows by half so that steady appends do not reallocate every frame
    hipError_t grow(size_t n, size_t keep, hipStream_t stream)
    {
        if (n <= cap)
            return hipSuccess;
        const size_t want = std::max(n, cap + cap / 2);
        T* fresh = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&fresh), want * sizeof(T));
        if (e != hipSuccess)
            return e;
        if (ptr && keep) {
            e = hipMemcpyAsync(fresh, ptr, std::min(keep, cap) * sizeof(T), hipMemcpyDeviceToDevice, stream);
            if (e == hipSuccess)
                e = hipStreamSynchronize(stream);
            if (e != hipSuccess) {
                (void)hipFree(fresh);
                return e;
            }
        }
        if (ptr)
            (void)hipFree(ptr);
        ptr = fresh;
        cap = want;
        return hipSuccess;
    }
    void release()
    {
        if (ptr)
            (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

template <typename T>
struct PinnedBuf {
    T* ptr = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t n)
    {
        if (n <= cap)
            return hipSuccess;
        if (ptr)
            (void)hipHostFree(ptr);
        ptr = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess)
            cap = n;
        return e;
    }
    hipError_t grow(size_t n, size_t keep)  // the caller has drained every async copy that reads this buffer
    {
        if (n <= cap)
            return hipSuccess;
        const size_t want = std::max(n, cap + cap / 2);
        T* fresh = nullptr;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&fresh), want * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess)
            return e;
        if (ptr && keep)
            memcpy(fresh, ptr, std::min(keep, cap) * sizeof(T));
        if (ptr)
            (void)hipHostFree(ptr);
        ptr = fresh;
        cap = want;
        return hipSuccess;
    }
    void release()
    {
        if (ptr)
            (void)hipHostFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

struct DirtyRange {
    uint32_t lo = UINT32_MAX, hi = 0;
    bool any() const { return lo < hi; }
    void add(uint32_t first, uint32_t count)
    {
        if (count == 0)
            return;
        lo = std::min(lo, first);
        // saturating: first + count must not wrap to a tiny `hi` (the mark would be dropped and the mirror go stale);
        // users clamp `hi` to the pool's occupancy
        hi = std::max(hi, (uint32_t)std::min<uint64_t>((uint64_t)first + count, UINT32_MAX));
    }
    void clear()
    {
        lo = UINT32_MAX;
        hi = 0;
    }
};

// One field of a bound pool: element i lives at ptr + i * stride. An AoS pool binds every field with the component
// stride and its offset folded into ptr; column (SoA) storage binds each field with its own array and element size.
struct Column {
    const uint8_t* ptr = nullptr;
    size_t stride = 0;
    const uint8_t* at(size_t i) const { return ptr + i * stride; }
    uint32_t u32(size_t i) const
    {
        uint32_t v;
        memcpy(&v, ptr + i * stride, 4);
        return v;
    }
    const float* f32(size_t i) const { return reinterpret_cast<const float*>(ptr + i * stride); }
    uint8_t u8(size_t i) const { return ptr[i * stride]; }
};

struct TransformBinding {
    Column entity, parent, position, scale, rotation, self_active, ancestors_active, model_with_ancestors;
    uint32_t occupancy = 0;
    const uint32_t* entity_to_transform = nullptr;
    uint32_t entity_capacity = 0;
    bool bound = false;
};

// What a piece of state derived from a pool's mirror (block boxes, sphere stream, emit seeds) was made from: the pool's epoch and the
// transform mirror's. Current when equal to the pair of the moment (gv_context.cpp cull_launch).
struct Stamp {
    uint64_t epoch = 0, xf_epoch = 0;
    bool operator==(const Stamp& o) const { return epoch == o.epoch && xf_epoch == o.xf_epoch; }
};

inline uint32_t blocks_of(uint32_t occupancy) { return (occupancy + kCullBlock - 1) / kCullBlock; }  // cull workgroups of a pool

// Behind the last copies that read a pinned staging / packet buffer: whoever rewrites the buffer next waits for THIS, not for the
// whole stream (the previous frame's cull may still be running: a scene in which something moves every frame would otherwise run
// host and device one after the other, 0.20 instead of 0.12 ms per frame at 10 M entities with ten movers, tools/moving_bench.py).
// The context has one for the mirror's staging arrays, packet buffers and the payload rows; the count and the geometry id mirror
// have one each: the context's may sit behind a payload copy that the very call which uploads them has just queued behind the
// frame's cull.
struct UploadFence {
    hipEvent_t event = nullptr;
    bool pending = false;
    hipError_t wait()
    {
        if (!pending)
            return hipSuccess;
        const hipError_t e = hipEventSynchronize(event);
        if (e == hipSuccess)
            pending = false;
        return e;
    }
    hipError_t record(hipStream_t stream)
    {
        hipError_t e = event ? hipSuccess : hipEventCreateWithFlags(&event, hipEventDisableTiming);
        if (e == hipSuccess)
            e = hipEventRecord(event, stream);
        if (e == hipSuccess)
            pending = true;
        return e;
    }
    void destroy()
    {
        if (event)
            (void)hipEventDestroy(event);
        event = nullptr;
        pending = false;
    }
};

// A side column of a pool on the device, one element per POOL SLOT (indexed by visible_idx; a re-order of the mirror does not
// concern it), kept by upload_slot_mirror (gv_mirror.cpp). T is the unit its buffers are counted in: bytes for the payload rows,
// words for the counts, the geometry ids and the LOD sizes (capacities grow by halves of what they were, in that unit).
template <typename T>
struct SlotMirror {
    uint32_t elem = sizeof(T);  // bytes of an element: 4 for counts and ids, the pitch for payload rows (set with it at the bind)
    uint32_t mirrored = 0;      // elements [0, mirrored) are on the device (0: everything is uploaded)
    DirtyRanges dirty;
    DeviceBuf<T> d_column;
    PinnedBuf<T> h_stage;       // the elements (and, behind them, the packet's slots) on their way up
    DeviceBuf<T> d_packet;
    void reset()                // rebound: everything is uploaded again
    {
        mirrored = 0;
        dirty.clear();
    }
    void release()              // (the caller has drained the stream)
    {
        d_column.release();
        h_stage.release();
        d_packet.release();
    }
};

struct PoolState {
    Column entity, is_enabled, aabb_min, aabb_max;
    RecordLayout record_layout{};  // gv_pool_set_record_layout (stride 0: none)
    struct RecordTarget {        // gv_pool_set_record_target: the caller's own array for a view's records
        uint8_t* host = nullptr;
        size_t bytes = 0;
    };
    RecordTarget record_target[GV_MAX_VIEWS];
    Column ready;              // gv_pool_bind_ready: per-slot ready count (ptr NULL: none, every slot counts 1)
    uint32_t ready_width = 0;  // 1 or 4 bytes
    uint32_t ready_count(size_t i) const { return !ready.ptr ? 1u : (ready_width == 4 ? ready.u32(i) : (uint32_t)ready.u8(i)); }
    std::vector<uint8_t> ready_many;  // per slot, kept by gather_meshes (empty without a column): kReadyLive for a candidate, and in
                                      // the low bits 1 when its ready count is above 1, 2 when it is above GV_MAX_DRAW_INSTANCES too
    static constexpr uint8_t kReadyLive = 4, kReadyLevel = 3;
    uint32_t ready_many_count = 0;    // ... and how many: such draws take several instances (gv_pool_emit_instances refuses them)
    uint32_t ready_over_count = 0;    // ... of those, above GV_MAX_DRAW_INSTANCES (flag 2 in ready_many): gv_pool_emit_draw_instances refuses them
    // gv_pool_set_instance_layout / gv_pool_emit_instances: buffers of their own, nothing a cull produced is touched
    struct Instances {
        GvInstanceLayout layout{};      // stride 0: none
        DeviceBuf<uint8_t> d_data;      // the library-owned target
        DeviceBuf<uint32_t> d_starts;   // [views + 1]
        PinnedBuf<uint8_t> h_data;      // staging of gv_pool_instances_fetch
        PinnedBuf<uint32_t> h_starts;
        // the last emission (views 0: none since the pool's last gv_cull)
        uint8_t* target = nullptr;      // d_data.ptr or the caller's device memory
        uint32_t capacity = 0;          // instances the target holds
        uint32_t views = 0;
        uint32_t listed[GV_MAX_VIEWS] = {};  // ... which, in the order listed (gv_pool_emit_draw_commands walks the same views)
        GvInstanceLayout emitted{};     // the layout it was made with
        uint32_t emitted_payload = 0;   // ... and the payload fields it wrote: (at, bytes) each
        uint32_t emitted_at[GV_MAX_PAYLOAD_FIELDS] = {}, emitted_bytes[GV_MAX_PAYLOAD_FIELDS] = {};
        // gv_pool_emit_draw_instances (a draw takes its ready count of instances): starts[] then holds instance starts
        uint32_t index_at = GV_NONE;       // gv_pool_set_instance_index_field: the uint32 "index within the draw"
        uint32_t emitted_index = GV_NONE;  // ... as the last emission wrote it (GV_NONE: it did not)
        bool draws = false;                // the last emission was a draw emission: the buffers below describe it
        DeviceBuf<uint32_t> d_first;       // first_instance[draw_starts[v] + k], one more word: the grand total
        DeviceBuf<uint32_t> d_draw_starts; // [views + 1]
        DeviceBuf<uint32_t> d_local, d_chunk_total;  // scratch between the two launches
        PinnedBuf<uint32_t> h_first;       // staging of gv_pool_draw_bases_fetch
        void release()                     // (the caller has drained the stream; so for every release() below)
        {
            d_data.release(), d_starts.release(), h_data.release(), h_starts.release(), d_first.release(), d_draw_starts.release();
            d_local.release(), d_chunk_total.release(), h_first.release();
        }
    } instances;
    // The ready column on the device, one uint32 per POOL SLOT (indexed by visible_idx like the payload rows; a re-order of the
    // mirror does not concern it): exists only once gv_pool_emit_draw_instances has been called for a pool with a ready column
    struct Counts : SlotMirror<uint32_t> {  // dirty: the pool's GV_DIRTY_MESH marks
        bool wanted = false;
        uint64_t sum = 0;                  // of the mirrored counts: the host's bound of a view's instances
        std::vector<uint32_t> held;        // what was uploaded, slot by slot (keeps `sum` exact under partial uploads)
        std::vector<uint32_t> over;        // the slots whose mirrored count is above GV_MAX_DRAW_INSTANCES (few, if any): a mark made
                                           // after the last sync may have put one there, which ready_over_count has not seen
        UploadFence staged;                // guards h_stage (its own: see UploadFence)
        void reset()                       // the column was rebound: everything is uploaded again
        {
            SlotMirror::reset();
            sum = 0;
            over.clear();
        }
        void release()                     // everything (SlotMirror::release(): the mirror alone, its fence stays)
        {
            SlotMirror::release();
            staged.destroy();
        }
    } counts;
    // gv_pool_bind_geometry: the geometry id column and the table it indexes. The ids on the device, one uint32 per POOL SLOT like
    // the counts above (indexed by visible_idx; a re-order of the mirror does not concern them): the mirror exists only once
    // gv_pool_emit_draw_commands has been called for a pool with an id column
    struct Geometry : SlotMirror<uint32_t> {  // dirty: GV_DIRTY_GEOMETRY and GV_DIRTY_MESH marks of the pool
        bool bound = false;                // a table is bound (with or without an id column)
        Column ids;                        // ptr NULL: none, every slot has id 0
        uint32_t width = 0;                // 1, 2 or 4 bytes
        uint32_t occupancy = 0;            // slots the column covers
        uint32_t id(size_t i) const
        {
            if (width == 4)
                return ids.u32(i);
            uint16_t v = 0;
            if (width == 2)
                memcpy(&v, ids.at(i), 2);
            return width == 2 ? (uint32_t)v : (uint32_t)ids.u8(i);
        }
        uint32_t table_count = 0;
        DeviceBuf<GvGeometry> d_table;     // re-uploaded on every bind
        bool wanted = false;
        UploadFence staged;                // guards h_stage (its own: see UploadFence)
        void release()                     // everything (SlotMirror::release(): the mirror alone)
        {
            SlotMirror::release();
            staged.destroy();
            d_table.release();
        }
    } geometry;
    // gv_pool_set_command_layout / gv_pool_emit_draw_commands: buffers of their own, no cull result or instance data is touched
    struct Commands {
        GvCommandLayout layout{};          // stride 0: none
        DeviceBuf<uint8_t> d_data;         // the library-owned target
        DeviceBuf<uint32_t> d_counts;      // command_counts[views]
        DeviceBuf<uint32_t> d_rank, d_chunk_total, d_draw_of, d_first_of;  // run mode's scratch
        PinnedBuf<uint8_t> h_data;         // staging of gv_pool_draw_commands_fetch
        PinnedBuf<uint32_t> h_counts;
        // the last emission (views 0: none since the pool's last gv_cull or instance emission)
        uint8_t* target = nullptr;         // d_data.ptr or the caller's device memory
        uint32_t capacity = 0;             // command positions the target holds
        uint32_t views = 0, stride = 0, region = 0;
        void release()
        {
            d_data.release(), d_counts.release(), d_rank.release(), d_chunk_total.release(), d_draw_of.release(), d_first_of.release();
            h_data.release(), h_counts.release();
        }
    } commands;
    // gv_pool_bind_clusters / gv_pool_cull_clusters: the tables as bound and the last call's commands, buffers of their own — no cull
    // result, no instance data and no per-draw command buffer (Commands above) is touched. Header-only: no other host source calls
    // gv_clusters.cpp but gv_cluster_runs.cpp, the run form, gv_cluster_cones.cpp, the normal-cone form, and gv_cluster_lods.cpp, the
    // level-of-detail form, which share its body (cull_clusters below).
    struct Clusters {
        bool bound = false;
        uint32_t range_count = 0, cluster_count = 0;
        uint32_t max_range = 0;            // the largest count of a bound range: the host's bound of a draw's candidates
        DeviceBuf<GvClusterRange> d_ranges;  // re-uploaded on every bind
        DeviceBuf<GvCluster> d_clusters;
        DeviceBuf<uint8_t> d_data;         // the library-owned target
        DeviceBuf<uint32_t> d_counts;      // [2 * GV_MAX_VIEWS]: commands per view, then clusters tested per view
        DeviceBuf<uint32_t> d_draw_geometry, d_draw_local, d_block_total, d_block_tested, d_totals, d_tile_count, d_tile_block;  // scratch of a call
        DeviceBuf<unsigned long long> d_survive;
        DeviceBuf<unsigned long long> d_link, d_head;  // gv_pool_cull_cluster_runs: a link and a head bit per candidate ...
        DeviceBuf<uint32_t> d_head_count;              // ... and the heads per tile
        // gv_pool_bind_cluster_cones (gv_cluster_cones.cpp): one cone per entry of the cluster table; dropped with the tables
        bool cones_bound = false;
        DeviceBuf<GvClusterCone> d_cones;
        // gv_pool_bind_cluster_lods (gv_cluster_lods.cpp): one LOD entry per entry of the cluster table; dropped with the tables
        bool lods_bound = false;
        DeviceBuf<GvClusterLod> d_lods;
        PinnedBuf<uint8_t> h_data;         // staging of gv_pool_cluster_commands_fetch
        PinnedBuf<uint32_t> h_counts;
        // the last call (views 0: none since the pool's last gv_cull, instance emission or gv_pool_bind_clusters)
        uint8_t* target = nullptr;         // d_data.ptr or the caller's device memory
        uint32_t capacity = 0;             // command positions the target holds
        uint32_t views = 0, stride = 0, region = 0;
        // what the second phase needs of the last call K1 beside what K1 left on the device: its arguments as launched, the host's
        // bound of its candidates, the pyramid every queried view named, and whether the geometry table or the command layout was
        // set again since (K1's kept ids may lie outside a new table)
        ClusterLaunch launch{};
        uint64_t candidate_bound = 0;
        uint32_t pyramid[kMaxInstanceViews] = {};
        bool rebound = false;
        // the last call was gv_pool_cull_cluster_cones (second_test non-NULL): its eyes, kept with the launch, and the test launch
        // the second phase enqueues in place of its own to apply the same conjunction (gv_cluster_cones.cpp: the sources of the
        // other forms name no cone launch)
        int (*second_test)(GvCtx* ctx, Clusters& K, const ClusterSecondLaunch& launch) = nullptr;
        float eyes[kMaxInstanceViews][4] = {};
        // ... or gv_pool_cull_cluster_lods: its LOD views, kept with the launch likewise (second_test tells which)
        GvClusterLodView lod_views[kMaxInstanceViews] = {};
        // gv_pool_cull_clusters_second_phase (gv_clusters_second.cpp): the last call's commands and scratch, buffers of their own —
        // nothing of K1 above is written. views 0: none since K1 (it ends wherever K1 ends, and at a new K1)
        struct Second {
            DeviceBuf<uint8_t> d_data;     // the library-owned target
            DeviceBuf<uint32_t> d_counts;  // [2 * GV_MAX_VIEWS]: commands per view, then pending clusters re-tested per view
            DeviceBuf<uint32_t> d_pending_count, d_pending_tile, d_kept_count, d_totals;  // scratch of a call
            DeviceBuf<unsigned long long> d_kept;
            PinnedBuf<uint8_t> h_data;     // staging of gv_pool_cluster_second_commands_fetch
            PinnedBuf<uint32_t> h_counts;
            uint8_t* target = nullptr;
            uint32_t capacity = 0;
            uint32_t views = 0, stride = 0, region = 0;
            void release()
            {
                d_data.release(), d_counts.release(), d_pending_count.release(), d_pending_tile.release(), d_kept_count.release(), d_totals.release();
                d_kept.release(), h_data.release(), h_counts.release();
            }
        } second;
        void release()
        {
            d_ranges.release(), d_clusters.release(), d_data.release(), d_counts.release(), d_draw_geometry.release(), d_draw_local.release();
            d_block_total.release(), d_block_tested.release(), d_totals.release(), d_tile_count.release(), d_tile_block.release(), d_survive.release();
            d_link.release(), d_head.release(), d_head_count.release(), d_cones.release(), d_lods.release();
            h_data.release(), h_counts.release(), second.release();
        }
    } clusters;
    // gv_pool_bind_lod / gv_pool_select_lods: the size column as bit patterns, one word per POOL SLOT like the ids above (the mirror
    // exists only once gv_pool_select_lods has been called for a pool with a size column), the table the base ids index, and the
    // selection made behind the pool's last instance emission
    struct Lod : SlotMirror<uint32_t> {  // dirty: GV_DIRTY_LOD and GV_DIRTY_MESH marks of the pool
        bool bound = false;                // a table is bound (with or without a size column)
        Column sizes;                      // ptr NULL: none, every slot has size 1
        uint32_t occupancy = 0;            // slots the column covers
        uint32_t table_count = 0;
        DeviceBuf<GvLodGeometry> d_table;  // re-uploaded on every bind
        bool wanted = false;
        UploadFence staged;                // guards h_stage (its own: see UploadFence)
        // the selection (views 0: none since the pool's last gv_cull or instance emission)
        uint32_t views = 0;
        DeviceBuf<uint32_t> d_draw_geometry;  // g_k of the listed views' draws, back to back
        DeviceBuf<uint32_t> d_level_counts;   // [GV_MAX_VIEWS * GV_MAX_LOD_LEVELS]
        PinnedBuf<uint32_t> h_draw_geometry, h_level_counts;  // staging of gv_pool_lods_fetch
        void release()                        // everything (SlotMirror::release(): the mirror alone)
        {
            SlotMirror::release();
            staged.destroy();
            d_table.release(), d_draw_geometry.release(), d_level_counts.release(), h_draw_geometry.release(), h_level_counts.release();
        }
    } lod;
    // gv_pool_view_bounds: the bounds of the listed views' draws, buffers of their own (nothing a cull produced is touched)
    struct Bounds {
        uint32_t items = 0;                   // of the last call (0: none since the pool's last gv_cull or second phase)
        DeviceBuf<BoundsPartial> d_partial;   // one row of keys per bounds_fold_kernel workgroup
        DeviceBuf<BoundsResult> d_out;        // GvViewBounds[GV_MAX_BOUNDS_ITEMS]
        PinnedBuf<BoundsResult> h_out;        // staging of gv_pool_view_bounds_fetch
        void release() { d_partial.release(), d_out.release(), h_out.release(); }
    } bounds;
    // gv_pool_view_delta: per channel the set of POOL slots its last call saw (the baseline, one bit per slot) and that call's answer.
    // HISTORY, not something made from the views: no cull, emission, sort, re-order or re-bind ends it (end_derived has no line for
    // it); only the drop call, the call's own commit and gv_destroy change it. Header-only: no other host source calls gv_delta.cpp.
    struct Delta {
        struct Channel {
            DeviceBuf<unsigned long long> d_set[2];  // d_set[held]: the baseline; the other one receives the next call's current set,
            uint32_t held = 0;                       // ... and the commit is the swap (a failed call has touched the spare only)
            uint32_t baseline_slots = 0;             // slots the baseline covers (0: empty — before the first call, after a drop)
            bool result = false;                     // the buffers below hold an answer
            uint32_t universe = 0;                   // U of that answer: the room of d_slots it may use
            DeviceBuf<uint32_t> d_slots;             // appeared at [0, a), vanished at [a, a + v)
            DeviceBuf<uint32_t> d_counts;            // {a, v, |C|, U}
            PinnedBuf<uint32_t> h_slots, h_counts;   // staging of gv_pool_view_delta_fetch (GvViewDelta points into it)
            void drop() { baseline_slots = 0, result = false, universe = 0; }
            void release() { d_set[0].release(), d_set[1].release(), d_slots.release(), d_counts.release(), h_slots.release(), h_counts.release(); }
        } channel[GV_MAX_DELTA_CHANNELS];
        DeviceBuf<DeltaTotals> d_totals;             // scratch between the count and the place launch (stream order: shared by the channels)
        void release()
        {
            for (Channel& c : channel)
                c.release();
            d_totals.release();
        }
    } delta;
    // gv_pool_keep_models / gv_pool_forget_models: the models a view delivered, one 64-byte row per POOL slot (12 floats verbatim, the
    // epoch they were kept at, three zero words). HISTORY like Delta above: no cull, emission, sort, group, re-order or re-bind ends it
    // (end_derived has no line for it); only those two calls and gv_destroy change it. Header-only: no other host source calls gv_previous.cpp.
    struct Models {
        DeviceBuf<float4> d_rows;          // [4 per slot]; rows at or beyond `slots` hold nothing anybody reads
        uint32_t epoch = 0;                // e: 0 = empty
        uint32_t slots = 0;                // H.slots: the coverage
        float view_proj[16] = {};          // of the view kept at epoch e, as given to its cull
        float camera_position[3] = {};
        void empty() { epoch = 0, slots = 0; }  // (the buffers stay)
        void release() { d_rows.release(); }
    } models;
    // gv_pool_emit_previous: the last answer, made from a view (ends under Ends::ViewsReplaced), buffers of its own
    struct Previous {
        bool result = false;               // the buffers below hold an answer of a view of the pool's last cull
        GvPreviousLayout emitted{};        // the layout it was made with
        uint8_t* target = nullptr;         // d_data.ptr or the caller's device memory
        uint32_t capacity = 0;             // items the target holds
        DeviceBuf<uint8_t> d_data;         // the library-owned target
        DeviceBuf<uint32_t> d_counts;      // {n, kept draws, items written, e}
        PinnedBuf<uint8_t> h_data;         // staging of gv_pool_previous_fetch
        PinnedBuf<uint32_t> h_counts;
        void release() { d_data.release(), d_counts.release(), h_data.release(), h_counts.release(); }
    } previous;
    // gv_pool_bind_occluders: the occluder boxes, mirrored as one 32-byte row per POOL SLOT (min in words 0-2, max in words 4-6; indexed
    // by visible_idx like the ids above): the mirror exists only once gv_pool_draw_occluders has been called for the pool
    struct Occluders : SlotMirror<uint8_t> {  // dirty: GV_DIRTY_OCCLUDER and GV_DIRTY_MESH marks of the pool
        Column box_min, box_max;           // ptr NULL: no binding
        uint32_t occupancy = 0;            // slots the columns cover
        bool wanted = false;
        UploadFence staged;                // guards h_stage (its own: see UploadFence)
        void release()                     // everything (SlotMirror::release(): the mirror alone)
        {
            SlotMirror::release();
            staged.destroy();
        }
    } occluders;
    // gv_pool_bind_payload / gv_pool_set_payload_layout: the component bytes an instance carries next to mvp, mirrored as one packed
    // row per POOL SLOT (never the mirror's order: the instance kernel indexes by the record's visible_idx, and a re-order of the
    // transform mirror does not concern it); read by gv_pool_emit_instances only
    struct Payload : SlotMirror<uint8_t> {  // dirty: GV_DIRTY_PAYLOAD and GV_DIRTY_MESH marks of the pool
        uint32_t count = 0;                        // fields (0: none bound)
        Column src[GV_MAX_PAYLOAD_FIELDS];         // read only inside upload_payload
        uint32_t bytes[GV_MAX_PAYLOAD_FIELDS] = {};
        uint32_t offset[GV_MAX_PAYLOAD_FIELDS] = {};  // of the field inside a row (fields back to back)
        uint32_t at[GV_MAX_PAYLOAD_FIELDS] = {GV_NONE, GV_NONE, GV_NONE, GV_NONE};  // destinations in the instance
        uint32_t pitch = 0;                        // 16, 32 or 64: a row never straddles a 64-byte boundary; elem while a payload is bound
        uint32_t occupancy = 0;
        bool any_destination() const
        {
            for (uint32_t f = 0; f < count; f++)
                if (at[f] != GV_NONE)
                    return true;
            return false;
        }
    } payload;
    uint8_t* is_visible = nullptr;  // write-back target (NULL: none), element i at is_visible + i * is_visible_stride
    size_t is_visible_stride = 0;
    uint32_t occupancy = 0;
    bool bound = false;
    bool need_full = false;
    uint32_t mapping = kMapGeneral;  // MeshMapping, chosen at full gather (kMapExact may only be demoted afterwards)
    DirtyRanges dirty;               // itemised (scattered enable / ready / AABB edits re-mirror what they touched)
    // spatial mirror order (empty = slot order): perm[j] = pool slot held by mirror entry j, inv = its inverse
    std::vector<uint32_t> perm, inv;
    uint64_t order_epoch = 0;    // bumped whenever the entry -> slot table changes (full build, appended slots, re-order): gv_pool_mirror_epoch
    DeviceBuf<uint32_t> d_orig;  // perm on the device: emit reports original pool slots
    DeviceBuf<uint32_t> d_inv;   // inv on the device: the device-side gather of dirty mesh ranges (upload_meshes_device)
    DirtyRange staging_stale;    // slots whose host staging entries lag behind the device (written by that path)
    DeviceBuf<uint32_t> d_index_map;  // gv_pool_set_index_map: pool slot -> the caller's global id (exchange shards)
    uint32_t index_map_count = 0;     // 0: none
    std::vector<uint32_t> h_index_map;  // the same table on the host (the mapped write-back of isVisible walks it)
    uint32_t index_map_wide = 0;        // entries of the table that name a slot of 2^28 or more (gv_pick cannot encode them)
    // gv_pool_set_result_mapping: results in the caller's WORLD numbering
    uint32_t result_flags = 0;          // GV_RESULTS_MAP_*
    uint8_t* visible_base = nullptr;    // GV_RESULTS_MAP_VISIBLE: byte of slot i -> visible_base + h_index_map[i] * visible_stride
    size_t visible_stride = 0;
    uint32_t visible_count = 0;
    // GV_CONFIG_BLOCK_BOUNDS: per-workgroup world boxes, valid for bounds_at
    DeviceBuf<float4> d_blk_lo, d_blk_hi;
    DeviceBuf<uint8_t> d_blk_dirty;  // one byte per block: holds an entry re-mirrored since the boxes (and seeds) were last current
    uint32_t small_streak = 0;       // syncs in a row that re-mirrored only a few entries of this pool (a pool that keeps changing a
                                     // little gets its boxes rebuilt once, then patched; one that keeps changing a lot goes without)
    bool patch_valid = false;        // every change of the mirror since then is recorded in d_blk_dirty (flat, exactly paired pools):
                                     // the next cull re-derives the flagged blocks instead of going without boxes
    // the sphere stream (MeshMirror::hot; flat, exactly paired pools), valid for hot_at; hot_patch_valid: every
    // change since then is flagged kDirtyHot in d_blk_dirty, so the next cull re-derives those blocks' entries
    DeviceBuf<float4> d_hot;
    Stamp hot_at;
    bool hot_patch_valid = false;
    bool recording() const { return patch_valid || hot_patch_valid; }  // some consumer wants this sync's changes flagged
    void stop_recording() { patch_valid = hot_patch_valid = false; }
    DeviceBuf<EmitSeed> d_seed;    // emit seeds (gv_kernels.hpp), valid for seed_at
    Stamp seed_at;
    DeviceBuf<uint32_t> d_kept;    // [2 alternating counters, 2 words of padding | list entries] of launch_cull_listed
    DeviceBuf<uint8_t> d_kept_flag;  // per list entry (Hi-Z views)
    uint32_t kept_parity = 0;      // which counter the next classify launch adds into
    uint32_t mirrored = 0, appended = 0;  // entries the mirror holds / of those, appended (unsorted) since the last full build
    uint64_t epoch = 1;         // bumped whenever this pool's mirror changes
    Stamp bounds_at, seen_at;   // seen_at: state at this pool's previous gv_cull
    bool changed_prev = false;  // ... and whether it had changed then too (dynamic pool)
    // device mirror + pinned staging
    DeviceBuf<float4> d_a;
    DeviceBuf<float2> d_b;
    DeviceBuf<uint32_t> d_link;
    PinnedBuf<float4> h_a;
    PinnedBuf<float2> h_b;
    PinnedBuf<uint32_t> h_link;
    void release()  // every buffer of the pool and of what is derived from it (the record targets are the caller's: gv_destroy)
    {
        d_a.release(), d_b.release(), d_link.release(), h_a.release(), h_b.release(), h_link.release();
        d_orig.release(), d_inv.release(), d_index_map.release();
        d_blk_lo.release(), d_blk_hi.release(), d_blk_dirty.release(), d_hot.release(), d_seed.release(), d_kept.release(), d_kept_flag.release();
        instances.release(), payload.release(), counts.release(), geometry.release(), commands.release(), lod.release(), bounds.release();
        delta.release(), occluders.release(), models.release(), previous.release(), clusters.release();
    }
};

struct ViewState {
    DeviceBuf<unsigned long long> mask;
    DeviceBuf<uint32_t> chunk_count, chunk_count2, chunk_offset, draw_count;
    uint32_t count_parity = 0;  // which totals buffer the next cull adds into (see launch_emit self_prefix)
    uint32_t stale_chunks[2] = {0, 0};  // entries of each totals buffer that may be non-zero right now
    // One turn of the totals behind a cull of `chunks` chunks whose self-prefixing emit is about to be launched: that emit leaves the
    // buffer the cull added into as it is and clears the other one, into which the next cull then adds. Returns how many entries of
    // the other one it must clear. (view_buffers() of this cull is taken BEFORE the turn.)
    uint32_t turn_totals(uint32_t chunks)
    {
        const uint32_t other = count_parity ^ 1u, clear = std::max(chunks, stale_chunks[other]);
        stale_chunks[other] = 0;
        stale_chunks[count_parity] = chunks;
        count_parity = other;
        return clear;
    }

    DeviceBuf<uint8_t> is_visible;        // mirror order, written by the cull
    DeviceBuf<uint8_t> vis_flags;         // ViewBuffers::vis_flags: which quarter-chunks of is_visible may hold a non-zero
    bool vis_flags_current = false;       // false: something other than the self-prefixing emit wrote is_visible since (or the
                                          // buffers are new): the flags are set to "may be non-zero" before the next emit
    DeviceBuf<uint8_t> is_visible_slots;  // pool-slot order, filled by gv_results_fetch of a large, spatially ordered pool
    DeviceBuf<uint32_t> visible_idx;
    DeviceBuf<float> baked_model, distance_sq;
    // gv_sort: alternate record set + radix-sort scratch (allocated on first use)
    DeviceBuf<uint32_t> alt_idx, sort_keys[2], sort_vals[2], sort_slots[2], sort_hist;
    DeviceBuf<float> alt_model, alt_dist;
    PinnedBuf<uint32_t> h_visible_idx, h_draw_count;
    PinnedBuf<float> h_baked_model, h_distance_sq;
    PinnedBuf<uint8_t> h_is_visible;
    PinnedBuf<uint8_t> h_records;    // results in the pool's record layout (gv_pool_results_records)
    DeviceBuf<uint8_t> d_records;    // ... packed on the device first for pools too large to publish directly
    // Delivery of the record structs (place_records in gv_results.cpp). A view goes: culled (records_fetched false) -> published by
    // the publish launch or the small-pool sort / fetched by the large path (records_fetched true: h_records holds this cull's records
    // once the stream has been waited for; records_staged true while a record target still has to receive them) -> staged copy done
    // (records_staged false: records_at holds them). A new cull, sort, layout, target or mapping starts over.
    bool records_fetched = false;
    uint8_t* records_at = nullptr;   // where the caller reads them: h_records, or the caller's array (gv_pool_set_record_target)
    bool records_staged = false;     // this view has a record target (never page-locked) that h_records has not been copied into yet
    uint32_t count_hint = 0xFFFFFFFFu;  // draw count of this view's previous fetch (unknown: none)
    bool ballots_current = false;    // `mask` holds this cull's ballot words (not after the one-launch cull + emit of a small pool)
    std::vector<uint32_t> instance_bases;  // gv_pool_results_instance_bases (built on request)
    uint32_t pool_id = 0, occupancy = 0;
    bool main_pass = false, emitted = false, valid = false;
    float view_proj[16] = {};  // GvView::view_proj of this view's cull (gv_pool_emit_instances multiplies the records' models by it)
    float planes[6][4] = {};   // ... and the planes that cull extracted from it, plane_count of them (gv_pool_cull_clusters tests with the same)
    uint32_t plane_count = 0;
    uint8_t use_hiz = 0;       // GvView::use_hiz of this view's cull: 0, or 1 + the pyramid slot it names (Context::pyramid_of)
    float camera_position[3] = {};  // GvView::camera_position likewise (gv_pool_keep_models keeps it, gv_pool_emit_previous takes the difference)
    // fused cull + emit (launch_cull_emit): look-back words, ticket counter and their running epoch / base
    DeviceBuf<unsigned long long> tile_status;
    DeviceBuf<uint32_t> tile_ticket;
    uint32_t tile_ticket_base = 0, tile_epoch = 0;
    uint32_t sort_parity = 0;  // which of the two counter sets in sort_hist the next large sort uses (gv_sort.hip)
    size_t sort_set_words = 0; // size of one set as laid out in sort_hist (0: not initialised)
    DeviceBuf<uint16_t> sort_ranks;
    DeviceBuf<uint32_t> group_hist;  // gv_pool_group_draws: group and tile digit counts (gv_group_kernels.hpp; keys, pairs and ranks: the sort's scratch)
    DeviceBuf<unsigned long long> seen;  // gv_pool_cull_second_phase, the SECOND view's: one bit per mirror entry, set for the first view's records
    uint8_t sort_pending = 0;  // small pool: gv_sort asked for (1 ascending, 2 descending), not launched yet (flush_sorts)
    uint8_t sorted_dir = 0;    // the direction of the last gv_pool_sort since this view's cull (1 ascending, 2 descending; 0: none):
                               // what gv_merge_sorted asks of a member
    bool published = false;  // small pool: the host buffers already hold this view's results (gv_results_fetch of a sibling view)
    void release()
    {
        mask.release(), chunk_count.release(), chunk_count2.release(), chunk_offset.release(), draw_count.release();
        is_visible.release(), vis_flags.release(), is_visible_slots.release(), visible_idx.release(), baked_model.release(), distance_sq.release();
        alt_idx.release(), alt_model.release(), alt_dist.release(), sort_hist.release(), sort_ranks.release(), group_hist.release(), seen.release();
        for (int k = 0; k < 2; k++)
            sort_keys[k].release(), sort_vals[k].release(), sort_slots[k].release();
        h_visible_idx.release(), h_draw_count.release(), h_baked_model.release(), h_distance_sq.release(), h_is_visible.release();
        h_records.release(), d_records.release(), tile_status.release(), tile_ticket.release();
    }
};

struct PendingEvent {
    hipEvent_t start, stop;
    int kernel;
};


// Everything a context owns. The C-ABI's opaque `GvCtx` (a global-scope name) derives from it below.
struct Context {
    GvConfig config{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string error;

    // ---- transform pool: binding, change tracking, device mirror + pinned staging ----
    TransformBinding xf;
    bool xf_need_full = false;     // (re)build the whole mirror at the next sync
    bool xf_links_dirty = false;   // a ranged GV_DIRTY_HIERARCHY: parent links changed -> re-validate depth / cycles
    DirtyRanges xf_dirty;
    uint64_t xf_epoch = 1;         // bumped whenever the transform mirror changes
    uint32_t xf_mirrored = 0, xf_appended = 0;  // as PoolState::mirrored / appended, for the transform pool
    uint32_t max_depth = 0;        // longest parent chain in the mirror
    DeviceBuf<XfAB> d_xab;         // {pos|scale.x, quat} per entry
    DeviceBuf<float2> d_xc;
    DeviceBuf<uint8_t> d_xflags;
    DeviceBuf<unsigned long long> d_xactive;  // bit-plane of kXfActive, derived on the device
    DeviceBuf<uint32_t> d_xparent;
    PinnedBuf<XfAB> h_xab;
    PinnedBuf<float2> h_xc;
    PinnedBuf<uint8_t> h_xflags;
    PinnedBuf<uint32_t> h_xparent;
    // spatial mirror order of the transform pool (empty = slot order)
    std::vector<uint32_t> xperm, xinv;
    DeviceBuf<uint32_t> d_xinv;    // slot -> mirror entry (gv_get_world, device-side gather)
    // device-side gather of dirty AoS ranges
    DeviceBuf<uint8_t> d_raw;      // raw component bytes of the dirty slot range
    PinnedBuf<uint8_t> h_raw[2];   // the library's own pinned chunks the span travels through (double-buffered)
    hipEvent_t raw_done[2] = {nullptr, nullptr};  // chunk buffer k may be rewritten once its last copy has run
    DirtyRange staging_stale;      // slots whose host staging entries lag behind the device (written by that path)
    UploadFence uploads;           // guards the pinned staging arrays, the packet buffers and the payload rows' staging
    PinnedBuf<uint32_t> h_ranges;  // a sync's dirty ranges on their way to mark_dirty_blocks_kernel
    DeviceBuf<uint32_t> d_ranges;
    DeviceBuf<uint32_t> d_e2t;     // entity -> transform slot table on the device, refreshed by every device-side mesh gather
    DeviceBuf<uint32_t> d_flag;    // one word: "a candidate no longer pairs with its own index" (aos_meshes_kernel)
    PinnedBuf<uint32_t> h_flag;
    // scratch of the scattered (dirty-range) host upload path
    PinnedBuf<XfPacket> sc_xf;       // one packet of {entry, record} per sync and side (gv_sort_kernels.hpp)
    DeviceBuf<XfPacket> dsc_xf;
    PinnedBuf<MeshPacket> sc_mesh;
    DeviceBuf<MeshPacket> dsc_mesh;
    DeviceBuf<float4> dsc_a;         // device scratch of gv_get_world (the gathered matrices of a permuted mirror) ...
    DeviceBuf<float2> dsc_c;         // ... and of gv_debug_stream_peak (its sink)
    DeviceBuf<unsigned long long> d_pick_keys;  // gv_pick: one key per ray (its own: no cull buffer is touched)
    PinnedBuf<unsigned long long> h_pick_keys;

    // gv_merge_sorted (gv_merge.cpp): one result slot per group id; buffers of their own, no member's result is touched
    struct MergeSlot {
        bool valid = false;             // merged since the last gv_cull of any member pool
        uint32_t pools = 0;             // bit p: pool p is a member
        uint32_t items = 0, stride = 0;
        uint8_t* target = nullptr;      // d_records.ptr or the caller's device memory
        uint32_t capacity = 0;          // records the target holds
        DeviceBuf<uint8_t> d_records;   // the library-owned target
        DeviceBuf<uint32_t> d_counts;   // [items + 1]
        PinnedBuf<uint8_t> h_records;   // staging of gv_merge_fetch
        PinnedBuf<uint32_t> h_counts;
        void release() { d_records.release(), d_counts.release(), h_records.release(), h_counts.release(); }
    } merges[GV_MAX_MERGE_GROUPS];

    PoolState pools[GV_MAX_POOLS];
    // results are kept per (pool, view): every mesh system's cull can be issued before the first result is read
    // (gv_pool_results_fetch ...); the view-indexed entry points address the pool of the most recent gv_cull
    ViewState views[GV_MAX_POOLS][GV_MAX_VIEWS];
    uint32_t last_pool = 0;

    // ---- a tick of engine-sized pools (gv_cull_batch_begin): culls recorded, launched together at the first read ----
    struct CullJob {
        uint32_t pool_id, view_count;
        ViewParams vps[GV_MAX_VIEWS];
    };
    bool cull_batching = false;
    std::vector<CullJob> cull_jobs;
    PinnedBuf<uint8_t> h_tick[2];  // descriptor tables on their way to d_tick (double-buffered: the host may run ahead)
    hipEvent_t tick_done[2] = {nullptr, nullptr};
    uint32_t tick_turn = 0;
    DeviceBuf<uint8_t> d_tick;

    // ---- world-matrix cache (gv_sweep) ----
    DeviceBuf<float4> d_world;
    bool world_valid = false;          // d_world holds the world matrices of the current mirror, except ...
    bool world_partial = false;        // ... for the chains through entries flagged in d_xdirty (subtree-scoped sweep)
    bool xdirty_set = false;           // some flag in d_xdirty may be 1
    DeviceBuf<uint8_t> d_xdirty;       // 1 byte per transform mirror entry: re-mirrored since the cache was brought up to date
    bool sweep_with_cull = false;      // GV_SWEEP_WITH_CULL[_VALU] requested: the next gv_cull also writes the world matrices
    bool sweep_with_cull_mfma = true;  // ... with the MFMA or the VALU chain

    // ---- block bounds (GV_CONFIG_BLOCK_BOUNDS) statistics ----
    DeviceBuf<uint8_t> d_examined;     // of the LAST bounded cull: 1 byte per workgroup
    uint64_t bounds_blocks_total = 0;

    // ---- Hi-Z ----
    DeviceBuf<float> d_depth;
    const float* depth_ptr = nullptr;  // d_depth.ptr or caller's device memory
    DeviceBuf<float2> d_mips;
    DeviceBuf<uint64_t> d_mip_offset;
    uint32_t hiz_w = 0, hiz_h = 0, hiz_mips = 0;
    uint32_t mip_w[GV_MAX_MIPS]{}, mip_h[GV_MAX_MIPS]{};
    uint64_t mip_off[GV_MAX_MIPS]{};
    bool hiz_valid = false;
    bool hiz_nested = false;           // every level bounds all the texels it covers (see HizDevice::nested)
    PinnedBuf<uint32_t> h_done;  // the word the done-flag kernel writes (wait_for_stream)
    uint32_t done_seq = 0;
    bool publish_sync_pending = false;  // a small-pool sort has published its views; nobody has synchronised the stream since
    bool hiz_level1_virtual = false;   // decided in gv_hiz_build: sizes whose first six levels take the fused kernel
    bool hiz_level1_stored = false;    // ... and whether gv_hiz_read_level has materialised it since the last build

    // ---- pyramid slots (gv_hiz_select): the fields above are the SELECTED pyramid — what gv_hiz_build, _rebuild, _read_level and
    // _mip_count address. Every other slot's pyramid rests here; gv_hiz_select swaps (pointer moves, no device work). A view names
    // its pyramid by index (GvView::use_hiz); hiz_device(ctx, k) resolves it at the launch, whichever slot is selected then.
    struct HizParked {
        DeviceBuf<float> d_depth;
        const float* depth_ptr = nullptr;
        DeviceBuf<float2> d_mips;
        DeviceBuf<uint64_t> d_mip_offset;
        uint32_t hiz_w = 0, hiz_h = 0, hiz_mips = 0;
        uint32_t mip_w[GV_MAX_MIPS]{}, mip_h[GV_MAX_MIPS]{};
        uint64_t mip_off[GV_MAX_MIPS]{};
        bool hiz_valid = false, hiz_nested = false, hiz_level1_virtual = false, hiz_level1_stored = false;
        bool holds_anything() const { return d_depth.ptr || d_mips.ptr || d_mip_offset.ptr || depth_ptr; }  // false: never built, or dropped
        void release() { d_depth.release(), d_mips.release(), d_mip_offset.release(); }  // (the caller has drained the stream)
    } parked[GV_MAX_PYRAMIDS];         // parked[selected] is empty: that pyramid is in the live fields
    uint32_t selected = 0;
    HizParked hiz_live() const         // the live fields in the parked form (pointers and sizes: nothing is moved)
    {
        HizParked k;
        k.d_depth = d_depth, k.depth_ptr = depth_ptr, k.d_mips = d_mips, k.d_mip_offset = d_mip_offset;
        k.hiz_w = hiz_w, k.hiz_h = hiz_h, k.hiz_mips = hiz_mips;
        memcpy(k.mip_w, mip_w, sizeof(mip_w)), memcpy(k.mip_h, mip_h, sizeof(mip_h)), memcpy(k.mip_off, mip_off, sizeof(mip_off));
        k.hiz_valid = hiz_valid, k.hiz_nested = hiz_nested, k.hiz_level1_virtual = hiz_level1_virtual, k.hiz_level1_stored = hiz_level1_stored;
        return k;
    }
    HizParked hiz_slot(uint32_t k) const { return k == selected ? hiz_live() : parked[k]; }  // slot k's state, selected or parked
    HizParked hiz_take_live()          // ... and the live fields are left empty ("not built")
    {
        const HizParked k = hiz_live();
        hiz_put_live(HizParked{});
        return k;
    }
    void hiz_put_live(const HizParked& k)
    {
        d_depth = k.d_depth, depth_ptr = k.depth_ptr, d_mips = k.d_mips, d_mip_offset = k.d_mip_offset;
        hiz_w = k.hiz_w, hiz_h = k.hiz_h, hiz_mips = k.hiz_mips;
        memcpy(mip_w, k.mip_w, sizeof(mip_w)), memcpy(mip_h, k.mip_h, sizeof(mip_h)), memcpy(mip_off, k.mip_off, sizeof(mip_off));
        hiz_valid = k.hiz_valid, hiz_nested = k.hiz_nested, hiz_level1_virtual = k.hiz_level1_virtual, hiz_level1_stored = k.hiz_level1_stored;
    }
    // GvView::use_hiz -> the pyramid it names: 1 + k for k < GV_MAX_PYRAMIDS; any larger value means pyramid 0, as every non-zero value once did
    static uint32_t pyramid_of(uint8_t use_hiz) { return use_hiz >= 1 && use_hiz <= GV_MAX_PYRAMIDS ? use_hiz - 1u : 0u; }
    bool pyramid_built(uint32_t k) const { return k == selected ? hiz_valid : parked[k].hiz_valid; }
    // Some pyramid — the selected one or a parked one — reads `image` as its level 0 (a pyramid built from a device image READS it).
    bool pyramid_reads(const float* image) const
    {
        if (!image)
            return false;
        bool reads = depth_ptr == image;
        for (const HizParked& k : parked)
            reads = reads || k.depth_ptr == image;
        return reads;
    }
    // The image a begin takes, of a set of kHizImages: `current` unless some pyramid reads it; then the lowest-index image that no
    // pyramid reads (one always exists: GV_MAX_PYRAMIDS pyramids read at most that many of the GV_MAX_PYRAMIDS + 1 images). With
    // pyramid 0 alone in use these are images 0 and 1 in turn.
    static constexpr uint32_t kHizImages = GV_MAX_PYRAMIDS + 1;
    uint32_t free_image(const DeviceBuf<float> (&images)[kHizImages], uint32_t current) const
    {
        if (!pyramid_reads(images[current].ptr))
            return current;
        for (uint32_t i = 0; i < kHizImages; i++)
            if (!pyramid_reads(images[i].ptr))
                return i;
        return current;  // (not reached)
    }

    // ---- occluder depth (gv_occluders.cpp): GV_MAX_PYRAMIDS + 1 images, allocated at first use, so that one a pyramid reads
    // (depth_ptr: level 0 IS the depth image) is never cleared, redrawn or reallocated under it (free_image). Accumulated state like
    // the delta baselines: end_derived has no line for it.
    struct OccluderDepth {
        DeviceBuf<float> d_image[kHizImages];
        uint32_t current = 0;              // the image of the last gv_occluder_begin
        uint32_t width = 0, height = 0;    // ... and its size (0: no begin yet)
        bool open = false;                 // begun and not built since: draws go into it
        DeviceBuf<OccluderCounts> d_counts;
        PinnedBuf<OccluderCounts> h_counts;  // staging of gv_occluder_depth_fetch
        PinnedBuf<float> h_image;
        // scratch of a draw, shared by all pools (stream order)
        DeviceBuf<uint32_t> d_local;
        DeviceBuf<unsigned long long> d_base;
        void release()
        {
            for (auto& image : d_image)
                image.release();
            d_counts.release(), h_counts.release(), h_image.release();
            d_local.release(), d_base.release();
        }
    } occluder_depth;

    // ---- receiver mask (gv_receivers.cpp): GV_MAX_PYRAMIDS + 1 images of its own, by the same rule — one a pyramid reads is never
    // cleared, redrawn or reallocated under it. Accumulated state like the occluder images: end_derived has no line for it. A draw's
    // scratch is occluder_depth.d_local / d_base: every user is ordered on the one stream.
    struct ReceiverMask {
        DeviceBuf<float> d_image[kHizImages];
        uint32_t current = 0;              // the image of the last gv_receiver_begin
        uint32_t width = 0, height = 0;    // ... and its size (0: no begin yet)
        bool open = false;                 // begun and not built since: draws go into it
        DeviceBuf<ReceiverCounts> d_counts;
        PinnedBuf<ReceiverCounts> h_counts;  // staging of gv_receiver_mask_fetch
        PinnedBuf<float> h_image;
        void release()
        {
            for (auto& image : d_image)
                image.release();
            d_counts.release(), h_counts.release(), h_image.release();
        }
    } receiver_mask;

    // ---- multi-GPU exchange (gv_exchange.cpp) ----
    void* exchange_comm = nullptr;     // ncclComm_t
    int exchange_rank = 0, exchange_world = 1;
    uint32_t exchange_mode = GV_EXCHANGE_ALLGATHER;  // GvExchangeMode
    DeviceBuf<uint32_t> d_shard;       // [count, indices...] of this rank
    // gv_exchange_visible: library-owned rows, sized from the previous frame's headers, completed when a list outgrew its room
    struct ExchangeSlot {
        DeviceBuf<uint32_t> rows;      // [world][row_words]
        DeviceBuf<uint32_t> shard;     // this rank's WHOLE [count, indices ...] of the slot's frame: the first exchange reads its leading
                                       // 1 + room[me] words, a completing exchange the tail behind them (both on exchange_stream)
        hipEvent_t produced = nullptr; // on ctx->stream behind the shard copy: exchange_stream waits for it
        hipEvent_t done = nullptr;     // on exchange_stream behind collective + headers (+ tails): GvExchangeFrame::ready_event
        // GV_EXCHANGE_PEER (gv_exchange_init_peers): `sent` on this rank's exchange stream behind its stores into everybody's rows;
        // on rank 0's exchange stream — the hub — `all_produced` behind every rank's `produced` (nobody still reads the rows about to
        // be overwritten) and `all_sent` behind every rank's `sent` (every row has arrived everywhere)
        hipEvent_t sent = nullptr, all_produced = nullptr, all_sent = nullptr;
        PinnedBuf<uint32_t> hdr;       // [1] sequence word + [world][hdr_words] leading words of every row, written by exchange_headers_kernel
        uint32_t hdr_words = 1;        // 1 (the count header) + the lists of a gv_exchange_views frame
        uint32_t items = 0;            // gv_exchange_views: lists per rank in this slot's frame (0: a single-list frame)
        std::vector<uint32_t> item_counts;  // settled: [world][items] per-list counts (GvExchangeFrame::item_counts)
        PinnedBuf<ShardItem> h_items;  // the frame's list descriptors on their way to d_items
        DeviceBuf<ShardItem> d_items;
        std::vector<ShardItem> items_uploaded, items_wanted;  // what d_items holds (empty: unknown) / this frame's descriptors
        uint32_t row_words = 0;
        uint32_t room[GV_EXCHANGE_MAX_RANKS] = {};        // list entries rank r's row was predicted to need in this slot's frame
        uint32_t travelled[GV_EXCHANGE_MAX_RANKS] = {};   // words of row r on the links in the first exchange
        uint32_t counts[GV_EXCHANGE_MAX_RANKS] = {};      // settled: the frame's own headers
        uint32_t tail_words[GV_EXCHANGE_MAX_RANKS] = {};  // settled: what the completing exchange carried
        uint64_t cut = 0;              // settled: ranks whose list outgrew its room
        uint64_t frame = 0;
        uint32_t mode = 0;
        bool in_flight = false;        // sent; its headers have not been read yet
        bool settled = false;          // headers read, rooms updated, tails delivered: the rows are complete behind `done`
    } exchange_slots[2];
    hipStream_t exchange_stream = nullptr;              // EVERY collective of the communicator runs here (one communicator, one stream): the next frame's cull (ctx->stream) does not wait for the links
    hipEvent_t exchange_in = nullptr, exchange_out = nullptr;  // hand-over events of the caller-owned forms (gv_exchange_shards / _masks)
    uint64_t exchange_frame = 0;                        // the next frame's number
    uint32_t exchange_room[GV_EXCHANGE_MAX_RANKS] = {};  // room the next frame gives each rank
    uint32_t exchange_timeout_ms = 30000;               // bound of every host wait of the exchange (gv_exchange_set_timeout)
    bool exchange_broken = false;                       // a wait ran out: the communicator is aborted, not destroyed
    bool exchange_by_group = false;                     // made by gv_exchange_init_all / _init_peers: driven through the *_all forms only
    std::vector<GvCtx*> exchange_peers;                 // gv_exchange_init_peers: the group's contexts by rank (empty: a communicator, or nothing)

    // ---- profiling ----
    std::vector<PendingEvent> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> free_events;
    GvStats stats{};
    uint32_t profile_every = 1;                      // gv_profile_sampling
    uint32_t profile_mask = 0;                       // bit k: launches of GvKernelId k are bracketed (gv_create from the config flags; gv_profile_kernels)
    uint64_t profile_seen[GV_K_COUNT] = {}, profile_timed[GV_K_COUNT] = {};

    int fail(int code, const char* fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        error = buf;
        return code;
    }
    int hip_fail(hipError_t e, const char* what)
    {
        return fail(e == hipErrorOutOfMemory ? GV_E_OOM : GV_E_HIP, "%s: %s", what, hipGetErrorString(e));
    }
};

}  // namespace gv

struct GvCtx final : gv::Context {};


#define GV_HIP(ctx, call)                                   \
    do {                                                    \
        hipError_t e__ = (call);                            \
        if (e__ != hipSuccess)                              \
            return (ctx)->hip_fail(e__, #call);             \
    } while (0)

namespace gv {

// roctx ranges named after the reference's profiler zones (SET_CPU_ZONE_SCOPED / SET_GPU_DEBUG_LABEL:
// "Meshes Prepare" source/system/render/mesh.cpp:334, "Meshes Sort" :267, "HiZ Downsample" hiz.cpp:146), so a
// rocprofv3 --marker-trace timeline reads like the engine's Tracy capture.
struct ZoneScope {
    explicit ZoneScope(const char* name) { roctxRangePushA(name); }
    ~ZoneScope() { roctxRangePop(); }
};

// ---- profiling events ----
struct KernelTimer {
    GvCtx* ctx;
    int kernel;
    hipEvent_t start = nullptr, stop = nullptr;
    bool on = false;
    KernelTimer(GvCtx* c, int k) : ctx(c), kernel(k)
    {
        ctx->stats.launches[k]++;
        if (!((ctx->profile_mask >> k) & 1u))
            return;
        if (ctx->profile_seen[k]++ % ctx->profile_every != 0)  // gv_profile_sampling
            return;
        if (!ctx->free_events.empty()) {
            start = ctx->free_events.back().first;
            stop = ctx->free_events.back().second;
            ctx->free_events.pop_back();
        } else if (hipEventCreate(&start) != hipSuccess || hipEventCreate(&stop) != hipSuccess) {
            return;
        }
        on = hipEventRecord(start, ctx->stream) == hipSuccess;
        if (on)
            ctx->profile_timed[k]++;
    }
    ~KernelTimer()
    {
        if (!on)
            return;
        (void)hipEventRecord(stop, ctx->stream);
        ctx->pending.push_back({start, stop, kernel});
    }
};

// one launch, counted (and bracketed, when profiling asks for it) as kernel `k`; a failure returns like GV_HIP
#define GV_LAUNCH(ctx, k, call) do { gv::KernelTimer timer__((ctx), (k)); GV_HIP((ctx), call); } while (0)

// host worker threads for the gathers (AoS component pools -> SoA staging) and the isVisible write-back: gv_workers.hpp

// ---- derived results: what is made from a view's delivered records and kept per pool (PoolState::instances, commands, lod, bounds)
// or per group (Context::merges) ----

// When a derived result ends. The table, stated once:
//     views     -> {instances, bounds, previous, merges the pool is a member of}
//     instances -> {commands, cluster commands, selection}
//     cluster commands -> {second-phase cluster commands}   (also ended by gv_pool_bind_clusters and a new gv_pool_cull_clusters)
// A result ends when what it was made from is replaced. A new derived result is one more line here, under what it is made from.
// PoolState::delta (gv_pool_view_delta) has NO line: its baseline is history — the set a channel saw at its last call, kept in pool
// slot numbers so that neither a cull nor a re-order of the mirror concerns it — and its answer is self-contained slot numbers that
// stay true whatever replaces the views. Both live until the channel's next call, its drop call or gv_destroy.
// Context::occluder_depth (gv_pool_draw_occluders) has NO line either: the image is accumulated over the draws of several pools and
// views since gv_occluder_begin, and what it holds — depths of boxes as they stood when they were drawn — is not made any less true by
// a later cull. It lives until the begin that takes it again (never the image the current pyramid reads) or gv_destroy.
// Context::receiver_mask (gv_pool_draw_receivers) likewise: accumulated since gv_receiver_begin, ended by nothing but the next begin.
// PoolState::models (gv_pool_keep_models) has NO line: last frame's models by pool slot are history exactly as the delta baselines are.
// PoolState::previous (gv_pool_emit_previous), the answer made from a view and that history, HAS one: it ends with the view.
enum class Ends {
    ViewsReplaced,     // gv_cull, gv_pool_cull_second_phase: the views' results are replaced
    EmissionReplaced,  // gv_pool_emit_instances, gv_pool_emit_draw_instances: the instance data is replaced
    SelectionDropped,  // gv_pool_select_lods(NULL, 0), gv_pool_bind_lod without a table
};
static inline void end_derived(GvCtx* ctx, PoolState& p, Ends cause)
{
    switch (cause) {
    case Ends::ViewsReplaced:
        p.instances.views = 0;
        p.bounds.items = 0;
        p.previous.result = false;
        for (auto& m : ctx->merges)
            if ((m.pools >> (uint32_t)(&p - ctx->pools)) & 1u)
                m.valid = false;
        [[fallthrough]];  // the instances have ended, and with them:
    case Ends::EmissionReplaced:
        p.commands.views = 0;
        p.clusters.views = 0;
        p.clusters.second.views = 0;  // the second phase of the cluster cull reads what that cull left
        [[fallthrough]];
    case Ends::SelectionDropped:
        p.lod.views = 0;
    }
}

// What the readers of a view's records check alike (`fn`: the entry point's name, as it appears in the message).
// The pool, when it is bound; NULL with the message set otherwise (GV_E_ARG).
static inline PoolState* bound_pool(GvCtx* ctx, const char* fn, uint32_t pool_id)
{
    if (pool_id < GV_MAX_POOLS && ctx->pools[pool_id].bound)
        return &ctx->pools[pool_id];
    ctx->fail(GV_E_ARG, "%s: pool %u is not bound", fn, pool_id);
    return nullptr;
}
// The views of the pool's last gv_cull: its leading valid ones.
static inline uint32_t culled_views(const GvCtx* ctx, uint32_t pool_id)
{
    uint32_t culled = 0;
    while (culled < GV_MAX_VIEWS && ctx->views[pool_id][culled].valid)
        culled++;
    return culled;
}
// A side column with one element per pool slot, when one is bound, must cover the slots a view was culled with: GV_E_STATE otherwise.
struct ColumnName { const char *subject, *verb, *hint; };
constexpr ColumnName kGeometryIds{"the geometry ids", "cover", ""}, kLodSizes{"the sizes", "cover", ""}, kReadyColumn{"the ready column", "covers", ""},
    kPayloadRows{"the payload", "covers", " (gv_pool_bind_payload)"}, kOccluderBoxes{"the occluder boxes", "cover", " (gv_pool_bind_occluders)"};
static inline int column_covers(GvCtx* ctx, const char* fn, const ColumnName& name, uint32_t pool_id, const Column& column, uint32_t covered,
                                const ViewState& vs, uint32_t view_index)
{
    if (!column.ptr || covered >= vs.occupancy)
        return GV_OK;
    return ctx->fail(GV_E_STATE, "%s: %s of pool %u %s %u of the %u slots view %u was culled with%s", fn, name.subject, pool_id, name.verb, covered,
                     vs.occupancy, view_index, name.hint);
}
// ... and its mirror (PoolState::counts, geometry, lod) is wanted from here on and brought up to date: the first use uploads the column,
// later ones the marks made since (upload: upload_counts, upload_geometry, upload_lod of gv_mirror.cpp). No column: no mirror.
template <typename Mirror>
static int want_column(GvCtx* ctx, PoolState& p, const Column& column, Mirror& mirror, int (*upload)(GvCtx*, PoolState&))
{
    if (!column.ptr)
        return GV_OK;
    mirror.wanted = true;
    return upload(ctx, p);
}
// The read pointers of a view's delivered records; the launch fillers copy what they need into their own kernel arguments.
struct ViewRecords { const uint32_t *count, *idx; const float *model, *dist; };
static inline ViewRecords records_of(const ViewState& vs) { return ViewRecords{vs.draw_count.ptr, vs.visible_idx.ptr, vs.baked_model.ptr, vs.distance_sq.ptr}; }

// Where an emission writes: the caller's device memory, clamped to the host's bound of the total, or the library's buffer, reserved
// for that bound (16 bytes at least). *capacity: the items of `stride` bytes the target holds.
static inline int choose_target(GvCtx* ctx, void* dst_device, size_t capacity_bytes, uint32_t stride, uint64_t bound, DeviceBuf<uint8_t>& own, uint8_t** target,
                         uint32_t* capacity)
{
    if (dst_device) {
        *target = static_cast<uint8_t*>(dst_device);
        *capacity = (uint32_t)std::min<uint64_t>({capacity_bytes / stride, bound, UINT32_MAX});
        return GV_OK;
    }
    GV_HIP(ctx, own.reserve(std::max<size_t>((size_t)bound * stride, 16)));
    *target = own.ptr;
    *capacity = (uint32_t)bound;
    return GV_OK;
}
// A fetch: `count` elements from the device into the result's pinned staging (reserved for `room` elements), waited for, and — `to`
// non-NULL — on into the caller's (pageable, never page-locked) array.
template <typename T>
static int fetch_staged(GvCtx* ctx, PinnedBuf<T>& stage, size_t room, const void* device, size_t count, void* to = nullptr)
{
    GV_HIP(ctx, stage.reserve(room));
    GV_HIP(ctx, hipMemcpyAsync(stage.ptr, device, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    GV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (to)
        memcpy(to, stage.ptr, count * sizeof(T));
    return GV_OK;
}

void drain_events(GvCtx* ctx);

// gv_exchange.cpp
void exchange_release(GvCtx* ctx);            // destroys the communicator, if any
int exchange_drain(GvCtx* ctx);    // bounded wait for what is queued on the exchange stream; a timeout aborts the communicator (GV_E_TIMEOUT)

// gv_context.cpp (the cull side)
int flush_culls(GvCtx* ctx);                             // launches the culls recorded since gv_cull_batch_begin; ends the batch
int flush_recorded_culls(GvCtx* ctx, uint32_t pool);    // ... those that read `pool` (GV_MAX_POOLS: any), recording goes on
ViewBuffers view_buffers(ViewState& vs);
// what gv_cull does per view in front of its launches, and the way out behind a cull that left ballot words and chunk totals
// (gv_pool_cull_second_phase, gv_second.cpp, sets its view up and emits it the same way)
int begin_view(GvCtx* ctx, ViewState& vs, uint32_t pool_id, const GvView& view, ViewParams* vp);  // buffers, the view's state as of a new cull, *vp
HizDevice hiz_device(const GvCtx* ctx);                    // of the selected pyramid
HizDevice hiz_device(const GvCtx* ctx, uint32_t pyramid);  // of pyramid `pyramid`, selected or parked (not built: all zero)
int emit_view(GvCtx* ctx, ViewState& vs, const MeshMirror& mesh, const TransformMirror& xf, const ViewParams& vp, const ViewBuffers& vb,
              bool self_prefix, const float4* emit_world, const EmitSeed* seeds);
// gv_results.cpp (the reader side)
int flush_sorts(GvCtx* ctx);                             // flush_culls + the sorts of small pools that were asked for and not launched yet
// a reorder of a view's records: inputs = its current records, outputs = its alternate set (reserved here), which swap_in_sorted
// makes the view's records once the reorder is enqueued (gv_pool_sort, gv_pool_group_draws)
int sort_records_of(GvCtx* ctx, ViewState& vs, SortRecords& r);
void swap_in_sorted(ViewState& vs);
int wait_for_stream(GvCtx* ctx);                         // until the stream has drained (a polled word; hipStreamSynchronize as fallback)
ViewState* view_of(GvCtx* ctx, uint32_t pool_id, uint32_t view_index);  // NULL: no valid results
bool release_record_target(PoolState::RecordTarget& target);            // false: the range was found unmapped
int copy_shard_of_pool(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, void* dst_device, uint32_t capacity, uint32_t index_base);

// gv_clusters.cpp
// The body of every form of the cluster cull (gv_pool_cull_clusters there, gv_pool_cull_cluster_runs in gv_cluster_runs.cpp,
// gv_pool_cull_cluster_cones in gv_cluster_cones.cpp, gv_pool_cull_cluster_lods in gv_cluster_lods.cpp): every check, the bound, the
// target, the shared scratch and the bookkeeping.
// `forms` holds per form what reserves the scratch the form adds and enqueues its launches — launch is complete, tiles = ceil(B /
// kClusterTile), eyes as below; `fn` names the entry point in messages. `allowed_flags`: the flag bits the entry point takes;
// GV_CLUSTERS_RUNS among them picks forms.runs. `cones` (NULL: the forms without the cone test): the caller's eyes, checked here
// against the views of E and kept with the launch. `lods` (NULL: the forms without the LOD cut): the caller's LOD views, likewise.
typedef int (*ClusterCullLaunches)(GvCtx* ctx, PoolState::Clusters& K, const ClusterLaunch& launch, size_t tiles, const GvClusterEye* eyes,
                                   const GvClusterLodView* lod_views);
struct ClusterCullForms {
    ClusterCullLaunches survivors;  // one command per survivor
    ClusterCullLaunches runs;       // one command per run (NULL: the entry point has no run flag)
    int (*second_test)(GvCtx* ctx, PoolState::Clusters& K, const ClusterSecondLaunch& launch);  // PoolState::Clusters::second_test behind the call
};
struct ClusterConeRequest {
    const GvClusterEye* eyes;
    uint32_t eye_count;
};
// gv_cluster_runs.cpp: the run form's scratch reserved and its launch struct around `launch` (the cone form's run launches share it)
int reserve_runs(GvCtx* ctx, PoolState::Clusters& K, const ClusterLaunch& launch, size_t tiles, ClusterRunLaunch* run);
// the cone table of K and the eyes of `views` views as a launch carries them (the views behind them: all-zero eyes, never read)
inline ClusterConeArgs cluster_cone_args(const PoolState::Clusters& K, uint32_t views, const void* eyes)
{
    ClusterConeArgs args{};
    args.cones = reinterpret_cast<const float4*>(K.d_cones.ptr);
    memcpy(args.eyes, eyes, (size_t)views * sizeof(GvClusterEye));
    return args;
}
struct ClusterLodRequest {
    const GvClusterLodView* views;
    uint32_t view_count;
};
int cull_clusters(GvCtx* ctx, const char* fn, ClusterCullForms forms, uint32_t allowed_flags, const ClusterConeRequest* cones, const char* zone_name,
                  uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device, size_t capacity_bytes,
                  const ClusterLodRequest* lods = nullptr);

// gv_mirror.cpp
// brings the device mirror up to date with the bound pools + dirty marks: per side a full rebuild, or growth and the dirty
// ranges; then the payload rows; then, when a tail is due, the re-order on the device (rules: gv_dirty_ranges.hpp)
int sync_mirror(GvCtx* ctx);
int upload_payload(GvCtx* ctx, PoolState& p);  // a pool's payload rows likewise (new slots + its own dirty set); sync_mirror calls it too
int upload_counts(GvCtx* ctx, PoolState& p);   // ... and its count mirror (PoolState::Counts), once gv_pool_emit_draw_instances wants one
int upload_geometry(GvCtx* ctx, PoolState& p);  // ... and its geometry id mirror (PoolState::Geometry), once gv_pool_emit_draw_commands wants one
int upload_lod(GvCtx* ctx, PoolState& p);       // ... and its size mirror (PoolState::Lod), once gv_pool_select_lods wants one
int upload_occluders(GvCtx* ctx, PoolState& p); // ... and its occluder box mirror (PoolState::Occluders), once gv_pool_draw_occluders wants one
TransformMirror xf_mirror(const GvCtx* ctx);  // the transform mirror as the kernels see it
MeshMirror mesh_mirror(const PoolState& p);   // a pool's mirror likewise (hot: null; the sphere stream's upkeep in cull_launch sets it)

}  // namespace gv
