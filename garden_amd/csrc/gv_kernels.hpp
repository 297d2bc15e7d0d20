// gv_kernels.hpp — host-visible launch interface of the gfx950 kernels (internal to libgarden_vis).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gv {

// ---- device mirror of the component pools (HBM layout) ----
// Streams are split so that a kernel reads only what the pool needs: 65 B per entity for a flat pool whose
// meshes and transforms pair up 1:1 (TRS 40 + flags 1 + AABB 24), +4 B parent entry with a hierarchy, +4 B transform
// entry when mesh and transform pools are ordered independently. A flat, exactly paired pool also keeps a 16 B sphere
// stream (MeshMirror::hot) from which the cull decides most entries; the 65 B are then read near the frustum only.
constexpr uint32_t kSlotMask = 0x0FFFFFFFu;
constexpr uint32_t kSlotNone = 0x0FFFFFFFu;
constexpr uint32_t kXfActive = 1u;         // selfActive && ancestorsActive (transform.hpp:110)
constexpr uint32_t kXfWithAncestors = 2u;  // modelWithAncestors (transform.hpp:60)
constexpr uint32_t kXfLive = 4u;           // entity != 0
constexpr uint32_t kMeshCandidate = 1u << 28;  // entity != 0 && isEnabled (mesh.cpp:142), in MeshMirror::link

// One 32-byte record per transform entry: {pos.xyz, scale.x | quat xyzw}. Kept together because every reader wants
// both halves: the streaming kernels read the pair at full rate (round-1 probe tools/stream_probe.hip, in the history: 6.8 TB/s interleaved vs
// 6.7 TB/s as two arrays) and every gather (emit, ancestor walks) pays one 64-byte sector instead of two.
struct XfAB {
    float4 a;  // (pos.x, pos.y, pos.z, scale.x)
    float4 b;  // quat xyzw
};
struct TransformMirror {
    const XfAB* ab;
    const float2* c;         // (scale.y, scale.z)
    const uint8_t* flags;    // kXf* bits
    const unsigned long long* active_bits;  // bit e of word e/64 = kXfActive of entry e (derived from flags[] on the
                                            // device after every upload); lets a flat, exactly-paired pool fetch its
                                            // 64 flags with one wave-uniform 8-byte load instead of a byte per lane
    const uint32_t* parent;  // parent entry or kSlotNone; read only when max_depth > 0
    uint32_t count;
    uint32_t max_depth;  // longest parent chain (bounds the walk; a cycle is rejected at mirror build)
};
enum MeshMapping : uint32_t {
    kMapGeneral = 0,    // read link[], then the transform entry it names
    kMapSpeculate = 1,  // >= 90 % of the entries map to their own index: prefetch xf[i] beside mesh[i], verify with link[]
    kMapExact = 2       // every candidate maps to its own index: link[] is not read at all
};
struct MeshMirror {
    const float4* a;       // (aabb.min.xyz, aabb.max.x)
    const float2* b;       // (aabb.max.y, aabb.max.z); non-candidate entries hold an empty box (min == max == 0)
    const uint32_t* link;  // transform entry | kMeshCandidate
    uint32_t count;
    uint32_t mapping;      // MeshMapping, decided at mirror build (speed only: every mapping is handled correctly)
    const uint32_t* orig;  // mirror entry -> pool slot (null: the mirror is in pool order)
    const float4* hot;     // flat, exactly paired pools (kMapExact, max_depth 0): the sphere stream, one HotEntry per entry, or null
};
// The sphere stream: what the cull's sphere pre-test needs of an entry of a flat, exactly paired pool, 16 bytes instead of 65:
// (pos.xyz, r) with r the view-independent part of the sphere (sphere_radius), or r = kHotDropped (negative; a computed r is
// >= +0 or NaN) when the filter chain drops the entry (non-candidate, empty box, inactive transform, no transform entry). The
// TRS / AABB streams are read only by the lanes that need corners. Derived on the device from the entry's own mirrored fields
// (launch_hot_build / launch_hot_patch) and kept current at every cull through the dirty-block flags.
constexpr float kHotDropped = -1.0f;
// PoolState::d_blk_dirty bits: a block holds an entry re-mirrored since the boxes / the sphere stream were last current
constexpr uint8_t kDirtyBounds = 1u, kDirtyHot = 2u, kDirtyAll = kDirtyBounds | kDirtyHot;
constexpr uint32_t kHotMinSlots = 65536;  // smaller pools cull in one launch with their emit (kFusedEmitMaxSlots) or are launch-bound
// 256-entry tiles per workgroup of the sphere-stream cull (cull_hot_kernel, K sphere loads in flight per lane), chosen so that the
// grid still fills the chip several times: 4 from 16 Ki tiles (4 Mi entries), 2 from 8 Ki tiles, 1 (cull_kernel) below
inline uint32_t hot_tiles_per_workgroup(uint32_t tiles)
{
    return tiles >= 16384u ? 4u : (tiles >= 8192u ? 2u : 1u);
}
// A Hi-Z view takes fewer tiles per workgroup than a frustum-only view of the same pool: its workgroups inside the frustum run many
// times longer than the ones outside (pyramid queries, the exact path of the corner candidates). It is not the walk of a wave over
// its K tiles one after the other that makes a long super-tile lose: with the candidates of the whole super-tile settled in dense
// rounds by all four waves (gv_dense_rounds.hpp) K = 4 still takes 52.8 us at the bench's 39 063 tiles where K = 2 takes 48.3, as it
// took 59.7 against 56.2 before (profiles/r34_dense_rounds.md); why is not known. The steps below are those measured before the
// dense rounds: frame of the bench scene, 4096^2 pyramid, K = 1 / 2 / 4: 8 204 tiles 47.6 / 50.1 / 60.2 us,
// 16 387 tiles 62.8 / 61.9 / 69.5, 23 438 tiles 75.7 / 69.9 / 77.2, 39 063 tiles (the bench) 105.2 / 90.6 / 95.2; K = 2 / 4: 46 875
// tiles 99.2 / 102.4, 54 688 tiles 109.9 / 109.8, 65 537 tiles 131.6 / 127.9, 78 125 tiles 151.5 / 144.2 (profiles/r33_cull_order.md).
constexpr uint32_t kHizHotK2Tiles = 16384;
constexpr uint32_t kHizHotK4Tiles = 57344;
inline uint32_t hot_tiles_per_workgroup_hiz(uint32_t tiles)
{
    return tiles >= kHizHotK4Tiles ? 4u : (tiles >= kHizHotK2Tiles ? 2u : 1u);
}
hipError_t launch_hot_build(const MeshMirror& mesh, const TransformMirror& xf, float4* hot, hipStream_t stream);
// re-derives the entries of the blocks flagged kDirtyHot (flags padded to a multiple of 16) and clears that bit
hipError_t launch_hot_patch(const MeshMirror& mesh, const TransformMirror& xf, float4* hot, uint8_t* flags, hipStream_t stream);

struct HizDevice {
    const float* depth;          // mip 0
    const float2* mips;          // levels >= 1, (min,max); rg16f: the same texels as packed binary16 pairs (uint32_t each)
    const uint64_t* mip_offset;  // device array [GV_MAX_MIPS], in texels
    uint32_t width, height, mip_count;
    uint32_t level1_virtual;  // level 1 is not stored (even sizes, fused build): a query derives its texels from the depth
    uint32_t rg16f;   // GV_CONFIG_HIZ_RG16F: texels are RG16F, min rounded toward -inf / max toward +inf (level 0 stays the depth)
    uint32_t nested;  // every level's min bounds ALL texels it covers (even sizes all the way, or the conservative rule):
                      // a coarser level may then prove occlusion early (exact shortcut, see hiz_occluded)
};

constexpr uint32_t kCullBlock = 256;   // slots per cull workgroup (4 waves)
constexpr uint32_t kFusedEmitMaxSlots = 32768;  // pools up to this size cull + emit in one launch: the look-back chain costs
                                                // ~16 ns per tile, so it only pays while a launch costs more (6.9 vs 9.8 us at 10 k
                                                // slots, equal at 100 k, 64 vs 24 us at 1 M; profiles/r02i_fused_emit.txt)
constexpr uint32_t kAutoBoundsMinSlots = 262144;  // pools above this size get block bounds unless GV_CONFIG_LINEAR_SCAN (smaller
                                                  // ones are launch-bound and keep the one-launch / batched paths)
constexpr uint32_t kEmitChunk = 4096;  // slots per compaction chunk = 64 ballot words
constexpr uint32_t kEmitParts = 4;     // emit workgroups per chunk: 1024 slots = 16 ballot words each

struct ViewParams {
    float planes[6][4];
    uint32_t plane_count;
    float cam[3];
    float cam_offset[3];
    float vp[16];
    uint32_t write_is_visible;  // main pass. The cull kernels store the bytes only when no emit follows the launch (count-only
                                // views, the one-launch cull + emit): with records requested the emit kernel expands them from
                                // the ballot words it reads anyway, as whole sectors — the byte stores cost the bandwidth-bound
                                // cull kernel 5-7 us of 105 at 10 M entities for 1.5 % of its bytes (round-3 probe tools/read_probe.hip, in the history)
    uint32_t use_hiz;           // 0 / 1
    uint32_t hiz_index;         // ... and the pyramid slot the view names (host side: resolved to a HizDevice when the launch is made)
    uint32_t distance_2d;
};

struct ViewBuffers {
    unsigned long long* mask;  // one ballot word per 64 slots
    uint32_t* chunk_count;     // visible per kEmitChunk slots (atomically summed by the cull workgroups, re-zeroed by scan)
    uint32_t* chunk_count_next;  // the other of the two alternating totals buffers (cleared by the self-prefixing emit)
    uint32_t* chunk_offset;    // exclusive scan of chunk_count (scan path only)
    uint32_t* draw_count;      // total
    uint8_t* is_visible;       // per slot (main pass)
    uint8_t* vis_flags;        // per emit workgroup (kEmitParts per chunk): 1 = its quarter of the chunk's isVisible bytes may hold
                               // a non-zero, 0 = known to be all zero. Lets the self-prefixing emit leave an EMPTY chunk after one
                               // load (behind an occlusion pass most chunks are empty). NULL: every workgroup writes its bytes
    uint32_t* visible_idx;     // compact records [0, draw_count), ascending slot order
    float* baked_model;        // 12 floats per record
    float* distance_sq;
};

// Emit seeds (round 3): for a flat, exactly paired pool that is at rest, everything the emit kernel gathers per visible entry —
// TRS record, scale tail, pool slot: three 64-byte sectors for 44 useful bytes, and the sparse gather is what bounds the emit
// behind an occlusion pass (316 k records -> 60 MB of sectors at cfg3) — as ONE 64-byte record per mirror entry, built on the
// device while the pool's mirror is clean (like the block bounds; a pool that changes every frame goes without). Same bits.
struct EmitSeed {
    float4 a, b;      // XfAB
    float2 c;         // (scale.y, scale.z)
    uint32_t orig;    // pool slot of the entry
    uint32_t pad[5];
};
static_assert(sizeof(EmitSeed) == 64, "one sector per visible entry");
constexpr uint32_t kEmitSeedMinSlots = 262144;  // smaller pools are launch-bound (and take other emit paths)
hipError_t launch_emit_seeds(const MeshMirror& mesh, const TransformMirror& xf, EmitSeed* seeds, hipStream_t stream);

// Block bounds (opt-in, GV_CONFIG_BLOCK_BOUNDS): world-space AABB of all corners of the candidates of each 256-entry
// cull workgroup, built while the mirror is clean. A workgroup whose box lies behind one frustum plane by more than
// the rounding margin skips its streams: every entity in it would have failed that plane in the per-entity test.
struct BlockBounds {
    const float4* lo = nullptr;   // xyz = min corner (+inf when the block has no candidate; -inf when a member is non-finite);
                                  // w = the largest sphere reach of its candidates (block_window; +inf likewise)
    const float4* hi = nullptr;   // xyz = max corner (-inf / +inf likewise)
    uint8_t* examined = nullptr;  // per workgroup: 1 = ran the per-entity path, 0 = skipped (statistics)
};
hipError_t launch_block_bounds(const MeshMirror& mesh, const TransformMirror& xf, float4* lo, float4* hi, hipStream_t stream);
// ... kept current while a few entries change per frame: flags (one byte per 256-entry block, padded to a multiple of 16, set by
// launch_mark_dirty_blocks for every block that holds a re-mirrored entry) name the blocks whose box — and whose entries' emit
// seeds, when `seeds` is given — are re-derived; the flags are cleared.
hipError_t launch_block_patch(const MeshMirror& mesh, const TransformMirror& xf, float4* lo, float4* hi, EmitSeed* seeds, uint8_t* flags,
                              hipStream_t stream);
// the dirty slot ranges of a sync (start[nranges + 1]: running slot counts, first[nranges]: first slots; device memory) -> flags
hipError_t launch_mark_dirty_blocks(const uint32_t* start, const uint32_t* first, uint32_t nranges, uint32_t total, const uint32_t* inv,
                                    uint32_t slots, uint32_t entries, uint8_t* flags, hipStream_t stream);
hipError_t launch_cull(const MeshMirror& mesh, const TransformMirror& xf, const HizDevice& hiz, const ViewParams& vp,
                       const ViewBuffers& out, hipStream_t stream);
// Block bounds as classify (+ window test for Hi-Z views) + cull over the listed workgroups (two or three launches; same outputs
// as a cull of every workgroup). kept_count / next_count: two alternating device counters (both zero before the first use; each
// launch clears the other one for the next); kept_list: cull_list_entry_bytes() per workgroup; kept_flag: a byte per workgroup.
size_t cull_list_entry_bytes();
hipError_t launch_cull_listed(const MeshMirror& mesh, const TransformMirror& xf, const HizDevice& hiz, const ViewParams& vp,
                              const ViewBuffers& out, const BlockBounds& bounds, uint32_t* kept_count, uint32_t* next_count,
                              void* kept_list, uint8_t* kept_flag, hipStream_t stream);
// Cull + order-stable compaction + record emission of one view in ONE launch (decoupled look-back over the 256-entry
// tiles; gv_cull.hip): same outputs as launch_cull + launch_emit except mask / chunk counts, which it does not produce.
// status: one 64-bit word per tile (zero-initialised once, never cleared: words carry `epoch`); ticket: a running
// counter whose value before this launch is ticket_base.
hipError_t launch_cull_emit(const MeshMirror& mesh, const TransformMirror& xf, const HizDevice& hiz, const ViewParams& vp,
                            const ViewBuffers& out, unsigned long long* status, uint32_t* ticket, uint32_t ticket_base, uint32_t epoch,
                            hipStream_t stream);
// One pass over the streams for up to kMaxBatchViews views that share views[0].cam (Hi-Z only on view 0).
constexpr uint32_t kMaxBatchViews = 8;
struct MultiViewPlanes {
    float planes[6][4];
    uint32_t plane_count;
    uint32_t write_is_visible;
};
hipError_t launch_cull_multi(const MeshMirror& mesh, const TransformMirror& xf, const HizDevice& hiz,
                             const ViewParams* views, const ViewBuffers* outs, uint32_t nviews, hipStream_t stream,
                             const BlockBounds* bounds = nullptr);
// ... with the Hi-Z query on every view whose ViewParams::use_hiz is set, view v against hiz[v] (its own pyramid) and views[v].vp:
// one pass over the streams all the same (cull_multi_hiz_kernel; bounds: the frustum skip of the form above, no window test)
hipError_t launch_cull_multi_hiz(const MeshMirror& mesh, const TransformMirror& xf, const HizDevice* hiz, const ViewParams* views,
                                 const ViewBuffers* outs, uint32_t nviews, hipStream_t stream, const BlockBounds* bounds = nullptr);
// gv_pick (gv_pick.hip): every ray against every entry of one pool that passes the cull's filter chain; keys[r] = min(keys[r], the
// smallest key (bits(distSq) << 32) | order_bits | slot of a hit), keys initialised to ~0 by the caller
constexpr uint32_t kPickBlock = 256;
constexpr uint32_t kPickMaxRays = 8;  // GV_MAX_PICK_RAYS
struct PickLaunch {
    float cam[3];
    float ray[kPickMaxRays][6];       // origin xyz, direction xyz (camera-relative)
    uint32_t rays;
    uint32_t order_bits;              // the pool's position in the call's list << 28
    uint32_t exclude;                 // slot never picked (kSlotNone-compatible: GV_NONE = none)
    const uint32_t* index_map;        // pool slot -> the caller's slot (NULL: none)
    unsigned long long* keys;         // [rays]
};
hipError_t launch_pick(const MeshMirror& mesh, const TransformMirror& xf, const PickLaunch& p, hipStream_t stream);
// gv_pool_emit_instances (gv_instance.hip): the records of up to kMaxInstanceViews views of one pool -> instance structs, back to
// back in the order listed, in ONE launch. The counts stay on the device: the grid is sized from the views' occupancies
// (first_block[v]: workgroups in front of view v), every workgroup adds up the counts of the views in front of its own.
constexpr uint32_t kInstanceBlock = 256;
constexpr uint32_t kMaxInstanceViews = 8;  // GV_MAX_VIEWS
constexpr uint32_t kMinInstanceStride = 64, kMaxInstanceStride = 256;
constexpr uint32_t kNoField = 0xFFFFFFFFu;  // GV_NONE
struct InstanceView {
    const uint32_t* count;  // device draw count
    const uint32_t* idx;    // records in delivery order
    const float* model;
    const float* dist;
    float view_proj[16];    // GvView::view_proj of the view's cull, column-major
};
struct InstanceLaunch {
    InstanceView view[kMaxInstanceViews];
    uint32_t first_block[kMaxInstanceViews + 1];
    uint32_t views;
    uint32_t stride, mvp, model, slot, distance_sq;  // GvInstanceLayout
    const uint32_t* index_map;                       // pool slot -> the caller's slot (NULL: none)
    uint8_t* dst;
    uint32_t capacity;                               // instances dst holds: those at or beyond it are not written
    uint32_t* starts;                                // [views + 1], written by workgroup 0
    // the pool's payload (gv_pool_bind_payload); payload_rows NULL: none, instance_kernel<false> is launched and reads none of this
    const uint8_t* payload_rows;                     // one packed row per POOL SLOT (the record's visible_idx, never index-mapped)
    uint32_t payload_pitch;                          // 16, 32 or 64
    uint32_t staged;                                 // fields + payload cover the whole stride (<= kMaxStagedInstanceStride): built in LDS
    uint16_t piece_at[4];                            // 16-byte piece j of the row -> a 16-byte aligned offset in the instance, or
    uint16_t word_at[16];                            // word w of the row -> its offset (kNoPayloadPlace: not written)
};
constexpr uint16_t kNoPayloadPlace = 0xFFFFu;
constexpr uint32_t kMaxStagedInstanceStride = 128;   // 256 x 128 B = 32 KB of LDS per workgroup
hipError_t launch_instances(const InstanceLaunch& launch, hipStream_t stream);
// gv_pool_emit_draw_instances (gv_instance.hip): the same records, but draw k takes count[visible_idx[k]] instances (the pool's
// mirrored ready column). TWO launches, no atomics, no host read: draw_counts_kernel scans the counts per chunk of kDrawChunk
// records (chunk-local prefix per record + one total per chunk; a chunk beyond its view's device count stores 0, so ONE flat
// prefix over the chunk table also carries the views in front), draw_instances_kernel adds up the totals in front of its chunk,
// writes first_instance[] and expands every record's instance into its count consecutive instances.
constexpr uint32_t kDrawChunk = 4096;                // records per chunk: 16 per lane of a kInstanceBlock workgroup
constexpr uint32_t kDirectImagePieces = 12;          // the direct way's LDS image per record: mvp 4, model 3, (slot, distance_sq) 1, row 4
struct DrawInstanceLaunch {
    InstanceLaunch base;                             // views, layout, target, payload tables; first_block: 256-record workgroups.
                                                     // staged: fields + payload + index field cover the whole stride (<= 128);
                                                     // starts: INSTANCE starts [views + 1]
    uint32_t first_chunk[kMaxInstanceViews + 1];     // chunks in front of view v
    const uint32_t* counts;                          // one per POOL SLOT (NULL: no ready column, every count is 1)
    uint32_t index_at;                               // offset of the uint32 "index within the draw" (kNoField: none)
    uint32_t* local;                                 // record k of view v at first_block[v] * kInstanceBlock + k: prefix inside its chunk
    uint32_t* chunk_total;                           // [first_chunk[views]]
    uint32_t* first_instance;                        // [draw_starts[v] + k]; one more word behind the last draw: the grand total
    uint32_t* draw_starts;                           // [views + 1]: prefix of the listed views' draw counts
};
// LDS of a draw_instances_kernel workgroup (dynamic: the bare layout's 16 KB image leaves room for 9 workgroups per CU, the direct
// way's 48 KB for 3): the image, then the 257-entry prefix and a few words of scratch
constexpr uint32_t kDrawLdsTail = 1088;
inline __host__ __device__ uint32_t draw_image_bytes(uint32_t staged, uint32_t stride)
{
    return kInstanceBlock * (staged ? stride : kDirectImagePieces * 16u);
}
hipError_t launch_draw_instances(const DrawInstanceLaunch& launch, hipStream_t stream);
// gv_pool_emit_draw_commands (gv_commands.hip): one indirect command per draw of the pool's last emission E — or, merged, per run
// of consecutive draws of one geometry id — in the caller's command struct. Per-draw mode: ONE launch
// (command_kernel). Run mode: command_heads_kernel (head flags + chunk-local head ranks per chunk of kDrawChunk draws, one head
// total per chunk) and command_runs_kernel (every head writes draw_of / first_of at its rank) in front of the same command_kernel.
// No atomics, no host read, no workgroup waits for another; grids sized from the views' occupancies.
constexpr uint32_t kCommandBlock = kInstanceBlock;  // command positions per command_kernel workgroup; draws per command_runs_kernel one
constexpr uint32_t kMinCommandStride = 16, kMaxCommandStride = 64;  // 256 x 64 B = 16 KB of LDS per workgroup
constexpr uint32_t kCommandHead = 0x80000000u;      // in CommandLaunch::rank: the draw opens a run
struct CommandGeometry {                            // GvGeometry
    uint32_t count, first;
    int32_t vertex_offset;
};
struct CommandView {
    const uint32_t* count;  // device draw count
    const uint32_t* idx;    // records in delivery order: POOL slots
};
struct CommandLaunch {
    CommandView view[kMaxInstanceViews];             // the views of E, in E's order
    uint32_t first_block[kMaxInstanceViews + 1];     // command_kernel workgroups in front of view v (packed: of its occupancy; regions: of the region)
    uint32_t first_draw_block[kMaxInstanceViews + 1];  // 256-draw workgroups in front of view v (command_runs_kernel; where rank[] begins)
    uint32_t first_chunk[kMaxInstanceViews + 1];     // chunks in front of view v
    uint32_t views;
    uint32_t merge_runs;                             // GV_COMMANDS_MERGE_RUNS
    uint32_t region;                                 // 0: packed
    uint32_t stride, count, instance_count, first, first_instance, vertex_offset, draw;  // GvCommandLayout
    const uint32_t* ids;                             // geometry id per POOL SLOT (NULL: every slot has id 0)
    const CommandGeometry* table;
    uint32_t table_count;
    const uint32_t* starts;                          // E: instance starts [views + 1]
    const uint32_t* first_instance_of;               // E, a draw emission: first_instance[draw_starts[v] + k]; NULL: first_k = starts[v] + k
    const uint32_t* draw_starts;
    // run mode's scratch; view v's draws at first_draw_block[v] * kCommandBlock (rank) and, one word more per view, + v (draw_of, first_of)
    uint32_t* rank;                                  // head rank inside the draw's chunk | kCommandHead
    uint32_t* chunk_total;                           // [first_chunk[views]] heads per chunk (0 beyond the view's count)
    uint32_t* draw_of;                               // run r of view v -> its head draw
    uint32_t* first_of;                              // ... and that draw's first instance
    uint8_t* dst;
    uint32_t capacity;                               // command positions dst holds: those at or beyond it are not written
    uint32_t* command_counts;                        // [views], written by workgroup 0 of command_kernel
    // (last, so that every argument above keeps its offset: the <false> instantiations are the instruction streams they were)
    const uint32_t* draw_ids;                        // the pool's LOD selection: the id of draw k of view v at D_v + k, D_v the sum of
                                                     // the draw counts in front (the <true> instantiations read it; NULL: ids it is)
};
hipError_t launch_command_heads(const CommandLaunch& launch, hipStream_t stream);  // run mode only, in this order
hipError_t launch_command_runs(const CommandLaunch& launch, hipStream_t stream);
hipError_t launch_commands(const CommandLaunch& launch, hipStream_t stream);
// gv_pool_select_lods (gv_lod.hip): the level of detail of every draw of the pool's last emission, all
// listed views in ONE launch of the shape of instance_kernel: one lane per draw, grid sized from the occupancies, the counts
// stay on the device. level_counts is zeroed in front of the launch (integer atomics: the histogram is deterministic).
constexpr uint32_t kLodBlock = kInstanceBlock;
constexpr uint32_t kMaxLodLevels = 8;              // GV_MAX_LOD_LEVELS
struct LodEntry {                                  // GvLodGeometry: two 16-byte pieces
    uint32_t levels;
    float switch_at[kMaxLodLevels - 1];
};
struct LodView {
    const uint32_t* count;  // device draw count
    const uint32_t* idx;    // records in delivery order: POOL slots
    const float* model;     // ... and their bakedModel, 12 floats each
    float scale;            // view_scale[v]
};
struct LodLaunch {
    LodView view[kMaxInstanceViews];               // the views of E, in E's order
    uint32_t first_block[kMaxInstanceViews + 1];   // workgroups in front of view v
    uint32_t views;
    const uint32_t* ids;                           // base geometry id per POOL SLOT (NULL: every slot has id 0)
    const uint32_t* sizes;                         // fp32 bit patterns per POOL SLOT (NULL: every slot has size 1)
    const LodEntry* table;                         // 32-byte aligned
    uint32_t table_count;
    uint32_t* draw_geometry;                       // [sum of the draw counts]
    uint32_t* level_counts;                        // [views * kMaxLodLevels]
};
hipError_t launch_lod(const LodLaunch& launch, hipStream_t stream);
// read-only pass over the cull kernel's input streams (65 B per entry); gv_debug_stream_peak
hipError_t launch_stream_probe(const MeshMirror& mesh, const TransformMirror& xf, float* sink, hipStream_t stream);
// Table-driven tick (gv_cull_batch_begin): the culls of several small pools in one launch, their emits in one launch.
// The descriptor structs are private to gv_cull.hip: the host fills a table of entries through these.
size_t cull_table_entry_bytes();
void fill_cull_table_entry(void* entry, const MeshMirror& mesh, const TransformMirror& xf, const HizDevice& hiz,
                           const ViewParams* views, const ViewBuffers* outs, uint32_t nviews);
hipError_t launch_cull_table(const void* device_table, uint32_t jobs, uint32_t max_slots, hipStream_t stream);
size_t emit_table_entry_bytes();
void fill_emit_table_entry(void* entry, const MeshMirror& mesh, const TransformMirror& xf, const ViewParams& vp,
                           const ViewBuffers& out, uint32_t clear_chunks, const float4* world);
hipError_t launch_emit_table(const void* device_table, uint32_t entries, uint32_t max_slots, hipStream_t stream);
hipError_t launch_scan(const ViewBuffers& out, uint32_t chunk_count, hipStream_t stream);
// self_prefix: every emit workgroup derives its chunk's base from the chunk totals itself (no launch_scan in front;
// pools of up to kSelfPrefixMaxChunks chunks); out.chunk_count / chunk_count_next then alternate from cull to cull.
constexpr uint32_t kSelfPrefixMaxChunks = 4096;
// world: the resident world matrices of the current transform mirror (3 float4 per entry), or NULL — records then take
// world[slot] instead of re-walking the parent chain (same bits)
hipError_t launch_emit(const MeshMirror& mesh, const TransformMirror& xf, const ViewParams& vp, const ViewBuffers& out,
                       hipStream_t stream, bool self_prefix = false, uint32_t clear_chunks = 0, const float4* world = nullptr,
                       const EmitSeed* seeds = nullptr);
// all views of a batched cull in one launch (self-prefixing form; views[v] / outs[v] / clear_chunks[v] per view)
hipError_t launch_emit_batch(const MeshMirror& mesh, const TransformMirror& xf, const ViewParams* views, const ViewBuffers* outs,
                             const uint32_t* clear_chunks, uint32_t nviews, hipStream_t stream, const float4* world = nullptr);
// map: pool slot -> caller's global id (NULL: identity), applied before `base`
hipError_t launch_copy_idx(const uint32_t* src, const uint32_t* count, uint32_t* dst, uint32_t capacity, uint32_t base,
                           const uint32_t* map, hipStream_t stream);
hipError_t launch_copy_shard(const uint32_t* src, const uint32_t* count, uint32_t* dst, uint32_t capacity, uint32_t base,
                             const uint32_t* map, hipStream_t stream);
// gv_exchange_views: every list of a frame into ONE shard [n + total, c_0 .. c_{n-1}, list 0, list 1 ...] (gv_shard.hip)
struct ShardItem {
    const uint32_t* src;    // the view's visible_idx
    const uint32_t* count;  // its device draw count
    const uint32_t* map;    // pool slot -> caller's global id (NULL: identity)
    uint32_t base, capacity;
};
hipError_t launch_copy_shard_batch(const ShardItem* device_items, uint32_t n, uint32_t widest, uint32_t* dst, hipStream_t stream);
// gv_exchange_visible / _views: the leading hdr_words words of all `world` gathered rows (the true counts; the per-list counts of
// a batched frame), then `seq`, into pinned host memory (host_words[1 + r * hdr_words + w] = rows[r * row_words + w], host_words[0]
// = seq with system-scope release): the host learns the counts of a frame without an event record or a synchronisation — it
// looks at the word a frame or two later
hipError_t launch_exchange_headers(const uint32_t* rows, uint32_t row_words, uint32_t world, uint32_t hdr_words, uint32_t* host_words, uint32_t seq,
                                   hipStream_t stream);
// GV_EXCHANGE_PEER: the 1 + shard[0] leading words of a rank's staging shard (at most cap_words) into its row of EVERY rank's rows
// (rows.dst[r]: this rank's row in rank r's buffer — the rank's own, or a peer device's over xGMI), one launch
struct PeerRows {
    uint32_t* dst[64];  // GV_EXCHANGE_MAX_RANKS (garden_vis.h; asserted in gv_exchange.cpp)
};
hipError_t launch_peer_scatter(const uint32_t* shard, uint32_t cap_words, const PeerRows& rows, uint32_t world, hipStream_t stream);
// gv_results_fetch of a pool of up to kPublishMaxSlots slots: device results -> pinned host buffers in one launch
// (up to kPublishLdsSlots slots the isVisible bytes are put back into pool-slot order in LDS by the same kernel)
constexpr uint32_t kPublishMaxSlots = 262144;
constexpr uint32_t kPublishLdsSlots = 32768;
// the caller's record struct (GvRecordLayout); stride == 0: none
struct RecordLayout {
    uint32_t stride, component_offset, baked_model, distance_sq, buffer_index, component_stride, buffer_index_value;
    uint32_t pad_;
    const uint32_t* slot_map;  // GV_RESULTS_MAP_RECORDS: componentOffset = slot_map[slot] * component_stride (NULL: slot itself); filled in
                               // when results are delivered, never kept in PoolState::record_layout
};
__host__ __device__ inline uint32_t record_slot(const RecordLayout& L, uint32_t slot) { return L.slot_map ? L.slot_map[slot] : slot; }
constexpr uint32_t kMaxRecordStride = 128;
struct PublishArgs {
    const uint32_t* count;  // device draw_count
    const uint32_t* idx;
    const float* model;
    const float* dist;
    const uint8_t* is_visible;  // mirror order
    const uint32_t* orig;       // mirror entry -> pool slot (NULL: the mirror is in slot order)
    uint32_t* host_count;       // pinned host memory from here on (device-accessible: hipHostMalloc)
    uint32_t* host_idx;         // NULL: no records emitted
    float* host_model;
    float* host_dist;
    uint8_t* host_is_visible;   // pool-slot order; NULL: not the main pass
    uint32_t occupancy;
    uint8_t* host_records;      // records in the caller's struct layout instead of host_idx / host_model / host_dist (or NULL)
    RecordLayout layout;
};
constexpr uint32_t kMaxPublishViews = 32;  // views of SEVERAL pools per launch (>= GV_MAX_VIEWS, checked in gv_context.cpp)
struct PublishBatch {
    PublishArgs view[kMaxPublishViews];  // blockIdx.y
};
hipError_t launch_publish(const PublishBatch& batch, uint32_t views, uint32_t occupancy, hipStream_t stream);
// records [0, *count) of a view as an array of the caller's structs (device or device-visible host memory)
hipError_t launch_pack_records(const uint32_t* count, const uint32_t* idx, const float* model, const float* dist, const RecordLayout& layout,
                               uint32_t capacity, uint8_t* dst, hipStream_t stream);
hipError_t launch_unpermute_bytes(const uint8_t* src, const uint32_t* orig, uint32_t count, uint8_t* dst, hipStream_t stream);

}  // namespace gv

#include "gv_sort_kernels.hpp"  // gv_sort.hip's launch interface

namespace gv {
static_assert(kMaxSortViews == kMaxPublishViews, "a tick's sort and publish batches hold the same views");

// derives TransformMirror::active_bits from flags[]
// Byte layout of one TransformComponent inside a raw AoS copy (all offsets within `stride`).
struct AosTransformLayout {
    uint32_t stride, entity, position, scale, rotation, self_active, ancestors_active, model_with_ancestors;
};
// dirty (may be NULL): set to 1 for every entry written (subtree-scoped world-matrix sweep)
hipError_t launch_aos_transforms(const uint8_t* raw, const AosTransformLayout& layout, uint32_t first, uint32_t count,
                                 const uint32_t* xinv, XfAB* ab, float2* c, uint8_t* flags, uint8_t* dirty, hipStream_t stream);
hipError_t launch_pack_active(const uint8_t* flags, uint32_t count, unsigned long long* bits, hipStream_t stream);
// The same for dirty MeshRenderComponents (GV_DIRTY_MESH): raw AoS span -> mesh mirror entries. inv: pool slot -> mirror entry
// (NULL: slot order); e2t: the entity -> transform slot table on the device; xinv: transform slot -> mirror entry (or NULL);
// *demoted |= 1 when a candidate does not pair with its own mirror index.
struct AosMeshLayout {
    uint32_t stride, entity, is_enabled, aabb_min, aabb_max;
};
hipError_t launch_aos_meshes(const uint8_t* raw, const AosMeshLayout& layout, uint32_t first, uint32_t count, const uint32_t* inv,
                             const uint32_t* e2t, uint32_t entity_capacity, uint32_t xf_occupancy, const uint32_t* xinv, float4* a, float2* b,
                             uint32_t* link, uint32_t* demoted, hipStream_t stream);
// out[k] = world[xinv[first + k]] (3 float4 per slot)
hipError_t launch_gather_world(const float4* world, const uint32_t* xinv, uint32_t first, uint32_t count, float4* out,
                               hipStream_t stream);

// world matrices (camera = 0) of every transform slot: 3 float4 per slot (float4x3 order)
hipError_t launch_sweep_valu(const TransformMirror& xf, float4* world, hipStream_t stream);
hipError_t launch_sweep_mfma(const TransformMirror& xf, float4* world, hipStream_t stream);
// only the entries whose chain contains an entry flagged in dirty[] (1 byte per mirror entry); same bits
hipError_t launch_sweep_subtree(const TransformMirror& xf, const uint8_t* dirty, float4* world, hipStream_t stream);
// Sweep (MFMA or VALU chain) + cull of an exactly paired pool (mesh.mapping == kMapExact) in one pass: world matrices AND the cull
// outputs of one view; same bits as launch_sweep_* followed by launch_cull.
hipError_t launch_sweep_cull(const MeshMirror& mesh, const TransformMirror& xf, const HizDevice& hiz,
                             const ViewParams& vp, const ViewBuffers& out, float4* world, bool mfma, hipStream_t stream);

// Hi-Z pyramid. Level k >= 1 lives at mips + mip_offset[k]; level 0 is the depth image.
// Generic one-level reduction (any size, shaders/hiz.frag:27-56 incl. the odd-size branches).
// rg16f: src_pairs / dst (and HizFusedDst::level) point to packed binary16 pairs, 4 bytes per texel
hipError_t launch_hiz_level(const float* src_depth, const float2* src_pairs, float2* dst, uint32_t sw, uint32_t sh,
                            uint32_t dw, uint32_t dh, uint32_t rule, bool rg16f, hipStream_t stream);
// Levels [first, first + count) by ONE workgroup, one after the other (any sizes; a level's source is the level before it, the
// depth image for level 1). For the small levels of a pyramid: at most kHizTailTexels texels in the first of them.
constexpr uint32_t kHizTailTexels = 8192;  // two levels of this size fit the LDS
struct HizTailArgs {
    const float* depth;
    float2* mips;          // level k >= 1 at mips + offset[k] (texels; packed binary16 pairs when rg16f)
    uint64_t offset[16];
    uint32_t w[16], h[16];
    uint32_t first, count, rule;
};
hipError_t launch_hiz_tail(const HizTailArgs& args, bool rg16f, hipStream_t stream);
// Fused 6-level reduction of 64x64 source tiles through LDS; needs sw % 64 == 0 && sh % 64 == 0.
// dst[l] = level (src+1+l), l = 0..5.
struct HizFusedDst {
    float2* level[6];
};
hipError_t launch_hiz_fused(const float* src_depth, const float2* src_pairs, const HizFusedDst& dst, uint32_t sw,
                            uint32_t sh, bool rg16f, hipStream_t stream);

}  // namespace gv
