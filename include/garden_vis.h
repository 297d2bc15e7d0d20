/*
 * garden_vis.h — C-ABI of libgarden_vis.so: the MI355X (gfx950) visibility pass that stands in for
 * Garden's CPU MeshRenderSystem::prepareMeshes + Vulkan HizRenderSystem::downsampleHiz pair.
 *
 * Citations are relative to the reference checkout (cfnptr/garden). The reference has no FFI for
 * this path — it is C++ calling C++ inside one process — so each entry point below names the
 * C++ interface it replaces; INTEGRATION.md shows the shim (an ecsm System) a maintainer adds.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 (GV_OK) or a negative
 * GvStatus; no exceptions or abort() cross this boundary (the reference throws GardenError,
 * include/garden/error.hpp:32-55 — the C++ shim converts). Not re-entrant per context; call from
 * the thread that runs Manager::update() (source/system/input.cpp:361-379). Matrices are
 * column-major float[16] (c0..c3), quaternions xyzw, as in include/garden/system/physics-impl.hpp:45-63.
 *
 * Streams: all device work is enqueued on the context's own stream (gv_stream; created hipStreamNonBlocking: it is NOT
 * ordered against the null stream or any stream of the caller's). Device memory the caller hands in — a GV_MEM_DEVICE depth
 * image, the destination of gv_results_copy_*_device / gv_exchange_shards / gv_exchange_masks — must be ready (its last
 * writer finished, e.g. a fill on another stream) when the call is made, or the caller orders gv_stream() behind its producer
 * itself (hipStreamWaitEvent(gv_stream(ctx), event)); consumers of device results order themselves behind gv_stream().
 */
#ifndef GARDEN_VIS_H
#define GARDEN_VIS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GV_ABI_VERSION 4u /* 3: every exchanged frame is complete (gv_exchange_acquire fills the frame; GV_EXCHANGE_EXACT and
                             gv_exchange_counts are gone); one thread can drive N contexts (gv_exchange_*_all); GV_E_TIMEOUT
                             4: ONE exchange per frame for all its (pool, view) lists (gv_exchange_views[_all]); a rank's results in
                             the WORLD's slots (gv_pool_set_result_mapping, gv_pool_update_index_map); GvStats grew; GvExchangeFrame grew;
                             gv_exchange_init_peers / GV_EXCHANGE_PEER (one process, no communicator) */
#define GV_NONE 0xFFFFFFFFu
#define GV_MAX_POOLS 16u
#define GV_MAX_VIEWS 8u
#define GV_MAX_PYRAMIDS 8u /* pyramid slots of a context (gv_hiz_select): one per view of a cull */
#define GV_MAX_MIPS 16u

typedef enum GvStatus {
    GV_OK = 0,
    GV_E_ARG = -1,     /* bad argument / unbound pool / capacity exceeded */
    GV_E_HIP = -2,     /* a HIP runtime call failed (text in gv_last_error) */
    GV_E_OOM = -3,     /* host or device allocation failed */
    GV_E_RCCL = -4,    /* collective failed (multi-GPU exchange) */
    GV_E_STATE = -5,   /* call out of order (e.g. cull before bind, Hi-Z query before build) */
    GV_E_NODEVICE = -6, /* no gfx950 device / kernels not loadable: there is NO CPU fallback */
    GV_E_TIMEOUT = -7   /* a bounded wait ran out (a peer rank of the exchange stalled or left): gv_exchange_set_timeout */
} GvStatus;

typedef struct GvCtx GvCtx;

typedef struct GvConfig {
    uint32_t struct_size; /* = sizeof(GvConfig) */
    int32_t device;       /* HIP device ordinal: one context per GPU; the contexts of a node's GPUs may live in one process and be
                             driven by one thread (gv_exchange_*_all) */
    uint32_t hiz_rule;    /* GvHizRule */
    uint32_t flags;       /* GvConfigFlags */
} GvConfig;

typedef enum GvHizRule {
    GV_HIZ_RULE_REFERENCE = 0,   /* shaders/hiz.frag:49-55 exactly as written (odd-height row uses gather .y/.z) */
    GV_HIZ_RULE_CONSERVATIVE = 1 /* full extra row: min/max bound every covered texel */
} GvHizRule;

typedef enum GvConfigFlags {
    GV_CONFIG_PROFILE_EVENTS = 1u << 0,   /* bracket every kernel with hipEvents; durations via gv_stats */
    GV_CONFIG_PROFILE_CULL_ONLY = 1u << 1, /* with PROFILE_EVENTS: only GV_K_CULL is bracketed (2 events per view
                                             instead of ~10 per frame: each event record costs ~2 us of stream time) */
    GV_CONFIG_KEEP_SLOT_ORDER = 1u << 2,  /* keep the device mirror in pool-slot order. Default: entries are ordered
                                             spatially (Morton code of the root ancestor's position) at every full
                                             rebuild so that neighbouring lanes touch neighbouring Hi-Z texels; all
                                             outputs are reported in pool slots either way */
    GV_CONFIG_BLOCK_BOUNDS = 1u << 3,     /* keep a world-space box per 256-entry cull workgroup (built on the device
                                             while the pool's mirror is clean) and let a workgroup whose box lies behind
                                             a frustum plane by more than the rounding margin — or, for a Hi-Z view over a
                                             nested pyramid, wholly behind what the pyramid holds over the box's footprint —
                                             skip its streams. Same results bit for bit (both tests are conservative w.r.t. the
                                             per-entity ones); pools that change every frame are culled without boxes. Pays
                                             off with the default spatial mirror order. Batched views skip a workgroup when
                                             every view does. DEFAULT for pools of more than 262144 slots (round 3); this flag
                                             forces it for pools of every size (they then take neither the one-launch cull + emit
                                             nor the batched tick) */
    GV_CONFIG_LINEAR_SCAN = 1u << 5,      /* never use block bounds: every workgroup tests every entity every frame, with no
                                             block skipping and nothing that can go stale (the flat loop of mesh.cpp:137-175, which
                                             SURVEY.md §8d prices; bench.py's headline and roofline kernel). A flat, exactly paired
                                             pool reads its 16-byte sphere stream for every entity and the 49 further bytes of
                                             TRS + AABB only for the entities near or inside the frustum */
    GV_CONFIG_HIZ_RG16F = 1u << 4         /* keep the pyramid in the reference's image format (HizRenderSystem::bufferFormat =
                                             SfloatR16G16, render/hiz.hpp:41): levels >= 1 are binary16 (min, max) pairs, half the
                                             bytes. The reference lets the render target round to nearest, which can move a min
                                             up or a max down; here min is rounded toward -inf and max toward +inf, so a texel
                                             still bounds every depth it covers and the occlusion query stays conservative (it may
                                             keep a few boxes an fp32 pyramid would cull, never the other way). Level 0 stays the
                                             fp32 depth image. gv_hiz_read_level returns the stored halfs widened to float. */
} GvConfigFlags;

/* ---- pool binding: replaces LinearPool::getData/getOccupancy (docs/ECS/Components.md:137-170) as
 * consumed at source/system/render/mesh.cpp:119-120,139,360,411,460 ---- */

/* Field byte offsets inside one TransformComponent (include/garden/system/transform.hpp:31-61). */
typedef struct GvTransformLayout {
    uint32_t entity;               /* Component::entity, u32, 0 = free slot */
    uint32_t parent;               /* ID<Entity> parent, u32, 0 = none */
    uint32_t position;             /* f32x4 posChildCount (xyz used) */
    uint32_t scale;                /* f32x4 scaleChildCap (xyz used) */
    uint32_t rotation;             /* quat xyzw */
    uint32_t self_active;          /* volatile bool */
    uint32_t ancestors_active;     /* volatile bool */
    uint32_t model_with_ancestors; /* volatile bool */
} GvTransformLayout;

/* Field byte offsets inside one MeshRenderComponent-derived struct (render/mesh.hpp:45-55). */
typedef struct GvMeshLayout {
    uint32_t entity;
    uint32_t is_enabled;
    uint32_t is_visible; /* written back by gv_results_fetch on main-pass views */
    uint32_t aabb_min;   /* f32x4 */
    uint32_t aabb_max;   /* f32x4 */
} GvMeshLayout;

/* Binds the TransformComponent pool and the entity -> transform-slot map that stands in for
 * Manager::tryGet<TransformComponent>(entity) (mesh.cpp:149) / Manager::get (transform.hpp:206).
 * Re-issue whenever getData() may have moved (create() can reallocate: docs/ECS/Entities.md:44-46).
 * Pointers must stay valid until the next gv_sync()/gv_cull() returns; nothing is retained after.
 * Occupancy may grow from one bind to the next (entities were created): the new slots are appended to the device
 * mirror at the next sync — no rebuild; a smaller occupancy rebuilds it. The same holds for gv_pool_bind. Slots whose
 * contents changed (filled, emptied, edited) are reported with gv_mark_dirty as always. */
int gv_transform_bind(GvCtx* ctx, const void* base, size_t stride, uint32_t occupancy,
                      const GvTransformLayout* layout, const uint32_t* entity_to_transform,
                      uint32_t entity_capacity);

/* Binds one IMeshRenderSystem's component pool (render/mesh.hpp:127-131). pool_id < GV_MAX_POOLS. */
int gv_pool_bind(GvCtx* ctx, uint32_t pool_id, void* base, size_t stride, uint32_t occupancy,
                 const GvMeshLayout* layout);

/* Column (SoA) form of the two binds, for engines and loaders whose components are not an array of structs: every
 * field is its own array, element i at data + i * stride (stride >= the field's width; an AoS pool is the special case
 * data = base + offsetof(field), stride = sizeof(component), which is what gv_transform_bind / gv_pool_bind pass).
 * Same lifetime and dirty-range rules as the AoS binds. position/scale: 3 floats, rotation: 4 floats (xyzw),
 * aabb_min/aabb_max: 3 floats, flags: 1 byte, entity/parent: uint32 entity ids. */
typedef struct GvColumn {
    const void* data;
    uint32_t stride; /* bytes between consecutive elements */
} GvColumn;
typedef struct GvTransformColumns {
    GvColumn entity, parent, position, scale, rotation, self_active, ancestors_active, model_with_ancestors;
} GvTransformColumns;
typedef struct GvMeshColumns {
    GvColumn entity, is_enabled, aabb_min, aabb_max;
    void* is_visible;           /* write-back target of gv_results_fetch (may be NULL) */
    uint32_t is_visible_stride; /* bytes between consecutive isVisible bytes */
} GvMeshColumns;
int gv_transform_bind_columns(GvCtx* ctx, const GvTransformColumns* columns, uint32_t occupancy,
                              const uint32_t* entity_to_transform, uint32_t entity_capacity);
int gv_pool_bind_columns(GvCtx* ctx, uint32_t pool_id, const GvMeshColumns* columns, uint32_t occupancy);
/* Optional per-slot READY COUNT of a pool: what a derived system's getReadyMeshesAsync returns for a mesh that passed
 * the frustum test — 0 while its resources are not loaded (SpriteRenderSystem: descriptorSet, sprite.cpp:90-97;
 * UiLabelSystem: text data ready, label.cpp:271-276), otherwise the number of instances it draws (1 for the default
 * predicate, render/mesh.hpp:142-146). Element i at data + i * stride, `width` = 1 (uint8) or 4 (uint32) bytes.
 * A slot whose count is 0 is treated exactly like the reference treats readyCount == 0 (mesh.cpp:158-165): not drawn,
 * isVisible = false; GvResult.instance_count becomes the sum of the counts of the drawn meshes (mesh.cpp:174).
 * Same lifetime rules as gv_pool_bind (re-issue when the storage may have moved); changed counts are reported with
 * gv_mark_dirty(GV_DIRTY_MESH). data == NULL removes the column (every slot counts 1 again).
 * Which meshes are DRAWN is decided by the counts as mirrored at the cull; instance_count and the instance bases are summed on the
 * host from the column as it stands when the results are fetched (the reference reads getInstancesAsync at draw time too,
 * mesh.cpp:596): change counts between frames — after a frame's results have been read, before the next gv_cull — not in between. */
int gv_pool_bind_ready(GvCtx* ctx, uint32_t pool_id, const void* data, uint32_t stride, uint32_t width);

typedef enum GvDirtyKind {
    GV_DIRTY_TRANSFORM = 0, /* TRS / active flags of transform slots [first, first+count) changed
                               (setPosition/Scale/Rotation transform.hpp:74-104, setActive transform.cpp:75-127) */
    GV_DIRTY_HIERARCHY = 1, /* count > 0: transform slots [first, first+count) were re-parented (setParent
                               transform.cpp:130-195): their links are re-gathered in place and depth / cycles
                               re-validated; count == 0: entities came or went (destroy :30-73, create): rebuild and
                               re-order the whole mirror */
    GV_DIRTY_MESH = 2,      /* mesh slots changed; pool id in the top 4 bits of `first` */
    GV_DIRTY_PAYLOAD = 3,   /* the bound payload bytes (gv_pool_bind_payload) of mesh slots changed; pool id in the top 4 bits of
                               `first`, like GV_DIRTY_MESH. Read by no cull: a recorded cull of a batch is not launched by it */
    GV_DIRTY_GEOMETRY = 4,  /* the bound geometry ids (gv_pool_bind_geometry) of mesh slots changed; pool id in the top 4 bits of
                               `first`. Read by no cull either */
    GV_DIRTY_LOD = 5,       /* the bound sizes (gv_pool_bind_lod) of mesh slots changed; pool id in the top 4 bits of `first`. Read
                               by no cull either */
    GV_DIRTY_OCCLUDER = 6   /* the bound occluder boxes (gv_pool_bind_occluders) of mesh slots changed; pool id in the top 4 bits of
                               `first`. Read by no cull either */
} GvDirtyKind;
int gv_mark_dirty(GvCtx* ctx, uint32_t kind, uint32_t first, uint32_t count);

/* Re-derives the whole device mirror (parent slots, transform slot per mesh, flags) from the bound
 * pools and uploads it. Implied by the first gv_sync after a bind. */
int gv_hierarchy_rebuild(GvCtx* ctx);
/* Uploads whatever is dirty (host gather AoS -> SoA staging, then H2D). Called by gv_cull too. */
int gv_sync(GvCtx* ctx);

/* ---- per-frame inputs: replaces the CommonConstants read at mesh.cpp:866-869,899-902 and the
 * per-cascade viewProj/cameraOffset of renderShadows (mesh.cpp:795-847) ---- */
typedef struct GvView {
    float view_proj[16];      /* cc.viewProj = projection * view, view translation zeroed (graphics.cpp:201,243) */
    float camera_position[4]; /* cc.cameraPos (graphics.cpp:202); xyz used */
    float camera_offset[4];   /* shadow cascades (render/mesh.hpp:166); zero for the main camera */
    int8_t shadow_pass;       /* < 0: main pass, isVisible is produced (mesh.cpp:121) */
    uint8_t use_hiz;          /* 0: no Hi-Z query. 1 + k with k < GV_MAX_PYRAMIDS: also run the occlusion query against pyramid k
                                 (which must be built: gv_hiz_select / gv_hiz_build). Any larger value: pyramid 0, as 1 */
    uint8_t distance_2d;      /* sorted twin key translation.z + 1 (mesh.cpp:250) */
    uint8_t emit_records;     /* 1: produce visibleIdx/bakedModel/distanceSq; 0: isVisible + count only */
} GvView;

/* Host-visible results of one view: the SoA form of UnsortedBuffer::combinedMeshes[0..drawCount)
 * (render/mesh.hpp:191-217). Pointers are library-owned pinned memory, valid until the next
 * gv_cull on this context. Record order is deterministic (reproducible run to run): ascending pool slot with
 * GV_CONFIG_KEEP_SLOT_ORDER, otherwise the mirror's spatial order; gv_sort orders them by distance. The
 * reference's order is fetch_add arrival order (mesh.cpp:177), i.e. unspecified, and its consumers sort by
 * distanceSq afterwards (mesh.cpp:548-551). is_visible is always indexed by pool slot. */
typedef struct GvResult {
    const uint32_t* visible_idx; /* pool slot; componentOffset = visible_idx * stride (mesh.cpp:170) */
    const float* baked_model;    /* 12 floats per record: c0.xyz c1.xyz c2.xyz c3.xyz (float4x3, mesh.cpp:171) */
    const float* distance_sq;    /* mesh.cpp:172 / :250-251 */
    const uint8_t* is_visible;   /* one byte per pool slot; NULL for shadow passes */
    uint32_t draw_count;         /* UnsortedBuffer::drawCount (render/mesh.hpp:210) */
    uint32_t instance_count;     /* sum of the drawn meshes' ready counts (mesh.cpp:174): == draw_count unless a ready column
                                    with counts above 1 is bound (gv_pool_bind_ready) */
} GvResult;

/* Device-side cull of one pool against `view_count` views: frustum test (+ Hi-Z query) + compaction.
 * Asynchronous: returns once the work is enqueued on the context's stream. Replaces
 * MeshRenderSystem::prepareMeshes' threaded loop (mesh.cpp:331-553 -> :111-184).
 * Everything a view's results consist of is enqueued by this call, in stream order: a consumer on gv_stream() may use the
 * pointers of gv_results_device without calling into the library again (round 3 held a single occlusion view's record emission
 * back until the next gv_hiz_build; withdrawn in round 4 — only a loop that never looks at its results gained from it). */
int gv_cull(GvCtx* ctx, uint32_t pool_id, const GvView* views, uint32_t view_count);
/* Blocks until all enqueued work is done. */
int gv_wait(GvCtx* ctx);
/* Waits, copies view `view_index`'s records to pinned host memory, and — for a main-pass view — when
 * write_back != 0 scatters isVisible into the bound pool (mesh.cpp:144,152,161,166). */
int gv_results_fetch(GvCtx* ctx, uint32_t view_index, int write_back, GvResult* out);
/* draw count only (4-byte readback). */
int gv_result_count(GvCtx* ctx, uint32_t view_index, uint32_t* draw_count);
/* Device pointers of view `view_index`'s compacted list, for an exchange step that stays on the GPU
 * (multi-GPU all-gatherv). Valid until the next gv_cull. */
typedef struct GvDeviceResult {
    const void* visible_idx; /* uint32_t[draw_count], device memory */
    const void* baked_model; /* float[12 * draw_count] */
    const void* distance_sq; /* float[draw_count] */
    const void* is_visible;  /* uint8_t[occupancy] or NULL; indexed by MIRROR entry (pool slot only with
                                GV_CONFIG_KEEP_SLOT_ORDER) — use gv_results_fetch for the pool-slot view */
    const void* draw_count;  /* uint32_t, device memory */
} GvDeviceResult;
int gv_results_device(GvCtx* ctx, uint32_t view_index, GvDeviceResult* out);
/* Copies visible_idx (+ `index_base` added to each) into caller-owned device memory. */
int gv_results_copy_idx_device(GvCtx* ctx, uint32_t view_index, void* dst_device, uint32_t capacity,
                               uint32_t index_base);
/* Exchange shard for the multi-GPU all-gather: dst[0] = draw_count (the true count, also when it
 * exceeds `capacity`), dst[1 .. 1 + min(draw_count, capacity)) = visible_idx + index_base. dst holds 1 + capacity
 * uint32. No host synchronisation: ranks can gather fixed-size padded shards and read the counts from the headers. */
int gv_results_copy_shard_device(GvCtx* ctx, uint32_t view_index, void* dst_device, uint32_t capacity,
                                 uint32_t index_base);

/* The same visible set as a BIT per entry of the pool's device mirror: dst[0] = draw_count, bit (e & 31) of dst[1 + (e >> 5)]
 * = mirror entry e is in the view's visible list; dst holds 1 + word_count uint32, word_count >= ceil(occupancy / 32). The
 * size does not depend on the view: 1/32 of a word per slot where the index list costs a word per visible slot — smaller above
 * ~3 % visibility, 1/7 of the list at the bench's 21 % — and an equal-size all-gather by construction: the encoding for dense
 * views on the links of a multi-GPU node. It is the cull kernel's own output, so producing it is a 1.6 MB copy per 12.5 M
 * entries (bits in pool-slot order would cost a scatter per frame: measured, +126 us). Entry e is pool slot
 * gv_pool_mirror_slots()[e]: that table only changes when the mirror is rebuilt, grown or re-ordered (gv_hierarchy_rebuild, a pool
 * bound with another occupancy; gv_pool_mirror_epoch says when), so consumers fetch it once per change — with GV_CONFIG_KEEP_SLOT_ORDER it is the identity. Main-pass
 * views of any pool, and every view that took the ordinary cull launch (GV_E_STATE otherwise). No host synchronisation. */
int gv_results_copy_mask_device(GvCtx* ctx, uint32_t view_index, void* dst_device, uint32_t word_count);
/* entry_to_slot[e] = pool slot of mirror entry e, e < min(occupancy, capacity); host memory. Synchronises the mirror first. */
int gv_pool_mirror_slots(GvCtx* ctx, uint32_t pool_id, uint32_t* entry_to_slot, uint32_t capacity);
/* A counter that changes whenever that table does — a (re)build, slots appended after a bind with a larger occupancy, the
 * re-order of the mirror after entity churn: a consumer of the bit shards compares it with the value it fetched the table at.
 * Synchronises the mirror first (like gv_pool_mirror_slots: the two are consistent with each other). */
int gv_pool_mirror_epoch(GvCtx* ctx, uint32_t pool_id, uint64_t* epoch);

/* A spatial tile's pool slots are not a contiguous range of the world's (roots -> tile, descendants
 * follow): `global_ids[slot]` is the id the exchange should carry for pool slot `slot` (e.g. the mesh slot in the
 * unpartitioned world, garden_amd/multi.py::partition_world's mesh_global). Uploaded once; from then on
 * gv_results_copy_idx_device / gv_results_copy_shard_device / gv_exchange_shards write global_ids[visible_idx] +
 * index_base instead of visible_idx + index_base whenever the table covers the culled pool. count == 0 removes it. */
int gv_pool_set_index_map(GvCtx* ctx, uint32_t pool_id, const uint32_t* global_ids, uint32_t count);
/* Entries [first, first + count) of that table replaced (a few slots of a rank's share changed hands: a root crossed into another
 * rank's cell and its tree moved, SURVEY.md §8e "re-bin only roots whose position crosses a cell"); first + count may exceed the
 * table's size — it grows (slots appended to the share). GV_NONE marks a slot that stands for no world slot (a hole in the share:
 * never visible, skipped by the write-back below). Ordered on gv_stream(ctx) behind the work already queued. */
int gv_pool_update_index_map(GvCtx* ctx, uint32_t pool_id, uint32_t first, const uint32_t* global_ids, uint32_t count);
/* A rank's results delivered in the WORLD's numbering (one process, N contexts: the host fills the engine's buffers from every
 * rank's results, mesh.cpp:144-183). flags:
 *   GV_RESULTS_MAP_RECORDS  records in the pool's record layout (gv_pool_set_record_layout) carry componentOffset =
 *                           index_map[slot] * component_stride (mesh.cpp:170 in the engine's own pool): a rank's records are copied
 *                           into combinedMeshes as they are
 *   GV_RESULTS_MAP_VISIBLE  the write-back of gv_pool_results_fetch(write_back != 0) stores slot i's isVisible byte at
 *                           visible_base + index_map[i] * visible_stride — straight into the engine's pool (mesh.cpp:144,152,161,
 *                           166), wherever the rank's share keeps slot i — instead of into the bound share; entries that are GV_NONE
 *                           or >= visible_count are skipped. The caller guarantees [visible_base, + visible_count * visible_stride)
 *                           until the fetch returns; ranks write disjoint slots.
 * Both need the pool's index map (GV_E_STATE at the fetch while it does not cover the culled pool). GvResult.is_visible stays in
 * the share's own slots. Not available together with gv_pool_bind_ready (GV_E_STATE). flags == 0 removes the mapping. */
#define GV_RESULTS_MAP_RECORDS 1u
#define GV_RESULTS_MAP_VISIBLE 2u
int gv_pool_set_result_mapping(GvCtx* ctx, uint32_t pool_id, uint32_t flags, void* visible_base, size_t visible_stride, uint32_t visible_count);

/* Results are kept per (pool, view). The view-indexed calls above address the pool of the most recent gv_cull; these
 * name the pool, so that a frame can issue the culls (and sort requests) of ALL its mesh systems first and read the
 * results afterwards — the reference's prepareMeshes does the same with its thread pool (dispatch every system's tasks,
 * mesh.cpp:408-546, then one wait, :548) — the device works through the systems back to back, and for engine-sized
 * pools (up to 262144 slots) the first fetch publishes the results of every pool with ONE launch and ONE
 * synchronisation; the other fetches find theirs in the pinned host buffers. A (pool, view)'s results stay valid until
 * the next gv_cull of that pool. */
/* Records in the ENGINE'S OWN struct layout. The reference appends `UnsortedMesh { psize componentOffset; float4x3
 * bakedModel; float distanceSq; }` / `SortedMesh { ... uint32 bufferIndex; }` (render/mesh.hpp:191-205) to combinedMeshes;
 * their padding depends on the math library's alignment of float4x3, so the layout is described, not assumed: once a
 * pool has a record layout, the results of its views are ALSO delivered as an array of such structs in pinned host memory
 * (gv_pool_results_records) — combinedMeshes is then filled with one memcpy instead of a loop over three arrays, and the
 * SoA pointers of GvResult (visible_idx / baked_model / distance_sq) are NULL for that pool (draw_count, instance_count and
 * is_visible are delivered as always). stride: bytes per record, a multiple of 16, at most 128; offsets inside the record:
 * component_offset (uint64 = visible slot * component_stride, mesh.cpp:170), baked_model (12 floats, mesh.cpp:171),
 * distance_sq (float, mesh.cpp:172 / :250-251), buffer_index (uint32 = buffer_index_value, mesh.cpp:252; GV_NONE: the struct
 * has none); bytes not covered by a field are zero. layout == NULL removes it. */
typedef struct GvRecordLayout {
    uint32_t stride;
    uint32_t component_offset, baked_model, distance_sq, buffer_index;
    uint32_t component_stride;   /* getMeshComponentSize() */
    uint32_t buffer_index_value; /* SortedMesh::bufferIndex of this pool's system */
} GvRecordLayout;
int gv_pool_set_record_layout(GvCtx* ctx, uint32_t pool_id, const GvRecordLayout* layout);
/* After gv_pool_results_fetch of the same (pool, view): the records [0, *count) in the pool's record layout (library-owned
 * pinned memory, valid until the next gv_cull of that pool). GV_E_STATE when the pool has no record layout. */
int gv_pool_results_records(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, const void** records, uint32_t* count);
/* The records of (pool, view) into the CALLER'S array — `UnsortedBuffer::combinedMeshes.data()`, which the reference grows and
 * never shrinks (mesh.cpp:377-395): the fetch leaves each frame's records [0, draw_count) there (one memcpy from the library's
 * pinned buffer, inside the fetch — the engine's own copy loop disappears) and gv_pool_results_records returns `records` itself.
 * The array is never page-locked: letting the device write it in place (round 2: hipHostRegister once per address, 4 us less
 * per 10 k-entity tick) made LATER, unrelated copies into pageable memory abort inside the runtime now and then once such an
 * array had been freed and its addresses reused (round 3: 4 of 16 runs of the GPU test tier). The pool needs a
 * record layout; `bytes` >= occupancy * stride of every pool culled while the target is set (GV_E_ARG at the fetch otherwise);
 * `records` 16-byte aligned. The range must stay allocated until it is replaced (another call for the same pool and view),
 * removed (records == NULL) or the context is destroyed. A range that is found unmapped when it is WRITTEN fails that fetch with
 * GV_E_STATE; one found unmapped when it is let go is counted in GvStats::record_targets_lost and described in gv_last_error —
 * the call that replaces it succeeds, the new target is in place (a freed heap block that is still mapped cannot be told from a
 * live one). */
int gv_pool_set_record_target(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, void* records, size_t bytes);

/* The first instance index of every fetched record: bases[k] = sum of the ready counts (gv_pool_bind_ready; 1 per record
 * without) of records [0, k), bases[*count] = the view's instance_count. This is what `instanceCount.fetch_add(
 * getInstancesAsync(view))` hands out draw by draw in the reference's render loops (mesh.cpp:596-599, :624-627, :709-712),
 * available up front and in record order (after gv_sort: in sorted order), so a threaded draw loop needs no atomic and
 * gives the same instance layout every frame. Library-owned host memory ([*count + 1] words), valid until the next gv_cull
 * of the pool; fetches the results first if that has not happened yet. GV_E_STATE for a count-only view. */
int gv_pool_results_instance_bases(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, const uint32_t** bases, uint32_t* count);

/* ---- instance data: what every plugin's drawAsync writes first (sprite.cpp:107-108,122-126) ----
 * `instanceData[instanceIndex].mvp = viewProj * model` for every draw of a view, on the device: the record's bakedModel completed
 * with the bottom row (0,0,0,1) as mesh.cpp:596 does, multiplied from the left by the GvView::view_proj the view was culled with
 * (the reference passes the same matrix to prepareMeshes and to the render loops, mesh.cpp:815,824-838). Arithmetic: DESIGN.md
 * §4 item 9. Instance k of a view belongs to record k of that view as a fetch would deliver it at that moment (after
 * gv_pool_sort: the sorted order); the instance index of draw k is k, because no system of the reference overrides
 * getInstancesAsync (mesh.hpp:89 returns 1). The plugin's instance struct is described, not assumed (like GvRecordLayout):
 * stride: bytes per instance, a multiple of 16, 64 ... 256; mvp: offset of the float4x4 (column-major, 64 bytes, 16-byte aligned),
 * required; model: offset of a copy of the 12 bakedModel floats, or GV_NONE; slot: offset of a uint32 — the record's pool slot
 * (index-mapped when the pool has an index map, as in gv_pick), what a device consumer needs to find the component's own data —
 * or GV_NONE; distance_sq: offset of the record's float key, or GV_NONE. The optional fields are 4-byte aligned; fields lie inside
 * the stride and do not overlap (GV_E_ARG otherwise). layout == NULL removes it. */
typedef struct GvInstanceLayout {
    uint32_t stride;
    uint32_t mvp;
    uint32_t model;
    uint32_t slot;
    uint32_t distance_sq;
} GvInstanceLayout;
int gv_pool_set_instance_layout(GvCtx* ctx, uint32_t pool_id, const GvInstanceLayout* layout);
/* Instance data of the listed views of one pool, back to back in the order listed: view_indices[0]'s draws take instances
 * [0, n0), the next view's [n0, n0 + n1), ... — one main-pass view for the base buffer; the shadow passes in pass order for the
 * shadow buffer, which the reference fills pass after pass behind shadowInstanceIndex (instance.cpp:164,215). One kernel launch
 * on gv_stream(ctx), asynchronous: the counts are read on the device, the host is not synchronised. Counts as a read: culls
 * recorded since gv_cull_batch_begin and sorts that are still deferred are launched first.
 * dst_device NULL: a library-owned device buffer (grown, never shrunk), valid until the next gv_cull of the pool.
 * dst_device non-NULL: caller-owned device memory of capacity_bytes (16-byte aligned); instances that do not fit are not written
 * and the true total is still reported. ONLY the bytes of the layout's fields are written — the rest of each instance belongs to
 * the plugin (sprite.cpp:127-129 writes colour and uv next to mvp; a pool may have those written here too: gv_pool_bind_payload below). The cull side is left as a read through
 * gv_pool_results_device leaves it: recorded culls and deferred sorts have been launched (a small sorted pool with a record layout
 * has then also published its records to the host, and the launches count in GvStats), no result changes.
 * The library-owned buffer is sized for the sum of the listed views' OCCUPANCIES times the stride — the host does not know the
 * counts without a synchronisation — and is never shrunk: four views of a 10^7-slot pool with a 128-byte layout are 5.1 GB for
 * some 2 M records. Large pools should pass a caller-owned target sized for what they expect to draw; what does not fit is
 * not written and the total says so.
 * GV_E_ARG: an unbound pool, view_count 0 or above the views of the pool's last gv_cull, a view index of GV_MAX_VIEWS or more or
 * listed twice, a misaligned dst_device. GV_E_STATE: no instance layout, a count-only view (emit_records == 0), a view with no results,
 * an index map that does not cover the pool, or a ready column (gv_pool_bind_ready) that holds a live count above 1 — such a
 * draw takes several instances, which needs a device scan of the counts (not available; counts of 0 / 1 work). */
int gv_pool_emit_instances(GvCtx* ctx, uint32_t pool_id, const uint32_t* view_indices, uint32_t view_count, void* dst_device,
                           size_t capacity_bytes);
/* Device pointers of the pool's last emission: the instances (dst_device, or the library's buffer) and uint32
 * starts[view_count + 1] (starts[v] = first instance of listed view v, starts[view_count] = the total), both written in stream
 * order on gv_stream(ctx). GV_E_STATE when the pool has no emission since its last gv_cull. */
int gv_pool_instances_device(GvCtx* ctx, uint32_t pool_id, const void** instances, const void** starts);
/* What the pool's last emission was made with (no synchronisation): the number of listed views, the layout's stride and the
 * instances its target holds (any of the pointers may be NULL). GV_E_STATE when there is none since the pool's last gv_cull. */
int gv_pool_instances_info(GvCtx* ctx, uint32_t pool_id, uint32_t* view_count, uint32_t* stride, uint32_t* capacity);
/* Waits for the pool's last emission and delivers it to the host: starts[0 .. view_count] (starts_capacity >= view_count + 1) and
 * — dst_host non-NULL — the instances into the caller's array (the engine's mapped instance buffer), field by field, so that the
 * plugin's own bytes survive; they travel through the library's pinned staging, the caller's memory is never page-locked (the
 * rule of gv_pool_set_record_target). GV_E_ARG when bytes < total * stride or starts_capacity is too small (nothing is written);
 * instances the emission could not fit into a caller-owned device target are not delivered either. */
int gv_pool_instances_fetch(GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* starts, uint32_t starts_capacity);

/* ---- instance data for draws that take several instances (a ready count above 1, gv_pool_bind_ready) ----
 * gv_pool_emit_draw_instances is gv_pool_emit_instances — its arguments, view ordering, "counts as a read", target rules and errors —
 * for a pool whose draws take their ready count of instances, as `instanceCount.fetch_add(getInstancesAsync(view))` hands them out
 * in the reference's draw loops (mesh.cpp:596-599, :624-627, :709-712, :753-756). Draw k of a listed view is record k in delivery
 * order (after gv_pool_sort: the sorted order) and takes c_k = count[visible_idx[k]] instances, read ON THE DEVICE from a mirror of
 * the ready column (one uint32 per pool slot; u8 columns are widened on the way up). Its first instance is
 * first_k = starts[v] + sum of c_j over j < k, starts[v] the instance total of the views listed in front. EVERY instance
 * first_k + j, 0 <= j < c_k, receives the layout's fields of draw k (mvp, model, slot, distance_sq: bit for bit what
 * gv_pool_emit_instances writes for that record), the payload row of the record's pool slot at the payload destinations, and j
 * at the index field when one is set (gv_pool_set_instance_index_field) — no system of the reference overrides getInstancesAsync
 * (mesh.hpp:89), so what the extra instances hold is this build's rule. Only those bytes are written;
 * instances at or beyond the target's capacity are not written, also when the cut falls inside one draw, and the true totals are
 * still reported. A draw whose count has become 0 since the cull takes no instance (first_{k+1} == first_k). Without a ready column
 * every count is 1 and the bytes are those of gv_pool_emit_instances. Two kernel launches on gv_stream(ctx), no host
 * synchronisation; the host never reads a count.
 * The count mirror exists only for a pool with a ready column that has called this function: the first call uploads the whole
 * column; from then on the pool's GV_DIRTY_MESH marks feed a dirty set of its own, which gv_sync or the pool's next draw emission
 * consumes, whichever comes first — a count changed and marked between the cull and the emission is what the emission uses
 * (the reference reads getInstancesAsync at draw time, mesh.cpp:592-597), while the records stay those of the cull. Uploaded bytes
 * count in GvStats::upload_bytes; rebinding or removing the ready column resets the mirror.
 * The library-owned target (dst_device NULL) is sized for the listed views times the sum of the mirrored counts.
 * GV_E_STATE in addition to gv_pool_emit_instances' errors: a ready column together with a result mapping
 * (gv_pool_set_result_mapping); a live count above GV_MAX_DRAW_INSTANCES (in the column at the last gv_sync, or
 * marked since); a library-owned target whose bound does not fit 32 bits of instances (pass a caller-owned target). Counts above 1
 * are NOT refused here. "Live" means a candidate as of the last gv_sync, which is what that sync's culls could draw: a slot that
 * was disabled then and is marked above the limit afterwards goes unnoticed until the next gv_sync. The refusal for marked counts
 * comes after they have been uploaded (nothing is launched; the next upload corrects the mirror). Whatever a count holds, the
 * kernels write inside the target only. */
#define GV_MAX_DRAW_INSTANCES 65535u
int gv_pool_emit_draw_instances(GvCtx* ctx, uint32_t pool_id, const uint32_t* view_indices, uint32_t view_count, void* dst_device,
                                size_t capacity_bytes);
/* Where gv_pool_emit_draw_instances writes a uint32 "index within the draw" (j above) into every instance: 4-byte aligned, inside
 * the stride, disjoint from mvp / model / slot / distance_sq and from the payload destinations — checked here, in
 * gv_pool_set_instance_layout and gv_pool_set_payload_layout against the offset in place, and at the draw emission (GV_E_ARG).
 * GV_NONE removes it. gv_pool_emit_instances ignores it entirely. */
int gv_pool_set_instance_index_field(GvCtx* ctx, uint32_t pool_id, uint32_t offset);
/* Device pointers of the pool's last DRAW emission, written in stream order on gv_stream(ctx): uint32 draw_starts[view_count + 1],
 * the prefix of the listed views' draw counts, and uint32 first_instance[], where first_instance[draw_starts[v] + k] = first_k of
 * draw k of listed view v (an indirect draw's firstInstance); one more word behind the last draw,
 * first_instance[draw_starts[view_count]], holds the grand total. GV_E_STATE when the pool's last emission was not a draw emission.
 * gv_pool_instances_device / _info / _fetch serve the pool's last emission, whichever call made it: after a draw emission starts[]
 * holds INSTANCE starts, and the fetch also delivers the index field when it was written. */
int gv_pool_draw_bases_device(GvCtx* ctx, uint32_t pool_id, const void** first_instance, const void** draw_starts);
/* Waits for the pool's last draw emission and delivers both arrays through the library's pinned staging: draw_starts[0 ..
 * view_count] (starts_capacity >= view_count + 1) and — first_instance non-NULL — first_instance[0 .. draws], the closing total
 * included (capacity >= draws + 1 words). GV_E_ARG when either array is too small: nothing is written. */
int gv_pool_draw_bases_fetch(GvCtx* ctx, uint32_t pool_id, uint32_t* first_instance, uint32_t capacity, uint32_t* draw_starts,
                             uint32_t starts_capacity);

/* ---- indirect draw commands, built on the device ----
 * After a cull and an instance emission the device holds every draw's instances at a known instance index, in draw order.
 * gv_pool_emit_draw_commands writes, behind that emission, one indirect command per draw (or per run of consecutive draws of one
 * geometry) in the caller's own command struct — the buffer a renderer hands to its indirect draw (the reference's
 * DrawIndirectCommand / DrawIndexedIndirectCommand take such a buffer with offset, drawCount and stride,
 * graphics/command-buffer.hpp:210-229) without the host having read a record. No system of the reference issues indirect draws, so
 * the rule is this build's; it holds no arithmetic:
 *   E is the pool's last emission since its last gv_cull (gv_pool_emit_instances or gv_pool_emit_draw_instances); it lists views
 *   v = 0 .. m-1, view v has n_v draws, draw k is record k in delivery order (after gv_pool_sort: the sorted order).
 *   s_k = visible_idx[k] is the record's POOL slot (never the index-mapped slot, never a mirror entry).
 *   first_k, c_k: what E defines — after gv_pool_emit_instances first_k = starts[v] + k and c_k = 1; after a draw emission
 *   first_k = first_instance[draw_starts[v] + k] and c_k = first_{k+1} - first_k, the word behind a view's last draw being starts[v+1].
 *   g_k = id[s_k], read from the geometry id mirror as it stands when the command emission is issued (marks made after the cull
 *   are consumed by it, as for payload and counts); without an id column g_k = 0. While the pool holds a LOD selection made
 *   behind E (gv_pool_select_lods, below), g_k is the selected id of the draw instead, and the id mirror is not read.
 *   G(g) = table[g] if g < table_count, else the void geometry {0, 0, 0}.
 * Per-draw mode (flags 0): view v has C_v = n_v commands, command k = {count G(g_k).count, instance_count c_k (0 when
 *   g_k >= table_count), first G(g_k).first, vertex_offset G(g_k).vertex_offset, first_instance first_k, draw k}.
 * Run mode (GV_COMMANDS_MERGE_RUNS): draw k is a head iff k == 0 || g_k != g_{k-1} (raw ids; a run never crosses a view); C_v is
 *   the number of heads; command r stands for the r-th run [h_r, h_{r+1}): geometry G(g_{h_r}), first_instance first_{h_r},
 *   instance_count first_{h_{r+1}} - first_{h_r} (closing value starts[v+1]; 0 when the id is out of range), draw h_r. Draws whose
 *   count is 0 take part like any other. A run's instances are contiguous in draw order, sorted views included.
 * Placement: region_commands == 0 packs view v's commands at positions sum of C_u (u < v) + j. R = region_commands > 0 puts them
 *   at v * R + j for j < min(C_v, R); commands with j >= R are not written and positions v * R + j, C_v <= j < R, are written as
 *   all-zero commands, so that a host can submit drawCount = R at a host-known offset without reading anything back. A written
 *   command has every byte of its stride defined (bytes outside the layout's fields are 0). Positions at or beyond
 *   capacity_bytes / stride are not written, padding included. command_counts[v] = C_v is always the true count.
 * An id at or beyond table_count is NOT an error: it yields the void command. Whatever an id holds, the kernels read inside the
 * table only. */
#define GV_MAX_GEOMETRIES 65536u
typedef struct GvGeometry {
    uint32_t count, first;   /* indexCount / firstIndex (vertexCount / firstVertex of a non-indexed draw) */
    int32_t vertex_offset;
} GvGeometry;
/* The pool's geometry ids and the table they index. ids: element i at ids + i * stride, width 1, 2 or 4 bytes (widened to uint32 on
 * the way up, like the ready column), covering `occupancy` slots; ids == NULL: every slot draws table[0] and no mirror is kept. The
 * table (<= GV_MAX_GEOMETRIES entries) is copied at the call. ids == NULL && table == NULL removes both. Lifetime of `ids` as
 * gv_pool_bind_ready. The id mirror — one uint32 per POOL slot — exists only once gv_pool_emit_draw_commands has been called for a
 * pool with an id column: that call uploads the column; from then on GV_DIRTY_GEOMETRY and the pool's GV_DIRTY_MESH marks feed a
 * dirty set of its own, consumed by gv_sync or the pool's next command emission, whichever comes first. Uploaded bytes (ids, the
 * packet's slots, the table) count in GvStats::upload_bytes; a rebind resets the mirror.
 * GV_E_ARG: a pool out of range, a width other than 1, 2 or 4, stride < width, a NULL table with table_count > 0, table_count 0
 * with a table or ids, table_count above the limit, an occupancy beyond the 28-bit slot range. */
int gv_pool_bind_geometry(GvCtx* ctx, uint32_t pool_id, const void* ids, uint32_t stride, uint32_t width, uint32_t occupancy,
                          const GvGeometry* table, uint32_t table_count);
typedef struct GvCommandLayout {   /* described, not assumed - like GvInstanceLayout */
    uint32_t stride;               /* a multiple of 4, 16 ... 64 */
    uint32_t count, instance_count, first, first_instance;   /* required uint32 fields */
    uint32_t vertex_offset;        /* int32, or GV_NONE (non-indexed draws) */
    uint32_t draw;                 /* uint32, or GV_NONE */
} GvCommandLayout;                 /* fields 4-byte aligned, inside the stride, disjoint: GV_E_ARG otherwise */
int gv_pool_set_command_layout(GvCtx* ctx, uint32_t pool_id, const GvCommandLayout* layout);   /* NULL removes it */
#define GV_COMMANDS_MERGE_RUNS 1u
/* The commands of the views of E, in E's order. Asynchronous on gv_stream(ctx), the host reads no count; counts as a read
 * (recorded culls and deferred sorts are launched first, as for the emissions); changes no cull result and no instance data. The
 * result is valid until the next gv_cull or the next instance emission of the pool. dst_device NULL: a library-owned buffer, grown
 * and never shrunk — packed, sized for the sum of the listed views' occupancies x stride; with regions for m * R x stride. A
 * non-NULL dst_device is caller-owned and 16-byte aligned. One launch in per-draw mode, three in run mode, counted under
 * GvStats::launches[GV_K_EMIT].
 * GV_E_ARG: a pool out of range, unknown flag bits, a misaligned dst_device, m * R beyond 32 bits. GV_E_STATE: no command
 * layout, no geometry bound, no emission since the pool's last gv_cull, an id column whose occupancy is below a listed view's. */
int gv_pool_emit_draw_commands(GvCtx* ctx, uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device,
                               size_t capacity_bytes);
/* Device pointers of the pool's last command emission, written in stream order: the commands and uint32 command_counts[m]. */
int gv_pool_draw_commands_device(GvCtx* ctx, uint32_t pool_id, const void** commands, const void** command_counts);
/* Waits for the pool's last command emission; copies command_counts[0 .. m-1] (counts_capacity >= m) and — dst_host non-NULL — the
 * command positions the target holds (packed: min(sum of C_v, capacity); regions: min(m * R, capacity)) through the library's
 * pinned staging, whole commands (the library wrote every byte). GV_E_ARG when either array is too small: nothing is written. */
int gv_pool_draw_commands_fetch(GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* command_counts,
                                uint32_t counts_capacity);

/* ---- level of detail per draw, selected on the device ----
 * The geometry id of a draw is id[s_k], one value per pool slot; with levels of detail it depends on the view too. The reference
 * carries the data and no rule: ModelRenderComponent::lods is a vector<ModelLOD> (include/garden/system/render/model.hpp:29-41)
 * and nothing in source/ picks among its entries, so the rule is this build's. gv_pool_select_lods applies
 * it behind the pool's last instance emission E, in draw order, from what the device already holds; a command emission that
 * follows takes the selected ids. With E, v, k and s_k as for the draw commands above:
 *   b_k = id[s_k], read from the geometry id mirror as it stands when the selection is issued; without an id column b_k = 0.
 *   r_k = size[s_k]: the bound size column, one fp32 per pool slot, copied verbatim (the engine decides what it measures, for
 *     example a world-space bounding radius); without a column r_k = 1.0f.
 *   t = the translation column of the record's bakedModel as delivered (floats 9, 10, 11): the pivot relative to
 *     camera_position, WITHOUT camera_offset. d2 = fmaf(tz, tz, fmaf(ty, ty, tx * tx)).
 *   x = d2 * view_scale[v], one fp32 multiply; view_scale[v] may hold (tan(fov / 2) / height)^2, a quality bias, or 1.
 *   e = lod_table[b_k] if b_k < lod_table_count, otherwise one level.
 *   For i = 0 .. e.levels - 2: y_i = r_k * e.switch_at[i], q_i = y_i * y_i.
 *   level_k = the NUMBER of i with x > q_i. A count: unsorted thresholds are defined. A comparison with a NaN is false, so a NaN
 *     size, distance or scale gives level 0, the finest; an infinite x gives the coarsest level over finite thresholds; an exact
 *     tie keeps the finer level.
 *   g_k = b_k + level_k as a uint32 add: the levels of one geometry are consecutive entries of the geometry table. An id at or
 *     beyond the geometry table's count yields the void command, as above.
 * Views that share camera_position select the same level for a slot given the same scale: that follows from the rule. */
#define GV_MAX_LOD_LEVELS 8u
typedef struct GvLodGeometry {
    uint32_t levels;                            /* 1 .. GV_MAX_LOD_LEVELS */
    float switch_at[GV_MAX_LOD_LEVELS - 1];     /* the first levels - 1 are read; in units of distance per size */
} GvLodGeometry;                                /* 32 bytes */
/* The pool's sizes and the table the BASE ids index. sizes: element i at sizes + i * stride (stride >= 4), fp32, covering
 * `occupancy` slots; sizes == NULL with a table: every slot has size 1 and no mirror is kept. The table (<= GV_MAX_GEOMETRIES
 * entries, levels 1 .. GV_MAX_LOD_LEVELS each) is copied at the call. sizes == NULL && table == NULL removes the binding (and a
 * selection the pool holds). Lifetime of `sizes` as gv_pool_bind_ready. The size mirror — one word per POOL slot — exists only
 * once gv_pool_select_lods has been called for a pool with a size column: that call uploads the column; from then on GV_DIRTY_LOD
 * and the pool's GV_DIRTY_MESH marks feed a dirty set of its own, consumed by gv_sync or the pool's next selection, whichever
 * comes first. No cull reads it. Uploaded bytes count in GvStats::upload_bytes; a rebind resets the mirror.
 * GV_E_ARG: a pool out of range, stride < 4, sizes without a table, a NULL table with table_count > 0, table_count 0 with a
 * table, table_count above the limit, levels outside 1 .. 8 in an entry, an occupancy beyond the 28-bit slot range. */
int gv_pool_bind_lod(GvCtx* ctx, uint32_t pool_id, const void* sizes, uint32_t stride, uint32_t occupancy, const GvLodGeometry* table,
                     uint32_t table_count);
/* Selects the level of every draw of E: draw_geometry[D_v + k] = g_k with D_v the sum of the draw counts of the views listed in
 * front (read on the device), and level_counts[v * GV_MAX_LOD_LEVELS + L] = the draws of view v at level L. Asynchronous on
 * gv_stream(ctx); counts as a read (recorded culls and deferred sorts are launched first); consumes the pending id and size marks.
 * One kernel launch (plus a memset of the histogram), counted under GvStats::launches[GV_K_EMIT]. The buffers are library-owned,
 * sized for the sum of the listed views' occupancies, grown and never shrunk. view_scale: one float per view of E, in E's order.
 * While the pool holds a selection made behind E, gv_pool_emit_draw_commands takes g_k from draw_geometry instead of id[s_k], in
 * both modes (run heads compare the selected ids), and does not re-read marks made after the selection. The selection ends where
 * E's commands end: at the pool's next gv_cull or instance emission. view_scale == NULL with view_count == 0 drops it.
 * GV_E_ARG: a pool that is not bound, view_scale NULL with view_count > 0, view_count other than E's. GV_E_STATE: no LOD binding,
 * no geometry bound, no emission since the pool's last gv_cull, a size or id column whose occupancy is below a listed view's. */
int gv_pool_select_lods(GvCtx* ctx, uint32_t pool_id, const float* view_scale, uint32_t view_count);
/* Device pointers of the pool's selection, written in stream order: uint32 draw_geometry[sum of n_v] and uint32
 * level_counts[m * GV_MAX_LOD_LEVELS]. GV_E_STATE: the pool holds no selection. */
int gv_pool_lods_device(GvCtx* ctx, uint32_t pool_id, const void** draw_geometry, const void** level_counts);
/* Waits for the pool's selection; copies level_counts[0 .. m * GV_MAX_LOD_LEVELS) (counts_capacity at least that) and —
 * draw_geometry non-NULL — the selected ids of the listed views, back to back (capacity >= the sum of the draw counts, which is
 * the sum of level_counts). GV_E_ARG when either array is too small: nothing is written. */
int gv_pool_lods_fetch(GvCtx* ctx, uint32_t pool_id, uint32_t* draw_geometry, uint32_t capacity, uint32_t* level_counts,
                       uint32_t counts_capacity);

/* ---- mesh clusters, culled per draw on the device ----
 * The commands above draw a geometry whole, however much of it lies outside the frustum or behind the occluders the pyramid
 * describes. A pool may bind, per geometry id, a range of CLUSTERS: each a model-space box and a range of the geometry's indices.
 * gv_pool_cull_clusters tests every cluster of every draw of E with the draw's own matrix and writes one indirect command per
 * surviving cluster. The reference has no clusters (ModelLOD carries index ranges and nothing smaller), so the rule is this
 * build's; it holds no new arithmetic: a cluster is tested exactly as the cull tests an entity. With E, v,
 * k, s_k, g_k, first_k, c_k and G(g) as for the draw commands above (g_k the selected id while the pool holds a LOD selection made
 * behind E, id[s_k] from the id mirror otherwise; pending id marks are consumed as the command emission consumes them):
 *   M_k = the record's 12 bakedModel floats as delivered, completed with the row (0, 0, 0, 1). VP_v = the view_proj view v was
 *   culled with, planes = the cull's plane extraction of VP_v; camera_offset plays no part, as in the entity test.
 *   range_k = ranges[g_k] if g_k < range_count, else {0, 0}.
 *   A draw with g_k >= table_count (the void geometry) or c_k == 0 emits nothing.
 *   A draw whose range_k.count == 0 is DRAWN WHOLE: one command exactly as per-draw mode writes it, untested (the draw was culled
 *   already; sprites beside clustered models keep working).
 *   Otherwise, for j = 0 .. range_k.count - 1, cl = clusters[range_k.first + j]: cluster j SURVIVES iff its eight corners
 *   (cl's box through M_k, the cull's packed-fp32 corner form) are not all behind one plane and — unless GV_CLUSTERS_FRUSTUM_ONLY
 *   is set or view v named no pyramid (use_hiz == 0) — the cull's Hi-Z query of those corners against the pyramid view v names, as
 *   that pyramid stands when the call is issued, does not find them occluded. A NaN box behaves as it does for an entity.
 *   A surviving cluster emits {count cl.count, instance_count c_k, first G(g_k).first + cl.first (uint32 add), vertex_offset
 *   G(g_k).vertex_offset, first_instance first_k, draw k} in the pool's GvCommandLayout.
 * Order: by view, then draw k ascending, then j ascending; reproducible run to run. counts[v] = commands of view v, always the
 * true count; counts[m + v] = clusters tested for view v (whole draws are not tested). Placement (region_commands), zero padding,
 * "every byte of the stride" and "positions at or beyond capacity are not written" as for gv_pool_emit_draw_commands. */
#define GV_MAX_CLUSTERS          (1u << 22)   /* entries of a pool's cluster table (128 MB) */
#define GV_MAX_GEOMETRY_CLUSTERS 65535u       /* clusters of one geometry */
typedef struct GvCluster {      /* 32 bytes */
    float box_min[3]; uint32_t first;   /* model-space box; first index RELATIVE to G(g).first */
    float box_max[3]; uint32_t count;   /* index count of the cluster */
} GvCluster;
typedef struct GvClusterRange { uint32_t first, count; } GvClusterRange;  /* into the cluster table, indexed by geometry id g */
#define GV_CLUSTERS_FRUSTUM_ONLY 1u
/* Both tables are copied at the call (uploaded bytes count in GvStats::upload_bytes); NULL / 0 for both removes the binding. Either
 * way a cluster result the pool holds ends. Box values are not checked. GV_E_ARG: a pool out of range, one table without the other,
 * range_count above GV_MAX_GEOMETRIES or cluster_count above GV_MAX_CLUSTERS, a range with count > GV_MAX_GEOMETRY_CLUSTERS or
 * first + count > cluster_count (64-bit sum). */
int gv_pool_bind_clusters(GvCtx* ctx, uint32_t pool_id, const GvClusterRange* ranges, uint32_t range_count, const GvCluster* clusters,
                          uint32_t cluster_count);
/* The cluster commands of the views of E, in E's order. Asynchronous on gv_stream(ctx), the host reads no count; counts as a read
 * (recorded culls and deferred sorts are launched first); changes no cull result, no instance data and no per-draw command buffer
 * (buffers of its own: both kinds of commands coexist). FIVE kernel launches whatever the data holds — candidate counts per draw,
 * their scan, the test, the survivors' scan, the writer — counted under GvStats::launches[GV_K_EMIT]. The scratch is sized from
 * the host's bound of the candidates, B = the sum of the listed views' occupancies x max(1, the largest bound range count): 8 bytes
 * per 256 candidates and one bit per candidate. dst_device NULL: a library-owned buffer, grown and never shrunk, sized for B (with
 * regions: m * R) commands; where that exceeds 2 GiB the call is refused and asks for a caller-owned target. A non-NULL dst_device
 * is caller-owned and 16-byte aligned. The result ends at the pool's next gv_cull, second phase, instance emission or
 * gv_pool_bind_clusters.
 * GV_E_ARG: a pool out of range or not bound, unknown flag bits, a misaligned dst_device, m * R beyond 32 bits. GV_E_STATE: no
 * cluster binding, no command layout, no geometry bound, no emission since the pool's last gv_cull, an id column whose occupancy is
 * below a listed view's, a view that names a pyramid that is not built (without GV_CLUSTERS_FRUSTUM_ONLY), B beyond 2^32 - 1, a
 * library-owned target beyond 2 GiB. A refused call changes nothing. */
int gv_pool_cull_clusters(GvCtx* ctx, uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device, size_t capacity_bytes);
/* Device pointers of the pool's last cluster cull, written in stream order: the commands and uint32 counts[2 * m]. */
int gv_pool_cluster_commands_device(GvCtx* ctx, uint32_t pool_id, const void** commands, const void** counts);
/* Waits for the pool's last cluster cull; copies counts[0 .. 2 * m) (counts_capacity at least that) and — dst_host non-NULL — the
 * command positions the target holds (packed: min(sum of counts[v], capacity); regions: min(m * R, capacity)), whole commands.
 * GV_E_ARG when either array is too small: nothing is written. */
int gv_pool_cluster_commands_fetch(GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* counts, uint32_t counts_capacity);

/* ---- the second phase of the cluster cull ----
 * gv_pool_cull_clusters tests against the pyramid a view names, and that pyramid is a frame old: a cluster that has just come out
 * from behind an occluder is rejected for a frame. gv_pool_cull_clusters_second_phase tests what the pool's cluster cull left out
 * again, against the pyramid as it stands now. The draws the draw-level second phase
 * (gv_pool_cull_second_phase) newly delivers are an ordinary view: an emission and gv_pool_cull_clusters cover them. Frame order:
 *   cull -> emit -> gv_pool_cull_clusters -> draw -> gv_hiz_build / _rebuild -> gv_pool_cull_clusters_second_phase -> draw ->
 *   gv_pool_cull_second_phase -> emit -> gv_pool_cull_clusters for the second view.
 * Let K1 be the pool's current cluster result, and E, v, k, j, M_k, VP_v, the planes, g_k, c_k and first_k exactly the ones K1
 * used: g_k is the id K1 kept for the draw — an id mark made after K1 plays no part, nor does a LOD selection made or dropped
 * after K1.
 *   A cluster candidate is PENDING iff K1 tested it, K1 did not keep it, and K1 queried a pyramid for its view (the view's use_hiz
 *   != 0 and K1 was made without GV_CLUSTERS_FRUSTUM_ONLY). Whole draws, void draws, K1's survivors and the clusters of a view K1
 *   did not query are never pending.
 *   A pending cluster SURVIVES iff the unchanged test keeps it: the same corners through M_k, the same planes, the Hi-Z query
 *   against the pyramid view v names as that pyramid stands when THIS call is issued. A frustum reject of K1 is pending and is
 *   rejected again by the same arithmetic.
 *   A survivor emits the command K1 would have written for it: {cl.count, c_k, G(g_k).first + cl.first, G(g_k).vertex_offset,
 *   first_k, k} in the pool's GvCommandLayout.
 * Order: by view, then k, then j. counts[v] = commands of view v, always the true count; counts[m + v] = pending clusters
 * re-tested for view v. Placement (region_commands), zero padding, "every byte of the stride", "positions at or beyond capacity are
 * not written", the library-owned (sized for K1's bound B, or m * R) or caller-owned 16-byte aligned target and the 2 GiB refusal
 * as for gv_pool_cull_clusters. The result lives in buffers of its own: K1's commands, counts, bits and scratch are not written, so
 * K1's fetch returns the same bytes before and after, the call is repeatable (twice against the same pyramid: identical bytes), and
 * against the pyramid K1 itself queried it gives zero commands in every view.
 * Asynchronous on gv_stream(ctx), the host reads no count; counts as a read. FIVE kernel launches whatever the data holds — pending
 * counts per candidate tile, their scan, the test with one lane per PENDING cluster, the survivors' scan, the writer — counted
 * under GvStats::launches[GV_K_EMIT]. Scratch from B: 12 bytes per 256 candidates and one bit per candidate. The result ends
 * wherever K1 ends (gv_cull, gv_pool_cull_second_phase, an instance emission, gv_pool_bind_clusters) and at a new
 * gv_pool_cull_clusters of the pool.
 * flags must be 0. GV_E_ARG: a pool out of range or not bound, flags != 0, a misaligned dst_device, m * R beyond 32 bits.
 * GV_E_STATE: the pool holds no cluster result; a queried view names a pyramid that is not built (gv_hiz_drop);
 * gv_pool_bind_geometry or gv_pool_set_command_layout was called since K1 (K1's kept ids may lie outside a new table: cull the
 * clusters again); a library-owned target beyond 2 GiB. A refused call changes nothing. */
int gv_pool_cull_clusters_second_phase(GvCtx* ctx, uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device,
                                       size_t capacity_bytes);
/* Device pointers of the pool's last cluster second phase, written in stream order: the commands and uint32 counts[2 * m]. */
int gv_pool_cluster_second_commands_device(GvCtx* ctx, uint32_t pool_id, const void** commands, const void** counts);
/* As gv_pool_cluster_commands_fetch, of the pool's last cluster second phase. */
int gv_pool_cluster_second_commands_fetch(GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* counts,
                                          uint32_t counts_capacity);

/* ---- the cluster cull, adjacent survivors merged into runs ----
 * A cluster table usually lays a geometry's clusters out back to back in the index buffer (first[j + 1] == first[j] + count[j]), and
 * most clusters of a delivered draw survive: one command per cluster then writes, and makes the renderer walk, many commands where
 * a few draw the same indices. gv_pool_cull_cluster_runs makes the decisions of gv_pool_cull_clusters and writes one command per RUN
 * of adjacent surviving clusters (this build's rule, the reference has no clusters). E, v, k, j, M_k, g_k,
 * c_k, first_k, G(g), range_k, "drawn whole", "void", SURVIVES and the order are exactly those of gv_pool_cull_clusters: a cluster
 * survives under precisely the same test. With cl_j = clusters[range_k.first + j]:
 *   Cluster j of draw k is LINKED to its predecessor iff j > 0, j % GV_CLUSTER_RUN_SPAN != 0, (uint64)cl_{j-1}.first +
 *   cl_{j-1}.count == cl_j.first, and (uint64)cl_j.first + cl_j.count <= 0xFFFFFFFF. Linked is static: a property of the bound
 *   tables and j alone, not of the matrix, the view, or which other views or draws E holds.
 *   A surviving cluster j is a HEAD iff it is not linked, or cluster j - 1 did not survive.
 *   A RUN is a head plus every following cluster j + 1, j + 2, ... of the same draw, taken while each survives and is linked. So a
 *   run never leaves its draw, holds at most GV_CLUSTER_RUN_SPAN clusters, and its index range is one interval that cannot wrap.
 *   A run from head h to last cluster l emits {count cl_l.first + cl_l.count - cl_h.first (= the sum of its clusters' counts),
 *   instance_count c_k, first G(g_k).first + cl_h.first (uint32 add, as gv_pool_cull_clusters), vertex_offset G(g_k).vertex_offset,
 *   first_instance first_k, draw k} in the pool's GvCommandLayout. Zero-count clusters need no special case.
 *   A draw drawn whole emits its one command as gv_pool_cull_clusters writes it and is never merged with anything.
 * Order: by view, draw k ascending, head j ascending. counts[v] = commands of view v (whole draws + runs), always the true count;
 * counts[m + v] = clusters tested, as gv_pool_cull_clusters. flags (0 or GV_CLUSTERS_FRUSTUM_ONLY), placement (packed or regions),
 * zero padding, "every byte of the stride", "positions at or beyond capacity are not written", the library-owned target sized for B
 * (with regions m * R), its 2 GiB refusal, the 16-byte alignment of a caller-owned one, every GV_E_ARG and GV_E_STATE row and "a
 * refused call changes nothing": as for gv_pool_cull_clusters.
 * GV_CLUSTER_RUN_SPAN bounds the writer's walk from a head to its run's end to SPAN / 64 + 1 = five 64-candidate ballot words,
 * whatever a draw's cluster count; it costs one extra command per 256 clusters of an unbroken layout.
 * The call IS a cluster cull of the pool: its result replaces the pool's cluster result and is replaced by the next one of either
 * form; gv_pool_cluster_commands_device / _fetch serve it unchanged, and it ends where a cluster result ends.
 * gv_pool_cull_clusters_second_phase behind it works as behind the plain form (the same pending set) and writes one command per
 * cluster. Asynchronous on gv_stream(ctx), the host reads no count; counts as a read. SIX kernel launches whatever the data holds —
 * candidate counts per draw, their scan, the test (which also marks the links), the heads, their scan, the writer — counted under
 * GvStats::launches[GV_K_EMIT]. Scratch from B: that of gv_pool_cull_clusters plus two bits per candidate and 4 bytes per 256.
 * Not built: runs for the second phase's commands, runs longer than the span, merging across draws of one geometry. */
#define GV_CLUSTER_RUN_SPAN 256u
int gv_pool_cull_cluster_runs(GvCtx* ctx, uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device,
                              size_t capacity_bytes);

/* ---- the cluster cull with normal-cone backface rejection ----
 * On a closed mesh about half of the clusters that pass the frustum face away from the viewer; neither the frustum test nor the
 * pyramid removes them. A pool may bind one normal CONE per entry of its cluster table (meshoptimizer's meshopt_Bounds cone_apex /
 * cone_axis / cone_cutoff fit as they are), and gv_pool_cull_cluster_cones makes the decisions of gv_pool_cull_clusters with one
 * more rejection (this build's rule, the reference has no clusters). A triangle faces away from an eye
 * exactly when the eye lies behind its plane, and an affine map with positive determinant keeps that relation: the cone is tested IN
 * MODEL SPACE. The eye is carried there with the adjugate of the draw's 3x3 block; no normal is transformed, nothing is divided, no
 * root is taken, and non-uniform scale needs no special case.
 * An EYE is given per view of E, in the records' space (bakedModel as delivered: relative to the cull's camera_position):
 *   eye[3] != 0: a point eye P = eye[0..2]; the main camera is (0, 0, 0, 1).
 *   eye[3] == 0: parallel rays that travel along D = eye[0..2]; a shadow cascade passes the light's direction.
 *   An all-zero eye switches the cone test off for that view (by the rule below, no special case).
 * With E, v, k, j, M_k as for gv_pool_cull_clusters, the draw's 12 bakedModel floats f (a_rc = f[3c + r], t_r = f[9 + r]), and
 * cone = cones[range_k.first + j], in fp32, every step as written (fmaf: one rounding):
 *   j_rc: the nine adjugate entries, each p * q - r * s as fmaf(p, q, -(r * s)):
 *     j00 = a11 a22 - a12 a21, j01 = a02 a21 - a01 a22, j02 = a01 a12 - a02 a11,
 *     j10 = a12 a20 - a10 a22, j11 = a00 a22 - a02 a20, j12 = a02 a10 - a00 a12,
 *     j20 = a10 a21 - a11 a20, j21 = a01 a20 - a00 a21, j22 = a00 a11 - a01 a10  (the expressions of gv_pick's affine inverse);
 *   det = fmaf(a00, j00, fmaf(a01, j10, a02 * j20));  facing = det > 0 && det < +inf.
 *   Point eye, r = 0, 1, 2: u_r = P_r - t_r; w_r = fmaf(det, apex_r, -fmaf(j_r0, u_0, fmaf(j_r1, u_1, j_r2 * u_2))).
 *   Direction eye: w_r = fmaf(j_r0, D_0, fmaf(j_r1, D_1, j_r2 * D_2)).
 *   s = fmaf(w_0, axis_0, fmaf(w_1, axis_1, w_2 * axis_2)); ww = fmaf(w_0, w_0, fmaf(w_1, w_1, w_2 * w_2));
 *   q = s * s; r = (cutoff * cutoff) * ww.
 *   Cluster j of draw k is CONE-REJECTED in view v iff facing && s > 0 && q > 0 && q < +inf && q >= r.
 * w is det * (apex - the eye in model space): the test is meshoptimizer's dot(normalize(apex - eye), axis) >= cutoff multiplied
 * through by positive quantities. Consequences: a NaN anywhere keeps the cluster; a zero axis (meshoptimizer's degenerate cone)
 * keeps it; an eye at the apex keeps it; an overflowing q keeps it; a mirrored, singular or non-finite model (det <= 0, inf, NaN)
 * is never cone-rejected — a mirrored model flips the winding, and what the renderer does with that is not ours to guess; cutoff
 * enters squared, so its sign is not read (a cutoff below 0 names a cone wider than a half-space: give such a cluster a zero axis).
 * The rule is bit-defined but NOT padded: the tool that builds the cones carries the rounding margin in cutoff.
 *   A cluster SURVIVES iff it survives gv_pool_cull_clusters' unchanged test and is not cone-rejected.
 * Whole draws, void draws, the order, the commands, placement, counts[v] and counts[m + v] (a cone-rejected cluster counts as
 * tested) are exactly those of gv_pool_cull_clusters. */
typedef struct GvClusterCone {   /* 32 bytes */
    float apex[3];  float cutoff;
    float axis[3];  uint32_t reserved;   /* not read */
} GvClusterCone;
typedef struct GvClusterEye { float eye[4]; } GvClusterEye;   /* one per view of E */
#define GV_CLUSTERS_RUNS 2u   /* gv_pool_cull_cluster_cones and gv_pool_cull_cluster_lods only: write runs, as gv_pool_cull_cluster_runs */
/* Binds cones[0 .. cone_count), parallel to the pool's cluster table; copied at the call, the bytes counted in upload_bytes. NULL /
 * 0 removes the binding. Either way a cluster result the pool holds ends. gv_pool_bind_clusters (a new table, or removal) also drops
 * the cones. Cone values are not checked. GV_E_ARG: a pool out of range, a pointer without a count or a count without a pointer,
 * cone_count different from the bound cluster_count. GV_E_STATE: no cluster binding. */
int gv_pool_bind_cluster_cones(GvCtx* ctx, uint32_t pool_id, const GvClusterCone* cones, uint32_t cone_count);
/* The cluster commands of the views of E under the rule above. eyes[0 .. eye_count): one per view of E, in E's order, copied at the
 * call. flags: a subset of {GV_CLUSTERS_FRUSTUM_ONLY, GV_CLUSTERS_RUNS}; only this call takes GV_CLUSTERS_RUNS (gv_pool_cull_clusters
 * and gv_pool_cull_cluster_runs refuse it). Without GV_CLUSTERS_RUNS one command per survivor, in FIVE kernel launches; with it the
 * survivors are written as the runs of gv_pool_cull_cluster_runs — the same LINKED / HEAD / RUN rule over these decisions — in SIX.
 * The launches are those of the form it takes, the test launch carrying the cone test in front of the Hi-Z query; counted under
 * GvStats::launches[GV_K_EMIT]; the scratch is that of the form it takes. Placement, targets, capacity, counts: as the form it takes.
 * The call IS a cluster cull of the pool: its result replaces the pool's cluster result and is replaced by the next one of any form;
 * gv_pool_cluster_commands_device / _fetch serve it, and it ends where a cluster result ends (and at gv_pool_bind_cluster_cones).
 * gv_pool_cull_clusters_second_phase behind a cone result applies the same conjunction — the unchanged test against the pyramid as
 * it stands at that call, and the cone test with this call's eyes and the cone table. Its pending set is defined as before (tested,
 * not kept, in a queried view), so CONE-REJECTED CLUSTERS ARE PENDING: they are re-tested, rejected again, counted in its
 * counts[m + v], and cost one cone test each. Behind a plain or a run result the second phase is unchanged.
 * Errors: those of gv_pool_cull_clusters, plus GV_E_ARG: eyes NULL, eye_count different from the views of E; GV_E_STATE: no cone
 * binding. A refused call changes nothing.
 * Not built: cones packed into 16 bytes (meshoptimizer's cone_axis_s8 / cone_cutoff_s8), a per-view count of cone-rejected
 * clusters, leaving cone-rejected clusters out of the second phase's pending set (a second bit per candidate), cones for mirrored
 * models, eyes derived from view_proj. */
int gv_pool_cull_cluster_cones(GvCtx* ctx, uint32_t pool_id, uint32_t flags, const GvClusterEye* eyes, uint32_t eye_count,
                               uint32_t region_commands, void* dst_device, size_t capacity_bytes);

/* ---- the cluster cull with a level-of-detail cut per draw ----
 * The tools that build clusters (meshoptimizer's clusterlod, Nanite-style builders) build a DAG of them: the leaves plus coarser
 * clusters, each simplified from a group of finer ones. Every cluster carries the bounds and error of the group it was simplified
 * FROM (self) and of the group it was merged INTO (parent), and the renderer draws the CUT: a cluster is drawn exactly when its own
 * error is small enough on screen and its parent's is not. A pool may bind one GvClusterLod per entry of its cluster table, and
 * gv_pool_cull_cluster_lods makes the decisions of gv_pool_cull_clusters (and, given eyes, of gv_pool_cull_cluster_cones) over the
 * cut alone (this build's rule, the reference has no clusters).
 * A GvClusterLodView is given per view of E, in E's order. The eye is in the records' space (bakedModel as delivered), with the
 * meaning GvClusterEye has:
 *   eye[3] != 0: a point P = eye[0..2]; the main camera is (0, 0, 0, 1), and a cascade that wants the main view's cut names the
 *                same point.
 *   eye[3] == 0: a parallel projection whose error does not depend on distance.
 *   scale is k: the projection factor divided by the pixel threshold tau. Perspective: k = (height / 2) / tan(fovy / 2) / tau.
 *   Parallel: k = pixels per world unit / tau, with near_distance = 1.
 *   scale == 0 (+-0) switches the test off for that view: every cluster is LOD-kept, the call's bytes equal the plain form's.
 * With E, v, k, j, M_k as for gv_pool_cull_clusters, the draw's 12 bakedModel floats f (a_rc = f[3c + r], t_r = f[9 + r]) and
 * lod = lods[range_k.first + j], in fp32, every step as written (fmaf: one rounding):
 *   Per draw: n_c = fmaf(a_2c, a_2c, fmaf(a_1c, a_1c, a_0c * a_0c)) for c = 0, 1, 2;
 *     s2 = 0.0f; s2 = n_0 > s2 ? n_0 : s2; then the same for n_1 and n_2 — the largest squared column norm: for one TRS exactly
 *     the largest scale squared, for sheared chains an approximation.
 *   Per triple (c, r, e), for the self triple and for the parent triple:
 *     C_r = fmaf(a_r0, c_0, fmaf(a_r1, c_1, fmaf(a_r2, c_2, t_r)))   (item 5's nesting)
 *     u_r = C_r - P_r;  D = fmaf(u_2, u_2, fmaf(u_1, u_1, u_0 * u_0))   (item 7's nesting)
 *     q = e * k;  a = q + r;  A = (a * a) * s2;  Q = (q * q) * s2;  N = near_distance * near_distance.
 *     Point eye:    EXCEEDS iff Q > N && A > D.
 *     Parallel eye: EXCEEDS iff Q > N.
 *   This is e * k * s > max(dist - r * s, near) multiplied through by positive quantities: nothing is divided, no root is taken.
 *   Cluster j of draw k is LOD-KEPT in view v iff !EXCEEDS(self) && EXCEEDS(parent).
 * Consequences: a leaf (e = 0) never exceeds; a root (parent_error = +inf) is always refined-from, unless D overflows or s2 is 0;
 * a comparison with a NaN is false, so a NaN in the self triple makes the cluster "fine enough" and a NaN in the parent triple
 * rejects it; an eye inside a sphere gives A > D by itself, so refinement goes on until the error is below the near clamp. All
 * clusters of one group carry the same parent triple, so they get the same bits and the same decision: that is why the cut has no
 * cracks, and it is the table builder's property, not checked here. The rule is bit-defined and NOT padded: monotone errors and
 * nested spheres are the builder's business, as the cone's cutoff margin is.
 *   A cluster SURVIVES iff it is LOD-kept, survives gv_pool_cull_clusters' unchanged test and, when eyes are given, is not
 *   cone-rejected.
 * Whole draws, void draws, the order (view, draw, cluster), the commands, placement, counts[v] and counts[m + v] (a LOD-rejected
 * cluster counts as tested) are exactly those of gv_pool_cull_clusters. */
typedef struct GvClusterLod {   /* 48 bytes; meshoptimizer clusterlod bounds fit as they are */
    float self_center[3];   float self_radius;    /* model space: the group this cluster was simplified FROM */
    float parent_center[3]; float parent_radius;  /* the group this cluster was merged INTO */
    float self_error, parent_error;               /* model-space units; leaves 0, roots +inf as parent_error */
    uint32_t reserved[2];                         /* not read */
} GvClusterLod;
typedef struct GvClusterLodView { float eye[4]; float scale; float near_distance; float reserved[2]; } GvClusterLodView;   /* 32 bytes */
/* Binds lods[0 .. lod_count), parallel to the pool's cluster table; copied at the call, the bytes counted in upload_bytes. NULL / 0
 * removes the binding. Either way a cluster result the pool holds ends. gv_pool_bind_clusters (a new table, or removal) also drops
 * the LOD table, as it drops the cones. Values are not checked. GV_E_ARG: a pool out of range, a pointer without a count or a count
 * without a pointer, lod_count different from the bound cluster_count. GV_E_STATE: no cluster binding. */
int gv_pool_bind_cluster_lods(GvCtx* ctx, uint32_t pool_id, const GvClusterLod* lods, uint32_t lod_count);
/* The cluster commands of the views of E under the rule above. views[0 .. view_count): one per view of E, copied at the call.
 * eyes: NULL / 0 for no cone test; otherwise one GvClusterEye per view of E and gv_pool_cull_cluster_cones' test too (it needs a
 * cone binding). flags: a subset of {GV_CLUSTERS_FRUSTUM_ONLY, GV_CLUSTERS_RUNS} (the three older entry points keep refusing what
 * they refuse). Without GV_CLUSTERS_RUNS one command per survivor, in FIVE kernel launches; with it the runs of
 * gv_pool_cull_cluster_runs over these decisions, in SIX — whatever the data holds. The launches are those of the form it takes,
 * the test launch carrying the LOD test IN FRONT of the plane tests: a LOD-rejected cluster gets no plane test, no cone test and
 * no Hi-Z query. Counted under GvStats::launches[GV_K_EMIT]. Placement, targets, capacity, counts: as the form it takes.
 * The call IS a cluster cull of the pool: its result replaces the pool's cluster result and is replaced by the next one of any form;
 * gv_pool_cluster_commands_device / _fetch serve it, and it ends where a cluster result ends (and at gv_pool_bind_cluster_lods).
 * gv_pool_cull_clusters_second_phase behind a LOD result applies the same conjunction with this call's LOD views (and eyes, if
 * any) against the pyramid as it stands at that call. Its pending set keeps its definition (tested, not kept, in a queried view),
 * so LOD-REJECTED CLUSTERS ARE PENDING: re-tested, rejected again, counted in its counts[m + v]. With a DAG that is MOST of the
 * pending set — practically every candidate, 180 to 622 times the leaves' own in the measured scenes. Behind the three older forms the second phase is unchanged.
 * Errors: those of gv_pool_cull_clusters, plus GV_E_ARG: views NULL, view_count different from the views of E, a scale or a
 * near_distance that is negative or NaN, one of eyes / eye_count without the other, eye_count different from the views of E;
 * GV_E_STATE: no LOD binding, eyes without a cone binding. A refused call changes nothing.
 * Not built: a per-view count of LOD-rejected clusters, LOD-rejected clusters left out of the second phase's pending set, LOD
 * entries packed below 48 bytes, a hierarchical traversal that never visits the rejected sub-DAG, error metrics other than the
 * sphere form above, LOD views derived from view_proj, clusters for the merged multi-rank order. */
int gv_pool_cull_cluster_lods(GvCtx* ctx, uint32_t pool_id, uint32_t flags, const GvClusterLodView* views, uint32_t view_count,
                              const GvClusterEye* eyes, uint32_t eye_count, uint32_t region_commands, void* dst_device, size_t capacity_bytes);

/* ---- instance payload: the component fields a plugin copies next to mvp (sprite.cpp:127-129, 9-slice.cpp:25-44) ----
 * setInstanceData writes mvp and then copies a few fields of the draw's own component — color, uvSize, uvOffset — found through
 * the record's componentOffset. A pool may bind those bytes (its PAYLOAD: up to GV_MAX_PAYLOAD_FIELDS fields, GV_MAX_PAYLOAD_BYTES
 * bytes per slot in all); the library mirrors them on the device, one packed row per POOL SLOT (row pitch 16, 32 or 64 bytes),
 * keeps the rows current through dirty marks, and gv_pool_emit_instances writes the row of each record's slot at the destinations
 * gv_pool_set_payload_layout names, so that a sprite system's whole instance is produced on the device, in draw order.
 * The bytes are OPAQUE: copied verbatim, no conversion, no arithmetic — NaN patterns and -0 survive bit for bit. In particular
 * srgbToRgb(color) (sprite.cpp:127) is NOT applied: the reference's libraries/math is empty, so its text is unpinned,
 * and a pow cannot be bit-defined across host and device. An engine binds a column that already holds the value it wants in the
 * buffer; the same goes for the 9-slice borders, which are computed rather than copied.
 *
 * gv_pool_bind_payload — the sources. Element i of field f at fields[f].data + i * fields[f].stride (AoS: base + offsetof(field),
 * stride = sizeof(component)). Lifetime as gv_pool_bind: re-issue when the storage may have moved; the pointers are read only inside
 * the calls that upload — gv_sync (hence gv_cull) and gv_pool_emit_instances of the pool — and must be valid there; nothing is
 * retained. count == 0 removes the payload and frees its mirror. A rebind with the same field shape (count and every `bytes`) and
 * an equal or larger occupancy keeps the rows that are clean and uploads only the new slots; another shape or a smaller occupancy
 * uploads everything. After every bind all destinations are GV_NONE. GV_E_ARG: an unbound pool, count above GV_MAX_PAYLOAD_FIELDS,
 * a NULL data, bytes that is 0, not a multiple of 4 or above 64, a sum above GV_MAX_PAYLOAD_BYTES, stride < bytes.
 *
 * gv_pool_set_payload_layout — the destinations, kept apart from the bind because the base and the shadow instance structs differ
 * (instance.hpp:82-86): at[f] is the 4-byte-aligned offset of field f in the instance, GV_NONE: mirrored but not written. Read by
 * the next emission, like the instance layout. Destinations lie inside the stride and are disjoint from each other and from the
 * instance layout's mvp / model / slot / distance_sq: checked here against the current instance layout, in
 * gv_pool_set_instance_layout against the current destinations (only while a payload is bound), and once more at the emission
 * for the pair as it then stands — GV_E_ARG each time. `count` must be the bound field count (GV_E_ARG); without a bound payload
 * GV_E_STATE.
 *
 * Keeping it current: GV_DIRTY_PAYLOAD marks, and the pool's GV_DIRTY_MESH marks (a slot filled anew has a new payload), add to the
 * payload's own dirty set, which gv_sync or the pool's gv_pool_emit_instances consumes, whichever comes first: a mark made between
 * the cull and the emission is seen by that emission (the reference reads the component at draw time too, mesh.cpp:592). Uploaded
 * bytes count in GvStats::upload_bytes.
 *
 * The emission: GV_E_STATE when a destination is set and the payload's occupancy is below a listed view's; with no payload bound
 * or no destination set it is exactly the emission described above. gv_pool_instances_fetch delivers the payload fields the
 * emission wrote like the other fields. */
#define GV_MAX_PAYLOAD_FIELDS 4u
#define GV_MAX_PAYLOAD_BYTES 64u /* sum over the fields, per slot */
typedef struct GvPayloadField {
    const void* data; /* element i at data + i * stride */
    uint32_t stride;  /* bytes between consecutive elements, >= bytes */
    uint32_t bytes;   /* 4 .. 64, a multiple of 4 */
} GvPayloadField;
int gv_pool_bind_payload(GvCtx* ctx, uint32_t pool_id, const GvPayloadField* fields, uint32_t count, uint32_t occupancy);
int gv_pool_set_payload_layout(GvCtx* ctx, uint32_t pool_id, const uint32_t* at, uint32_t count);

/* A tick of engine-sized pools (the reference's everyday 10^3..10^4 entities per mesh system) is bound by launches,
 * not by bytes. Between gv_cull_batch_begin and the first call that reads results (gv_pool_results_* / gv_results_* /
 * gv_wait, or gv_cull_batch_end), gv_cull of a pool of up to 32768 slots whose views all emit records only RECORDS the
 * cull; the first read then launches all recorded culls as ONE kernel, their emits as ONE kernel, the requested sorts
 * (gv_pool_sort; pools of up to 16384 slots) as ONE kernel and publishes every view's results to the host with ONE kernel and ONE synchronisation —
 * four launches per frame however many mesh systems and shadow passes there are. Other culls (larger pools, count-only
 * views, GV_SWEEP_WITH_CULL, block bounds) run at once as usual. Same results. A bind or gv_mark_dirty of a pool a recorded cull
 * reads (its mesh pool; the transform pool, gv_sync and gv_hierarchy_rebuild concern every recorded cull) first launches what
 * has been recorded so far — the recorded culls see the pools as they were when gv_cull was called — and recording goes on. */
int gv_cull_batch_begin(GvCtx* ctx);
int gv_cull_batch_end(GvCtx* ctx);
int gv_pool_results_fetch(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, int write_back, GvResult* out);
int gv_pool_result_count(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t* draw_count);
int gv_pool_results_device(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, GvDeviceResult* out);
int gv_pool_sort(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, int descending);

/* ---- a view's draws grouped by geometry, on the device ----
 * Run mode of gv_pool_emit_draw_commands merges CONSECUTIVE draws of one id, and records arrive in space or distance order: random
 * ids give one command per draw. gv_pool_group_draws reorders the records of (pool, view) by geometry key, stable, where
 * gv_pool_sort makes its reorder, so that every later step — the fetches, the record structs, the instance bases, both instance
 * emissions, the LOD selection, the commands in both modes — sees draw k as record k of the new order and composes unchanged. Run
 * mode then writes one command per geometry (or per level of one) with instance_count = the group's instance total.
 *   Records 0 .. n-1: those of the view in the order a fetch would deliver them when the call is issued; n is the device draw
 *     count, never read by the host. s_k = visible_idx[k], the record's POOL slot.
 *   b_k = id[s_k], read from the geometry id mirror as it stands when the call is issued (the call uploads the column on first use
 *     and consumes pending GV_DIRTY_GEOMETRY / GV_DIRTY_MESH marks, as gv_pool_select_lods); without an id column b_k = 0.
 *   flags == 0: g_k = b_k, view_scale is ignored. GV_GROUP_BY_LOD: g_k = b_k + level_k, level_k exactly that of gv_pool_select_lods
 *     above (d2 from floats 9, 10, 11 of the record's bakedModel, x = d2 * view_scale, the size mirror and the table of
 *     gv_pool_bind_lod; size marks are uploaded and consumed as the selection does). The level depends on the record's own bytes
 *     only: a gv_pool_select_lods issued later with the same scale selects the same g for every draw.
 *   Key: kappa_k = min(g_k, K), K the bound geometry table's table_count: every void id shares the last bucket.
 *   After the call record j of the view is the old record pi(j), pi the stable ascending order of kappa: within one key the previous
 *     order is kept (behind gv_pool_sort every group is still ordered by distance). visible_idx, baked_model and distance_sq all
 *     move; draw_count, is_visible and instance_count do not change.
 * Asynchronous on gv_stream(ctx); counts as a read (recorded culls and deferred sorts are launched first). 2 launches per 8-bit
 * digit of the VALUE K — one digit for K <= 255, two for K <= 65535, three for K = 65536 — counted under
 * GvStats::launches[GV_K_SORT]: fixed by the host, never derived from a count read back. Afterwards the view counts as not
 * distance-sorted (gv_merge_sorted refuses it with GV_E_STATE) until a later gv_pool_sort, and the next fetch delivers the new
 * order. Without an id column and without the flag every key is 0: GV_OK, nothing is launched, nothing changes.
 * GV_E_ARG: a NULL ctx, a pool out of range or not bound, unknown flag bits, a view without emitted records. GV_E_STATE: no
 * geometry bound; GV_GROUP_BY_LOD without an LOD binding; an id or size column whose occupancy is below the view's; the pool holds
 * an instance emission since its last gv_cull — group first, then emit: instance data written before the reorder would no longer
 * match its draws. */
#define GV_GROUP_BY_LOD 1u
int gv_pool_group_draws(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t flags, float view_scale);

/* ---- two-phase occlusion culling: the second phase, on the device ----
 * The pyramid a Hi-Z view queries is a frame old (it is built behind the previous frame's depth pass), so a box that has just come
 * into view stays "occluded" for a frame. The remedy: cull against the old pyramid and draw the result (gv_cull, phase 1), rebuild
 * the pyramid from what was drawn (gv_hiz_build), then re-test what phase 1 left out and draw the newly visible rest — this call.
 *   S1: the pool slots in the records of (pool_id, first_view) as a fetch would deliver them when the call is issued —
 *     visible_idx[0 .. n1), n1 the device draw count, never read by the host. POOL slots: never index-mapped, never mirror entries.
 *     Derived from the records, so a gv_pool_sort, a gv_pool_group_draws or a re-order of the mirror between the phases changes nothing.
 *   R: the records a gv_cull(pool_id, view, 1) issued at this moment would deliver — the mirror brought up to date as gv_cull does
 *     it (pending gv_mark_dirty marks are consumed), against the pyramid as it stands. Every field of `view` is honoured as gv_cull
 *     honours it (use_hiz, distance_2d, shadow_pass, camera_offset); emit_records must be 1.
 *   Afterwards `second_view` is an ordinary emitted view of the pool, whatever it held before is replaced: its records are the
 *     records of R whose slot is not in S1, in R's relative order (the mirror's spatial order; ascending slots with
 *     GV_CONFIG_KEEP_SLOT_ORDER); visible_idx, baked_model and distance_sq bit for bit what R holds for them; draw_count their number;
 *     instance_count follows from the records as for any emitted view; view_proj is kept for the instance emission. The fetches,
 *     record structs, gv_pool_sort, gv_pool_group_draws, both instance emissions, gv_pool_select_lods and
 *     gv_pool_emit_draw_commands take it unchanged.
 *   is_visible (view->shadow_pass < 0; a shadow-pass view yields NULL as usual): the byte of slot s is 1 iff s is in S1 OR in the new
 *     records. DELIBERATELY MORE THAN THE VIEW'S OWN RECORDS: it is the frame's final answer, which is what the light pass and
 *     write_back want. gv_results_copy_mask_device of the second view carries the new entries only (bits and dst[0] match the records).
 *   The first view is not touched: its records, count, is_visible, sort state and delivery state stay as they are.
 * State: a read of the first view (recorded culls and deferred sorts are launched first) and, for the pool, a cull: it ends the
 * pool's instance emission, commands and LOD selection and every merged array the pool is a member of. The pool's OTHER views stay
 * valid; the pool's next gv_cull ends the second view like any view beyond its count. Asynchronous on gv_stream(ctx): no host
 * synchronisation, no count read back. Launches, fixed by the host: the seen set and the masked cull under
 * GvStats::launches[GV_K_CULL]; compaction and records as a cull's (GV_K_SCAN / GV_K_EMIT); the union of the isVisible bytes of a
 * main-pass view under GV_K_EMIT. An empty pool, or a first view without draws, is GV_OK; with S1 empty the second view is exactly R.
 * GV_E_ARG: a NULL ctx or view; a pool out of range or not bound; first_view == second_view; an index >= GV_MAX_VIEWS; a first
 * view that is not valid or holds no emitted records; view->emit_records == 0. GV_E_STATE: view->use_hiz before gv_hiz_build; the
 * pool's occupancy differs from the one the first view was culled with (cull again first). */
int gv_pool_cull_second_phase(GvCtx* ctx, uint32_t pool_id, uint32_t first_view, uint32_t second_view, const GvView* view);

/* ---- the bounds of a view's visible draws, on the device ----
 * The reference fits every shadow cascade to its slice of the camera frustum and then pulls the light's near and far planes apart
 * by a constant zCoeff (source/system/render/csm.cpp:294-295), because nobody knows where the casters are. gv_pool_view_bounds
 * answers that question from the records a cull delivered: the box, in a basis the caller names, of every corner of every draw.
 *   Items: item i is the pair (view_indices[i], bases + 12 i). A basis B is an affine 3x4 in the layout of bakedModel — c0.xyz
 *     c1.xyz c2.xyz c3.xyz, column-major — for example the rotation and translation of a light view. A view may be listed more
 *     than once with different bases.
 *   Records: those of (pool_id, view) as a fetch would deliver them when the call is issued (after a gv_pool_sort, a
 *     gv_pool_group_draws, of a second-phase view alike), n = the device draw count, never read by the host. Per record k: the POOL
 *     slot s = visible_idx[k] (never index-mapped, never a mirror entry); M = the record's own bakedModel (camera-relative,
 *     camera_offset NOT included); the box = aabb_min / aabb_max of slot s as the device mirror holds them when the call is issued —
 *     the call uploads nothing and consumes no gv_mark_dirty mark; a slot that has stopped being a candidate since holds the empty
 *     box (min == max == 0): its eight corners coincide at the pivot.
 *   The eight corners p = M * (x, y, z, 1) with every row r as fma(c0[r], x, fma(c1[r], y, fma(c2[r], z, c3[r]))) — the cull's
 *     own corners — and q[r] = fma(B.c0[r], p.x, fma(B.c1[r], p.y, fma(B.c2[r], p.z, B.c3[r]))) for r = 0, 1, 2.
 *   lo[r] / hi[r]: the minimum / maximum of q[r] over all records and corners, in the order of the key bits ^ (sign ? 0xFFFFFFFF :
 *     0x80000000): -0 sorts below +0, +-inf take part, a NaN takes no part (in that coordinate only). draw_count = n. nan_records =
 *     the records with a NaN among their 24 coordinates. With nothing taking part lo[r] = +inf and hi[r] = -inf: lo > hi is how a
 *     consumer sees "empty". The order of evaluation cannot change any output bit.
 * State: a read (recorded culls and deferred sorts are launched first); asynchronous on gv_stream(ctx), no host synchronisation;
 * two kernel launches whatever the counts, under GvStats::launches[GV_K_EMIT]. Records, sort state, emissions, selection and
 * commands stay as they are. The result is the pool's (one per pool: a new call replaces it) and ends with the pool's next
 * gv_cull or gv_pool_cull_second_phase.
 * GV_E_ARG: a NULL ctx; a pool that is not bound; item_count 0 or above GV_MAX_BOUNDS_ITEMS; NULL view_indices or bases; a view
 * index >= GV_MAX_VIEWS; an index no cull of the pool has ever had a view at. GV_E_STATE: a view without results (a later cull
 * of fewer views ended it); a count-only view (emit_records == 0); a mirror that no longer covers the occupancy the view was culled
 * with. An empty pool or a view without draws: GV_OK with the empty answer. A non-finite basis is not an error. */
#define GV_MAX_BOUNDS_ITEMS 8u
typedef struct GvViewBounds { /* 32 bytes */
    float lo[3];
    uint32_t draw_count;
    float hi[3];
    uint32_t nan_records;
} GvViewBounds;
int gv_pool_view_bounds(GvCtx* ctx, uint32_t pool_id, const uint32_t* view_indices, const float* bases, uint32_t item_count);
/* The last call's GvViewBounds[*item_count] in device memory, as plain floats (valid behind the call on gv_stream(ctx)).
 * GV_E_STATE: no result since the pool's last cull. */
int gv_pool_view_bounds_device(GvCtx* ctx, uint32_t pool_id, const void** bounds, uint32_t* item_count);
/* Waits for the result and copies 32 bytes per item. GV_E_ARG: capacity below the item count (nothing is written). GV_E_STATE as above. */
int gv_pool_view_bounds_fetch(GvCtx* ctx, uint32_t pool_id, GvViewBounds* bounds, uint32_t capacity);

/* ---- what came into view and what left it since the last call, on the device ----
 * Every step above answers "what is visible now". The consumers of visibility on the host ask "what CHANGED": streaming, animation
 * and audio want the slots that came into view and the slots that left it, and the isVisible write-back only has to touch the bytes
 * that differ from last frame's — a few percent under a moving camera. The reference keeps no history of visibility: the rule is
 * this build's.
 *   Channels: a pool has GV_MAX_DELTA_CHANNELS channels that know nothing of each other (one for the light pass's write-back,
 *     another for "visible in any cascade" ...). A channel keeps a BASELINE P, a set of POOL slots covering P.slots slots; empty
 *     (P.slots = 0) until the channel's first call.
 *   The current set C: the union over the listed views (1 .. GV_MAX_VIEWS, none twice) of
 *     - a view with emitted records: the slots visible_idx[0 .. n) as a fetch would deliver them when the call is issued, n the
 *       device draw count, never read by the host. POOL slots: never index-mapped, never mirror entries. Sorted, grouped and
 *       second-phase views alike;
 *     - a count-only view of the main pass (emit_records == 0, shadow_pass < 0): the slots whose is_visible byte is 1 in the bytes a
 *       fetch would deliver at that moment.
 *     C.slots = the largest occupancy among the listed views; a record slot at or beyond it is ignored. Listing the two views of a
 *     two-phase frame gives the union of the phases (the set of the second view's is_visible bytes), the second view alone the
 *     newly visible rest.
 *   The answer: U = max(P.slots, C.slots); a set that does not cover a slot does not hold it. appeared = C \ P and vanished = P \ C,
 *     each in ASCENDING slot order, in one device buffer of U words — appeared at [0, a), vanished at [a, a + v) — and
 *     counts = {a, v, |C|, U} as four uint32. Every output word is defined by the two sets alone.
 *   Commit: the same call makes C the channel's baseline, on the device, in stream order: a second call with nothing culled in
 *     between answers two empty lists and the same |C|. GV_DELTA_RESTART takes P as empty for this call (appeared = all of C).
 *     gv_pool_view_delta(ctx, pool, channel, NULL, 0, 0) drops the channel's baseline and result. A failed call changes nothing
 *     (an allocation failure, GV_E_OOM, may end the channel's previous result; never its baseline).
 *   Lifetime: the baseline is history. gv_cull, gv_pool_cull_second_phase, emissions, sorts, re-orders of the mirror and re-binds of
 *     the pool with another occupancy leave it alone; only the drop call, the call's own commit and gv_destroy change it. The result
 *     is slot numbers of its own and lives until the channel's next call.
 * State: a read (recorded culls and deferred sorts are launched first); uploads nothing, consumes no mark, changes nothing any other
 * call can observe. Asynchronous on gv_stream(ctx), no host synchronisation. Launches, fixed by the host from view_count alone and
 * counted under GvStats::launches[GV_K_EMIT]: one per listed view, then two.
 * GV_E_ARG: a NULL ctx; a pool that is not bound; channel >= GV_MAX_DELTA_CHANNELS; view_count > GV_MAX_VIEWS; NULL view_indices
 * with a non-zero count; a view index >= GV_MAX_VIEWS or listed twice; an index no cull of the pool ever had a view at; unknown
 * flag bits. GV_E_STATE: a listed view without results (a later cull of fewer views ended it); a count-only shadow view (it has
 * neither records nor bytes). An empty pool or views without draws: GV_OK with C empty. */
#define GV_MAX_DELTA_CHANNELS 4u
#define GV_DELTA_RESTART 1u
typedef struct GvViewDelta {
    const uint32_t* appeared;  /* [appeared_count] pool slots, ascending */
    const uint32_t* vanished;  /* [vanished_count] pool slots, ascending */
    uint32_t appeared_count, vanished_count;
    uint32_t visible_count;    /* |C| */
    uint32_t slots;            /* U */
} GvViewDelta;
int gv_pool_view_delta(GvCtx* ctx, uint32_t pool_id, uint32_t channel, const uint32_t* view_indices, uint32_t view_count, uint32_t flags);
/* The channel's last answer in device memory: *slots the U words, *counts the four (valid behind the call on gv_stream(ctx)).
 * GV_E_ARG: a NULL ctx or output, a pool or channel out of range. GV_E_STATE: the channel holds no result. */
int gv_pool_view_delta_device(GvCtx* ctx, uint32_t pool_id, uint32_t channel, const void** slots, const void** counts);
/* Copies the four counts, waits, copies a + v words, waits. The pointers of *out go into the result's pinned staging and stay valid
 * until the channel's next call. write_back != 0: stores 1 into the isVisible byte of every appeared slot and 0 into that of every
 * vanished slot, and touches NO other byte — the target is the one gv_pool_results_fetch(write_back = 1) uses: the bound component
 * column or, with GV_RESULTS_MAP_VISIBLE, visible_base + index_map[slot] * visible_stride (holes and slots beyond visible_count
 * skipped); on the library's worker threads from the same floor up. Slots at or beyond the pool's bound occupancy are skipped: a
 * pool that shrank has no component there any more.
 * THE CONTRACT of the write-back: the caller's bytes are right afterwards only if they held the BASELINE before. The first frame
 * therefore does a normal gv_pool_results_fetch(..., write_back = 1), or a GV_DELTA_RESTART call over zeroed bytes; and nobody else
 * writes those bytes in between.
 * GV_E_ARG: a NULL ctx or out, a pool or channel out of range. GV_E_STATE: no result; write_back without a target. */
int gv_pool_view_delta_fetch(GvCtx* ctx, uint32_t pool_id, uint32_t channel, int write_back, GvViewDelta* out);

/* ---- occluder depth, drawn on the device ----
 * The Hi-Z query (GvView::use_hiz, gv_pool_cull_second_phase) reads a depth image; the reference takes it from its renderer's depth
 * buffer. A headless server, a shadow cascade or a pass that has not been drawn yet has none. These calls draw one: every draw of a
 * delivered view whose slot has an OCCLUDER BOX — a box in the slot's model space, the space aabb_min / aabb_max live in — writes
 * the farthest depth of that box into the pixels the box's projected silhouette wholly covers, shrunk by a margin that pays for the
 * snapping of its vertices. One depth per box, conservative in area and in depth; the image then goes through gv_hiz_build.
 *   Frame order: gv_cull (no Hi-Z) -> gv_occluder_begin -> gv_pool_draw_occluders per pool and view -> gv_hiz_build_from_occluders
 *     -> gv_cull with use_hiz, or gv_pool_cull_second_phase.
 *   The rule, per draw k of the view (slot s = visible_idx[k], M = the record's own bakedModel, VP = the view's view_proj as culled):
 *     1. has a box <=> omin.x < omax.x && omin.y < omax.y && omin.z < omax.z (a NaN fails); otherwise counted no_box.
 *     2. corners and clip coordinates exactly as the Hi-Z query computes them for an AABB (fma nesting, IEEE 1 / w, u = fma(x / w, .5,
 *        .5), v likewise, z / w): an occluder box equal to the slot's AABB gets the query's own words.
 *     3. any corner with !(w > 0): skipped, counted behind.   4. d = min(minNum of the 8 z, 1.0f); !(d > 0): skipped, counted behind.
 *     5. X = floorf(u * 16 W), Y = floorf(v * 16 H) (four sub-pixel bits); any !(|.| < 2^22): skipped, counted range.
 *     6. the silhouette: the box edges between a face of positive and a face of non-positive projected area (int64); no positive
 *        face: skipped, counted flat. Mirrored models and mirrored projections give the same silhouette.
 *     7. a pixel is covered <=> each of its four corners (cx, cy) passes ex (16 cy - Y_a) - ey (16 cx - X_a) >= 2 (|ex| + |ey|) for
 *        every silhouette edge a -> b (int64).
 *     8. pixel range x0 = max(min X >> 4, 0) .. x1 = min(max X >> 4, W - 1), y likewise; empty, or narrower or lower than
 *        min_pixels: skipped, counted small. Otherwise counted drawn.
 *     9. depth[py W + px] = max(0.0f, max over the covering occluders of d): order-independent, reproducible bit for bit.
 *   THE BINDER'S CONTRACT: the library does not check that an occluder box lies inside the slot's AABB, nor inside the geometry the
 *     slot draws. A box that sticks out of solid geometry culls what is visible. */
typedef struct GvOccluderCounts { /* 24 bytes; summed over the draws of every gv_pool_draw_occluders since gv_occluder_begin */
    uint32_t drawn, no_box, behind, range, flat, small;
} GvOccluderCounts;
/* Binds the occluder boxes of a pool's slots: 3 fp32 each at box_min + i * stride and box_max + i * stride, i < occupancy (stride >=
 * 12). box_min == NULL && box_max == NULL removes the binding. Lifetime of the pointers as for gv_pool_bind_ready. The boxes are
 * mirrored per POOL slot (one 32-byte row: min in words 0-2, max in words 4-6), only once gv_pool_draw_occluders has been called
 * for the pool: that call uploads the column; from then on GV_DIRTY_OCCLUDER and the pool's GV_DIRTY_MESH marks feed a dirty set
 * of its own, consumed by gv_sync or the pool's next draw, whichever comes first (bytes under GvStats::upload_bytes). A rebind
 * uploads everything again.
 * GV_E_ARG: a NULL ctx; a pool out of range; exactly one of the pointers NULL; stride < 12; occupancy beyond the 28-bit slot range. */
int gv_pool_bind_occluders(GvCtx* ctx, uint32_t pool_id, const void* box_min, const void* box_max, uint32_t stride, uint32_t occupancy);
/* Opens an occluder image of width x height (1 .. 32768 each): sized, cleared to 0 (reversed Z: "nothing in front of anything")
 * and its six counts zeroed, asynchronously on gv_stream(ctx). The context owns GV_MAX_PYRAMIDS + 1 images (each allocated at
 * first use) and takes the one of the last begin unless a built pyramid reads it, then the lowest-numbered one that no built pyramid
 * reads (with one pyramid in use: two images in turn): a pyramid's level 0 is the depth image, so an image a pyramid reads is never cleared, redrawn or reallocated
 * under it (gv_hiz_rebuild keeps reproducing the old pyramid). A begin on an open image starts it over.
 * GV_E_ARG: a NULL ctx; a size of 0 or above 32768 (nothing changes). GV_E_OOM: an open image that had to grow is gone; the pyramid's
 * image is not touched. */
int gv_occluder_begin(GvCtx* ctx, uint32_t width, uint32_t height);
/* Draws the occluders of one delivered view of one pool into the open image; several pools and views may draw into one image. A
 * read of the view, as gv_pool_view_bounds (recorded culls and deferred sorts are launched first; records of sorted, grouped and
 * second-phase views alike, in delivery order, the device draw count never read by the host); asynchronous on gv_stream(ctx): three
 * kernel launches whatever the counts, under GvStats::launches[GV_K_HIZ]. The image is accumulated state, like the baselines of
 * gv_pool_view_delta: no cull, emission or sort ends it.
 * MEMORY: the call's scratch is one word per slot of the occupancy the view was culled with and 8 bytes per 256 slots (40 MB at
 * 10^7 slots), allocated at the first draw, shared by all pools and kept; a later view with a larger occupancy replaces it,
 * which waits for the device once. No row is stored per occluder: the raster launch computes it again from the record.
 * GV_E_ARG: a NULL ctx; a pool that is not bound; a view index >= GV_MAX_VIEWS, or one no cull of the pool ever had a view at.
 * GV_E_STATE: no open image (gv_occluder_begin; gv_hiz_build_from_occluders closes it); no occluder binding; a view without results
 * or culled count-only; boxes that cover fewer slots than the view was culled with. */
int gv_pool_draw_occluders(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t min_pixels);
/* The image of the last gv_occluder_begin (open or built) in device memory, width * height fp32 in rows, and its six counts as
 * uint32 (valid behind the draws on gv_stream(ctx)). GV_E_ARG: a NULL ctx or output. GV_E_STATE: no gv_occluder_begin yet. */
int gv_occluder_depth_device(GvCtx* ctx, const void** depth, uint32_t* width, uint32_t* height, const void** counts);
/* Waits for the draws and copies the image (depth may be NULL: counts only; `bytes` is the room at depth) and the counts (may be NULL).
 * GV_E_ARG: a NULL ctx; both outputs NULL; bytes below width * height * 4 (nothing is written). GV_E_STATE as above. */
int gv_occluder_depth_fetch(GvCtx* ctx, float* depth, size_t bytes, GvOccluderCounts* counts);
/* gv_hiz_build(image, width, height, GV_MEM_DEVICE) of the open image, and closes it: further draws need a new gv_occluder_begin
 * (which takes another image). GV_E_STATE: no open image. Otherwise as gv_hiz_build. A caller who hands the open image's pointer
 * (gv_occluder_depth_device) to gv_hiz_build himself closes it the same way: no image takes a draw once a pyramid reads it. */
int gv_hiz_build_from_occluders(GvCtx* ctx);

/* ---- receiver mask: shadow-caster culling against what the main view sees ----
 * A shadow cascade's box is long towards the light, so a plain frustum cull of it keeps many casters whose shadows fall on nothing the
 * main camera sees. The remedy (Bittner et al. 2011): draw the bounds of what the main view SEES into the light's clip space, keeping
 * per texel the farthest depth any visible receiver reaches, +inf where none does; a caster wholly behind every receiver under its
 * footprint, or over empty texels, is dropped. No new cull: the Hi-Z query reports "occluded" iff the box's nearest depth is less than
 * the minimum of the pyramid over its footprint, which over such an image reads "behind every visible receiver it could shadow". Every
 * consumer of the pyramid compares and never computes, so the infinity is harmless. These calls draw the image: every draw of a
 * delivered view writes one depth — its cull AABB's farthest, against the matrix the caller names — into every pixel the AABB's projected
 * silhouette TOUCHES, grown by the margin the occluder raster shrinks by; each pixel keeps the minimum. The boxes are the ones the cull
 * already mirrors: there is no binding and no binder's contract.
 *   Frame order: 1. gv_cull of the main view (which may itself use Hi-Z against the renderer's depth). 2. For each cascade k:
 *     gv_hiz_select(1 + k) -> gv_receiver_begin -> gv_pool_draw_receivers(pool, main view, L_k) for every pool that receives
 *     shadows -> gv_hiz_build_from_receivers (into the selected slot). 3. gv_hiz_select(0), then ONE gv_cull of [main, cascade 0, cascade 1, ...]
 *     with use_hiz = [the main view's own, 2, 3, ...]: every view is held against its own image in one pass over the pool (views
 *     that share the camera position; others take a launch each, against their own pyramids all the same). The main view's depth
 *     pyramid — slot 0 — is not touched by the masks, so gv_pool_cull_second_phase of the main view may follow in the same frame.
 *   Frame order without pyramid slots (a caller who never calls gv_hiz_select; it still works): per cascade k gv_receiver_begin ->
 *     the draws -> gv_hiz_build_from_receivers -> gv_cull of cascade k with use_hiz = 1. The context has ONE pyramid then: the main
 *     view's depth pyramid is rebuilt next frame (as it is every frame anyway), and cascades culled this way go one at a time — they
 *     leave the batched multi-view pass. A gv_cull replaces ALL views of its pool: a cull that names cascade k alone ends the main
 *     view's records, which the next cascade's mask is drawn from — name the main view again in front of it.
 *   The rule, per draw k of the source view (slot s = visible_idx[k], M = the record's own bakedModel, (amin, amax) = the slot's cull
 *   AABB as mirrored, L = light_view_proj):
 *     1. corners and clip coordinates exactly as the Hi-Z query computes them against L: a caster that is also a receiver gets its
 *        own query's words, and is never culled by itself.
 *     2. any corner with !(w > 0): counted behind; +0.0f into EVERY pixel (a receiver that cannot be bounded keeps every caster). A
 *        NaN or infinite model lands here, not in step 4: every corner's w is NaN whatever L holds.
 *     3. d = the minNum of the 8 z when that is > 0, +0.0f otherwise (never -0.0f); no upper clamp.
 *     4. X = floorf(u * 16 W), Y = floorf(v * 16 H); any !(|.| < 2^22): counted range; d into every pixel.
 *     5. pixel range x0 = max((min X - 2) >> 4, 0) .. x1 = min((max X + 2) >> 4, W - 1), y likewise; empty: counted outside, nothing written.
 *     6. the silhouette edges as for occluders; no positive face: counted flat; d into every pixel of the range.
 *     7. otherwise counted drawn; a pixel is touched <=> for every silhouette edge a -> b SOME pixel corner passes
 *        ex (16 cy - Y_a) - ey (16 cx - X_a) >= -2 (|ex| + |ey|) (int64); d into every touched pixel.
 *     8. mask[py W + px] = min(+inf, min of the words written there) on the floats' bits: order-independent, reproducible bit for bit. */
typedef struct GvReceiverCounts { /* 24 bytes; summed over the draws of every gv_pool_draw_receivers since gv_receiver_begin */
    uint32_t drawn, flat, behind, range, outside, reserved; /* every record lands in exactly one of the first five; reserved is 0 */
} GvReceiverCounts;
/* Opens a receiver mask of width x height (1 .. 32768 each): sized, every word cleared to +inf (0x7F800000: "no receiver here") and
 * its counts zeroed, asynchronously on gv_stream(ctx). The context owns GV_MAX_PYRAMIDS + 1 receiver images of its own (each
 * allocated at first use), apart from the occluder images, and takes the one of the last begin unless a built pyramid reads it, then
 * the lowest-numbered one that no built pyramid reads: an image a pyramid reads is never cleared, redrawn or reallocated under it. A begin on an open mask starts it over. An open occluder image and an open receiver mask may coexist.
 * GV_E_ARG: a NULL ctx; a size of 0 or above 32768 (nothing changes). GV_E_OOM: an open mask that had to grow is gone; the pyramid's
 * image is not touched. */
int gv_receiver_begin(GvCtx* ctx, uint32_t width, uint32_t height);
/* Draws the cull AABBs of the records of one delivered view of one pool into the open mask, projected with light_view_proj (16 floats,
 * column-major like GvView::view_proj; copied by the call); several pools and views may draw into one mask. A read of the view, as
 * gv_pool_view_bounds and gv_pool_draw_occluders (recorded culls and deferred sorts are launched first; records of sorted, grouped and
 * second-phase views alike, in delivery order, the device draw count never read by the host); asynchronous on gv_stream(ctx): three
 * kernel launches whatever the counts, under GvStats::launches[GV_K_HIZ]. A receiver whose range holds at most 16 pixels is written
 * by the first launch; the tiles of the others are listed and walked by the third.
 * MEMORY: the scratch of gv_pool_draw_occluders, shared with it (one word per slot of the occupancy the view was culled with and 8
 * bytes per 256 slots), allocated at first use and kept.
 * GV_E_ARG: a NULL ctx or matrix; a pool that is not bound; a view index >= GV_MAX_VIEWS, or one no cull of the pool ever had a view at.
 * GV_E_STATE: no open mask (gv_receiver_begin; gv_hiz_build_from_receivers closes it); a view without results or culled count-only;
 * a mesh mirror that covers fewer slots than the view was culled with — a guard only, like gv_pool_view_bounds's: a cull synchronises
 * the mirror it reads, and no sequence of public calls is known to reach it. */
int gv_pool_draw_receivers(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, const float light_view_proj[16]);
/* The mask of the last gv_receiver_begin (open or built) in device memory, width * height fp32 in rows, and its counts as six
 * uint32 (valid behind the draws on gv_stream(ctx)). GV_E_ARG: a NULL ctx or output. GV_E_STATE: no gv_receiver_begin yet. */
int gv_receiver_mask_device(GvCtx* ctx, const void** mask, uint32_t* width, uint32_t* height, const void** counts);
/* Waits for the draws and copies the mask (may be NULL: counts only; `bytes` is the room at mask) and the counts (may be NULL).
 * GV_E_ARG: a NULL ctx; both outputs NULL; bytes below width * height * 4 (nothing is written). GV_E_STATE as above. */
int gv_receiver_mask_fetch(GvCtx* ctx, float* mask, size_t bytes, GvReceiverCounts* counts);
/* gv_hiz_build(mask, width, height, GV_MEM_DEVICE) of the open mask, and closes it: further draws need a new gv_receiver_begin
 * (which takes another image). GV_E_STATE: no open mask. Otherwise as gv_hiz_build. A caller who hands the open mask's pointer
 * (gv_receiver_mask_device) to gv_hiz_build himself closes it the same way. */
int gv_hiz_build_from_receivers(GvCtx* ctx);

/* ---- last frame's mvp per draw, for motion vectors ----
 * A velocity attachment filled from the camera alone (reprojecting depth with last frame's viewProj) gives every object that MOVES the
 * wrong motion vector. The cure is a second matrix per instance: last frame's viewProj * model of the same object; the vertex stage
 * then emits curr - prev. Last frame's models exist only in last frame's records on the device, in another order and for another
 * visible set: these calls keep them per POOL slot (never index-mapped, never mirror entries: a re-order of the mirror does not
 * concern them) and join them to this frame's draws on the device. The reference has no per-object velocity: the rule is this build's.
 *
 * THE PREVIOUS RULE (the same text stands in DESIGN.md §4 item 18, gv_device_math.hpp and tests/previous_twin.h). For draw k of a
 * view: slot s_k, record model M_k, VP = the view's view_proj, the pool's history H (per slot 12 floats and a stamp; an epoch e, 0 =
 * empty; a coverage H.slots; the kept view's view_proj KVP and camera position KC), PVP = prev_view_proj, or KVP when it is NULL,
 * d_r = view.camera_position[r] - KC[r] (one fp32 subtraction per component, done on the host).
 *  1. Cut: GV_PREVIOUS_CUT, or e == 0: every draw is fresh, with PVP = VP and d = (0, 0, 0).
 *  2. Kept <=> no cut && s_k < H.slots && stamp[s_k] == e: P_k = the row's 12 floats.
 *  3. Fresh otherwise: the draw is taken as static in the world. P_k = M_k with c3[r] = M_k.c3[r] + d_r (one fp32 add per component);
 *     the other nine floats verbatim.
 *  4. prev_mvp_k = PVP * P_k exactly as item 9: element i of column j = fma(PVP[12 + i], b3, fma(PVP[8 + i], b2, fma(PVP[4 + i], b1,
 *     fma(PVP[i], b0, +0)))) with (b0, b1, b2) = column j of P_k and b3 = 0, or 1 for j = 3. has_history_k = 1 when kept, 0 when fresh.
 * Under a cut the 64 bytes are bit for bit what gv_pool_emit_instances writes as mvp. Non-finite matrices are not an error.
 *
 * The frame a caller runs: cull -> (sort / group) -> gv_pool_emit_instances -> gv_pool_emit_previous -> gv_pool_keep_models.
 * Everything is in stream order, so the emission reads last frame's rows before the keep replaces them.
 * MEMORY: the history takes 64 bytes per pool slot of the largest occupancy kept (640 MB at 10^7 slots), allocated by the first keep.
 * Lifetime: the history is HISTORY like the baselines of gv_pool_view_delta: no cull, emission, sort, group, re-order or re-bind ends
 * it; only gv_pool_keep_models, gv_pool_forget_models and gv_destroy change it. It is deliberately NOT fed by GV_DIRTY_MESH marks: a
 * caller that refills a slot forgets it. One history per pool: one camera. The emission's result is made from a view and ends with
 * the pool's next gv_cull or gv_pool_cull_second_phase. */
#define GV_KEEP_ADD 1u         /* gv_pool_keep_models: the second view of a two-phase frame, kept into the same epoch */
#define GV_PREVIOUS_CUT 1u     /* gv_pool_emit_previous: a camera cut, every draw is fresh against the view's own view_proj */
typedef struct GvPreviousLayout { /* stride: a multiple of 16, 64 ... 256; the fields inside it and disjoint */
    uint32_t stride;
    uint32_t prev_mvp;         /* 64 bytes, 16-byte aligned */
    uint32_t has_history;      /* uint32 1 / 0, 4-byte aligned; GV_NONE: not written */
} GvPreviousLayout;
/* Keeps records 0 .. n-1 of (pool, view) as a fetch would deliver them when the call is issued (sorted, grouped and second-phase views
 * alike; n the device draw count, never read by the host). flags == 0: e advances by one (should it wrap to 0, every stamp is cleared
 * first and e becomes 1), the view's view_proj and camera_position are kept as given to its cull, and row[s_k] = {M_k verbatim, stamp
 * e} for every record; rows of other slots are not touched, their older stamp makes them stale. GV_KEEP_ADD does the same without
 * advancing e. The coverage grows to the view's occupancy: old rows survive (a device copy in stream order), new rows have stamp 0.
 * A read of the view (recorded culls and deferred sorts are launched first) that changes nothing any other call can observe;
 * asynchronous on gv_stream(ctx): one kernel launch under GvStats::launches[GV_K_EMIT] (one more should e wrap).
 * GV_E_ARG: a NULL ctx; a pool that is not bound; a view index >= GV_MAX_VIEWS, or one no cull of the pool ever had a view at; unknown
 * flag bits. GV_E_STATE: a view without results or culled count-only; GV_KEEP_ADD with an empty history (e == 0) or for a view whose
 * view_proj and camera_position do not equal the kept ones bit for bit. A failed call changes nothing. */
int gv_pool_keep_models(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t flags);
/* The stamps of slots [first, first + count) that the coverage holds become 0: those slots are fresh at the next emission (a
 * teleported entity, a slot filled anew). count == 0 empties the whole history: e = 0, coverage 0, buffers kept. One kernel launch
 * under GV_K_EMIT, or none. GV_E_ARG: a NULL ctx; a pool that is not bound. */
int gv_pool_forget_models(GvCtx* ctx, uint32_t pool_id, uint32_t first, uint32_t count);
/* Writes, for every draw k of (pool, view) in delivery order at the time of the call, prev_mvp_k and has_history_k by the rule above:
 * item k at dst + k * layout->stride, only the layout's bytes. layout NULL: {64, 0, GV_NONE}. prev_view_proj (16 floats, column-major,
 * copied by the call) NULL: the kept view_proj. dst_device NULL: a library-owned buffer sized for the view's occupancy (grown, never
 * shrunk). dst_device non-NULL: caller-owned device memory of capacity_bytes, 16-byte aligned; items at or beyond capacity_bytes /
 * stride are not written. It may be the instance buffer of the pool's emission at the first listed view — a plain emission puts draw k
 * at instance k, so a plugin struct {mvp, prevMvp} is filled by the two calls; keeping the fields apart from the instance layout's is
 * the caller's business. counts = {n, kept draws (of all n), items written, e} as four uint32 on the device.
 * A read of the view, asynchronous on gv_stream(ctx), no host synchronisation, no count read back: one memset and one kernel launch
 * under GvStats::launches[GV_K_EMIT]. One result per pool, valid until the pool's next cull.
 * GV_E_ARG: a NULL ctx; a pool that is not bound; a view index >= GV_MAX_VIEWS, or one no cull of the pool ever had a view at; unknown
 * flag bits; a bad layout; a misaligned dst_device. GV_E_STATE: a view without results or culled count-only. An empty pool or a view
 * without draws: GV_OK, counts = {0, 0, 0, e}. A failed call changes neither the history nor the previous result. */
int gv_pool_emit_previous(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, const GvPreviousLayout* layout, const float* prev_view_proj,
                          uint32_t flags, void* dst_device, size_t capacity_bytes);
/* The last emission in device memory: *items the target, *counts the four words (valid behind the call on gv_stream(ctx)).
 * GV_E_ARG: a NULL ctx or output; a pool that is not bound. GV_E_STATE: no result since the pool's last cull. */
int gv_pool_previous_device(GvCtx* ctx, uint32_t pool_id, const void** items, const void** counts);
/* Waits for the emission, delivers counts4[0 .. 3] and — dst_host non-NULL — the items written, field by field through the library's
 * pinned staging (the caller's memory is never page-locked; bytes between the fields stay as they are).
 * GV_E_ARG: a NULL ctx or counts4; a pool that is not bound; bytes below items written * stride (nothing is written). GV_E_STATE as above. */
int gv_pool_previous_fetch(GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* counts4);

/* ---- the shared sorted arrays: the sorted lists of several mesh systems merged into ONE array, on the device ----
 * The reference keeps one array per sorted kind — transSortedMeshes, uiSortedMeshes, one translucent array per shadow pass — into
 * which every sorted system appends SortedMesh records tagged with its bufferIndex (mesh.cpp:247-261); one std::sort orders the
 * whole array (mesh.cpp:296-326) and renderSorted switches system whenever bufferIndex changes (mesh.cpp:659-760).
 * gv_merge_sorted merges the already sorted lists of up to GV_MAX_MERGE_ITEMS (pool, view) members per GROUP into one array of
 * records, in ONE kernel launch for all groups of the call (translucent, UI, one group per shadow pass).
 * Order: the sort's own key order on the float's bits, T(u) = u ^ ((u >> 31) ? 0xFFFFFFFF : 0x80000000) — negative distance_2d
 * keys and -0.0 < +0.0 exactly as gv_pool_sort orders them. Ties go to the member listed first (then to the member's own order):
 * byte for byte what std::inplace_merge of the runs, taken in list order, gives.
 * A record is written as a fetch of a pool with a record layout writes one: component_offset (uint64 = slot * the ITEM's
 * component_stride, through the pool's index map when it has GV_RESULTS_MAP_RECORDS), baked_model (12 floats), distance_sq (the
 * key), buffer_index (uint32 = the ITEM's buffer_index; GV_NONE as the group's offset: the struct has none), every other byte of
 * the stride zero. stride: a multiple of 16, 16 ... 128; fields 4-byte aligned, inside the stride, disjoint.
 * dst_device NULL: a library-owned device buffer sized for the sum of the members' OCCUPANCIES times the stride (grown, never
 * shrunk). dst_device non-NULL: caller-owned device memory of capacity_bytes, 16-byte aligned; records whose position is at or
 * beyond capacity_bytes / stride are not written, the true total is still reported.
 * Asynchronous on gv_stream(ctx); counts as a read (culls recorded since gv_cull_batch_begin and deferred sorts are launched
 * first, as gv_pool_emit_instances documents); one launch, counted under GvStats::launches[GV_K_SORT]. No result of any member
 * changes. A group's result is valid until the next gv_cull of any member pool.
 * GV_E_ARG: group_count 0 or more than 32 items in all; a group_id of GV_MAX_MERGE_GROUPS or more, or listed twice; item_count 0
 * or above GV_MAX_MERGE_ITEMS; an unbound pool or a view index beyond the pool's last cull; the same (pool, view) twice in a
 * group; a bad stride, fields that overlap or leave the stride, a component_stride of 0; a misaligned dst_device.
 * GV_E_STATE: a count-only member or one with no results; a member that gv_pool_sort has not sorted in the group's direction
 * since its cull; an index map that does not cover a pool delivering GV_RESULTS_MAP_RECORDS. */
#define GV_MAX_MERGE_GROUPS 12u
#define GV_MAX_MERGE_ITEMS 16u /* per group; 32 per call */
typedef struct GvMergeItem {
    uint32_t pool_id, view_index;
    uint32_t buffer_index;     /* SortedMesh::bufferIndex of this member's records */
    uint32_t component_stride; /* getMeshComponentSize() of the member's system */
} GvMergeItem;
typedef struct GvMergeGroup {
    uint32_t group_id;         /* < GV_MAX_MERGE_GROUPS: which result slot of the context */
    uint32_t item_count;
    const GvMergeItem* items;  /* merge order == tie order */
    uint32_t descending;
    uint32_t stride, component_offset, baked_model, distance_sq, buffer_index; /* as GvRecordLayout; buffer_index may be GV_NONE */
    void* dst_device;          /* NULL: library-owned */
    size_t capacity_bytes;
} GvMergeGroup;
int gv_merge_sorted(GvCtx* ctx, const GvMergeGroup* groups, uint32_t group_count);
/* Device pointers of a group's last merge: the records, and uint32 counts[item_count + 1] (counts[i] = member i's draw count,
 * counts[item_count] = the total), both written in stream order on gv_stream(ctx). GV_E_STATE: no valid result. */
int gv_merge_device(GvCtx* ctx, uint32_t group_id, const void** records, const void** counts);
/* Waits for the group's merge and delivers counts[0 .. item_count] (counts_capacity >= item_count + 1) and — dst_host non-NULL —
 * the records [0, total) into the caller's array through the library's pinned staging; the caller's memory is never page-locked
 * (the rule of gv_pool_set_record_target). GV_E_ARG when bytes < total * stride or counts_capacity is too small (nothing is
 * written); records a caller-owned device target could not hold are not delivered either. GV_E_STATE: no valid result. */
int gv_merge_fetch(GvCtx* ctx, uint32_t group_id, void* dst_host, size_t bytes, uint32_t* counts, uint32_t counts_capacity);

/* ---- multi-GPU exchange (one process per GPU): the all-gatherv of the compacted visible lists over RCCL.
 * Replaces what the reference does inside one address space — every worker appends its range's records to the shared
 * array with `drawCount.fetch_add` + memcpy into combinedMeshes (source/system/render/mesh.cpp:177-183).
 * Rank 0 calls gv_exchange_unique_id and hands the 128 bytes to the other ranks by its own means (the engine's IPC, a
 * file, MPI ...); every rank then calls gv_exchange_init with its own context. RCCL is dlopen'ed at the first call — the
 * copy already in the process if there is one, else librccl.so.1, or the library the environment variable GV_RCCL_LIBRARY
 * names; failures return GV_E_RCCL with the RCCL text in gv_last_error. All ranks make the same calls in the same order. */
#define GV_EXCHANGE_ID_BYTES 128
#define GV_EXCHANGE_MAX_RANKS 64u
int gv_exchange_unique_id(void* out_id_128_bytes);
int gv_exchange_init(GvCtx* ctx, const void* unique_id_128_bytes, int rank, int world_size);

/* One host thread, N GPUs (the reference is ONE process with ONE Manager, source/editor/entry.cpp:135): the *_all forms take the
 * N contexts of the node's GPUs (contexts[r] = rank r) and issue their collectives inside ONE ncclGroupStart / ncclGroupEnd, which is
 * what RCCL requires of a thread that drives several devices. gv_exchange_init_all makes the unique id itself. A communicator
 * started with one form is used through that form only (per-rank calls from N threads or processes, or the *_all calls from one). */
int gv_exchange_init_all(GvCtx* const* contexts, int world_size);

/* One process, N GPUs, NO communicator: the devices of a node reach each other over xGMI with plain stores, so the ranks one thread
 * drives need neither RCCL nor a size prediction. gv_exchange_init_peers checks and enables peer access between every pair of the
 * contexts' devices (contexts may share a device) and fixes the travel pattern GV_EXCHANGE_PEER: per frame ONE kernel per rank
 * writes the words its list really has — known on the device, never on the host — from its staging shard straight into its row of
 * EVERY rank's rows (wide stores, all links at once), ordered between the ranks by events alone. Rows have room for a rank's whole
 * pool, so no frame is ever cut and nothing travels twice: tail_words / cut_ranks stay 0, room[r] = the row's capacity in entries,
 * travelled_words[r] (acquired frames) = 1 + counts[r]. Everything else — gv_exchange_visible_all / gv_exchange_views_all /
 * gv_exchange_acquire_all, the headers on the host, the bounded waits, alternating buffers — is as for the other patterns.
 * GV_E_STATE: some device cannot reach another (use gv_exchange_init_all). gv_exchange_shutdown / gv_destroy of ONE member drains
 * every member's exchange stream and dissolves the group (the others return GV_E_STATE until they are initialised again). */
int gv_exchange_init_peers(GvCtx* const* contexts, int world_size);

/* The per-frame exchange — the gather of mesh.cpp:177-183, which never loses a record: EVERY frame a consumer can acquire holds
 * every rank's complete list.
 *
 * gv_exchange_visible enqueues, on the context's stream, this rank's WHOLE shard [draw_count, visible_idx + index_base ...] into a
 * library-owned staging buffer (gv_results_copy_shard_device; the pool's gv_pool_set_index_map table applies) — the last thing
 * gv_stream(ctx) does for the frame, so the caller's next gv_hiz_build / gv_cull run while this list is still on the links — and,
 * on a second stream of the library's, the gather into library-owned rows (row r = rank r's shard). How many words of each rank's
 * row travel is PREDICTED from the previous frame's row headers, which every rank holds (they reach the host through pinned memory
 * behind that frame's collective): rank r gets count + max(count / 8, 1024) entries of room, rounded up to 1024 — grown at once,
 * given back when the list has shrunk by a quarter. Every rank sees the same headers, so every rank derives the same sizes.
 *
 * A prediction can be short (a camera cut). The frame is SETTLED — by gv_exchange_acquire of that frame or by the next
 * gv_exchange_visible, whichever comes first, and before any later collective of the communicator on every rank — by reading its
 * own headers on the host: where a header exceeds the room its row had, the missing tails travel in a second, exactly sized
 * exchange (one grouped ncclBroadcast per short rank, out of the staging buffer that still holds the whole list) to their place in
 * the rows, and only then is the frame handed out. out->cut_ranks is a statistic, not a caveat.
 *
 * Host waits: settling polls a pinned word that the frame's own collective writes — bounded (gv_exchange_set_timeout, default
 * 30 s; GV_E_TIMEOUT: a peer stalled), never a device-wide synchronisation. A caller that enqueues the next frame's cull before it
 * acquires this frame's rows keeps the device busy throughout. flags must be 0. Buffers alternate: a frame's rows stay valid until
 * the exchange after the next. */
typedef struct GvExchangeFrame {
    const void* gathered_device; /* uint32 [world_size][row_words], device memory owned by the library; NULL until the frame has
                                    been acquired (a second exchange may move the rows) */
    uint32_t row_words;          /* words between two rows, a multiple of 4 (>= 1 + the largest list) */
    uint32_t world_size;
    uint64_t frame;              /* 0, 1, 2 ... since gv_exchange_init */
    uint32_t room[GV_EXCHANGE_MAX_RANKS];            /* list entries rank r's row was PREDICTED to need (what travelled first) */
    uint32_t travelled_words[GV_EXCHANGE_MAX_RANKS]; /* of rank r's row, the words that crossed a link in the first exchange (header
                                                        included; the equal-size all-gather moves whole rows whatever the rooms) */
    uint32_t counts[GV_EXCHANGE_MAX_RANKS];          /* acquired frames: rank r's draw count = the entries behind row r's header */
    uint32_t tail_words[GV_EXCHANGE_MAX_RANKS];      /* acquired frames: words of rank r's list that travelled in the second exchange */
    uint64_t cut_ranks;          /* acquired frames: bit r = rank r's list outgrew its room and was completed (statistic) */
    uint32_t complete;           /* 1: acquired — every row holds its rank's whole list */
    uint32_t mode;               /* GvExchangeMode the rows travelled by */
    void* ready_event;           /* acquired frames: hipEvent_t behind the complete rows (hipStreamWaitEvent on a consumer's stream) */
    /* gv_exchange_views (0 for the single-list forms): the frame carries `items` lists per rank. Row r = [items + total, c_0 ..
     * c_{items-1}, list 0 (c_0 entries), list 1 ...]: the header counts the table too, so counts[] / room[] / tail_words[] above
     * are in words behind the header. item_counts (acquired frames; library-owned host memory, valid as long as the rows):
     * item_counts[r * items + i] = c_i of rank r. */
    uint32_t items;
    const uint32_t* item_counts;
} GvExchangeFrame;
int gv_exchange_visible(GvCtx* ctx, uint32_t view_index, uint32_t index_base, uint32_t flags, GvExchangeFrame* out);
/* view_index / index_base: [world_size] (index_bases NULL: all 0); frames: [world_size] outputs. */
int gv_exchange_visible_all(GvCtx* const* contexts, int world_size, const uint32_t* view_indices, const uint32_t* index_bases,
                            uint32_t flags, GvExchangeFrame* frames);
/* The same for a pool that is named (the view-indexed forms above address the pool of the most recent gv_cull): a frame that culls
 * several mesh systems first — gv_cull_batch_begin — exchanges each system's views afterwards. pool_id is the same on every rank. */
int gv_pool_exchange_visible(GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t index_base, uint32_t flags, GvExchangeFrame* out);
int gv_pool_exchange_visible_all(GvCtx* const* contexts, int world_size, uint32_t pool_id, const uint32_t* view_indices,
                                 const uint32_t* index_bases, uint32_t flags, GvExchangeFrame* frames);
/* ONE exchange for ALL the lists of a frame — the reference dispatches every mesh system's tasks and waits once
 * (source/system/render/mesh.cpp:408-546, :548): `items` names the (pool, view) pairs of the frame, the same list on every rank; a
 * rank's row is [item_count + total entries, c_0 .. c_{item_count-1}, list 0, list 1 ...] (lists packed back to back, each as
 * gv_pool_exchange_visible would send it: the pool's index map applied, index_base added), sized, completed and acquired as ONE
 * frame exactly like the single-list forms (the room prediction works on the row's words; a cut row's tail is one contiguous piece).
 * item_count <= GV_EXCHANGE_MAX_ITEMS. A consumer finds list i of rank r at row r + 1 + item_count + sum(c_0 .. c_{i-1}).
 * GvStats::exchanges counts frames sent, whatever their form. */
#define GV_EXCHANGE_MAX_ITEMS 128u
typedef struct GvExchangeItem {
    uint32_t pool_id, view_index, index_base;
} GvExchangeItem;
int gv_exchange_views(GvCtx* ctx, const GvExchangeItem* items, uint32_t item_count, uint32_t flags, GvExchangeFrame* out);
int gv_exchange_views_all(GvCtx* const* contexts, int world_size, const GvExchangeItem* items, uint32_t item_count, uint32_t flags,
                          GvExchangeFrame* frames);
/* Settles frame `frame` (one of the last two) if that has not happened yet — waits for its headers on the host, completes cut rows —
 * makes gv_stream(ctx) wait for the complete rows and fills *out (NULL: not wanted). Every rank acquires, or none does: the
 * completing exchange is a collective (ranks that skip it meet it inside their next gv_exchange_visible). */
int gv_exchange_acquire(GvCtx* ctx, uint64_t frame, GvExchangeFrame* out);
int gv_exchange_acquire_all(GvCtx* const* contexts, int world_size, uint64_t frame, GvExchangeFrame* frames);
/* Upper bound of every host wait of the exchange, in milliseconds (0: the default, 30 000; also GV_EXCHANGE_TIMEOUT_MS at
 * gv_exchange_init). A wait that runs out aborts the communicator on the spot (ncclCommAbort: the collective that will never finish
 * must not keep the device — and with it every hipFree / synchronise of the process — waiting) and returns GV_E_TIMEOUT; later
 * exchange calls return GV_E_STATE until gv_exchange_shutdown + gv_exchange_init. */
int gv_exchange_set_timeout(GvCtx* ctx, uint32_t milliseconds);

/* The same exchange with caller-owned buffers and caller-chosen sizes: row r of gathered_device (world_size * (capacity + 1)
 * uint32, device memory) = rank r's shard. capacities == NULL: every row travels whole (capacity + 1 words). Otherwise
 * capacities[world_size], each <= capacity and the same list on every rank: the direct patterns (GV_EXCHANGE_P2P /
 * _BROADCAST) move 1 + capacities[r] words of rank r's row, and this rank's shard is cut to capacities[rank] entries; the
 * equal-size all-gather moves capacity + 1 words per row regardless. No host synchronisation; a header above the row's room =
 * that rank's list was cut — this form is the caller's own sizing, with nothing behind it: use gv_exchange_visible for lists that
 * must arrive whole. */
int gv_exchange_shards(GvCtx* ctx, uint32_t view_index, uint32_t capacity, const uint32_t* capacities, uint32_t index_base,
                       void* gathered_device);
/* The exchange with bit shards (gv_results_copy_mask_device): row r of gathered_device = rank r's [draw_count, one bit per
 * mirror entry] (word_count + 1 uint32 per row; word_count the same on every rank, >= ceil(occupancy / 32) of the largest
 * pool). A fixed size whatever the view — the encoding for dense views (1/32 word per entry). */
int gv_exchange_masks(GvCtx* ctx, uint32_t view_index, uint32_t word_count, void* gathered_device);
/* Drains what is still queued (the same bounded wait: a frame that was sent and never acquired may sit behind a peer that has left —
 * GV_E_TIMEOUT / GV_E_RCCL then, the communicator aborted instead of drained) and releases the communicator, streams and rows in every
 * case; gv_destroy and a second gv_exchange_init do the same. */
int gv_exchange_shutdown(GvCtx* ctx);
/* How the rows travel (same result rows either way). The node's xGMI fabric is point to point and fully connected
 * (SURVEY.md §5, §8e): a ring all-gather serialises world-1 hops, the direct forms use every link at once and move only
 * what each rank's list needs. Default GV_EXCHANGE_ALLGATHER, or the environment variable GV_EXCHANGE_MODE (allgather | p2p |
 * broadcast) read by gv_exchange_init. */
typedef enum GvExchangeMode {
    GV_EXCHANGE_ALLGATHER = 0, /* one equal-size ncclAllGather */
    GV_EXCHANGE_P2P = 1,       /* one ncclGroup of ncclSend/ncclRecv pairs with every peer */
    GV_EXCHANGE_BROADCAST = 2, /* one ncclBroadcast per root, grouped */
    GV_EXCHANGE_PEER = 3       /* gv_exchange_init_peers only: direct stores into every rank's rows, no communicator */
} GvExchangeMode;
int gv_exchange_set_mode(GvCtx* ctx, uint32_t mode);

/* Sorts view `view_index`'s compact records on the device by distanceSq: ascending (descending == 0) as sortMeshes
 * does for unsorted buffers — front to back, operator< at render/mesh.hpp:196 — or descending for the sorted /
 * translucent ones (render/mesh.hpp:204; mesh.cpp:265-328). Stable: equal keys keep the order the records were
 * emitted in (std::sort in the reference leaves ties unspecified).
 * Call after gv_cull (records requested), before gv_results_fetch / gv_results_device. For pools of up to 2^20 slots
 * the launch is deferred to the first call that reads the records (gv_results_*, gv_exchange_*, gv_wait), where the pending
 * sorts of ALL views of ALL pools share their launches: one launch for the views of up to 16384 slots; for the larger ones one
 * set of launches — a one-launch rank sort AND the radix launches, list = blockIdx.y, the record count on the device deciding
 * per list which of them works (short lists: one launch's worth of time). A frame of many mid-sized mesh systems is bound by
 * its launches, not by bytes. Larger pools sort at once. */
int gv_sort(GvCtx* ctx, uint32_t view_index, int descending);

/* ---- picking: the editor's click selection (MeshSelectorEditorSystem::render, editor/system/render/mesh-selector.cpp:67-122) ----
 * Every ray is tested against every entry of the listed pools that passes the cull's filter chain (free slot, isEnabled, a box
 * with some extent, a transform, isActive: mesh.cpp:140-150), through the inverse of its camera-relative model
 * (calcModel(cameraPosition), transform.hpp:197-214). A ray hits a box when its entry point lies at or ahead of the origin
 * (a ray that starts inside a box does not pick it, :106). Of the hits, the one whose pivot — the model's translation — lies
 * nearest the ray origin wins (:109-110); ties go to the pool listed first, then to the lower slot (the reference's strict
 * `<` over its systems and ascending slots). Arithmetic: DESIGN.md §4 item 8. */
#define GV_MAX_PICK_RAYS 8u
typedef struct GvPickRay {
    float origin[4];    /* camera-relative, xyz used: globalOrigin of mesh-selector.cpp:73-74 */
    float direction[4]; /* camera-relative, xyz used, not normalised: globalDirection (:74-76) */
} GvPickRay;
typedef struct GvPickHit {
    uint32_t pool_id;   /* GV_NONE: the ray hit nothing */
    uint32_t slot;      /* pool slot, or the pool's index-map slot when one is installed (gv_pool_set_index_map) */
    float distance_sq;  /* distanceSq3(origin, getTranslation(model)), :109 */
    uint32_t reserved;
} GvPickHit;
/* pool_ids[0 .. pool_count): searched in this order (it decides ties). exclude_slots: NULL, or one slot per listed pool in the
 * slot space of the hits (GV_NONE: none) — the selected entity, which is never picked again (:110). camera_position: xyz used.
 * Syncs the mirror as gv_cull does, runs on gv_stream(ctx) and waits; fills hits[0 .. ray_count). The pick has buffers of its
 * own: cull results, pending sorts and device pointers are left as they were. The sync is gv_sync's, with gv_sync's one caveat:
 * edits made since a gv_cull that grow or re-order a pool (appended slots, a rebind) change the mirror's slot order, and a
 * fetch of that cull made after the pick reads is_visible through the new order — fetch before picking when the pools were
 * edited in between. GV_E_ARG: an unbound pool, ray_count 0 or above GV_MAX_PICK_RAYS, pool_count above GV_MAX_POOLS, a pool of
 * 2^28 slots or more (or an index map naming such a slot); GV_E_STATE: no transforms bound, an index map that does not cover
 * its pool, or a call between gv_cull_batch_begin and gv_cull_batch_end. */
int gv_pick(GvCtx* ctx, const uint32_t* pool_ids, uint32_t pool_count, const uint32_t* exclude_slots,
            const float camera_position[4], const GvPickRay* rays, uint32_t ray_count, GvPickHit* hits);

/* ---- scene ingest: a Garden scene file straight into column pools, no component AoS ----
 * Reads what ResourceSystem::loadScene (source/system/resource.cpp:2421-2510) hands to TransformSystem::deserialize /
 * postDeserialize (source/system/transform.cpp:517-583) and to the mesh systems' deserialize ("aabb", "isEnabled",
 * e.g. source/system/render/sprite.cpp:206-207), with the JSON typing rules of source/json-serialize.cpp. Entity ids
 * are 1, 2, ... in file order (a fresh Manager); transform / mesh slots are in order of appearance; parents are
 * resolved by uid after the whole file is read, in file order, with setParent's semantics (ancestorsActive from the
 * parent at that moment, transform.cpp:129-195). Parsing needs no device. */
typedef struct GvScene GvScene;
typedef struct GvScenePool {
    const char* component_type; /* the component's ".type" string, e.g. "Model", "Sprite" */
    uint32_t pool_id;           /* the gv_pool_bind id its meshes go to */
} GvScenePool;
typedef struct GvSceneInfo {
    uint32_t entity_count;     /* entities created (1 .. entity_count) */
    uint32_t transform_count;
    uint32_t mesh_count[GV_MAX_POOLS];
    uint32_t skipped_entities;   /* "components": [] — the reference creates no entity for them */
    uint32_t other_components;   /* components of types this pass does not read */
    uint32_t duplicate_uids;     /* later transforms with a uid already seen (the first keeps it) */
    uint32_t self_parents;       /* parent uid == own uid: no link */
    uint32_t unresolved_parents; /* parent uid not in the file: stays a root */
} GvSceneInfo;
/* flags: GV_SCENE_ADD_ROOT_ENTITY = loadScene's addRootEntity (resource.cpp:2398-2407,2497-2502): entity 1 is a default
 * transform and every loaded transform is parented to it before the file's own parent links are applied.
 * On failure returns GV_E_ARG and writes a message into `error` (may be NULL). */
#define GV_SCENE_ADD_ROOT_ENTITY 1u
int gv_scene_parse_json(const char* text, size_t length, const GvScenePool* pools, uint32_t pool_count, uint32_t flags,
                        GvScene** out_scene, char* error, size_t error_capacity);
/* The same scene as the packed builds carry it: the BSON document nlohmann::json::to_bson makes of the scene's JSON
 * (json2bson.cpp:41-66), which ResourceSystem::loadScene hands to JsonDeserializer::load(vector<uint8>) =
 * json::from_bson (resource.cpp:2359-2377, json-serialize.cpp:338-344). Same results as gv_scene_parse_json on the
 * text the document was made from: from_bson keeps the value categories the readers test (double -> float literal,
 * int32 / int64 / uint64 -> integer, bool, string, document, array by element order). Element types nlohmann's
 * from_bson rejects are rejected (GV_E_ARG). */
int gv_scene_parse_bson(const void* data, size_t length, const GvScenePool* pools, uint32_t pool_count, uint32_t flags,
                        GvScene** out_scene, char* error, size_t error_capacity);
void gv_scene_destroy(GvScene* scene);
int gv_scene_info(const GvScene* scene, GvSceneInfo* out);
/* The scene's columns (owned by the scene, valid until gv_scene_destroy); any out pointer may be NULL. */
int gv_scene_transform_columns(const GvScene* scene, GvTransformColumns* columns, uint32_t* occupancy,
                               const uint32_t** entity_to_transform, uint32_t* entity_capacity, const uint64_t** uids);
int gv_scene_mesh_columns(GvScene* scene, uint32_t pool_id, GvMeshColumns* columns, uint32_t* occupancy);
/* Binds the transform columns and every mapped mesh pool to `ctx` and schedules a full mirror build. The scene must
 * outlive the binding. For a tile (gv_scene_extract_tile) the pools' slot -> world-slot tables are installed too
 * (gv_pool_set_index_map), so exchange shards carry the world's mesh slots. */
int gv_scene_bind(GvCtx* ctx, GvScene* scene);
/* One spatial tile of a scene as a scene of its own (one process per GPU, entities sharded by spatial
 * tile; nearest reference analogue: the contiguous range split of ThreadPool::addItems, source/thread-pool.cpp:173-200).
 * The world cube of edge `side`, centred on the origin, is cut into grid[0] x grid[1] x grid[2] cells; `tile` = x + y *
 * grid[0] + z * grid[0] * grid[1]. Every ROOT transform goes to the cell its position falls in, every descendant follows
 * its root (no parent chain is cut: a tile computes the world's matrices bit for bit), a mesh follows its entity's
 * transform; free slots and meshes without a transform go to tile 0. Inside the tile slots keep their order, entity ids
 * are renumbered from 1, parents remapped. The same rule as garden_amd/multi.py::partition_world (tests compare them).
 * Each rank of a multi-GPU run parses the scene, keeps its own tile, binds it and culls; gv_scene_tile_maps gives the
 * tile-local -> world slot tables (what a gathered visible index means). Destroy with gv_scene_destroy. */
int gv_scene_extract_tile(const GvScene* scene, const uint32_t grid[3], double side, uint32_t tile, GvScene** out_tile);
/* What ONE RANK of `world_size` owns, as one scene: the cells of the same grid are put in Morton (Z-curve) order of their
 * (x, y, z) coordinates and dealt to the ranks in rounds — every `world_size` consecutive cells of that order (a compact block
 * of space) give one cell to every rank, in an order that rotates from round to round: the k-th cell goes to rank
 * (k + ((k / world_size * 2654435761 mod 2^32) >> 16)) % world_size — and the cells of `rank` are cut out together: one pool,
 * one cull launch per rank. With many more cells than ranks (16 x 16 x 16 for 8 GPUs) every rank holds an even share of
 * whatever region a view looks at: one cell per rank leaves the ranks behind the camera idle and the frame waiting for the one
 * in front of it. The reference's split is even by construction (equal contiguous index ranges,
 * source/thread-pool.cpp:180-194). Everything else as gv_scene_extract_tile (roots decide, descendants follow, ids
 * renumbered; gv_scene_tile_maps gives the local -> world slot tables), except that free slots and meshes without a
 * transform are dealt out too (slot % world_size) instead of piling up on rank 0. grid: at most 32768 cells. */
int gv_scene_extract_rank(const GvScene* scene, const uint32_t grid[3], double side, uint32_t rank, uint32_t world_size, GvScene** out_tile);
/* The same dealing rule for positions an engine holds itself: owners[i] = the rank whose cells contain position i (3 floats at
 * positions + i * stride bytes). Ownership is a matter of BALANCE, not of correctness — an entity is culled the same wherever it
 * lives — so a moving scene re-bins at its leisure: compare a root's owner with the rank it lives on now and then, and migrate
 * (destroy there, create here: the pools' own dirty marks) only the roots that have crossed into another rank's cell (SURVEY.md
 * §8e: "re-bin only roots whose position crosses a cell"). Host-only, no context needed. */
int gv_cell_owner(const uint32_t grid[3], double side, uint32_t world_size, const float* positions, uint32_t stride, uint32_t count,
                  uint32_t* owners);
int gv_scene_tile_maps(const GvScene* tile, uint32_t pool_id, const uint32_t** transform_global, uint32_t* transform_count,
                       const uint32_t** mesh_global, uint32_t* mesh_count);

/* ---- world matrices: TransformComponent::calcModel() with cameraPosition = 0 for every transform
 * slot (transform.hpp:197-214), cached on the device ---- */
typedef enum GvSweepMode {
    GV_SWEEP_VALU = 0, /* v_fma_f32 chain */
    GV_SWEEP_MFMA = 1, /* v_mfma_f32_4x4x1_16b_f32 chain (bit-identical; self-tested at gv_create) */
    /* Deferred: the NEXT gv_cull also produces the world matrices. When its pool is exactly paired with the transform
     * pool (mesh entry i belongs to transform slot i) the MFMA sweep and the cull of view 0 run as one pass over the
     * streams; otherwise the MFMA sweep is launched in front of the ordinary cull. Same bits either way. */
    GV_SWEEP_WITH_CULL = 2,
    GV_SWEEP_WITH_CULL_VALU = 3, /* the same with the v_fma_f32 chain */
    /* Brings the cache up to date with the least work (same bits as a full sweep): nothing is launched when no transform
     * changed since the last sweep; after gv_mark_dirty ranges (GV_DIRTY_TRANSFORM, ranged GV_DIRTY_HIERARCHY) only the
     * slots whose parent chain contains a re-mirrored transform are recomputed — a dirty subtree, not the pool
     * (setPosition / setParent of the reference invalidate nothing: calcModel is lazy, transform.hpp:197-214; this is the
     * device-side counterpart for a cache that is kept); a full sweep otherwise (first use, entities created or
     * destroyed, most of the pool dirty). */
    GV_SWEEP_INCREMENTAL = 4
} GvSweepMode;
int gv_sweep(GvCtx* ctx, uint32_t mode);
/* Reads back `count` world matrices (12 floats each, float4x3 order) starting at transform slot `first`. */
int gv_get_world(GvCtx* ctx, uint32_t first, uint32_t count, float* out12);

/* ---- Hi-Z: replaces HizRenderSystem::downsampleHiz (source/system/render/hiz.cpp:104-167,
 * shaders/hiz.frag:23-63). depth = reversed-Z fp32, row-major, `width` x `height`. ---- */
typedef enum GvMemKind { GV_MEM_HOST = 0, GV_MEM_DEVICE = 1 } GvMemKind;
int gv_hiz_build(GvCtx* ctx, const float* depth, uint32_t width, uint32_t height, uint32_t mem_kind);
/* Re-runs the reduction on the depth image already resident from the last gv_hiz_build. */
int gv_hiz_rebuild(GvCtx* ctx);
/* Copies mip `level` (>= 1) back as (min,max) float pairs; *w, *h receive its size. */
int gv_hiz_read_level(GvCtx* ctx, uint32_t level, float* out_pairs, uint32_t* w, uint32_t* h);
int gv_hiz_mip_count(GvCtx* ctx, uint32_t* mip_count);
/* ---- pyramid slots: several pyramids per context, one per view ----
 * A context holds up to GV_MAX_PYRAMIDS pyramids. ONE of them is selected (a new context: pyramid 0): the one gv_hiz_build,
 * gv_hiz_rebuild, gv_hiz_read_level, gv_hiz_mip_count, gv_hiz_build_from_occluders and gv_hiz_build_from_receivers address. Which
 * pyramid a VIEW queries is not a matter of the selection: the view names it (GvView::use_hiz = 1 + k), and the name is resolved
 * when the view's cull is launched, recorded culls of a batch included. A caller who never selects sees one pyramid, as before.
 * gv_hiz_select does no device work and does not synchronise; recorded culls (gv_cull_batch_begin) are launched first, as by
 * gv_hiz_build. GV_E_ARG: a NULL ctx; pyramid >= GV_MAX_PYRAMIDS (nothing changes). */
int gv_hiz_select(GvCtx* ctx, uint32_t pyramid);
/* Frees that pyramid's levels and its own copy of a host depth image (waits for gv_stream(ctx)); it is "not built" afterwards, selected
 * or not, and the selection does not change. A pyramid built from a device image — an occluder image, a receiver mask, the caller's
 * memory — only stops reading it: the image stays, and a later gv_occluder_begin / gv_receiver_begin may take it again. Recorded
 * culls are launched first. GV_OK for a pyramid that was never built. GV_E_ARG: a NULL ctx; pyramid >= GV_MAX_PYRAMIDS. */
int gv_hiz_drop(GvCtx* ctx, uint32_t pyramid);

/* ---- lifecycle, errors, metrics ---- */
int gv_create(const GvConfig* config, GvCtx** out_ctx);
void gv_destroy(GvCtx* ctx);
/* Text of the last failure on this context (or of the last failed gv_create when ctx == NULL). */
const char* gv_last_error(const GvCtx* ctx);
uint32_t gv_abi_version(void);

typedef enum GvKernelId {
    GV_K_CULL = 0,     /* frustum (+Hi-Z) test, isVisible, tile-compacted records, per-chunk counts */
    GV_K_SCAN = 1,     /* chunk-count scan */
    GV_K_EMIT = 2,     /* order-stable compaction of the record segments */
    GV_K_HIZ = 3,      /* pyramid reduction (all launches of one build) */
    GV_K_SWEEP = 4,    /* world-matrix sweep */
    GV_K_SORT = 5,     /* radix sort of the records (all launches of one gv_sort) */
    GV_K_COUNT = 6
} GvKernelId;
typedef struct GvStats {
    uint64_t launches[GV_K_COUNT];   /* kernel launches since gv_stats_reset */
    double device_ms[GV_K_COUNT];    /* summed hipEvent durations (GV_CONFIG_PROFILE_EVENTS only) */
    uint64_t upload_bytes;           /* H2D mirror bytes since reset */
    uint32_t max_depth;              /* longest parent chain in the mirror */
    uint32_t transform_count, mesh_count[GV_MAX_POOLS];
    uint64_t bounds_blocks_total;    /* GV_CONFIG_BLOCK_BOUNDS: workgroups of the last cull that ran with boxes (0: none
                                        since gv_stats_reset) ... */
    uint64_t bounds_blocks_examined; /* ... and how many of them had to run the per-entity path */
    uint64_t mirror_reorders;        /* spatial re-orders of the transform mirror done ON the device since gv_create (an unsorted
                                        tail of created entities past 1/8 of the pool; no PCIe re-upload) */
    uint64_t record_targets_lost;    /* gv_pool_set_record_target calls since gv_create that found the PREVIOUS target's range unmapped
                                        when they let it go (the caller freed it too early; text in gv_last_error). The call itself
                                        succeeds: the new target is in place */
    uint64_t exchanges;              /* exchange frames sent since gv_stats_reset (gv_exchange_visible* / gv_exchange_views*: one per call) */
    uint64_t exchange_tail_rounds;   /* ... and how many of them needed the second, exactly sized exchange (a short prediction) */
} GvStats;
int gv_stats(GvCtx* ctx, GvStats* out);
int gv_stats_reset(GvCtx* ctx);
/* Measurement aid: with GV_CONFIG_PROFILE_EVENTS, bracket only every `every`-th launch of each kernel kind (1 = all, the
 * default; the first launch after gv_stats_reset is always one of them). A bracket is two event packets on the stream, ≈ 5 us
 * of stream time per launch on MI355X (measured: frame 0.164 ms with, 0.159 ms without); bench.py samples so that the timed
 * region is the frame rather than its instrumentation. GvStats.device_ms then sums the bracketed launches only;
 * gv_profile_samples tells how many there were per kind since gv_stats_reset (divide by those, not by launches). */
int gv_profile_sampling(GvCtx* ctx, uint32_t every);
/* Which kernel kinds are bracketed from now on: bit k = GvKernelId k (0: none). gv_create derives the initial mask from the
 * config flags (PROFILE_EVENTS: all, + PROFILE_CULL_ONLY: GV_K_CULL); bench.py keeps the timed region on the dominant
 * kernel and takes the per-kernel breakdown of a frame from a few extra frames outside it. */
int gv_profile_kernels(GvCtx* ctx, uint32_t kernel_mask);
int gv_profile_samples(GvCtx* ctx, uint64_t samples[GV_K_COUNT]);

/* Measurement aid (bench.py `roofline.measured_stream_peak`): `launches` read-only passes over the five input streams
 * the cull kernel reads from pool `pool_id` (mesh a/b, transform ab/c/flags = 65 bytes per entry), with the cull's own
 * loads and launch geometry, each timed with hipEvents on the context's stream. *gb_per_s = 65 * entries / median
 * launch time: the read rate this box's HBM delivers to that access pattern. Synchronises. */
int gv_debug_stream_peak(GvCtx* ctx, uint32_t pool_id, uint32_t launches, double* gb_per_s);
/* The HIP stream all work is enqueued on (hipStream_t as void*), for callers timing with their own events. */
void* gv_stream(GvCtx* ctx);
/* The library's parked host workers for a caller's own O(N) passes over its pools (the reference runs such loops on its
 * ThreadPool, source/thread-pool.cpp:173-200: contiguous ranges, the calling thread takes part): fn(user, lo, hi) over contiguous
 * pieces of [first, first + count); one piece on the calling thread for short ranges. Returns when all pieces are done. */
void gv_host_parallel_ranges(uint32_t first, uint32_t count, void (*fn)(void* user, uint32_t lo, uint32_t hi), void* user);
/* The same workers for `count` independent tasks of some size each (fn(user, task), task = 0 .. count - 1; the calling thread takes
 * part; one task: on the calling thread). A task must not call back into gv_host_parallel_* (one run at a time per process). */
void gv_host_parallel_tasks(uint32_t count, void (*fn)(void* user, uint32_t task), void* user);

#ifdef __cplusplus
}
#endif
#endif
