// derived_results_test.cpp — TEST driver of the results DERIVED from a view's delivered records (instance data, draw bases, draw
// commands, LOD selection, view bounds, merged arrays), through include/garden_vis.h alone. It pins, as tables:
//   1. the lifetime matrix: which call ends which derived result (make the result, apply the event, read the result);
//   2. the code every reader returns for a bad context, pool, view, side column or target;
//   3. (stub build) every allocation of a whole sequence failing once, in turn: GV_E_OOM, and the same context completes it;
//   4. ownership: a context that has used every buffer of every derived result is destroyed, nothing is left behind.
// Built two ways from this file: against tests/cpp/hip_stub with the host sources under AddressSanitizer + UBSan
// (tests/test_derived_results.py; kernels are no-ops there, so codes and buffer sizes are checked, not values), and against
// libgarden_vis.so for the device (tests/cpp/derived_results.mk). Every step prints a line ending in "ok"; the last line is
// "derived results: ok".
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/garden_vis.h"
#ifdef GV_HIP_STUB
#include <hip/hip_runtime.h>  // tests/cpp/hip_stub: the fault-injection counters
#endif

struct Transform {  // include/garden/system/transform.hpp:31-61
    uint32_t entity, parent;
    uint64_t uid;
    float position[4], scale[4], rotation[4];
    void* childs;
    uint8_t selfActive, ancestorsActive, modelWithAncestors, pad[5];
};
static_assert(sizeof(Transform) == 80, "TransformComponent layout");
struct Mesh {  // include/garden/system/render/mesh.hpp:45-55
    uint32_t entity;
    uint8_t reserved[3], isEnabled, isVisible, pad[7];
    float aabbMin[4], aabbMax[4];
};
static_assert(sizeof(Mesh) == 48, "MeshRenderComponent layout");

static const char* g_where = "";
[[noreturn]] static void die(const char* file, int line, const char* what, int got, int want, GvCtx* ctx)
{
    std::fprintf(stderr, "%s:%d: [%s] %s -> %d, expected %d (%s)\n", file, line, g_where, what, got, want, ctx ? gv_last_error(ctx) : "");
    std::exit(1);
}
#define EXPECT(call, code)                                          \
    do {                                                            \
        const int rc__ = (call);                                    \
        if (rc__ != (code))                                         \
            die(__FILE__, __LINE__, #call, rc__, (int)(code), ctx); \
    } while (0)
#define CHECK(call) EXPECT(call, GV_OK)
// (inside a sequence that an injected allocation failure may end: the first code that is not GV_OK is the sequence's)
#define TRY(call)                   \
    do {                            \
        const int rc__ = (call);    \
        if (rc__ != GV_OK)          \
            return rc__;            \
    } while (0)

// ---- the shapes: a pool of 64 slots (below one 256-entry cull tile: every launch takes its smallest form), two pools of 1 slot
// (the second merge member; a pool that is a member of nothing) and a pool bound with occupancy 0 ----
constexpr uint32_t kSlots = 64, kViewSlots = 2 * kSlots;
constexpr uint32_t kMain = 0, kMember = 1, kEmpty = 2, kOther = 3, kUnbound = 5;
constexpr uint32_t kInstanceStride = 128, kCommandStride = 32, kRecordStride = 64;

struct Fixture {
    GvCtx* ctx = nullptr;
    std::vector<Transform> xf;
    std::vector<uint32_t> e2t;
    std::vector<Mesh> main, member, other, empty;
    std::vector<uint32_t> ids, ready, colour;
    std::vector<float> sizes;
    GvGeometry geometry[4] = {{36, 0, 0}, {24, 36, 0}, {12, 60, 0}, {6, 72, 0}};
    GvLodGeometry lods[4] = {};
    Fixture()
    {
        const uint32_t n = kSlots + 2;
        xf.assign(n, Transform{});
        e2t.assign(n + 1, GV_NONE);
        for (uint32_t i = 0; i < n; i++) {  // a sheet in front of a camera that looks down -z from the origin
            Transform& t = xf[i];
            t.entity = i + 1;
            e2t[t.entity] = i;
            t.uid = 100 + i;
            t.position[0] = (float)(i % 8) - 3.5f, t.position[1] = (float)(i / 8 % 8) - 3.5f, t.position[2] = -20.0f - (float)(i % 5);
            t.scale[0] = t.scale[1] = t.scale[2] = 1.0f;
            t.rotation[3] = 1.0f;
            t.selfActive = t.ancestorsActive = t.modelWithAncestors = 1;
        }
        auto mesh_of = [](uint32_t entity) {
            Mesh m{};
            m.entity = entity;
            m.isEnabled = 1;
            for (int k = 0; k < 3; k++)
                m.aabbMin[k] = -0.5f, m.aabbMax[k] = 0.5f;
            return m;
        };
        for (uint32_t i = 0; i < kSlots; i++)
            main.push_back(mesh_of(i + 1));
        member.push_back(mesh_of(kSlots + 1));
        other.push_back(mesh_of(kSlots + 2));
        empty.push_back(mesh_of(1));  // (storage for a pool bound with occupancy 0)
        for (uint32_t i = 0; i < kSlots; i++) {
            ids.push_back(i % 3);
            ready.push_back(1);
            colour.push_back(0xFF000000u | i);
            sizes.push_back(1.0f + (float)(i % 4));
        }
        for (auto& l : lods) {
            l.levels = 2;
            l.switch_at[0] = 10.0f;
        }
        GvConfig config{};
        config.struct_size = sizeof(config);
        if (gv_create(&config, &ctx) != GV_OK) {
            std::fprintf(stderr, "gv_create: %s\n", gv_last_error(nullptr));
            std::exit(1);
        }
    }
    ~Fixture() { gv_destroy(ctx); }
    Fixture(const Fixture&) = delete;
    Fixture& operator=(const Fixture&) = delete;
};

static GvView make_view(int8_t shadow_pass, uint8_t emit, uint8_t hiz = 0)
{
    GvView v{};
    v.view_proj[0] = 9.0f / 16.0f;  // infinite reversed-Z perspective, camera looking down -z
    v.view_proj[5] = 1.0f;
    v.view_proj[11] = -1.0f;
    v.view_proj[14] = 0.01f;
    v.shadow_pass = shadow_pass;
    v.use_hiz = hiz;
    v.emit_records = emit;
    return v;
}

static const GvInstanceLayout kInstanceLayout = {kInstanceStride, 0, 64, 112, 116};  // index word at 120, the payload's colour at 124
static const GvCommandLayout kCommandLayout = {kCommandStride, 0, 4, 8, 16, 12, 20};
static const float kIdentity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
static const float kScales[GV_MAX_VIEWS] = {1, 1, 1, 1, 1, 1, 1, 1};

// the pools and every side column, full size; `slots` of kMain for the rows that bind it smaller afterwards
static int bind_pools(Fixture& f, uint32_t main_slots = kSlots)
{
    GvCtx* ctx = f.ctx;
    const GvTransformLayout tl = {(uint32_t)offsetof(Transform, entity), (uint32_t)offsetof(Transform, parent), (uint32_t)offsetof(Transform, position),
                                  (uint32_t)offsetof(Transform, scale), (uint32_t)offsetof(Transform, rotation), (uint32_t)offsetof(Transform, selfActive),
                                  (uint32_t)offsetof(Transform, ancestorsActive), (uint32_t)offsetof(Transform, modelWithAncestors)};
    const GvMeshLayout ml = {(uint32_t)offsetof(Mesh, entity), (uint32_t)offsetof(Mesh, isEnabled), (uint32_t)offsetof(Mesh, isVisible),
                             (uint32_t)offsetof(Mesh, aabbMin), (uint32_t)offsetof(Mesh, aabbMax)};
    TRY(gv_transform_bind(ctx, f.xf.data(), sizeof(Transform), (uint32_t)f.xf.size(), &tl, f.e2t.data(), (uint32_t)f.e2t.size()));
    TRY(gv_pool_bind(ctx, kMain, f.main.data(), sizeof(Mesh), main_slots, &ml));
    TRY(gv_pool_bind(ctx, kMember, f.member.data(), sizeof(Mesh), 1, &ml));
    TRY(gv_pool_bind(ctx, kEmpty, f.empty.data(), sizeof(Mesh), 0, &ml));
    TRY(gv_pool_bind(ctx, kOther, f.other.data(), sizeof(Mesh), 1, &ml));
    return GV_OK;
}

static int bind_geometry(Fixture& f, uint32_t slots = kSlots) { return gv_pool_bind_geometry(f.ctx, kMain, f.ids.data(), 4, 4, slots, f.geometry, 4); }
static int bind_lod(Fixture& f, uint32_t slots = kSlots) { return gv_pool_bind_lod(f.ctx, kMain, f.sizes.data(), 4, slots, f.lods, 4); }
static int bind_payload(Fixture& f, uint32_t slots = kSlots)
{
    const GvPayloadField field = {f.colour.data(), 4, 4};
    const uint32_t at = 124;
    TRY(gv_pool_bind_payload(f.ctx, kMain, &field, 1, slots));
    return gv_pool_set_payload_layout(f.ctx, kMain, &at, 1);
}

static int bind_columns(Fixture& f)
{
    GvCtx* ctx = f.ctx;
    TRY(gv_pool_bind_ready(ctx, kMain, f.ready.data(), 4, 4));
    TRY(gv_pool_set_instance_layout(ctx, kMain, &kInstanceLayout));
    TRY(bind_payload(f));
    TRY(gv_pool_set_instance_index_field(ctx, kMain, 120));
    TRY(gv_pool_set_command_layout(ctx, kMain, &kCommandLayout));
    TRY(bind_geometry(f));
    TRY(bind_lod(f));
    // the empty pool: tables without columns
    TRY(gv_pool_set_instance_layout(ctx, kEmpty, &kInstanceLayout));
    TRY(gv_pool_set_command_layout(ctx, kEmpty, &kCommandLayout));
    TRY(gv_pool_bind_geometry(ctx, kEmpty, nullptr, 0, 0, 0, f.geometry, 4));
    TRY(gv_pool_bind_lod(ctx, kEmpty, nullptr, 0, 0, f.lods, 4));
    return GV_OK;
}

static GvMergeGroup merge_group(uint32_t id, const GvMergeItem* items, uint32_t count, void* dst = nullptr, size_t bytes = 0)
{
    GvMergeGroup g{};
    g.group_id = id;
    g.item_count = count;
    g.items = items;
    g.descending = 0;
    g.stride = kRecordStride, g.component_offset = 0, g.baked_model = 8, g.distance_sq = 56, g.buffer_index = 60;
    g.dst_device = dst;
    g.capacity_bytes = bytes;
    return g;
}
static const GvMergeItem kBothMembers[2] = {{kMain, 0, 0, sizeof(Mesh)}, {kMember, 0, 1, sizeof(Mesh)}};
static const GvMergeItem kMemberAlone[1] = {{kMember, 0, 1, sizeof(Mesh)}};
static const uint32_t kViews01[2] = {0, 1};

// kMain culled with three views (two with records, the third count-only), kMember and kOther with one
static int cull_all(Fixture& f)
{
    GvCtx* ctx = f.ctx;
    const GvView views[3] = {make_view(-1, 1), make_view(0, 1), make_view(1, 0)};
    TRY(gv_cull(ctx, kMain, views, 3));
    TRY(gv_cull(ctx, kMember, views, 1));
    TRY(gv_cull(ctx, kOther, views, 1));
    return GV_OK;
}

// ... and every derived result of kMain made: group 0 merges kMain and kMember, group 1 kMember alone
static int make_all(Fixture& f)
{
    GvCtx* ctx = f.ctx;
    TRY(bind_geometry(f));
    TRY(bind_lod(f));
    TRY(cull_all(f));
    TRY(gv_pool_sort(ctx, kMain, 0, 0));
    TRY(gv_pool_sort(ctx, kMember, 0, 0));
    TRY(gv_pool_emit_draw_instances(ctx, kMain, kViews01, 2, nullptr, 0));
    TRY(gv_pool_select_lods(ctx, kMain, kScales, 2));
    TRY(gv_pool_emit_draw_commands(ctx, kMain, 0, 0, nullptr, 0));
    TRY(gv_pool_view_bounds(ctx, kMain, kViews01, kIdentity, 1));
    const GvMergeGroup groups[2] = {merge_group(0, kBothMembers, 2), merge_group(1, kMemberAlone, 1)};
    TRY(gv_merge_sorted(ctx, groups, 2));
    return GV_OK;
}

enum { R_INSTANCES, R_DRAW_BASES, R_COMMANDS, R_LODS, R_BOUNDS, R_MERGE_MEMBER, R_MERGE_OTHER, R_COUNT };
static const char* const kResultNames[R_COUNT] = {"gv_pool_instances_device", "gv_pool_draw_bases_device", "gv_pool_draw_commands_device",
                                                  "gv_pool_lods_device",      "gv_pool_view_bounds_device", "gv_merge_device (member)",
                                                  "gv_merge_device (not a member)"};

static void read_results(GvCtx* ctx, uint32_t pool, uint32_t member_group, uint32_t other_group, int rc[R_COUNT])
{
    const void *a = nullptr, *b = nullptr;
    uint32_t n = 0;
    rc[R_INSTANCES] = gv_pool_instances_device(ctx, pool, &a, &b);
    rc[R_DRAW_BASES] = gv_pool_draw_bases_device(ctx, pool, &a, &b);
    rc[R_COMMANDS] = gv_pool_draw_commands_device(ctx, pool, &a, &b);
    rc[R_LODS] = gv_pool_lods_device(ctx, pool, &a, &b);
    rc[R_BOUNDS] = gv_pool_view_bounds_device(ctx, pool, &a, &n);
    rc[R_MERGE_MEMBER] = gv_merge_device(ctx, member_group, &a, &b);
    rc[R_MERGE_OTHER] = gv_merge_device(ctx, other_group, &a, &b);
}

// `row`: one character per result in the order of the enum, '1' the result is still read (GV_OK), '0' it has ended (GV_E_STATE)
static void expect_row(GvCtx* ctx, const char* event, uint32_t pool, uint32_t member_group, uint32_t other_group, const char* row)
{
    int rc[R_COUNT];
    read_results(ctx, pool, member_group, other_group, rc);
    for (int r = 0; r < R_COUNT; r++) {
        const int want = row[r] == '1' ? GV_OK : GV_E_STATE;
        if (rc[r] != want) {
            std::fprintf(stderr, "lifetime matrix: after %s, %s returns %d, pinned %d\n", event, kResultNames[r], rc[r], want);
            std::exit(1);
        }
    }
}

// ---- 1. the lifetime matrix ----------------------------------------------------------------------------------------------------
struct Event {
    const char* name;
    int (*apply)(Fixture&);
    int code;         // what the event itself returns
    const char* row;  // instances, draw bases, commands, LODs, bounds, merge (member), merge (not a member)
};

static const GvView kOneView = make_view(-1, 1);
static const GvView kHizView = make_view(-1, 1, 1);  // (no pyramid is ever built here: GV_E_STATE)
static const uint32_t kView0[1] = {0}, kCountOnly[1] = {2};

static const Event kEvents[] = {
    // a cull or a second phase ends everything of that pool, and every merge the pool is a member of
    {"gv_cull", [](Fixture& f) { const GvView v[2] = {make_view(-1, 1), make_view(0, 1)}; return gv_cull(f.ctx, kMain, v, 2); }, GV_OK, "0000001"},
    {"gv_cull recorded in a batch", [](Fixture& f) { TRY(gv_cull_batch_begin(f.ctx)); return gv_cull(f.ctx, kMain, &kOneView, 1); }, GV_OK, "0000001"},
    {"gv_pool_cull_second_phase", [](Fixture& f) { return gv_pool_cull_second_phase(f.ctx, kMain, 0, 3, &kOneView); }, GV_OK, "0000001"},
    // an instance emission ends the commands and the selection (draw bases are those of a DRAW emission: a plain one has none)
    {"gv_pool_emit_instances", [](Fixture& f) { return gv_pool_emit_instances(f.ctx, kMain, kView0, 1, nullptr, 0); }, GV_OK, "1000111"},
    {"gv_pool_emit_draw_instances", [](Fixture& f) { return gv_pool_emit_draw_instances(f.ctx, kMain, kViews01, 2, nullptr, 0); }, GV_OK, "1100111"},
    // a new selection does not end the commands made before it
    {"gv_pool_select_lods", [](Fixture& f) { return gv_pool_select_lods(f.ctx, kMain, kScales, 2); }, GV_OK, "1111111"},
    {"gv_pool_select_lods(NULL, 0)", [](Fixture& f) { return gv_pool_select_lods(f.ctx, kMain, nullptr, 0); }, GV_OK, "1110111"},
    // a re-bind of the LOD table with a table does not end the selection; an unbind does
    {"gv_pool_bind_lod with a table", [](Fixture& f) { return bind_lod(f); }, GV_OK, "1111111"},
    {"gv_pool_bind_lod without a table", [](Fixture& f) { return gv_pool_bind_lod(f.ctx, kMain, nullptr, 0, 0, nullptr, 0); }, GV_OK, "1110111"},
    {"gv_pool_bind_geometry", [](Fixture& f) { return bind_geometry(f); }, GV_OK, "1111111"},
    {"gv_pool_emit_draw_commands", [](Fixture& f) { return gv_pool_emit_draw_commands(f.ctx, kMain, GV_COMMANDS_MERGE_RUNS, 0, nullptr, 0); }, GV_OK, "1111111"},
    {"gv_pool_view_bounds", [](Fixture& f) { return gv_pool_view_bounds(f.ctx, kMain, kViews01 + 1, kIdentity, 1); }, GV_OK, "1111111"},
    {"gv_pool_sort", [](Fixture& f) { return gv_pool_sort(f.ctx, kMain, 1, 1); }, GV_OK, "1111111"},
    {"gv_merge_sorted", [](Fixture& f) { const GvMergeGroup g = merge_group(0, kBothMembers, 2); return gv_merge_sorted(f.ctx, &g, 1); }, GV_OK, "1111111"},
    // a cull of another pool ends nothing of this pool — but the merges THAT pool is a member of
    {"gv_cull of a pool that is a member of nothing", [](Fixture& f) { return gv_cull(f.ctx, kOther, &kOneView, 1); }, GV_OK, "1111111"},
    {"gv_cull of the empty pool", [](Fixture& f) { return gv_cull(f.ctx, kEmpty, &kOneView, 1); }, GV_OK, "1111111"},
    {"gv_cull of the other member", [](Fixture& f) { return gv_cull(f.ctx, kMember, &kOneView, 1); }, GV_OK, "1111100"},
    // a failed call ends nothing
    {"gv_cull, no views", [](Fixture& f) { return gv_cull(f.ctx, kMain, &kOneView, 0); }, GV_E_ARG, "1111111"},
    {"gv_cull, Hi-Z without a pyramid", [](Fixture& f) { return gv_cull(f.ctx, kMain, &kHizView, 1); }, GV_E_STATE, "1111111"},
    {"gv_cull in a batch, Hi-Z without a pyramid", [](Fixture& f) { TRY(gv_cull_batch_begin(f.ctx)); return gv_cull(f.ctx, kMain, &kHizView, 1); }, GV_E_STATE, "1111111"},
    {"gv_pool_cull_second_phase, one view twice", [](Fixture& f) { return gv_pool_cull_second_phase(f.ctx, kMain, 0, 0, &kOneView); }, GV_E_ARG, "1111111"},
    {"gv_pool_cull_second_phase, Hi-Z without a pyramid", [](Fixture& f) { return gv_pool_cull_second_phase(f.ctx, kMain, 0, 3, &kHizView); }, GV_E_STATE, "1111111"},
    {"gv_pool_emit_instances, no views", [](Fixture& f) { return gv_pool_emit_instances(f.ctx, kMain, kView0, 0, nullptr, 0); }, GV_E_ARG, "1111111"},
    {"gv_pool_emit_instances, a count-only view", [](Fixture& f) { return gv_pool_emit_instances(f.ctx, kMain, kCountOnly, 1, nullptr, 0); }, GV_E_STATE, "1111111"},
    {"gv_pool_emit_draw_instances, no views", [](Fixture& f) { return gv_pool_emit_draw_instances(f.ctx, kMain, kView0, 0, nullptr, 0); }, GV_E_ARG, "1111111"},
    {"gv_pool_emit_draw_instances, a count-only view", [](Fixture& f) { return gv_pool_emit_draw_instances(f.ctx, kMain, kCountOnly, 1, nullptr, 0); }, GV_E_STATE, "1111111"},
    {"gv_pool_select_lods, one scale for two views", [](Fixture& f) { return gv_pool_select_lods(f.ctx, kMain, kScales, 1); }, GV_E_ARG, "1111111"},
    {"gv_pool_select_lods(NULL, 2)", [](Fixture& f) { return gv_pool_select_lods(f.ctx, kMain, nullptr, 2); }, GV_E_ARG, "1111111"},
    {"gv_pool_select_lods, ids that cover half the view", [](Fixture& f) { TRY(bind_geometry(f, kSlots / 2)); return gv_pool_select_lods(f.ctx, kMain, kScales, 2); }, GV_E_STATE, "1111111"},
    {"gv_pool_bind_lod, a stride of 2", [](Fixture& f) { return gv_pool_bind_lod(f.ctx, kMain, f.sizes.data(), 2, kSlots, f.lods, 4); }, GV_E_ARG, "1111111"},
    {"gv_pool_bind_geometry, a width of 3", [](Fixture& f) { return gv_pool_bind_geometry(f.ctx, kMain, f.ids.data(), 4, 3, kSlots, f.geometry, 4); }, GV_E_ARG, "1111111"},
    {"gv_pool_emit_draw_commands, unknown flags", [](Fixture& f) { return gv_pool_emit_draw_commands(f.ctx, kMain, 0x80, 0, nullptr, 0); }, GV_E_ARG, "1111111"},
    {"gv_pool_emit_draw_commands, ids that cover half the view", [](Fixture& f) { TRY(bind_geometry(f, kSlots / 2)); return gv_pool_emit_draw_commands(f.ctx, kMain, 0, 0, nullptr, 0); }, GV_E_STATE, "1111111"},
    {"gv_pool_view_bounds, no items", [](Fixture& f) { return gv_pool_view_bounds(f.ctx, kMain, kView0, kIdentity, 0); }, GV_E_ARG, "1111111"},
    {"gv_pool_view_bounds, a count-only view", [](Fixture& f) { return gv_pool_view_bounds(f.ctx, kMain, kCountOnly, kIdentity, 1); }, GV_E_STATE, "1111111"},
    {"gv_pool_sort, a count-only view", [](Fixture& f) { return gv_pool_sort(f.ctx, kMain, 2, 0); }, GV_E_ARG, "1111111"},
    {"gv_pool_group_draws, unknown flags", [](Fixture& f) { return gv_pool_group_draws(f.ctx, kMain, 1, 0x80, 1.0f); }, GV_E_ARG, "1111111"},
    {"gv_pool_group_draws behind an emission", [](Fixture& f) { return gv_pool_group_draws(f.ctx, kMain, 1, 0, 1.0f); }, GV_E_STATE, "1111111"},
    {"gv_merge_sorted, no groups", [](Fixture& f) { const GvMergeGroup g = merge_group(0, kBothMembers, 2); return gv_merge_sorted(f.ctx, &g, 0); }, GV_E_ARG, "1111111"},
    {"gv_merge_sorted, a count-only member", [](Fixture& f) { const GvMergeItem item = {kMain, 2, 0, sizeof(Mesh)}; const GvMergeGroup g = merge_group(0, &item, 1); return gv_merge_sorted(f.ctx, &g, 1); }, GV_E_STATE, "1111111"},
};

static void lifetime_matrix()
{
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(bind_columns(f));
    uint32_t events = 0;
    for (const Event& e : kEvents) {
        g_where = e.name;
        CHECK(make_all(f));
        expect_row(ctx, "everything was made", kMain, 0, 1, "1111111");
        const int rc = e.apply(f);
        if (rc != e.code)
            die(__FILE__, __LINE__, e.name, rc, e.code, ctx);
        expect_row(ctx, e.name, kMain, 0, 1, e.row);
        CHECK(gv_cull_batch_end(ctx));  // (a recorded cull is launched; the rows above were read while it was only recorded)
        expect_row(ctx, e.name, kMain, 0, 1, e.row);
        events++;
    }
    // gv_pool_group_draws is refused behind an emission (above); in front of one it reorders the view and ends nothing: the bounds
    // taken of the view and the merged array it is a member of are still read (the view merely counts as unsorted from then on)
    g_where = "gv_pool_group_draws";
    CHECK(make_all(f));
    CHECK(cull_all(f));
    CHECK(gv_pool_sort(ctx, kMain, 0, 0));
    CHECK(gv_pool_sort(ctx, kMember, 0, 0));
    CHECK(gv_pool_view_bounds(ctx, kMain, kView0, kIdentity, 1));
    const GvMergeGroup groups[2] = {merge_group(0, kBothMembers, 2), merge_group(1, kMemberAlone, 1)};
    CHECK(gv_merge_sorted(ctx, groups, 2));
    expect_row(ctx, "culls, bounds and merges", kMain, 0, 1, "0000111");
    CHECK(gv_pool_group_draws(ctx, kMain, 0, GV_GROUP_BY_LOD, 1.0f));
    expect_row(ctx, "gv_pool_group_draws", kMain, 0, 1, "0000111");
    EXPECT(gv_merge_sorted(ctx, groups, 1), GV_E_STATE);  // (no longer in distance order)
    expect_row(ctx, "gv_merge_sorted of a grouped view", kMain, 0, 1, "0000111");
    events++;
    std::printf("lifetime matrix: %u events x %d results as pinned: ok\n", events, (int)R_COUNT);
}

// a pool bound with occupancy 0: the calls return early, and what they end has ended all the same
static void empty_pool()
{
    Fixture f;
    GvCtx* ctx = f.ctx;
    g_where = "empty pool";
    CHECK(bind_pools(f));
    CHECK(bind_columns(f));
    const GvMergeItem item = {kEmpty, 0, 0, sizeof(Mesh)};
    const GvMergeGroup groups[2] = {merge_group(2, &item, 1), merge_group(1, kMemberAlone, 1)};
    auto make = [&](bool emit) {
        CHECK(gv_cull(ctx, kEmpty, &kOneView, 1));
        CHECK(gv_cull(ctx, kMember, &kOneView, 1));
        CHECK(gv_pool_sort(ctx, kEmpty, 0, 0));
        CHECK(gv_pool_sort(ctx, kMember, 0, 0));
        if (emit) {
            CHECK(gv_pool_emit_draw_instances(ctx, kEmpty, kView0, 1, nullptr, 0));
            CHECK(gv_pool_select_lods(ctx, kEmpty, kScales, 1));
            CHECK(gv_pool_emit_draw_commands(ctx, kEmpty, GV_COMMANDS_MERGE_RUNS, 0, nullptr, 0));
        }
        CHECK(gv_pool_view_bounds(ctx, kEmpty, kView0, kIdentity, 1));
        CHECK(gv_merge_sorted(ctx, groups, 2));
    };
    make(true);
    expect_row(ctx, "everything was made of the empty pool", kEmpty, 2, 1, "1111111");
    CHECK(gv_pool_cull_second_phase(ctx, kEmpty, 0, 1, &kOneView));
    expect_row(ctx, "gv_pool_cull_second_phase of the empty pool", kEmpty, 2, 1, "0000001");
    make(true);
    CHECK(gv_cull(ctx, kEmpty, &kOneView, 1));
    expect_row(ctx, "gv_cull of the empty pool", kEmpty, 2, 1, "0000001");
    make(false);
    CHECK(gv_pool_group_draws(ctx, kEmpty, 0, GV_GROUP_BY_LOD, 1.0f));
    expect_row(ctx, "gv_pool_group_draws of the empty pool", kEmpty, 2, 1, "0000111");
    EXPECT(gv_merge_sorted(ctx, groups, 1), GV_E_STATE);  // the view no longer counts as sorted
    GvViewBounds bounds{};
    CHECK(gv_pool_view_bounds_fetch(ctx, kEmpty, &bounds, 1));
    uint32_t counts[2] = {7, 7};
    CHECK(gv_merge_fetch(ctx, 2, nullptr, 0, counts, 2));
    if (bounds.draw_count != 0 || counts[0] != 0 || counts[1] != 0) {
        std::fprintf(stderr, "empty pool: %u draws in the bounds, %u / %u in the merge\n", bounds.draw_count, counts[0], counts[1]);
        std::exit(1);
    }
    std::printf("empty pool: the early returns end what a cull, a second phase and a grouping end: ok\n");
}

// ---- 2. the readers' codes -----------------------------------------------------------------------------------------------------
enum { E_INSTANCES, E_DRAW_INSTANCES, E_COMMANDS, E_LODS, E_GROUP, E_SECOND, E_BOUNDS, E_MERGE, E_COUNT };
static const char* const kReaderNames[E_COUNT] = {"gv_pool_emit_instances", "gv_pool_emit_draw_instances", "gv_pool_emit_draw_commands", "gv_pool_select_lods",
                                                  "gv_pool_group_draws",    "gv_pool_cull_second_phase",   "gv_pool_view_bounds",        "gv_merge_sorted"};
constexpr int NA = 1000;  // the case does not exist for this reader (it takes no view, no target ...)

static int call_reader(int e, GvCtx* ctx, uint32_t pool, uint32_t view, void* dst, uint32_t group_flags = 0)
{
    const size_t bytes = dst ? 4096 : 0;
    switch (e) {
    case E_INSTANCES: return gv_pool_emit_instances(ctx, pool, &view, 1, dst, bytes);
    case E_DRAW_INSTANCES: return gv_pool_emit_draw_instances(ctx, pool, &view, 1, dst, bytes);
    case E_COMMANDS: return gv_pool_emit_draw_commands(ctx, pool, 0, 0, dst, bytes);
    case E_LODS: return gv_pool_select_lods(ctx, pool, kScales, 1);
    case E_GROUP: return gv_pool_group_draws(ctx, pool, view, group_flags, 1.0f);
    case E_SECOND: return gv_pool_cull_second_phase(ctx, pool, view, view == 3 ? 4 : 3, &kOneView);
    case E_BOUNDS: return gv_pool_view_bounds(ctx, pool, &view, kIdentity, 1);
    default: {
        const GvMergeItem item = {pool, view, 0, sizeof(Mesh)};
        const GvMergeGroup g = merge_group(3, &item, 1, dst, bytes);
        return gv_merge_sorted(ctx, &g, 1);
    }
    }
}

static uint32_t g_reader_cells = 0;
static void expect_reader(const char* name, int e, int got, int want, GvCtx* ctx)
{
    if (got != want) {
        std::fprintf(stderr, "reader prologues: %s, %s returns %d, pinned %d (%s)\n", name, kReaderNames[e], got, want, ctx ? gv_last_error(ctx) : "");
        std::exit(1);
    }
    g_reader_cells++;
}

static void reader_prologues()
{
    const int ARG = GV_E_ARG, STATE = GV_E_STATE;
    struct Case {
        const char* name;
        int want[E_COUNT];  // instances, draw instances, commands, LODs, group, second phase, bounds, merge
    };
    // every case: a fresh context, pools bound and culled as the case says, then each reader once. NOT uniform, pinned as they are:
    // a view without records is GV_E_ARG for the grouping and the second phase and GV_E_STATE for the emissions, and so on
    {
        const Case c = {"a NULL context", {ARG, ARG, ARG, ARG, ARG, ARG, ARG, ARG}};
        for (int e = 0; e < E_COUNT; e++)
            expect_reader(c.name, e, call_reader(e, nullptr, kMain, 0, nullptr), c.want[e], nullptr);
    }
    {
        Fixture f;
        GvCtx* ctx = f.ctx;
        CHECK(bind_pools(f));
        CHECK(bind_columns(f));
        CHECK(cull_all(f));
        const Case range = {"a pool index out of range", {ARG, ARG, ARG, ARG, ARG, ARG, ARG, ARG}};
        const Case unbound = {"an unbound pool", {ARG, ARG, ARG, ARG, ARG, ARG, ARG, ARG}};
        for (int e = 0; e < E_COUNT; e++) {
            expect_reader(range.name, e, call_reader(e, ctx, GV_MAX_POOLS, 0, nullptr), range.want[e], ctx);
            expect_reader(unbound.name, e, call_reader(e, ctx, kUnbound, 0, nullptr), unbound.want[e], ctx);
        }
        // (the commands and the selection take their views from the emission: without one, GV_E_STATE)
        const Case index = {"a view index out of range", {ARG, ARG, NA, NA, ARG, ARG, ARG, ARG}};
        const Case never = {"a view no cull has ever had", {STATE, STATE, STATE, STATE, ARG, ARG, ARG, ARG}};
        const Case count_only = {"a count-only view", {STATE, STATE, NA, NA, ARG, ARG, STATE, STATE}};
        for (int e = 0; e < E_COUNT; e++) {
            if (index.want[e] != NA)
                expect_reader(index.name, e, call_reader(e, ctx, kMain, GV_MAX_VIEWS, nullptr), index.want[e], ctx);
            expect_reader(never.name, e, call_reader(e, ctx, kMain, 5, nullptr), never.want[e], ctx);
            if (count_only.want[e] != NA)
                expect_reader(count_only.name, e, call_reader(e, ctx, kMain, 2, nullptr), count_only.want[e], ctx);
        }
        // a later, narrower cull: view 1 has had results and has none now
        CHECK(gv_cull(ctx, kMain, &kOneView, 1));
        const Case narrowed = {"a view a later, narrower cull has switched off", {STATE, STATE, NA, NA, ARG, ARG, STATE, ARG}};
        for (int e = 0; e < E_COUNT; e++)
            if (narrowed.want[e] != NA)
                expect_reader(narrowed.name, e, call_reader(e, ctx, kMain, 1, nullptr), narrowed.want[e], ctx);
    }
    {   // a side column that covers fewer slots than the view was culled with
        Fixture f;
        GvCtx* ctx = f.ctx;
        const char* name = "a side column that covers half the view";
        CHECK(bind_pools(f));
        CHECK(bind_columns(f));
        CHECK(cull_all(f));
        CHECK(bind_payload(f, kSlots / 2));
        expect_reader(name, E_INSTANCES, call_reader(E_INSTANCES, ctx, kMain, 0, nullptr), STATE, ctx);
        expect_reader(name, E_DRAW_INSTANCES, call_reader(E_DRAW_INSTANCES, ctx, kMain, 0, nullptr), STATE, ctx);
        CHECK(bind_payload(f));
        CHECK(bind_geometry(f, kSlots / 2));
        expect_reader(name, E_GROUP, call_reader(E_GROUP, ctx, kMain, 0, nullptr), STATE, ctx);
        CHECK(call_reader(E_INSTANCES, ctx, kMain, 0, nullptr));
        expect_reader(name, E_COMMANDS, call_reader(E_COMMANDS, ctx, kMain, 0, nullptr), STATE, ctx);
        expect_reader(name, E_LODS, call_reader(E_LODS, ctx, kMain, 0, nullptr), STATE, ctx);
        CHECK(bind_geometry(f));
        CHECK(bind_lod(f, kSlots / 2));
        expect_reader(name, E_LODS, call_reader(E_LODS, ctx, kMain, 0, nullptr), STATE, ctx);
        CHECK(cull_all(f));
        expect_reader(name, E_GROUP, call_reader(E_GROUP, ctx, kMain, 0, nullptr, GV_GROUP_BY_LOD), STATE, ctx);
        CHECK(bind_lod(f));
        // the merge's column is the index map of a pool that delivers its records in world slots
        CHECK(gv_pool_sort(ctx, kMain, 0, 0));
        CHECK(gv_pool_set_index_map(ctx, kMain, f.ids.data(), kSlots / 2));
        CHECK(gv_pool_set_result_mapping(ctx, kMain, GV_RESULTS_MAP_RECORDS, nullptr, 0, 0));
        expect_reader(name, E_MERGE, call_reader(E_MERGE, ctx, kMain, 0, nullptr), STATE, ctx);
        CHECK(gv_pool_set_result_mapping(ctx, kMain, 0, nullptr, 0, 0));
        CHECK(gv_pool_set_index_map(ctx, kMain, nullptr, 0));
        // the pool's own columns, bound smaller behind the cull: the ready column of the draw emission, the second phase's pool
        CHECK(bind_pools(f, kSlots / 2));
        expect_reader(name, E_DRAW_INSTANCES, call_reader(E_DRAW_INSTANCES, ctx, kMain, 0, nullptr), STATE, ctx);
        expect_reader(name, E_SECOND, call_reader(E_SECOND, ctx, kMain, 0, nullptr), STATE, ctx);
        // (gv_pool_view_bounds reads the mirror as it stands: the case does not exist for it)
    }
    {   // a caller target that is not 16-byte aligned: device memory of the library's own, four bytes in
        Fixture f;
        GvCtx* ctx = f.ctx;
        const char* name = "a caller target that is not 16-byte aligned";
        CHECK(bind_pools(f));
        CHECK(bind_columns(f));
        CHECK(cull_all(f));
        CHECK(gv_pool_sort(ctx, kMember, 0, 0));
        CHECK(gv_pool_emit_instances(ctx, kMain, kView0, 1, nullptr, 0));
        const void *instances = nullptr, *starts = nullptr;
        CHECK(gv_pool_instances_device(ctx, kMain, &instances, &starts));
        void* const odd = static_cast<uint8_t*>(const_cast<void*>(instances)) + 4;
        expect_reader(name, E_COMMANDS, call_reader(E_COMMANDS, ctx, kMain, 0, odd), ARG, ctx);
        expect_reader(name, E_MERGE, call_reader(E_MERGE, ctx, kMember, 0, odd), ARG, ctx);
        expect_reader(name, E_INSTANCES, call_reader(E_INSTANCES, ctx, kMain, 0, odd), ARG, ctx);
        expect_reader(name, E_DRAW_INSTANCES, call_reader(E_DRAW_INSTANCES, ctx, kMain, 0, odd), ARG, ctx);
        const void* still = nullptr;
        CHECK(gv_pool_instances_device(ctx, kMain, &still, &starts));  // (the refused emissions replaced nothing)
        if (still != instances)
            die(__FILE__, __LINE__, "the target of the emission in place", 1, 0, ctx);
    }
    std::printf("reader prologues: %d entry points x 9 cases, %u codes as pinned: ok\n", (int)E_COUNT, g_reader_cells);
}

// ---- 3. and 4.: one sequence through every buffer of every derived result ---------------------------------------------------------
// cull -> sort -> group -> emit draw instances -> select -> commands in run mode -> bounds -> merge -> every _fetch. The fetch
// arrays hold the host's bounds (the sum of the listed views' occupancies), so they are large enough whatever the counts are.
#ifdef GV_HIP_STUB
// the stub's kernels are no-ops and its "device" memory is zeroed host memory: counts written here make the fetches copy something
static void poke(const void* device, std::initializer_list<uint32_t> words)
{
    uint32_t* at = static_cast<uint32_t*>(const_cast<void*>(device));
    for (uint32_t w : words)
        *at++ = w;
}
#else
static void poke(const void*, std::initializer_list<uint32_t>) {}
#endif

constexpr int kWrongValues = -100;  // (not a code of the library's)

static int derived_sequence(Fixture& f)
{
    GvCtx* ctx = f.ctx;
    const void *a = nullptr, *b = nullptr;
    TRY(bind_pools(f));
    TRY(bind_columns(f));
    TRY(cull_all(f));
    TRY(gv_pool_sort(ctx, kMain, 0, 0));
    TRY(gv_pool_sort(ctx, kMember, 0, 0));
    TRY(gv_pool_group_draws(ctx, kMain, 1, GV_GROUP_BY_LOD, 1.0f));
    TRY(gv_pool_emit_draw_instances(ctx, kMain, kViews01, 2, nullptr, 0));
    TRY(gv_pool_instances_device(ctx, kMain, &a, &b));
    poke(b, {0, 10, 20});
    TRY(gv_pool_draw_bases_device(ctx, kMain, &a, &b));
    poke(b, {0, 10, 20});
    TRY(gv_pool_select_lods(ctx, kMain, kScales, 2));
    TRY(gv_pool_lods_device(ctx, kMain, &a, &b));
    poke(b, {10, 0, 0, 0, 0, 0, 0, 0, 4, 6});
    TRY(gv_pool_emit_draw_commands(ctx, kMain, GV_COMMANDS_MERGE_RUNS, 0, nullptr, 0));
    TRY(gv_pool_draw_commands_device(ctx, kMain, &a, &b));
    poke(b, {3, 4});
    TRY(gv_pool_view_bounds(ctx, kMain, kViews01, kIdentity, 1));
    const GvMergeGroup group = merge_group(0, kBothMembers, 2);
    TRY(gv_merge_sorted(ctx, &group, 1));
    TRY(gv_merge_device(ctx, 0, &a, &b));
    poke(b, {4, 1, 5});
    // every fetch
    std::vector<uint8_t> instances((size_t)kViewSlots * kInstanceStride), commands((size_t)kViewSlots * kCommandStride),
        records((size_t)(kSlots + 1) * kRecordStride);
    std::vector<uint32_t> first(kViewSlots + 1), ids(kViewSlots);
    uint32_t starts[3], draw_starts[3], command_counts[2], level_counts[2 * GV_MAX_LOD_LEVELS], merge_counts[3];
    GvViewBounds bounds[1];
    TRY(gv_pool_instances_fetch(ctx, kMain, instances.data(), instances.size(), starts, 3));
    TRY(gv_pool_draw_bases_fetch(ctx, kMain, first.data(), (uint32_t)first.size(), draw_starts, 3));
    TRY(gv_pool_draw_commands_fetch(ctx, kMain, commands.data(), commands.size(), command_counts, 2));
    TRY(gv_pool_lods_fetch(ctx, kMain, ids.data(), (uint32_t)ids.size(), level_counts, 2 * GV_MAX_LOD_LEVELS));
    TRY(gv_pool_view_bounds_fetch(ctx, kMain, bounds, 1));
    TRY(gv_merge_fetch(ctx, 0, records.data(), records.size(), merge_counts, 3));
#ifdef GV_HIP_STUB
    if (starts[2] != 20 || draw_starts[2] != 20 || command_counts[1] != 4 || level_counts[GV_MAX_LOD_LEVELS + 1] != 6 || merge_counts[2] != 5) {
        std::fprintf(stderr, "derived_sequence: the fetches did not deliver the counts written into the stub's device words\n");
        return kWrongValues;
    }
#else
    if (starts[2] > kViewSlots || draw_starts[2] != starts[2] || merge_counts[2] != merge_counts[0] + merge_counts[1] || bounds[0].draw_count > kSlots)
        return kWrongValues;
#endif
    return GV_OK;
}

#ifdef GV_HIP_STUB
static void allocation_failures()
{
    g_where = "allocation failures";
    long total = 0;
    {
        Fixture probe;
        const long before = gv_stub_allocations();
        GvCtx* ctx = probe.ctx;
        CHECK(derived_sequence(probe));
        total = gv_stub_allocations() - before;
    }
    int failed_calls = 0;
    for (long k = 1; k <= total; k++) {
        Fixture f;
        GvCtx* ctx = f.ctx;
        gv_stub_fail_countdown() = k;
        const int rc = derived_sequence(f);
        gv_stub_fail_countdown() = 0;
        if (rc != GV_E_OOM || !*gv_last_error(ctx)) {
            std::fprintf(stderr, "allocation %ld of %ld failing: the sequence returned %d (%s), not GV_E_OOM\n", k, total, rc, gv_last_error(ctx));
            std::exit(1);
        }
        failed_calls++;
        CHECK(derived_sequence(f));  // the same context completes the sequence
    }
    std::printf("allocation failures in the derived results: %ld allocations failed in turn, %d calls returned GV_E_OOM, every context completed "
                "the sequence: ok\n", total, failed_calls);
}
#endif

static void ownership()
{
    g_where = "ownership";
    {
        Fixture f;
        GvCtx* ctx = f.ctx;
        CHECK(derived_sequence(f));
        // ... and the buffers the sequence leaves out: a plain emission, per-draw commands, the empty pool's, a second phase's seen set
        CHECK(gv_pool_emit_instances(ctx, kMain, kView0, 1, nullptr, 0));
        CHECK(gv_pool_emit_draw_commands(ctx, kMain, 0, 8, nullptr, 0));
        CHECK(gv_pool_cull_second_phase(ctx, kMain, 0, 3, &kOneView));
        CHECK(gv_pool_view_bounds(ctx, kMain, kViews01, kIdentity, 1));
    }  // gv_destroy
    std::printf("ownership: a context that used every buffer of every derived result was destroyed: ok\n");
}

int main()
{
    lifetime_matrix();
    empty_pool();
    reader_prologues();
#ifdef GV_HIP_STUB
    allocation_failures();
#endif
    ownership();
    std::printf("derived results: ok\n");
    return 0;
}
