// view_delta_host_test.cpp — TEST driver of gv_pool_view_delta / _device / _fetch through include/garden_vis.h alone. It pins:
//   1. the code of every row of the header's error list, and that a refused call changes nothing;
//   2. lifetimes: a channel's baseline and answer survive gv_cull, a second phase, an emission, a sort and a re-bind of the pool;
//      channels do not disturb each other; the drop call; a restart;
//   3. (stub build) every allocation of a call sequence failing once, in turn: GV_E_OOM, and the same context completes it;
//   4. ownership: a context that used every channel of two pools is destroyed, nothing is left behind;
//   5. (stub build) the write-back loop on hand-made lists: the plain column, the index-mapped target with holes, slots beyond the
//      bound occupancy skipped, sentinel bytes of unlisted slots untouched.
// Built two ways from this file, as derived_results_test.cpp: against tests/cpp/hip_stub with every host source under
// AddressSanitizer + UBSan (tests/test_view_delta_host.py; the kernels are no-ops there, so codes, lifetimes and buffer sizes are
// checked and the lists are written by hand into the stub's "device" memory), and against libgarden_vis.so for the device
// (tests/cpp/view_delta_host.mk), where the answers' invariants are checked too. Every step prints a line ending in "ok"; the last
// line is "view delta: ok".
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/garden_vis.h"
#ifdef GV_HIP_STUB
#include <hip/hip_runtime.h>  // tests/cpp/hip_stub: the fault-injection counters
#include "gv_delta_kernels.hpp"
namespace gv {  // the four launches as no-ops (the generated stubs cover the headers make_kernel_stubs.py lists)
hipError_t launch_delta_mark_records(const uint32_t*, const uint32_t*, uint32_t, uint32_t, unsigned long long*, hipStream_t) { return hipSuccess; }
hipError_t launch_delta_mark_bytes(const uint8_t*, uint32_t, const uint32_t*, uint32_t, unsigned long long*, hipStream_t) { return hipSuccess; }
hipError_t launch_delta_count(const DeltaSets&, hipStream_t) { return hipSuccess; }
hipError_t launch_delta_place(const DeltaSets&, hipStream_t) { return hipSuccess; }
}  // namespace gv
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
[[noreturn]] static void die(const char* file, int line, const char* what, long got, long want, GvCtx* ctx)
{
    std::fprintf(stderr, "%s:%d: [%s] %s -> %ld, expected %ld (%s)\n", file, line, g_where, what, got, want, ctx ? gv_last_error(ctx) : "");
    std::exit(1);
}
#define EXPECT(call, code)                                                \
    do {                                                                  \
        const long rc__ = (long)(call);                                   \
        if (rc__ != (long)(code))                                         \
            die(__FILE__, __LINE__, #call, rc__, (long)(code), ctx);      \
    } while (0)
#define CHECK(call) EXPECT(call, GV_OK)
#define TRY(call)                   \
    do {                            \
        const int rc__ = (call);    \
        if (rc__ != GV_OK)          \
            return rc__;            \
    } while (0)

// a sheet of 64 boxes in front of a camera that looks down -z; a second pool of 8; a pool bound with occupancy 0
constexpr uint32_t kSlots = 64, kFew = 8;
constexpr uint32_t kMain = 0, kSecond = 1, kEmpty = 2, kUnbound = 5;
// the views of cull_all: 0 main emitted, 1 shadow emitted, 2 main count-only, 3 shadow count-only
constexpr uint32_t kCountOnlyMain = 2, kCountOnlyShadow = 3, kNever = 6;

struct Fixture {
    GvCtx* ctx = nullptr;
    std::vector<Transform> xf;
    std::vector<uint32_t> e2t;
    std::vector<Mesh> main, second, empty;
    Fixture()
    {
        const uint32_t n = kSlots + kFew;
        xf.assign(n, Transform{});
        e2t.assign(n + 1, GV_NONE);
        for (uint32_t i = 0; i < n; i++) {
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
        for (uint32_t i = 0; i < kFew; i++)
            second.push_back(mesh_of(kSlots + i + 1));
        empty.push_back(mesh_of(1));  // (storage for a pool bound with occupancy 0)
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

// zoom 1: the whole sheet lies inside the frustum; a larger zoom narrows it to the middle of the sheet
static GvView make_view(int8_t shadow_pass, uint8_t emit, float zoom = 1.0f)
{
    GvView v{};
    v.view_proj[0] = zoom * 9.0f / 16.0f;  // infinite reversed-Z perspective, camera looking down -z
    v.view_proj[5] = zoom;
    v.view_proj[11] = -1.0f;
    v.view_proj[14] = 0.01f;
    v.shadow_pass = shadow_pass;
    v.emit_records = emit;
    return v;
}

static const GvMeshLayout kMeshLayout = {(uint32_t)offsetof(Mesh, entity), (uint32_t)offsetof(Mesh, isEnabled), (uint32_t)offsetof(Mesh, isVisible),
                                         (uint32_t)offsetof(Mesh, aabbMin), (uint32_t)offsetof(Mesh, aabbMax)};

static int bind_pools(Fixture& f, uint32_t main_slots = kSlots)
{
    GvCtx* ctx = f.ctx;
    const GvTransformLayout tl = {(uint32_t)offsetof(Transform, entity), (uint32_t)offsetof(Transform, parent), (uint32_t)offsetof(Transform, position),
                                  (uint32_t)offsetof(Transform, scale), (uint32_t)offsetof(Transform, rotation), (uint32_t)offsetof(Transform, selfActive),
                                  (uint32_t)offsetof(Transform, ancestorsActive), (uint32_t)offsetof(Transform, modelWithAncestors)};
    TRY(gv_transform_bind(ctx, f.xf.data(), sizeof(Transform), (uint32_t)f.xf.size(), &tl, f.e2t.data(), (uint32_t)f.e2t.size()));
    TRY(gv_pool_bind(ctx, kMain, f.main.data(), sizeof(Mesh), main_slots, &kMeshLayout));
    TRY(gv_pool_bind(ctx, kSecond, f.second.data(), sizeof(Mesh), kFew, &kMeshLayout));
    TRY(gv_pool_bind(ctx, kEmpty, f.empty.data(), sizeof(Mesh), 0, &kMeshLayout));
    return GV_OK;
}

static int cull_all(Fixture& f, float zoom = 1.0f)
{
    const GvView views[4] = {make_view(-1, 1, zoom), make_view(0, 1, zoom), make_view(-1, 0, zoom), make_view(1, 0, zoom)};
    TRY(gv_cull(f.ctx, kMain, views, 4));
    TRY(gv_cull(f.ctx, kSecond, views, 4));
    return GV_OK;
}

static const uint32_t kView0[1] = {0}, kView1[1] = {1}, kViews01[2] = {0, 1}, kViewBytes[1] = {kCountOnlyMain};
static const GvInstanceLayout kInstanceLayout = {128, 0, 64, 112, 116};

// ascending, inside the universe, the two lists disjoint: what every answer satisfies whatever the sets are
static void check_answer(GvCtx* ctx, const GvViewDelta& d)
{
    const uint32_t* lists[2] = {d.appeared, d.vanished};
    const uint32_t counts[2] = {d.appeared_count, d.vanished_count};
    std::vector<uint8_t> seen(d.slots, 0);
    for (int l = 0; l < 2; l++)
        for (uint32_t k = 0; k < counts[l]; k++) {
            const uint32_t s = lists[l][k];
            if (s >= d.slots || seen[s] || (k && lists[l][k - 1] >= s))
                die(__FILE__, __LINE__, "an answer's slot (out of range, listed twice or out of order)", (long)s, (long)k, ctx);
            seen[s] = 1;
        }
    if (d.visible_count > d.slots || d.appeared_count > d.visible_count)
        die(__FILE__, __LINE__, "an answer's counts", (long)d.visible_count, (long)d.slots, ctx);
}

static GvViewDelta delta_of(GvCtx* ctx, uint32_t pool, uint32_t channel, const uint32_t* views, uint32_t count, uint32_t flags = 0)
{
    GvViewDelta d{};
    CHECK(gv_pool_view_delta(ctx, pool, channel, views, count, flags));
    CHECK(gv_pool_view_delta_fetch(ctx, pool, channel, 0, &d));
    check_answer(ctx, d);
    return d;
}

#ifdef GV_HIP_STUB
constexpr bool kDevice = false;
#else
constexpr bool kDevice = true;
#endif

// ---- 1. the error list ---------------------------------------------------------------------------------------------------------
static void error_list()
{
    g_where = "error list";
    uint32_t rows = 0;
    const void *a = nullptr, *b = nullptr;
    GvViewDelta d{};
    {
        GvCtx* ctx = nullptr;
        EXPECT(gv_pool_view_delta(nullptr, kMain, 0, kView0, 1, 0), GV_E_ARG);
        EXPECT(gv_pool_view_delta_device(nullptr, kMain, 0, &a, &b), GV_E_ARG);
        EXPECT(gv_pool_view_delta_fetch(nullptr, kMain, 0, 0, &d), GV_E_ARG);
        rows += 3;
    }
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(cull_all(f));
    // GV_E_ARG
    EXPECT(gv_pool_view_delta(ctx, kUnbound, 0, kView0, 1, 0), GV_E_ARG);
    EXPECT(gv_pool_view_delta(ctx, GV_MAX_POOLS, 0, kView0, 1, 0), GV_E_ARG);
    EXPECT(gv_pool_view_delta(ctx, kMain, GV_MAX_DELTA_CHANNELS, kView0, 1, 0), GV_E_ARG);
    EXPECT(gv_pool_view_delta(ctx, kMain, GV_MAX_DELTA_CHANNELS, nullptr, 0, 0), GV_E_ARG);
    const uint32_t nine[GV_MAX_VIEWS + 1] = {0, 1, 2, 3, 4, 5, 6, 7, 0};
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, nine, GV_MAX_VIEWS + 1, 0), GV_E_ARG);
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, nullptr, 1, 0), GV_E_ARG);
    const uint32_t beyond[1] = {GV_MAX_VIEWS}, twice[3] = {0, 1, 0}, never[2] = {0, kNever};
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, beyond, 1, 0), GV_E_ARG);
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, twice, 3, 0), GV_E_ARG);
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, never, 2, 0), GV_E_ARG);
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, kView0, 1, 2), GV_E_ARG);
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, kView0, 1, GV_DELTA_RESTART | 0x80000000u), GV_E_ARG);
    EXPECT(gv_pool_view_delta_device(ctx, kMain, 0, nullptr, &b), GV_E_ARG);
    EXPECT(gv_pool_view_delta_device(ctx, kMain, 0, &a, nullptr), GV_E_ARG);
    EXPECT(gv_pool_view_delta_device(ctx, GV_MAX_POOLS, 0, &a, &b), GV_E_ARG);
    EXPECT(gv_pool_view_delta_device(ctx, kMain, GV_MAX_DELTA_CHANNELS, &a, &b), GV_E_ARG);
    EXPECT(gv_pool_view_delta_fetch(ctx, kMain, 0, 0, nullptr), GV_E_ARG);
    EXPECT(gv_pool_view_delta_fetch(ctx, GV_MAX_POOLS, 0, 0, &d), GV_E_ARG);
    EXPECT(gv_pool_view_delta_fetch(ctx, kMain, GV_MAX_DELTA_CHANNELS, 0, &d), GV_E_ARG);
    rows += 18;
    // GV_E_STATE: no result yet (every refused call above left none), a count-only shadow view
    EXPECT(gv_pool_view_delta_device(ctx, kMain, 0, &a, &b), GV_E_STATE);
    EXPECT(gv_pool_view_delta_fetch(ctx, kMain, 0, 0, &d), GV_E_STATE);
    EXPECT(gv_pool_view_delta_device(ctx, kUnbound, 0, &a, &b), GV_E_STATE);
    const uint32_t shadow[2] = {0, kCountOnlyShadow};
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, shadow, 2, 0), GV_E_STATE);
    EXPECT(gv_pool_view_delta_device(ctx, kMain, 0, &a, &b), GV_E_STATE);
    rows += 5;
    // GV_OK: emitted views, the count-only main view (the empty pool: channels())
    const GvViewDelta first = delta_of(ctx, kMain, 0, kViews01, 2);
    delta_of(ctx, kMain, 1, kViewBytes, 1);
    rows += 2;
    // a refused call changes nothing: the answer of channel 0 is still read, and (device) the next call still differs from ITS set
    CHECK(gv_pool_view_delta_device(ctx, kMain, 0, &a, &b));
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, shadow, 2, 0), GV_E_STATE);
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, twice, 3, 0), GV_E_ARG);
    const void *a2 = nullptr, *b2 = nullptr;
    CHECK(gv_pool_view_delta_device(ctx, kMain, 0, &a2, &b2));
    if (a2 != a || b2 != b)
        die(__FILE__, __LINE__, "a refused call replaced the answer", 1, 0, ctx);
    const GvViewDelta again = delta_of(ctx, kMain, 0, kViews01, 2);
    if (again.appeared_count || again.vanished_count || again.visible_count != first.visible_count)
        die(__FILE__, __LINE__, "the call behind a refused one does not answer two empty lists", again.appeared_count, again.vanished_count, ctx);
    if (kDevice && (first.visible_count == 0 || first.appeared_count != first.visible_count || first.vanished_count != 0 || first.slots != kSlots))
        die(__FILE__, __LINE__, "a channel's first call", first.appeared_count, first.visible_count, ctx);
    rows += 3;
    // a later, narrower cull: view 1 has had results and has none now
    const GvView one = make_view(-1, 1);
    CHECK(gv_cull(ctx, kMain, &one, 1));
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, kView1, 1, 0), GV_E_STATE);
    EXPECT(gv_pool_view_delta(ctx, kMain, 0, kViews01, 2, 0), GV_E_STATE);
    rows += 2;
    // write_back without a target: a pool bound by columns without an isVisible array
    {
        Fixture g;
        GvCtx* ctx = g.ctx;
        CHECK(bind_pools(g));
        GvMeshColumns cols{};
        cols.entity = {&g.main[0].entity, sizeof(Mesh)};
        cols.is_enabled = {&g.main[0].isEnabled, sizeof(Mesh)};
        cols.aabb_min = {g.main[0].aabbMin, sizeof(Mesh)};
        cols.aabb_max = {g.main[0].aabbMax, sizeof(Mesh)};
        CHECK(gv_pool_bind_columns(ctx, kMain, &cols, kSlots));
        CHECK(cull_all(g));
        CHECK(gv_pool_view_delta(ctx, kMain, 0, kView0, 1, 0));
        EXPECT(gv_pool_view_delta_fetch(ctx, kMain, 0, 1, &d), GV_E_STATE);
        CHECK(gv_pool_view_delta_fetch(ctx, kMain, 0, 0, &d));
        rows += 1;
    }
    std::printf("error list: %u rows as pinned, a refused call changes nothing: ok\n", rows);
}

// ---- 2. lifetimes ----------------------------------------------------------------------------------------------------------------
static void lifetimes()
{
    g_where = "lifetimes";
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(gv_pool_set_instance_layout(ctx, kMain, &kInstanceLayout));
    CHECK(cull_all(f));
    const GvViewDelta wide = delta_of(ctx, kMain, 0, kView0, 1);
    const uint32_t wide_count = wide.visible_count;
    struct Event {
        const char* name;
        int (*apply)(Fixture&);
    };
    static const GvView kSecondView = make_view(-1, 1);
    const Event events[] = {
        {"gv_cull", [](Fixture& g) { return cull_all(g); }},
        {"gv_pool_cull_second_phase", [](Fixture& g) { return gv_pool_cull_second_phase(g.ctx, kMain, 0, 4, &kSecondView); }},
        {"gv_pool_emit_instances", [](Fixture& g) { return gv_pool_emit_instances(g.ctx, kMain, kView0, 1, nullptr, 0); }},
        {"gv_pool_sort", [](Fixture& g) { return gv_pool_sort(g.ctx, kMain, 0, 1); }},
        {"gv_cull of another pool", [](Fixture& g) { const GvView v = make_view(-1, 1); return gv_cull(g.ctx, kSecond, &v, 1); }},
        {"a re-bind with the same occupancy", [](Fixture& g) { return bind_pools(g); }},
    };
    uint32_t survived = 0;
    for (const Event& e : events) {
        g_where = e.name;
        const void *a = nullptr, *b = nullptr, *a2 = nullptr, *b2 = nullptr;
        CHECK(gv_pool_view_delta_device(ctx, kMain, 0, &a, &b));
        CHECK(e.apply(f));
        CHECK(gv_pool_view_delta_device(ctx, kMain, 0, &a2, &b2));  // the answer is still read ...
        GvViewDelta d{};
        CHECK(gv_pool_view_delta_fetch(ctx, kMain, 0, 0, &d));
        if (a2 != a || b2 != b)
            die(__FILE__, __LINE__, "the event replaced the answer", 1, 0, ctx);
        CHECK(cull_all(f));  // ... and the baseline is still the set of the last call: the same view again answers two empty lists
        const GvViewDelta same = delta_of(ctx, kMain, 0, kView0, 1);
        if (same.appeared_count || same.vanished_count || same.visible_count != wide_count)
            die(__FILE__, __LINE__, "the baseline did not survive the event", same.appeared_count, same.vanished_count, ctx);
        survived++;
    }
    g_where = "narrowed view";
    CHECK(cull_all(f, 16.0f));  // the middle of the sheet only: slots leave, none comes
    const GvViewDelta narrow = delta_of(ctx, kMain, 0, kView0, 1);
    if (narrow.appeared_count || narrow.visible_count + narrow.vanished_count != wide_count)
        die(__FILE__, __LINE__, "a narrowed view: |C| + vanished", narrow.visible_count + narrow.vanished_count, wide_count, ctx);
    if (kDevice && (narrow.vanished_count == 0 || narrow.visible_count == 0))
        die(__FILE__, __LINE__, "the narrowed view should keep some slots and lose some", narrow.visible_count, narrow.vanished_count, ctx);
    g_where = "restart";
    const GvViewDelta restart = delta_of(ctx, kMain, 0, kView0, 1, GV_DELTA_RESTART);
    if (restart.vanished_count || restart.appeared_count != restart.visible_count || restart.visible_count != narrow.visible_count)
        die(__FILE__, __LINE__, "a restart reports all of C", restart.appeared_count, narrow.visible_count, ctx);
    // a re-bind with fewer slots, then a cull: the universe is still the baseline's; what lay beyond the new occupancy has vanished
    g_where = "re-bind with fewer slots";
    CHECK(cull_all(f));
    delta_of(ctx, kMain, 0, kView0, 1);
    CHECK(bind_pools(f, kSlots / 2));
    const void *a = nullptr, *b = nullptr;
    CHECK(gv_pool_view_delta_device(ctx, kMain, 0, &a, &b));
    CHECK(cull_all(f));
    const GvViewDelta shrunk = delta_of(ctx, kMain, 0, kView0, 1);
    if (kDevice && (shrunk.slots != kSlots || shrunk.appeared_count || shrunk.vanished_count + shrunk.visible_count != wide_count))
        die(__FILE__, __LINE__, "a shrunken pool: universe and counts", shrunk.slots, shrunk.vanished_count, ctx);
    for (uint32_t k = 0; k < shrunk.vanished_count; k++)
        if (shrunk.vanished[k] < kSlots / 2)
            die(__FILE__, __LINE__, "a slot inside the new occupancy vanished", shrunk.vanished[k], kSlots / 2, ctx);
    const GvViewDelta after = delta_of(ctx, kMain, 0, kView0, 1);
    if (kDevice && (after.slots != kSlots / 2 || after.appeared_count || after.vanished_count))
        die(__FILE__, __LINE__, "the call behind the shrunken one", after.slots, after.vanished_count, ctx);
    CHECK(bind_pools(f));
    CHECK(cull_all(f));
    const GvViewDelta grown = delta_of(ctx, kMain, 0, kView0, 1);
    if (kDevice && (grown.slots != kSlots || grown.vanished_count || grown.visible_count != wide_count))
        die(__FILE__, __LINE__, "a grown pool: new slots can only appear", grown.slots, grown.vanished_count, ctx);
    for (uint32_t k = 0; k < grown.appeared_count; k++)
        if (grown.appeared[k] < kSlots / 2)
            die(__FILE__, __LINE__, "a slot of the old occupancy appeared", grown.appeared[k], kSlots / 2, ctx);
    std::printf("lifetimes: baseline and answer survived %u events, a narrowed view, a restart and both re-binds: ok\n", survived);
}

// ---- channels and the drop call ------------------------------------------------------------------------------------------------------
static void channels()
{
    g_where = "channels";
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(cull_all(f));
    const GvViewDelta c0 = delta_of(ctx, kMain, 0, kView0, 1);
    CHECK(cull_all(f, 16.0f));
    const GvViewDelta c1 = delta_of(ctx, kMain, 1, kViewBytes, 1);  // channel 1's first call: everything it sees appears
    if (c1.vanished_count || c1.appeared_count != c1.visible_count)
        die(__FILE__, __LINE__, "channel 1's first call", c1.appeared_count, c1.visible_count, ctx);
    const GvViewDelta c0b = delta_of(ctx, kMain, 0, kView0, 1);     // channel 0 differs from ITS baseline, the wide view
    if (c0b.appeared_count || c0b.visible_count + c0b.vanished_count != c0.visible_count || c0b.visible_count != c1.visible_count)
        die(__FILE__, __LINE__, "channel 0 behind channel 1", c0b.visible_count, c0b.vanished_count, ctx);
    const GvViewDelta other = delta_of(ctx, kSecond, 0, kView0, 1);  // another pool's channel 0 is another channel
    if (other.vanished_count || other.appeared_count != other.visible_count || other.slots != (kDevice ? kFew : 0u))
        die(__FILE__, __LINE__, "another pool's channel 0", other.appeared_count, other.slots, ctx);
    // the drop call: the result is gone, the other channel is not touched, the next call behaves as a first call
    CHECK(gv_pool_view_delta(ctx, kMain, 0, nullptr, 0, 0));
    GvViewDelta d{};
    const void *a = nullptr, *b = nullptr;
    EXPECT(gv_pool_view_delta_fetch(ctx, kMain, 0, 0, &d), GV_E_STATE);
    EXPECT(gv_pool_view_delta_device(ctx, kMain, 0, &a, &b), GV_E_STATE);
    CHECK(gv_pool_view_delta_fetch(ctx, kMain, 1, 0, &d));
    if (d.appeared_count != c1.appeared_count || d.visible_count != c1.visible_count)
        die(__FILE__, __LINE__, "channel 1 behind the drop of channel 0", d.appeared_count, c1.appeared_count, ctx);
    CHECK(gv_pool_view_delta(ctx, kMain, 0, nullptr, 0, 0));  // (dropping twice is fine)
    const GvViewDelta fresh = delta_of(ctx, kMain, 0, kView0, 1);
    if (fresh.vanished_count || fresh.appeared_count != fresh.visible_count || fresh.visible_count != c0b.visible_count)
        die(__FILE__, __LINE__, "the call behind a drop", fresh.appeared_count, fresh.visible_count, ctx);
    const GvViewDelta still = delta_of(ctx, kMain, 1, kViewBytes, 1);
    if (still.appeared_count || still.vanished_count)
        die(__FILE__, __LINE__, "channel 1 kept its baseline", still.appeared_count, still.vanished_count, ctx);
    // the empty pool: GV_OK with C empty
    const GvView one = make_view(-1, 1);
    CHECK(gv_cull(ctx, kEmpty, &one, 1));
    const GvViewDelta empty = delta_of(ctx, kEmpty, 3, kView0, 1);
    if (empty.appeared_count || empty.vanished_count || empty.visible_count || empty.slots)
        die(__FILE__, __LINE__, "the empty pool", empty.visible_count, empty.slots, ctx);
    std::printf("channels: independent of each other and of other pools, drop and empty pool: ok\n");
}

// ---- 3. to 5. --------------------------------------------------------------------------------------------------------------------
#ifdef GV_HIP_STUB
// the stub's kernels are no-ops and its "device" memory is zeroed host memory: lists written here are what the fetch delivers
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

static int delta_sequence(Fixture& f)
{
    GvCtx* ctx = f.ctx;
    const void *slots = nullptr, *counts = nullptr;
    GvViewDelta d{};
    TRY(bind_pools(f));
    TRY(cull_all(f));
    TRY(gv_pool_view_delta(ctx, kMain, 0, kViews01, 2, 0));
    TRY(gv_pool_view_delta_device(ctx, kMain, 0, &slots, &counts));
    poke(counts, {3, 2, 40, kSlots});
    poke(slots, {1, 5, 9, 2, 7});
    TRY(gv_pool_view_delta_fetch(ctx, kMain, 0, 1, &d));
#ifdef GV_HIP_STUB
    if (d.appeared_count != 3 || d.vanished_count != 2 || d.visible_count != 40 || d.slots != kSlots || d.appeared[2] != 9 || d.vanished[1] != 7)
        return kWrongValues;
#endif
    TRY(gv_pool_view_delta(ctx, kMain, 1, kViewBytes, 1, 0));
    TRY(gv_pool_view_delta_fetch(ctx, kMain, 1, 0, &d));
    TRY(gv_pool_view_delta(ctx, kMain, 0, kView0, 1, GV_DELTA_RESTART));
    TRY(gv_pool_view_delta_fetch(ctx, kMain, 0, 0, &d));
    TRY(gv_pool_view_delta(ctx, kMain, 0, nullptr, 0, 0));
    TRY(gv_pool_view_delta(ctx, kSecond, 3, kViews01, 2, 0));
    TRY(gv_pool_view_delta_fetch(ctx, kSecond, 3, 1, &d));
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
        CHECK(delta_sequence(probe));
        total = gv_stub_allocations() - before;
    }
    int failed_calls = 0;
    for (long k = 1; k <= total; k++) {
        Fixture f;
        GvCtx* ctx = f.ctx;
        gv_stub_fail_countdown() = k;
        const int rc = delta_sequence(f);
        gv_stub_fail_countdown() = 0;
        if (rc != GV_E_OOM || !*gv_last_error(ctx)) {
            std::fprintf(stderr, "allocation %ld of %ld failing: the sequence returned %d (%s), not GV_E_OOM\n", k, total, rc, gv_last_error(ctx));
            std::exit(1);
        }
        failed_calls++;
        CHECK(delta_sequence(f));  // the same context completes the sequence
    }
    std::printf("allocation failures in the view delta: %ld allocations failed in turn, %d calls returned GV_E_OOM, every context completed "
                "the sequence: ok\n", total, failed_calls);
}

// the write-back on hand-made lists
static void write_back_lists()
{
    g_where = "write-back";
    constexpr uint8_t kSentinel = 9;
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(cull_all(f));
    CHECK(gv_pool_view_delta(ctx, kMain, 0, kView0, 1, 0));
    const void *slots = nullptr, *counts = nullptr;
    CHECK(gv_pool_view_delta_device(ctx, kMain, 0, &slots, &counts));
    // appeared 1, 5, 40; vanished 2, 33, 63; the pool is then bound with 32 slots: 33, 40 and 63 have no component any more
    poke(counts, {3, 3, 30, kSlots});
    poke(slots, {1, 5, 40, 2, 33, 63});
    CHECK(bind_pools(f, kSlots / 2));
    for (Mesh& m : f.main)
        m.isVisible = kSentinel;
    GvViewDelta d{};
    CHECK(gv_pool_view_delta_fetch(ctx, kMain, 0, 1, &d));
    for (uint32_t i = 0; i < kSlots; i++) {
        const uint8_t want = (i == 1 || i == 5) ? 1 : i == 2 ? 0 : kSentinel;
        if (f.main[i].isVisible != want)
            die(__FILE__, __LINE__, "the component column: byte of slot", f.main[i].isVisible, want, ctx);
    }
    // write_back == 0 touches nothing
    for (Mesh& m : f.main)
        m.isVisible = kSentinel;
    CHECK(gv_pool_view_delta_fetch(ctx, kMain, 0, 0, &d));
    for (uint32_t i = 0; i < kSlots; i++)
        if (f.main[i].isVisible != kSentinel)
            die(__FILE__, __LINE__, "a fetch without write_back wrote slot", i, 0, ctx);
    // the index-mapped target: slot s -> world[map[s] * 2]; slot 5 is a hole, slot 2 maps beyond visible_count, the table covers 40
    // slots (so 40 and 63 are outside it)
    CHECK(bind_pools(f));
    constexpr uint32_t kWorld = 100, kStride = 2;
    std::vector<uint32_t> map(40);
    for (uint32_t s = 0; s < 40; s++)
        map[s] = 99 - 2 * s;
    map[5] = GV_NONE;
    map[2] = kWorld + 7;
    std::vector<uint8_t> world((size_t)(kWorld + 8) * kStride, kSentinel);
    CHECK(gv_pool_set_index_map(ctx, kMain, map.data(), (uint32_t)map.size()));
    CHECK(gv_pool_set_result_mapping(ctx, kMain, GV_RESULTS_MAP_VISIBLE, world.data(), kStride, kWorld));
    CHECK(gv_pool_view_delta_fetch(ctx, kMain, 0, 1, &d));
    for (size_t at = 0; at < world.size(); at++) {
        uint8_t want = kSentinel;
        if (at == (size_t)map[1] * kStride)
            want = 1;  // appeared
        if (at == (size_t)map[33] * kStride)
            want = 0;  // vanished
        if (world[at] != want)
            die(__FILE__, __LINE__, "the mapped target: byte", world[at], want, ctx);
    }
    for (uint32_t i = 0; i < kSlots; i++)
        if (f.main[i].isVisible != kSentinel)
            die(__FILE__, __LINE__, "the mapped write-back wrote the bound column at slot", i, 0, ctx);
    // an answer that claims more slots than its universe is refused, nothing is written
    poke(counts, {kSlots, 1, 30, kSlots});
    EXPECT(gv_pool_view_delta_fetch(ctx, kMain, 0, 1, &d), GV_E_HIP);
    std::printf("write-back: plain column, mapped target with holes, slots beyond the occupancy and unlisted bytes as pinned: ok\n");
}
#endif

static void ownership()
{
    g_where = "ownership";
    {
        Fixture f;
        GvCtx* ctx = f.ctx;
        CHECK(delta_sequence(f));
        for (uint32_t pool : {kMain, kSecond})
            for (uint32_t c = 0; c < GV_MAX_DELTA_CHANNELS; c++) {
                delta_of(ctx, pool, c, kViews01, 2);
                CHECK(cull_all(f, c & 1u ? 16.0f : 1.0f));
                delta_of(ctx, pool, c, kViewBytes, 1);  // (both sets of the channel and the staging have been used)
            }
    }  // gv_destroy
    std::printf("ownership: a context that used every channel of two pools was destroyed: ok\n");
}

int main()
{
    error_list();
    lifetimes();
    channels();
#ifdef GV_HIP_STUB
    allocation_failures();
    write_back_lists();
#endif
    ownership();
    std::printf("view delta: ok\n");
    return 0;
}
