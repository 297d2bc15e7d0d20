// previous_host_test.cpp — TEST driver of gv_pool_keep_models / gv_pool_forget_models / gv_pool_emit_previous / gv_pool_previous_device /
// gv_pool_previous_fetch through include/garden_vis.h alone. It pins:
//   1. the code of every row of the header's error lists, one failing argument at a time;
//   2. a failed call changes neither the history nor the result;
//   3. GV_KEEP_ADD's state: refused into an empty history and for a view whose view_proj or camera_position is not the kept one;
//   4. lifetimes: the result ends at the pool's next cull (and second phase) while the history does not; an emission, a sort and a
//      re-bind end neither; gv_pool_forget_models(count 0) empties the history;
//   5. the fetch: a capacity too small writes nothing; the items are copied field by field, the bytes between the fields stay.
// Built against tests/cpp/hip_stub with every host source under AddressSanitizer + UBSan (tests/test_previous_host.py). The kernels
// are no-ops there, so codes, lifetimes and buffer sizes are checked; the history's state is observed through what GV_KEEP_ADD
// answers, and the fetched items are written by hand into the stub's "device" memory. Every step prints a line ending in "ok"; the
// last line is "previous: ok".
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/garden_vis.h"
#ifdef GV_HIP_STUB
#include <hip/hip_runtime.h>
#include "gv_previous_kernels.hpp"
namespace gv {  // the launches as no-ops (the generated stubs cover the headers make_kernel_stubs.py lists)
hipError_t launch_previous_keep(const PreviousKeep&, hipStream_t) { return hipSuccess; }
hipError_t launch_previous_emit(const PreviousEmit&, hipStream_t) { return hipSuccess; }
hipError_t launch_previous_forget(float4*, uint32_t, uint32_t, hipStream_t) { return hipSuccess; }
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
        rows++;                                                           \
    } while (0)
#define CHECK(call)                                                       \
    do {                                                                  \
        const long rc__ = (long)(call);                                   \
        if (rc__ != (long)GV_OK)                                          \
            die(__FILE__, __LINE__, #call, rc__, (long)GV_OK, ctx);       \
    } while (0)
#define TRY(call)                   \
    do {                            \
        const int rc__ = (call);    \
        if (rc__ != GV_OK)          \
            return rc__;            \
    } while (0)

constexpr uint32_t kSlots = 64;
constexpr uint32_t kMain = 0, kEmpty = 2, kUnbound = 5;
// the views of cull_all: 0 main emitted, 1 shadow emitted, 2 main count-only, 3 shadow count-only
constexpr uint32_t kCountOnly = 2, kNever = 6;

struct Fixture {
    GvCtx* ctx = nullptr;
    std::vector<Transform> xf;
    std::vector<uint32_t> e2t;
    std::vector<Mesh> main, empty;
    Fixture()
    {
        xf.assign(kSlots, Transform{});
        e2t.assign(kSlots + 1, GV_NONE);
        for (uint32_t i = 0; i < kSlots; i++) {
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

static GvView make_view(int8_t shadow_pass, uint8_t emit, float zoom = 1.0f, float camera_x = 0.0f)
{
    GvView v{};
    v.view_proj[0] = zoom * 9.0f / 16.0f;  // infinite reversed-Z perspective, camera looking down -z
    v.view_proj[5] = zoom;
    v.view_proj[11] = -1.0f;
    v.view_proj[14] = 0.01f;
    v.camera_position[0] = camera_x;
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
    TRY(gv_pool_bind(ctx, kEmpty, f.empty.data(), sizeof(Mesh), 0, &kMeshLayout));
    return GV_OK;
}

static int cull_all(Fixture& f, float zoom = 1.0f, float camera_x = 0.0f)
{
    const GvView views[4] = {make_view(-1, 1, zoom, camera_x), make_view(0, 1, zoom, camera_x), make_view(-1, 0, zoom, camera_x),
                             make_view(1, 0, zoom, camera_x)};
    TRY(gv_cull(f.ctx, kMain, views, 4));
    TRY(gv_cull(f.ctx, kEmpty, views, 4));
    return GV_OK;
}

static const GvPreviousLayout kWide = {128, 32, 16};
static uint32_t rows = 0;  // calls whose code was pinned

// what a later call can observe of the pool's state: is there a result (and where), does GV_KEEP_ADD of view 0 find a matching history
struct Observed {
    int device_code, add_code;
    const void *items, *counts;
    bool operator==(const Observed& o) const { return device_code == o.device_code && add_code == o.add_code && items == o.items && counts == o.counts; }
};
static Observed observe(GvCtx* ctx, uint32_t pool = kMain)
{
    Observed o{};
    o.device_code = gv_pool_previous_device(ctx, pool, &o.items, &o.counts);
    if (o.device_code != GV_OK)
        o.items = o.counts = nullptr;
    o.add_code = gv_pool_keep_models(ctx, pool, 0, GV_KEEP_ADD);  // (changes nothing a later call observes when it succeeds: the same epoch)
    return o;
}

// every refused call of the lists; `before` must still be observed behind each of them
static void refused_calls(Fixture& f, const Observed& before)
{
    GvCtx* ctx = f.ctx;
    const void *a = nullptr, *b = nullptr;
    uint32_t counts4[4] = {7, 7, 7, 7};
    alignas(16) static uint8_t room[256];
    auto unchanged = [&](int line) {
        if (!(observe(ctx) == before))
            die(__FILE__, line, "a refused call changed the history or the result", 1, 0, ctx);
    };
#define REFUSED(call, code) do { EXPECT(call, code); unchanged(__LINE__); } while (0)
    // gv_pool_keep_models
    REFUSED(gv_pool_keep_models(ctx, kUnbound, 0, 0), GV_E_ARG);
    REFUSED(gv_pool_keep_models(ctx, GV_MAX_POOLS, 0, 0), GV_E_ARG);
    REFUSED(gv_pool_keep_models(ctx, kMain, GV_MAX_VIEWS, 0), GV_E_ARG);
    REFUSED(gv_pool_keep_models(ctx, kMain, kNever, 0), GV_E_ARG);
    REFUSED(gv_pool_keep_models(ctx, kMain, 0, 2), GV_E_ARG);
    REFUSED(gv_pool_keep_models(ctx, kMain, 0, GV_KEEP_ADD | 0x80000000u), GV_E_ARG);
    REFUSED(gv_pool_keep_models(ctx, kMain, kCountOnly, 0), GV_E_STATE);
    // gv_pool_forget_models
    REFUSED(gv_pool_forget_models(ctx, kUnbound, 0, 4), GV_E_ARG);
    REFUSED(gv_pool_forget_models(ctx, GV_MAX_POOLS, 0, 0), GV_E_ARG);
    // gv_pool_emit_previous
    REFUSED(gv_pool_emit_previous(ctx, kUnbound, 0, nullptr, nullptr, 0, nullptr, 0), GV_E_ARG);
    REFUSED(gv_pool_emit_previous(ctx, kMain, GV_MAX_VIEWS, nullptr, nullptr, 0, nullptr, 0), GV_E_ARG);
    REFUSED(gv_pool_emit_previous(ctx, kMain, kNever, nullptr, nullptr, 0, nullptr, 0), GV_E_ARG);
    REFUSED(gv_pool_emit_previous(ctx, kMain, 0, nullptr, nullptr, 2, nullptr, 0), GV_E_ARG);
    const GvPreviousLayout bad[] = {
        {48, 0, GV_NONE},    // a stride below 64
        {272, 0, GV_NONE},   // ... above 256
        {72, 0, GV_NONE},    // ... no multiple of 16
        {128, 8, GV_NONE},   // prev_mvp misaligned
        {64, 16, GV_NONE},   // ... leaving the stride
        {128, 0, 66},        // has_history misaligned
        {128, 0, 32},        // ... inside prev_mvp
        {128, 64, 124},      // ... inside prev_mvp, at its last word
        {128, 0, 128},       // ... leaving the stride
    };
    for (const GvPreviousLayout& L : bad)
        REFUSED(gv_pool_emit_previous(ctx, kMain, 0, &L, nullptr, 0, nullptr, 0), GV_E_ARG);
    REFUSED(gv_pool_emit_previous(ctx, kMain, 0, nullptr, nullptr, 0, room + 4, sizeof(room) - 4), GV_E_ARG);
    REFUSED(gv_pool_emit_previous(ctx, kMain, kCountOnly, nullptr, nullptr, 0, nullptr, 0), GV_E_STATE);
    // the readers
    REFUSED(gv_pool_previous_device(ctx, kUnbound, &a, &b), GV_E_ARG);
    REFUSED(gv_pool_previous_device(ctx, kMain, nullptr, &b), GV_E_ARG);
    REFUSED(gv_pool_previous_device(ctx, kMain, &a, nullptr), GV_E_ARG);
    REFUSED(gv_pool_previous_fetch(ctx, kUnbound, nullptr, 0, counts4), GV_E_ARG);
    REFUSED(gv_pool_previous_fetch(ctx, kMain, nullptr, 0, nullptr), GV_E_ARG);
#undef REFUSED
    for (uint32_t c : counts4)
        if (c != 7)
            die(__FILE__, __LINE__, "a refused fetch wrote counts", (long)c, 7, ctx);
}

// ---- 1 + 2. the error lists, on an empty and on a full state ----------------------------------------------------------------------
static void error_list()
{
    g_where = "error list";
    const void *a = nullptr, *b = nullptr;
    uint32_t counts4[4] = {};
    {
        GvCtx* ctx = nullptr;
        EXPECT(gv_pool_keep_models(nullptr, kMain, 0, 0), GV_E_ARG);
        EXPECT(gv_pool_forget_models(nullptr, kMain, 0, 0), GV_E_ARG);
        EXPECT(gv_pool_emit_previous(nullptr, kMain, 0, nullptr, nullptr, 0, nullptr, 0), GV_E_ARG);
        EXPECT(gv_pool_previous_device(nullptr, kMain, &a, &b), GV_E_ARG);
        EXPECT(gv_pool_previous_fetch(nullptr, kMain, nullptr, 0, counts4), GV_E_ARG);
    }
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    // a bound pool no cull has ever touched: no view index names a view of it
    EXPECT(gv_pool_keep_models(ctx, kMain, 0, 0), GV_E_ARG);
    EXPECT(gv_pool_emit_previous(ctx, kMain, 0, nullptr, nullptr, 0, nullptr, 0), GV_E_ARG);
    CHECK(cull_all(f));
    // the empty state: no history (GV_KEEP_ADD is refused), no result
    const Observed empty = observe(ctx);
    if (empty.device_code != GV_E_STATE || empty.add_code != GV_E_STATE)
        die(__FILE__, __LINE__, "the state before the first call", empty.device_code, empty.add_code, ctx);
    EXPECT(gv_pool_previous_fetch(ctx, kMain, nullptr, 0, counts4), GV_E_STATE);
    refused_calls(f, empty);
    // the full state: an emission and a kept view
    CHECK(gv_pool_emit_previous(ctx, kMain, 0, &kWide, nullptr, 0, nullptr, 0));
    CHECK(gv_pool_keep_models(ctx, kMain, 0, 0));
    const Observed full = observe(ctx);
    if (full.device_code != GV_OK || full.add_code != GV_OK || !full.items || !full.counts)
        die(__FILE__, __LINE__, "the state behind an emission and a keep", full.device_code, full.add_code, ctx);
    refused_calls(f, full);
    // a later, narrower cull: view 1 has had results and has none now
    const GvView one = make_view(-1, 1);
    CHECK(gv_cull(ctx, kMain, &one, 1));
    EXPECT(gv_pool_keep_models(ctx, kMain, 1, 0), GV_E_STATE);
    EXPECT(gv_pool_emit_previous(ctx, kMain, 1, nullptr, nullptr, 0, nullptr, 0), GV_E_STATE);
    // an empty pool: GV_OK whatever is asked of it
    CHECK(gv_pool_emit_previous(ctx, kEmpty, 0, nullptr, nullptr, 0, nullptr, 0));
    CHECK(gv_pool_keep_models(ctx, kEmpty, 0, 0));
    CHECK(gv_pool_keep_models(ctx, kEmpty, 0, GV_KEEP_ADD));
    CHECK(gv_pool_forget_models(ctx, kEmpty, 0, 10));
    CHECK(gv_pool_previous_fetch(ctx, kEmpty, nullptr, 0, counts4));
    if (counts4[0] || counts4[1] || counts4[2])
        die(__FILE__, __LINE__, "the counts of an empty pool", (long)counts4[0], 0, ctx);
    std::printf("error list: %u rows as pinned, a refused call changes neither history nor result: ok\n", rows);
}

// ---- 3. GV_KEEP_ADD ----------------------------------------------------------------------------------------------------------------
static void keep_add()
{
    g_where = "keep add";
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(cull_all(f));
    EXPECT(gv_pool_keep_models(ctx, kMain, 0, GV_KEEP_ADD), GV_E_STATE);  // e == 0
    CHECK(gv_pool_keep_models(ctx, kMain, 0, 0));
    CHECK(gv_pool_keep_models(ctx, kMain, 0, GV_KEEP_ADD));
    EXPECT(gv_pool_keep_models(ctx, kMain, 1, GV_KEEP_ADD), GV_OK);        // the shadow view shares matrix and camera in this fixture
    CHECK(cull_all(f, 2.0f));                                              // another view_proj
    EXPECT(gv_pool_keep_models(ctx, kMain, 0, GV_KEEP_ADD), GV_E_STATE);
    CHECK(cull_all(f, 1.0f, 0.25f));                                       // the kept view_proj, another camera_position
    EXPECT(gv_pool_keep_models(ctx, kMain, 0, GV_KEEP_ADD), GV_E_STATE);
    CHECK(cull_all(f, 1.0f, -0.0f));                                       // -0 is not +0 bit for bit
    EXPECT(gv_pool_keep_models(ctx, kMain, 0, GV_KEEP_ADD), GV_E_STATE);
    CHECK(cull_all(f));
    EXPECT(gv_pool_keep_models(ctx, kMain, 0, GV_KEEP_ADD), GV_OK);        // the kept ones again, frames later
    CHECK(cull_all(f, 2.0f));
    CHECK(gv_pool_keep_models(ctx, kMain, 0, 0));                          // a plain keep takes the new view ...
    EXPECT(gv_pool_keep_models(ctx, kMain, 0, GV_KEEP_ADD), GV_OK);
    CHECK(cull_all(f));
    EXPECT(gv_pool_keep_models(ctx, kMain, 0, GV_KEEP_ADD), GV_E_STATE);  // ... and the old one no longer matches
    std::printf("keep add: refused into an empty history and for another matrix or camera, bit for bit: ok\n");
}

// ---- 4. lifetimes ----------------------------------------------------------------------------------------------------------------
static void lifetimes()
{
    g_where = "lifetimes";
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    const GvInstanceLayout instance_layout = {128, 0, 64, 112, 116};
    CHECK(gv_pool_set_instance_layout(ctx, kMain, &instance_layout));
    CHECK(cull_all(f));
    CHECK(gv_pool_emit_previous(ctx, kMain, 0, nullptr, nullptr, 0, nullptr, 0));
    CHECK(gv_pool_keep_models(ctx, kMain, 0, 0));
    const Observed full = observe(ctx);
    // neither ends: an instance emission, a sort, a forgotten range, a re-bind with the same and with a smaller occupancy
    const uint32_t view0[1] = {0};
    CHECK(gv_pool_emit_instances(ctx, kMain, view0, 1, nullptr, 0));
    CHECK(gv_pool_sort(ctx, kMain, 0, 0));
    CHECK(gv_pool_forget_models(ctx, kMain, 8, 8));
    CHECK(gv_pool_forget_models(ctx, kMain, kSlots - 1, 1000));
    CHECK(gv_pool_forget_models(ctx, kMain, kSlots, 0xFFFFFFFFu));
    if (!(observe(ctx) == full))
        die(__FILE__, __LINE__, "an emission, a sort or a forgotten range ended the result or the history", 1, 0, ctx);
    CHECK(gv_pool_bind(ctx, kMain, f.main.data(), sizeof(Mesh), kSlots / 2, &kMeshLayout));
    // the result ends at the next cull; the history does not, nor did it at the re-bind with a smaller occupancy
    CHECK(cull_all(f));
    Observed now = observe(ctx);
    if (now.device_code != GV_E_STATE || now.add_code != GV_OK)
        die(__FILE__, __LINE__, "behind a cull: the result must have ended, the history not", now.device_code, now.add_code, ctx);
    uint32_t counts4[4] = {};
    EXPECT(gv_pool_previous_fetch(ctx, kMain, nullptr, 0, counts4), GV_E_STATE);
    // ... and at a second phase
    CHECK(gv_pool_emit_previous(ctx, kMain, 0, nullptr, nullptr, 0, nullptr, 0));
    const float depth[16] = {};
    CHECK(gv_hiz_build(ctx, depth, 4, 4, GV_MEM_HOST));
    GvView second = make_view(-1, 1);
    second.use_hiz = 1;
    CHECK(gv_pool_cull_second_phase(ctx, kMain, 0, 1, &second));
    now = observe(ctx);
    if (now.device_code != GV_E_STATE || now.add_code != GV_OK)
        die(__FILE__, __LINE__, "behind a second phase: the result must have ended, the history not", now.device_code, now.add_code, ctx);
    CHECK(gv_pool_keep_models(ctx, kMain, 1, GV_KEEP_ADD));  // the second view joins the epoch: the same matrix and camera
    // a cut and an explicit matrix are accepted whatever the history holds
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(gv_pool_emit_previous(ctx, kMain, 0, &kWide, identity, GV_PREVIOUS_CUT, nullptr, 0));
    CHECK(gv_pool_emit_previous(ctx, kMain, 1, &kWide, identity, 0, nullptr, 0));
    // the whole history forgotten: GV_KEEP_ADD finds none; the result stays
    CHECK(gv_pool_forget_models(ctx, kMain, 0, 0));
    now = observe(ctx);
    if (now.device_code != GV_OK || now.add_code != GV_E_STATE)
        die(__FILE__, __LINE__, "behind forget(count 0): the history must be empty, the result not", now.device_code, now.add_code, ctx);
    CHECK(gv_pool_keep_models(ctx, kMain, 0, 0));  // the buffers were kept: the next keep takes them again
    std::printf("lifetimes: the result ended at a cull and at a second phase, the history at nothing but forget: ok\n");
}

// ---- 5. the fetch ------------------------------------------------------------------------------------------------------------------
static void fetch()
{
    g_where = "fetch";
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(cull_all(f));
    CHECK(gv_pool_emit_previous(ctx, kMain, 0, &kWide, nullptr, 0, nullptr, 0));
    uint32_t counts4[4] = {7, 7, 7, 7};
    CHECK(gv_pool_previous_fetch(ctx, kMain, nullptr, 0, counts4));
    if (counts4[0] || counts4[1] || counts4[2] || counts4[3])
        die(__FILE__, __LINE__, "the counts behind the memset", (long)counts4[0], 0, ctx);
#ifdef GV_HIP_STUB
    // five items written by hand into the stub's device memory: every byte of item k is k + 1, the counts {5, 2, 5, 3}
    const void *items = nullptr, *counts = nullptr;
    CHECK(gv_pool_previous_device(ctx, kMain, &items, &counts));
    const uint32_t written = 5, stride = kWide.stride;
    for (uint32_t k = 0; k < written; k++)
        std::memset((uint8_t*)items + (size_t)k * stride, (int)(k + 1), stride);
    const uint32_t device_counts[4] = {5, 2, written, 3};
    std::memcpy((void*)counts, device_counts, sizeof(device_counts));
    std::vector<uint8_t> host((size_t)written * stride, 0xEE);
    uint32_t fresh[4] = {7, 7, 7, 7};
    EXPECT(gv_pool_previous_fetch(ctx, kMain, host.data(), host.size() - 1, fresh), GV_E_ARG);  // too small: nothing is written
    for (uint8_t byte : host)
        if (byte != 0xEE)
            die(__FILE__, __LINE__, "a refused fetch wrote the caller's array", byte, 0xEE, ctx);
    if (fresh[0] != 7 || fresh[3] != 7)
        die(__FILE__, __LINE__, "a refused fetch wrote the counts", (long)fresh[0], 7, ctx);
    CHECK(gv_pool_previous_fetch(ctx, kMain, host.data(), host.size(), fresh));
    if (std::memcmp(fresh, device_counts, sizeof(fresh)) != 0)
        die(__FILE__, __LINE__, "the fetched counts", (long)fresh[2], written, ctx);
    for (uint32_t k = 0; k < written; k++)
        for (uint32_t at = 0; at < stride; at++) {
            const bool field = (at >= kWide.prev_mvp && at < kWide.prev_mvp + 64) || (at >= kWide.has_history && at < kWide.has_history + 4);
            const uint8_t want = field ? (uint8_t)(k + 1) : 0xEE;
            if (host[(size_t)k * stride + at] != want)
                die(__FILE__, __LINE__, "a fetched byte (fields copied, the bytes between them left)", host[(size_t)k * stride + at], want, ctx);
        }
    // a caller-owned target too small for all items: what the fetch delivers is clamped to what the target holds
    alignas(16) static uint8_t target[3 * 128];
    CHECK(gv_pool_emit_previous(ctx, kMain, 0, &kWide, nullptr, 0, target, sizeof(target)));
    CHECK(gv_pool_previous_device(ctx, kMain, &items, &counts));
    if (items != target)
        die(__FILE__, __LINE__, "the caller's target is the result", 1, 0, ctx);
    std::memcpy((void*)counts, device_counts, sizeof(device_counts));
    EXPECT(gv_pool_previous_fetch(ctx, kMain, host.data(), 3 * stride - 1, fresh), GV_E_ARG);
    CHECK(gv_pool_previous_fetch(ctx, kMain, host.data(), 3 * stride, fresh));
#endif
    std::printf("fetch: a capacity too small writes nothing, fields copied and the bytes between them left: ok\n");
}

int main()
{
    error_list();
    keep_add();
    lifetimes();
    fetch();
    std::printf("previous: ok\n");
    return 0;
}
