// clusters_second_host_test.cpp — TEST driver of gv_pool_cull_clusters_second_phase / gv_pool_cluster_second_commands_device /
// gv_pool_cluster_second_commands_fetch through include/garden_vis.h alone. It pins:
//   1. the code of every row of the header's two error lists, one failing argument at a time;
//   2. a refused call changes nothing a later call can observe — of the second result and of the cluster cull's (K1);
//   3. the refusal after gv_pool_bind_geometry / gv_pool_set_command_layout since K1, whose message says to cull the clusters again,
//      and that a new cluster cull lifts it;
//   4. the lifetime line: the result ends wherever K1 ends — a cull, a draw-level second phase, an instance emission, a rebind of
//      the clusters — and at a new cluster cull; it does not end at gv_pool_emit_draw_commands, a sort of another pool or gv_hiz_build;
//   5. the fetch's capacity checks: an array too small gives GV_E_ARG and nothing is written;
//   6. K1's result is still there, in other buffers, and fetchable afterwards.
// Built against tests/cpp/hip_stub with every host source under AddressSanitizer + UBSan (tests/test_clusters_second_host.py). The
// kernels are no-ops there, so codes, lifetimes and buffer sizes are checked; counts are written by hand into the stub's "device"
// memory. Every step prints a line ending in "ok"; the last line is "clusters second: ok".
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/garden_vis.h"
#ifdef GV_HIP_STUB
#include <hip/hip_runtime.h>
#include "gv_cluster_second_kernels.hpp"
namespace gv {  // the launches as no-ops (the generated stubs cover the headers make_kernel_stubs.py lists)
hipError_t launch_cluster_count(const ClusterLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_scan_candidates(const ClusterLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_test(const ClusterLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_scan_survivors(const ClusterLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_write(const ClusterLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_second_count(const ClusterSecondLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_second_scan_pending(const ClusterSecondLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_second_test(const ClusterSecondLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_second_scan_survivors(const ClusterSecondLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_second_write(const ClusterSecondLaunch&, hipStream_t) { return hipSuccess; }
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
static uint32_t rows = 0;  // calls whose code was pinned
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
#define REQUIRE(cond)                                                     \
    do {                                                                  \
        if (!(cond))                                                      \
            die(__FILE__, __LINE__, #cond, 0, 1, ctx);                    \
    } while (0)

constexpr uint32_t kSlots = 64, kBigSlots = 8200;
constexpr uint32_t kMain = 0, kOther = 1, kBig = 2, kUnbound = 5;

static const GvMeshLayout kMeshLayout = {(uint32_t)offsetof(Mesh, entity), (uint32_t)offsetof(Mesh, isEnabled), (uint32_t)offsetof(Mesh, isVisible),
                                         (uint32_t)offsetof(Mesh, aabbMin), (uint32_t)offsetof(Mesh, aabbMax)};
static const GvInstanceLayout kInstances = {64, 0, GV_NONE, GV_NONE, GV_NONE};
static const GvCommandLayout kIndexed = {20, 0, 4, 8, 16, 12, GV_NONE};
static const GvGeometry kTable[3] = {{36, 0, 0}, {60, 36, 0}, {6, 96, 4}};
static const GvClusterRange kRanges[3] = {{0, 8}, {8, 64}, {0, 0}};

struct Fixture {
    GvCtx* ctx = nullptr;
    std::vector<Transform> xf;
    std::vector<uint32_t> e2t;
    std::vector<Mesh> main, other, big;
    std::vector<uint32_t> ids;
    std::vector<GvCluster> clusters;
    std::vector<float> depth;
    Fixture()
    {
        xf.assign(kBigSlots, Transform{});
        e2t.assign(kBigSlots + 1, GV_NONE);
        for (uint32_t i = 0; i < kBigSlots; i++) {
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
        for (uint32_t i = 0; i < kBigSlots; i++)
            big.push_back(mesh_of(i + 1));
        main.assign(big.begin(), big.begin() + kSlots);
        other.assign(big.begin(), big.begin() + kSlots);
        ids.assign(kSlots, 1);
        clusters.assign(2000, GvCluster{{-0.5f, -0.5f, -0.5f}, 0, {0.5f, 0.5f, 0.5f}, 3});
        depth.assign(16 * 8, 0.0f);
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

static GvView make_view(int8_t shadow_pass, uint8_t use_hiz = 0)
{
    GvView v{};
    v.view_proj[0] = 9.0f / 16.0f;  // infinite reversed-Z perspective, camera looking down -z
    v.view_proj[5] = 1.0f;
    v.view_proj[11] = -1.0f;
    v.view_proj[14] = 0.01f;
    v.shadow_pass = shadow_pass;
    v.emit_records = 1;
    v.use_hiz = use_hiz;
    return v;
}

// everything a cluster cull needs, then the cluster cull K1 itself: view 0 names pyramid 0, view 1 none
static void stand_up(Fixture& f)
{
    GvCtx* ctx = f.ctx;
    const GvTransformLayout tl = {(uint32_t)offsetof(Transform, entity), (uint32_t)offsetof(Transform, parent), (uint32_t)offsetof(Transform, position),
                                  (uint32_t)offsetof(Transform, scale), (uint32_t)offsetof(Transform, rotation), (uint32_t)offsetof(Transform, selfActive),
                                  (uint32_t)offsetof(Transform, ancestorsActive), (uint32_t)offsetof(Transform, modelWithAncestors)};
    CHECK(gv_transform_bind(ctx, f.xf.data(), sizeof(Transform), (uint32_t)f.xf.size(), &tl, f.e2t.data(), (uint32_t)f.e2t.size()));
    CHECK(gv_pool_bind(ctx, kMain, f.main.data(), sizeof(Mesh), kSlots, &kMeshLayout));
    CHECK(gv_pool_bind(ctx, kOther, f.other.data(), sizeof(Mesh), kSlots, &kMeshLayout));
    CHECK(gv_pool_bind_geometry(ctx, kMain, f.ids.data(), 4, 4, kSlots, kTable, 3));
    CHECK(gv_pool_set_instance_layout(ctx, kMain, &kInstances));
    CHECK(gv_pool_set_command_layout(ctx, kMain, &kIndexed));
    CHECK(gv_pool_bind_clusters(ctx, kMain, kRanges, 3, f.clusters.data(), 72));
    CHECK(gv_hiz_build(ctx, f.depth.data(), 16, 8, GV_MEM_HOST));
    const GvView views[2] = {make_view(-1, 1), make_view(0)};
    CHECK(gv_cull(ctx, kMain, views, 2));
    CHECK(gv_cull(ctx, kOther, views, 2));
    const uint32_t listed[2] = {0, 1};
    CHECK(gv_pool_emit_instances(ctx, kMain, listed, 2, nullptr, 0));
    CHECK(gv_pool_cull_clusters(ctx, kMain, 0, 0, nullptr, 0));
}

// what a later call can observe of the pool's two cluster results
struct Observed {
    int code, first_code;
    const void *commands, *counts, *first_commands, *first_counts;
    bool operator==(const Observed& o) const
    {
        return code == o.code && first_code == o.first_code && commands == o.commands && counts == o.counts && first_commands == o.first_commands &&
               first_counts == o.first_counts;
    }
};
static Observed observe(GvCtx* ctx, uint32_t pool = kMain)
{
    Observed o{};
    o.code = gv_pool_cluster_second_commands_device(ctx, pool, &o.commands, &o.counts);
    if (o.code != GV_OK)
        o.commands = o.counts = nullptr;
    o.first_code = gv_pool_cluster_commands_device(ctx, pool, &o.first_commands, &o.first_counts);
    if (o.first_code != GV_OK)
        o.first_commands = o.first_counts = nullptr;
    return o;
}

static void errors()
{
    g_where = "errors";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f);
    REQUIRE(observe(ctx).code == GV_E_STATE && observe(ctx).first_code == GV_OK);  // K1 alone is no second result
    CHECK(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0));
    const Observed before = observe(ctx);
    REQUIRE(before.code == GV_OK && before.first_code == GV_OK);
    REQUIRE(before.commands != before.first_commands && before.counts != before.first_counts);  // buffers of its own
    alignas(16) static uint8_t target[4096];
    const void *commands = nullptr, *command_counts = nullptr;
    uint32_t counts[4] = {};
    // GV_E_ARG, as for gv_pool_cull_clusters
    EXPECT(gv_pool_cull_clusters_second_phase(nullptr, kMain, 0, 0, nullptr, 0), GV_E_ARG);
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, GV_MAX_POOLS, 0, 0, nullptr, 0), GV_E_ARG);             // a pool out of range
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kUnbound, 0, 0, nullptr, 0), GV_E_ARG);                 // ... or not bound
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, GV_CLUSTERS_FRUSTUM_ONLY, 0, nullptr, 0), GV_E_ARG);  // flags must be 0
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0x80000000u, 0, nullptr, 0), GV_E_ARG);
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, target + 4, 1024), GV_E_ARG);              // a misaligned target
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0x80000000u, target, sizeof(target)), GV_E_ARG);  // m * R beyond 32 bits
    EXPECT(gv_pool_cluster_second_commands_device(nullptr, kMain, &commands, &command_counts), GV_E_ARG);
    EXPECT(gv_pool_cluster_second_commands_device(ctx, GV_MAX_POOLS, &commands, &command_counts), GV_E_ARG);
    EXPECT(gv_pool_cluster_second_commands_device(ctx, kMain, nullptr, nullptr), GV_E_ARG);
    EXPECT(gv_pool_cluster_second_commands_fetch(nullptr, kMain, nullptr, 0, counts, 4), GV_E_ARG);
    REQUIRE(observe(ctx) == before);
    // GV_E_STATE, one at a time
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kOther, 0, 0, nullptr, 0), GV_E_STATE);                 // the pool holds no cluster result
    EXPECT(gv_pool_cluster_second_commands_device(ctx, kOther, &commands, &command_counts), GV_E_STATE);
    EXPECT(gv_pool_cluster_second_commands_fetch(ctx, kOther, nullptr, 0, counts, 4), GV_E_STATE);
    CHECK(gv_hiz_drop(ctx, 0));
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);                  // view 0 names pyramid 0, which is gone
    REQUIRE(observe(ctx) == before);
    CHECK(gv_hiz_build(ctx, f.depth.data(), 16, 8, GV_MEM_HOST));
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_OK);
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 7, target, sizeof(target)), GV_OK);           // regions into the caller's memory
    REQUIRE(observe(ctx).commands == target);
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_OK);
    REQUIRE(observe(ctx) == before);
    std::printf("errors: every row of the two lists, a refused call changes nothing: ok\n");
}

static void rebinds()
{
    g_where = "rebinds";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f);
    CHECK(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0));
    const Observed before = observe(ctx);
    CHECK(gv_pool_bind_geometry(ctx, kMain, f.ids.data(), 4, 4, kSlots, kTable, 2));  // a smaller table: K1 kept ids up to 2
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);
    REQUIRE(std::strstr(gv_last_error(ctx), "cull the clusters again") != nullptr);
    REQUIRE(observe(ctx) == before);  // (the results made before the rebind stand)
    CHECK(gv_pool_cull_clusters(ctx, kMain, 0, 0, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_E_STATE);  // a new K1 ends the second result ...
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_OK);  // ... and lifts the refusal
    CHECK(gv_pool_set_command_layout(ctx, kMain, &kIndexed));  // (the same layout again: still a call since K1)
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);
    REQUIRE(std::strstr(gv_last_error(ctx), "cull the clusters again") != nullptr);
    CHECK(gv_pool_cull_clusters(ctx, kMain, 0, 0, nullptr, 0));
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_OK);
    CHECK(gv_pool_bind_geometry(ctx, kOther, nullptr, 0, 0, 0, kTable, 3));  // another pool's binding is not this pool's
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_OK);
    std::printf("rebinds: refused after a geometry or layout call since the cluster cull, lifted by a new one: ok\n");
}

static void lifetimes()
{
    g_where = "lifetimes";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f);
    const GvView views[2] = {make_view(-1, 1), make_view(0)};
    const uint32_t listed[2] = {0, 1};
    auto again = [&](bool emit) {
        if (emit)
            CHECK(gv_pool_emit_instances(ctx, kMain, listed, 2, nullptr, 0));
        CHECK(gv_pool_cull_clusters(ctx, kMain, 0, 0, nullptr, 0));
        REQUIRE(observe(ctx).code == GV_E_STATE);
        CHECK(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0));
        REQUIRE(observe(ctx).code == GV_OK);
    };
    again(false);
    // what does not end it
    CHECK(gv_pool_emit_draw_commands(ctx, kMain, 0, 0, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_OK);
    CHECK(gv_pool_sort(ctx, kOther, 0, 0));
    REQUIRE(observe(ctx).code == GV_OK);
    CHECK(gv_hiz_build(ctx, f.depth.data(), 16, 8, GV_MEM_HOST));
    REQUIRE(observe(ctx).code == GV_OK);
    CHECK(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0));  // repeatable
    REQUIRE(observe(ctx).code == GV_OK);
    // what ends it: wherever K1 ends, and a new K1
    CHECK(gv_cull(ctx, kMain, views, 2));
    REQUIRE(observe(ctx).code == GV_E_STATE && observe(ctx).first_code == GV_E_STATE);
    rows++;
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);
    again(true);
    CHECK(gv_pool_cull_second_phase(ctx, kMain, 0, 2, &views[0]));
    REQUIRE(observe(ctx).code == GV_E_STATE && observe(ctx).first_code == GV_E_STATE);
    CHECK(gv_cull(ctx, kMain, views, 2));
    again(true);
    CHECK(gv_pool_emit_instances(ctx, kMain, listed, 1, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_E_STATE && observe(ctx).first_code == GV_E_STATE);
    again(true);
    CHECK(gv_pool_emit_draw_instances(ctx, kMain, listed, 2, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_E_STATE && observe(ctx).first_code == GV_E_STATE);
    again(true);
    CHECK(gv_pool_bind_clusters(ctx, kMain, kRanges, 3, f.clusters.data(), 72));
    REQUIRE(observe(ctx).code == GV_E_STATE && observe(ctx).first_code == GV_E_STATE);
    again(false);
    CHECK(gv_pool_cull_clusters(ctx, kMain, GV_CLUSTERS_FRUSTUM_ONLY, 0, nullptr, 0));  // a new K1: its own result stands, the second is gone
    REQUIRE(observe(ctx).code == GV_E_STATE && observe(ctx).first_code == GV_OK);
    CHECK(gv_hiz_drop(ctx, 0));
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_OK);  // a frustum-only K1 queried no pyramid: none is asked for
    std::printf("lifetimes: ended wherever the cluster cull ends and by a new one; not by draw commands, another pool's sort or a pyramid build: ok\n");
}

static void fetch_capacity()
{
    g_where = "fetch";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f);
    CHECK(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0));
    const Observed o = observe(ctx);
    REQUIRE(o.code == GV_OK);
    uint32_t* device_counts = const_cast<uint32_t*>(static_cast<const uint32_t*>(o.counts));  // (the stub's device memory is host memory)
    device_counts[0] = 3, device_counts[1] = 2, device_counts[2] = 40, device_counts[3] = 30;
    uint32_t* first_counts = const_cast<uint32_t*>(static_cast<const uint32_t*>(o.first_counts));
    first_counts[0] = 1, first_counts[1] = 1, first_counts[2] = 9, first_counts[3] = 8;
    uint32_t counts[5] = {7, 7, 7, 7, 7};
    uint8_t data[5 * 20 + 1];
    std::memset(data, 0xA5, sizeof(data));
    EXPECT(gv_pool_cluster_second_commands_fetch(ctx, kMain, nullptr, 0, nullptr, 4), GV_E_ARG);
    EXPECT(gv_pool_cluster_second_commands_fetch(ctx, GV_MAX_POOLS, nullptr, 0, counts, 4), GV_E_ARG);
    EXPECT(gv_pool_cluster_second_commands_fetch(ctx, kMain, data, sizeof(data), counts, 3), GV_E_ARG);  // two views: four counts
    EXPECT(gv_pool_cluster_second_commands_fetch(ctx, kMain, data, 5 * 20 - 1, counts, 4), GV_E_ARG);    // five commands of 20 bytes
    for (uint32_t c : counts)
        REQUIRE(c == 7);
    for (uint8_t b : data)
        REQUIRE(b == 0xA5);
    EXPECT(gv_pool_cluster_second_commands_fetch(ctx, kMain, data, 5 * 20, counts, 4), GV_OK);
    REQUIRE(counts[0] == 3 && counts[1] == 2 && counts[2] == 40 && counts[3] == 30 && counts[4] == 7 && data[5 * 20] == 0xA5);
    EXPECT(gv_pool_cluster_second_commands_fetch(ctx, kMain, nullptr, 0, counts, 4), GV_OK);             // the counts alone
    // K1's result is still fetchable, from its own buffers
    EXPECT(gv_pool_cluster_commands_fetch(ctx, kMain, data, 2 * 20, counts, 4), GV_OK);
    REQUIRE(counts[0] == 1 && counts[1] == 1 && counts[2] == 9 && counts[3] == 8);
    std::printf("fetch: an array too small gives GV_E_ARG and nothing is written; the cluster cull's result is still fetchable: ok\n");
}

static void bounds_from_the_host()
{
    g_where = "host bounds";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f);
    CHECK(gv_pool_bind(ctx, kBig, f.big.data(), sizeof(Mesh), kBigSlots, &kMeshLayout));
    CHECK(gv_pool_bind_geometry(ctx, kBig, nullptr, 0, 0, 0, kTable, 3));
    CHECK(gv_pool_set_instance_layout(ctx, kBig, &kInstances));
    CHECK(gv_pool_set_command_layout(ctx, kBig, &kIndexed));
    GvView views[8];
    uint32_t listed[8];
    for (uint32_t v = 0; v < 8; v++)
        views[v] = make_view(v ? (int8_t)(v - 1) : (int8_t)-1), listed[v] = v;
    CHECK(gv_cull(ctx, kBig, views, 8));
    CHECK(gv_pool_emit_instances(ctx, kBig, listed, 8, nullptr, 0));
    // 8 views x 8200 slots x 2000 clusters = 131 200 000 candidates of 20 bytes: beyond a library-owned target, fine into the caller's
    const GvClusterRange some[1] = {{0, 2000}};
    CHECK(gv_pool_bind_clusters(ctx, kBig, some, 1, f.clusters.data(), 2000));
    alignas(16) static uint8_t target[4096];
    CHECK(gv_pool_cull_clusters(ctx, kBig, 0, 0, target, sizeof(target)));
    const Observed before = observe(ctx, kBig);
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kBig, 0, 0, nullptr, 0), GV_E_STATE);
    REQUIRE(observe(ctx, kBig) == before && before.code == GV_E_STATE && before.first_code == GV_OK);
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kBig, 0, 0, target, sizeof(target)), GV_OK);
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kBig, 0, 100, nullptr, 0), GV_OK);  // ... and regions are sized by m * R
    std::printf("bounds: a library-owned target beyond 2 GiB refused, a caller-owned one and regions taken: ok\n");
}

int main()
{
    errors();
    rebinds();
    lifetimes();
    fetch_capacity();
    bounds_from_the_host();
    std::printf("error list: %u rows as pinned\n", rows);
    std::printf("clusters second: ok\n");
    return 0;
}
