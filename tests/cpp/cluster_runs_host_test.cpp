// cluster_runs_host_test.cpp — TEST driver of gv_pool_cull_cluster_runs through include/garden_vis.h alone. It pins:
//   1. the code of every row of the two error lists it shares with gv_pool_cull_clusters, one failing argument at a time;
//   2. a refused call changes nothing a later call can observe;
//   3. the lifetime line: the result ends at a cull, a second phase, an instance emission, a rebind of the clusters and a cluster cull
//      of the other form (either way round; a second-phase cluster result behind it ends with it); it does not end at
//      gv_pool_emit_draw_commands, at a sort of another pool or at gv_hiz_build;
//   4. the fetch's capacity checks, served by gv_pool_cluster_commands_fetch unchanged;
//   5. the refusals that come from the host's bound B: more than 2^32 - 1 candidates, and a library-owned target beyond 2 GiB (which
//      a caller-owned target passes).
// Built against tests/cpp/hip_stub with every host source under AddressSanitizer + UBSan (tests/test_cluster_runs_host.py). The
// kernels are no-ops there, so codes, lifetimes and buffer sizes are checked; counts are written by hand into the stub's "device"
// memory. Every step prints a line ending in "ok"; the last line is "cluster runs: ok".
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/garden_vis.h"
#ifdef GV_HIP_STUB
#include <hip/hip_runtime.h>
#include "gv_cluster_run_kernels.hpp"
#include "gv_cluster_second_kernels.hpp"
namespace gv {  // the launches as no-ops (the generated stubs cover the headers make_kernel_stubs.py lists)
hipError_t launch_cluster_count(const ClusterLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_scan_candidates(const ClusterLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_test(const ClusterLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_scan_survivors(const ClusterLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_write(const ClusterLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_run_test(const ClusterRunLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_run_heads(const ClusterRunLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_run_scan(const ClusterRunLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_cluster_run_write(const ClusterRunLaunch&, hipStream_t) { return hipSuccess; }
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
        clusters.assign(GV_MAX_GEOMETRY_CLUSTERS, GvCluster{{-0.5f, -0.5f, -0.5f}, 0, {0.5f, 0.5f, 0.5f}, 3});
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

static const GvClusterRange kRanges[3] = {{0, 8}, {8, 64}, {0, 0}};

// everything a cluster cull needs, in this order: pools, geometry, layouts, clusters, a cull of two views, an emission of both
static void stand_up(Fixture& f, uint8_t use_hiz = 0)
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
    if (use_hiz)
        CHECK(gv_hiz_build(ctx, f.depth.data(), 16, 8, GV_MEM_HOST));
    const GvView views[2] = {make_view(-1, use_hiz), make_view(0)};
    CHECK(gv_cull(ctx, kMain, views, 2));
    CHECK(gv_cull(ctx, kOther, views, 2));
    const uint32_t listed[2] = {0, 1};
    CHECK(gv_pool_emit_instances(ctx, kMain, listed, 2, nullptr, 0));
}

// what a later call can observe of the pool's cluster result
struct Observed {
    int code;
    const void *commands, *counts;
    bool operator==(const Observed& o) const { return code == o.code && commands == o.commands && counts == o.counts; }
};
static Observed observe(GvCtx* ctx, uint32_t pool = kMain)
{
    Observed o{};
    o.code = gv_pool_cluster_commands_device(ctx, pool, &o.commands, &o.counts);
    if (o.code != GV_OK)
        o.commands = o.counts = nullptr;
    return o;
}

static void cull_errors()
{
    g_where = "cull errors";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f);
    CHECK(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0));
    const Observed before = observe(ctx);
    REQUIRE(before.code == GV_OK);
    alignas(16) static uint8_t target[4096];
    const void *commands = nullptr, *command_counts = nullptr;
    EXPECT(gv_pool_cull_cluster_runs(nullptr, kMain, 0, 0, nullptr, 0), GV_E_ARG);
    EXPECT(gv_pool_cull_cluster_runs(ctx, GV_MAX_POOLS, 0, 0, nullptr, 0), GV_E_ARG);               // a pool out of range
    EXPECT(gv_pool_cull_cluster_runs(ctx, kUnbound, 0, 0, nullptr, 0), GV_E_ARG);                   // ... or not bound
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 2, 0, nullptr, 0), GV_E_ARG);                      // unknown flag bits
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, target + 4, 1024), GV_E_ARG);                // a misaligned target
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0x80000000u, target, sizeof(target)), GV_E_ARG);  // m * R beyond 32 bits
    EXPECT(gv_pool_cluster_commands_device(ctx, GV_MAX_POOLS, &commands, &command_counts), GV_E_ARG);
    EXPECT(gv_pool_cluster_commands_device(ctx, kMain, nullptr, nullptr), GV_E_ARG);
    REQUIRE(observe(ctx) == before);
    // GV_E_STATE, one missing thing at a time (the result of the call above stands where the missing thing does not end it)
    EXPECT(gv_pool_cull_cluster_runs(ctx, kOther, 0, 0, nullptr, 0), GV_E_STATE);                   // no cluster binding
    CHECK(gv_pool_set_command_layout(ctx, kMain, nullptr));
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);                    // no command layout
    REQUIRE(observe(ctx) == before);
    CHECK(gv_pool_set_command_layout(ctx, kMain, &kIndexed));
    CHECK(gv_pool_bind_geometry(ctx, kMain, nullptr, 0, 0, 0, nullptr, 0));
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);                    // no geometry bound
    REQUIRE(observe(ctx) == before);
    CHECK(gv_pool_bind_geometry(ctx, kMain, f.ids.data(), 4, 4, kSlots - 1, kTable, 3));
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);                    // an id column below a listed view's occupancy
    REQUIRE(observe(ctx) == before);
    CHECK(gv_pool_bind_geometry(ctx, kMain, f.ids.data(), 4, 4, kSlots, kTable, 3));
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0), GV_OK);
    const GvView views[2] = {make_view(-1), make_view(0)};
    CHECK(gv_cull(ctx, kMain, views, 2));
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);                    // no emission since the pool's last gv_cull
    EXPECT(gv_pool_cluster_commands_device(ctx, kMain, &commands, &command_counts), GV_E_STATE);
    uint32_t counts[4] = {};
    EXPECT(gv_pool_cluster_commands_fetch(ctx, kMain, nullptr, 0, counts, 4), GV_E_STATE);
    std::printf("cull: every row of the error lists, a refused call changes nothing: ok\n");
}

static void unbuilt_pyramid()
{
    g_where = "a pyramid that is not built";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f, 1);
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0), GV_OK);
    const Observed before = observe(ctx);
    CHECK(gv_hiz_drop(ctx, 0));
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);                    // view 0 names pyramid 0, which is gone
    REQUIRE(observe(ctx) == before);
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, GV_CLUSTERS_FRUSTUM_ONLY, 0, nullptr, 0), GV_OK);  // the flag asks for no pyramid
    std::printf("pyramid: a view that names a pyramid that is not built is refused without the frustum-only flag: ok\n");
}

static void lifetimes()
{
    g_where = "lifetimes";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f, 1);
    const GvView views[2] = {make_view(-1, 1), make_view(0)};
    const uint32_t listed[2] = {0, 1};
    auto again = [&]() {
        CHECK(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0));
        REQUIRE(observe(ctx).code == GV_OK);
    };
    again();
    // what does not end it
    CHECK(gv_pool_emit_draw_commands(ctx, kMain, 0, 0, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_OK);
    CHECK(gv_pool_sort(ctx, kOther, 0, 0));
    REQUIRE(observe(ctx).code == GV_OK);
    CHECK(gv_hiz_build(ctx, f.depth.data(), 16, 8, GV_MEM_HOST));
    REQUIRE(observe(ctx).code == GV_OK);
    const void *commands = nullptr, *command_counts = nullptr;
    CHECK(gv_pool_draw_commands_device(ctx, kMain, &commands, &command_counts));  // ... and the per-draw commands stand beside it
    REQUIRE(commands != observe(ctx).commands);
    // what ends it
    CHECK(gv_cull(ctx, kMain, views, 2));
    REQUIRE(observe(ctx).code == GV_E_STATE);
    CHECK(gv_pool_emit_instances(ctx, kMain, listed, 2, nullptr, 0));
    again();
    CHECK(gv_pool_cull_second_phase(ctx, kMain, 0, 2, &views[0]));
    REQUIRE(observe(ctx).code == GV_E_STATE);
    CHECK(gv_cull(ctx, kMain, views, 2));
    CHECK(gv_pool_emit_instances(ctx, kMain, listed, 2, nullptr, 0));
    again();
    CHECK(gv_pool_emit_instances(ctx, kMain, listed, 1, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_E_STATE);
    again();
    CHECK(gv_pool_emit_draw_instances(ctx, kMain, listed, 2, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_E_STATE);
    again();
    CHECK(gv_pool_bind_clusters(ctx, kMain, kRanges, 3, f.clusters.data(), 72));
    REQUIRE(observe(ctx).code == GV_E_STATE);
    again();
    CHECK(gv_pool_bind_clusters(ctx, kMain, nullptr, 0, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_E_STATE);
    rows++;
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);  // ... and the binding is gone
    // a cluster cull of the other form replaces it, either way round: the pool holds ONE cluster result, the last call's, and a
    // second-phase result behind the replaced one ends with it
    CHECK(gv_pool_bind_clusters(ctx, kMain, kRanges, 3, f.clusters.data(), 72));
    alignas(16) static uint8_t target[8192];
    const void *second = nullptr, *second_counts = nullptr;
    CHECK(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, target, sizeof(target)));
    REQUIRE(observe(ctx).commands == target);
    CHECK(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0));          // behind the run form as behind the plain one
    REQUIRE(gv_pool_cluster_second_commands_device(ctx, kMain, &second, &second_counts) == GV_OK);
    CHECK(gv_pool_cull_clusters(ctx, kMain, 0, 0, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_OK && observe(ctx).commands != target);
    REQUIRE(gv_pool_cluster_second_commands_device(ctx, kMain, &second, &second_counts) == GV_E_STATE);
    CHECK(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0));
    CHECK(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, target, sizeof(target)));
    REQUIRE(observe(ctx).commands == target);
    REQUIRE(gv_pool_cluster_second_commands_device(ctx, kMain, &second, &second_counts) == GV_E_STATE);
    rows += 2;
    std::printf("lifetimes: ended by a cull, a second phase, an instance emission, a rebind and a cluster cull of the other form; not by draw "
                "commands, another pool's sort or a pyramid build: ok\n");
}

static void fetch_capacity()
{
    g_where = "fetch";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f);
    CHECK(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, nullptr, 0));
    const Observed o = observe(ctx);
    REQUIRE(o.code == GV_OK);
    uint32_t* device_counts = const_cast<uint32_t*>(static_cast<const uint32_t*>(o.counts));  // (the stub's device memory is host memory)
    device_counts[0] = 3, device_counts[1] = 2, device_counts[2] = 40, device_counts[3] = 30;
    uint32_t counts[5] = {7, 7, 7, 7, 7};
    uint8_t data[5 * 20 + 1];
    std::memset(data, 0xA5, sizeof(data));
    EXPECT(gv_pool_cluster_commands_fetch(ctx, kMain, nullptr, 0, nullptr, 4), GV_E_ARG);
    EXPECT(gv_pool_cluster_commands_fetch(ctx, GV_MAX_POOLS, nullptr, 0, counts, 4), GV_E_ARG);
    EXPECT(gv_pool_cluster_commands_fetch(ctx, kMain, data, sizeof(data), counts, 3), GV_E_ARG);  // two views: four counts
    EXPECT(gv_pool_cluster_commands_fetch(ctx, kMain, data, 5 * 20 - 1, counts, 4), GV_E_ARG);    // five commands of 20 bytes
    for (uint32_t c : counts)
        REQUIRE(c == 7);
    for (uint8_t b : data)
        REQUIRE(b == 0xA5);
    EXPECT(gv_pool_cluster_commands_fetch(ctx, kMain, data, 5 * 20, counts, 4), GV_OK);
    REQUIRE(counts[0] == 3 && counts[1] == 2 && counts[2] == 40 && counts[3] == 30 && counts[4] == 7 && data[5 * 20] == 0xA5);
    EXPECT(gv_pool_cluster_commands_fetch(ctx, kMain, nullptr, 0, counts, 4), GV_OK);             // the counts alone
    std::printf("fetch: an array too small gives GV_E_ARG and nothing is written: ok\n");
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
    // 8 views x 8200 slots x 65 535 clusters = 4 299 096 000 candidates: more than 32 bits hold
    const GvClusterRange full[1] = {{0, GV_MAX_GEOMETRY_CLUSTERS}};
    CHECK(gv_pool_bind_clusters(ctx, kBig, full, 1, f.clusters.data(), GV_MAX_GEOMETRY_CLUSTERS));
    alignas(16) static uint8_t target[4096];
    EXPECT(gv_pool_cull_cluster_runs(ctx, kBig, 0, 0, nullptr, 0), GV_E_STATE);
    EXPECT(gv_pool_cull_cluster_runs(ctx, kBig, 0, 0, target, sizeof(target)), GV_E_STATE);  // (whoever owns the target)
    REQUIRE(observe(ctx, kBig).code == GV_E_STATE);
    // x 2000 clusters = 131 200 000 candidates of 20 bytes: beyond a library-owned target, fine into the caller's
    const GvClusterRange some[1] = {{0, 2000}};
    CHECK(gv_pool_bind_clusters(ctx, kBig, some, 1, f.clusters.data(), 2000));
    EXPECT(gv_pool_cull_cluster_runs(ctx, kBig, 0, 0, nullptr, 0), GV_E_STATE);
    REQUIRE(observe(ctx, kBig).code == GV_E_STATE);
    EXPECT(gv_pool_cull_cluster_runs(ctx, kBig, 0, 0, target, sizeof(target)), GV_OK);
    EXPECT(gv_pool_cull_cluster_runs(ctx, kBig, 0, 100, nullptr, 0), GV_OK);                 // ... and regions are sized by m * R
    std::printf("bounds: more than 2^32 - 1 candidates refused, a library-owned target beyond 2 GiB refused and a caller-owned one taken: ok\n");
}

int main()
{
    cull_errors();
    unbuilt_pyramid();
    lifetimes();
    fetch_capacity();
    bounds_from_the_host();
    std::printf("error list: %u rows as pinned\n", rows);
    std::printf("cluster runs: ok\n");
    return 0;
}
