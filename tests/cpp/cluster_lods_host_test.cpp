// cluster_lods_host_test.cpp — TEST driver of gv_pool_bind_cluster_lods / gv_pool_cull_cluster_lods through include/garden_vis.h
// alone. It pins:
//   1. the code of every row of gv_pool_bind_cluster_lods' error list, the upload bytes, and that a refused bind changes nothing;
//   2. the code of every row of gv_pool_cull_cluster_lods' error list — those of gv_pool_cull_clusters, the LOD views, the eyes and
//      the two bindings — one failing argument at a time under every flag combination, without and with eyes, and that the three
//      older entry points keep refusing what they refuse;
//   3. a refused call changes nothing a later call can observe;
//   4. the LOD table is dropped by gv_pool_bind_clusters (a new table, or removal);
//   5. the lifetime line: the result is the pool's cluster result — ended where one ends and by gv_pool_bind_cluster_lods, replaced
//      by a cluster cull of any form; the launch counts (five, six with runs); the test launch of the form the call takes carries the
//      caller's views (and eyes); the second phase behind it launches the LOD test with the KEPT views (and eyes), behind the older
//      forms it does not.
// Built against tests/cpp/hip_stub with every host source under AddressSanitizer + UBSan (tests/test_cluster_lods_host.py). The
// kernels are no-ops there, so codes, lifetimes and buffer sizes are checked. Every step prints a line ending in "ok"; the last line
// is "cluster lods: ok".
#include <cmath>
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
#include "gv_cluster_cone_kernels.hpp"
#include "gv_cluster_lod_kernels.hpp"
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
static uint32_t cone_launches = 0, cone_second_launches = 0;  // the older forms' launches that carry the cone test, counted
hipError_t launch_cluster_cone_test(const ClusterConeLaunch&, hipStream_t) { cone_launches++; return hipSuccess; }
hipError_t launch_cluster_cone_run_test(const ClusterConeRunLaunch&, hipStream_t) { cone_launches++; return hipSuccess; }
hipError_t launch_cluster_cone_second_test(const ClusterConeSecondLaunch&, hipStream_t) { cone_second_launches++; return hipSuccess; }
static uint32_t lod_launches = 0, lod_cone_launches = 0, lod_second_launches = 0, lod_cone_second_launches = 0;  // ... the LOD test
static ClusterLodView last_views[8];
static float last_eyes[8][4];
static const void* last_table = nullptr;
static void keep(const ClusterLodArgs& lod, const ClusterConeArgs* cone)
{
    std::memcpy(last_views, lod.views, sizeof(last_views));
    last_table = lod.lods;
    if (cone)
        std::memcpy(last_eyes, cone->eyes, sizeof(last_eyes));
}
hipError_t launch_cluster_lod_test(const ClusterLodLaunch& l, hipStream_t) { lod_launches++; keep(l.lod, nullptr); return hipSuccess; }
hipError_t launch_cluster_lod_run_test(const ClusterLodRunLaunch& l, hipStream_t) { lod_launches++; keep(l.lod, nullptr); return hipSuccess; }
hipError_t launch_cluster_lod_cone_test(const ClusterLodConeLaunch& l, hipStream_t) { lod_cone_launches++; keep(l.lod, &l.c.cone); return hipSuccess; }
hipError_t launch_cluster_lod_cone_run_test(const ClusterLodConeRunLaunch& l, hipStream_t) { lod_cone_launches++; keep(l.lod, &l.c.cone); return hipSuccess; }
hipError_t launch_cluster_lod_second_test(const ClusterLodSecondLaunch& l, hipStream_t) { lod_second_launches++; keep(l.lod, nullptr); return hipSuccess; }
hipError_t launch_cluster_lod_cone_second_test(const ClusterLodConeSecondLaunch& l, hipStream_t)
{
    lod_cone_second_launches++;
    keep(l.lod, &l.c.cone);
    return hipSuccess;
}
}  // namespace gv
using namespace gv;
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

static const GvClusterEye kEyes[2] = {{{0.0f, 0.0f, 0.0f, 1.0f}}, {{0.25f, -0.5f, 0.75f, 0.0f}}};

static uint64_t emit_launches(GvCtx* ctx)
{
    GvStats stats{};
    if (gv_stats(ctx, &stats) != GV_OK)
        std::exit(1);
    return stats.launches[GV_K_EMIT];
}
static uint64_t upload_bytes(GvCtx* ctx)
{
    GvStats stats{};
    if (gv_stats(ctx, &stats) != GV_OK)
        std::exit(1);
    return stats.upload_bytes;
}

static GvClusterLodView lod_view(float w, float scale, float near_distance)
{
    return GvClusterLodView{{0.0f, 0.0f, 0.0f, w}, scale, near_distance, {0.0f, 0.0f}};
}
static const GvClusterLodView kViews[2] = {lod_view(1.0f, 540.0f, 0.1f), lod_view(0.0f, 3.0f, 1.0f)};

static void bind_errors(std::vector<GvClusterLod>& lods)
{
    g_where = "bind errors";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f);
    EXPECT(gv_pool_bind_cluster_lods(nullptr, kMain, lods.data(), 72), GV_E_ARG);
    EXPECT(gv_pool_bind_cluster_lods(ctx, GV_MAX_POOLS, lods.data(), 72), GV_E_ARG);   // a pool out of range
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 0), GV_E_ARG);            // a pointer without a count
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, nullptr, 72), GV_E_ARG);               // a count without a pointer
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 71), GV_E_ARG);           // not the bound cluster_count
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 73), GV_E_ARG);
    EXPECT(gv_pool_bind_cluster_lods(ctx, kOther, lods.data(), 72), GV_E_STATE);        // no cluster binding
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);  // ... and none of them bound a table
    const uint64_t before = upload_bytes(ctx);
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 72), GV_OK);
    REQUIRE(upload_bytes(ctx) - before == 72u * sizeof(GvClusterLod));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_OK);
    const Observed standing = observe(ctx);
    REQUIRE(standing.code == GV_OK);
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 71), GV_E_ARG);
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, nullptr, 72), GV_E_ARG);
    REQUIRE(observe(ctx) == standing);
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_OK);
    // a bind, and a removal, end a cluster result the pool holds — of any form
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 72), GV_OK);
    REQUIRE(observe(ctx).code == GV_E_STATE);
    CHECK(gv_pool_cull_clusters(ctx, kMain, 0, 0, nullptr, 0));
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, nullptr, 0), GV_OK);
    REQUIRE(observe(ctx).code == GV_E_STATE);
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);  // the binding is gone
    EXPECT(gv_pool_cull_clusters(ctx, kMain, 0, 0, nullptr, 0), GV_OK);                                   // ... and the other forms run without one
    std::printf("bind: every row of the error list, the bytes are counted, a refused bind changes nothing, a bind ends the result: ok\n");
}

static void cull_errors(std::vector<GvClusterLod>& lods, std::vector<GvClusterCone>& cones)
{
    g_where = "cull errors";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f);
    CHECK(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 72));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, kEyes, 2, 0, nullptr, 0), GV_E_STATE);  // eyes without a cone binding
    CHECK(gv_pool_bind_cluster_cones(ctx, kMain, cones.data(), 72));
    CHECK(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0));
    const Observed before = observe(ctx);
    REQUIRE(before.code == GV_OK);
    alignas(16) static uint8_t target[4096];
    const float nan = std::nanf("");
    const GvClusterLodView negative_scale[2] = {kViews[0], lod_view(0.0f, -1.0f, 1.0f)}, nan_scale[2] = {lod_view(1.0f, nan, 1.0f), kViews[1]};
    const GvClusterLodView negative_near[2] = {lod_view(1.0f, 1.0f, -0.5f), kViews[1]}, nan_near[2] = {kViews[0], lod_view(0.0f, 1.0f, nan)};
    const GvClusterLodView zeros[2] = {lod_view(1.0f, -0.0f, 0.0f), lod_view(0.0f, 0.0f, 0.0f)};  // (+-0 is neither negative nor NaN)
    for (uint32_t flags : {0u, (uint32_t)GV_CLUSTERS_FRUSTUM_ONLY, (uint32_t)GV_CLUSTERS_RUNS, (uint32_t)(GV_CLUSTERS_FRUSTUM_ONLY | GV_CLUSTERS_RUNS)})
        for (int with_eyes = 0; with_eyes < 2; with_eyes++) {
            const GvClusterEye* eyes = with_eyes ? kEyes : nullptr;
            const uint32_t n = with_eyes ? 2u : 0u;
            EXPECT(gv_pool_cull_cluster_lods(nullptr, kMain, flags, kViews, 2, eyes, n, 0, nullptr, 0), GV_E_ARG);
            EXPECT(gv_pool_cull_cluster_lods(ctx, GV_MAX_POOLS, flags, kViews, 2, eyes, n, 0, nullptr, 0), GV_E_ARG);              // a pool out of range
            EXPECT(gv_pool_cull_cluster_lods(ctx, kUnbound, flags, kViews, 2, eyes, n, 0, nullptr, 0), GV_E_ARG);                  // ... or not bound
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags | 4u, kViews, 2, eyes, n, 0, nullptr, 0), GV_E_ARG);                // unknown flag bits
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, kViews, 2, eyes, n, 0, target + 4, 1024), GV_E_ARG);               // a misaligned target
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, kViews, 2, eyes, n, 0x80000000u, target, sizeof(target)), GV_E_ARG);  // m * R beyond 32 bits
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, nullptr, 2, eyes, n, 0, nullptr, 0), GV_E_ARG);                    // views NULL
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, kViews, 1, eyes, n, 0, nullptr, 0), GV_E_ARG);                     // not the views of E
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, kViews, 3, eyes, n, 0, nullptr, 0), GV_E_ARG);
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, kViews, 0, eyes, n, 0, nullptr, 0), GV_E_ARG);
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, negative_scale, 2, eyes, n, 0, nullptr, 0), GV_E_ARG);             // a scale below 0
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, nan_scale, 2, eyes, n, 0, nullptr, 0), GV_E_ARG);                  // ... or NaN
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, negative_near, 2, eyes, n, 0, nullptr, 0), GV_E_ARG);              // a near_distance below 0
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, nan_near, 2, eyes, n, 0, nullptr, 0), GV_E_ARG);                   // ... or NaN
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, kViews, 2, kEyes, 0, 0, nullptr, 0), GV_E_ARG);                    // eyes without a count
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, kViews, 2, nullptr, 2, 0, nullptr, 0), GV_E_ARG);                  // a count without eyes
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, kViews, 2, kEyes, 1, 0, nullptr, 0), GV_E_ARG);                    // not the views of E
            EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, flags, kViews, 2, kEyes, 3, 0, nullptr, 0), GV_E_ARG);
            REQUIRE(observe(ctx) == before);
        }
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, zeros, 2, nullptr, 0, 0, nullptr, 0), GV_OK);
    CHECK(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0));
    // the older entry points keep refusing what they refuse
    EXPECT(gv_pool_cull_clusters(ctx, kMain, GV_CLUSTERS_RUNS, 0, nullptr, 0), GV_E_ARG);
    EXPECT(gv_pool_cull_cluster_runs(ctx, kMain, GV_CLUSTERS_RUNS, 0, nullptr, 0), GV_E_ARG);
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, GV_CLUSTERS_RUNS, 0, nullptr, 0), GV_E_ARG);
    EXPECT(gv_pool_cull_cluster_cones(ctx, kMain, 4u, kEyes, 2, 0, nullptr, 0), GV_E_ARG);
    EXPECT(gv_pool_cull_cluster_cones(ctx, kMain, 0, nullptr, 0, 0, nullptr, 0), GV_E_ARG);  // (NULL eyes mean "no cone test" to the LOD call only)
    REQUIRE(observe(ctx) == before);
    // GV_E_STATE, one missing thing at a time
    EXPECT(gv_pool_cull_cluster_lods(ctx, kOther, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);                         // no cluster binding
    CHECK(gv_pool_set_command_layout(ctx, kMain, nullptr));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);                          // no command layout
    REQUIRE(observe(ctx) == before);
    CHECK(gv_pool_set_command_layout(ctx, kMain, &kIndexed));
    CHECK(gv_pool_bind_geometry(ctx, kMain, nullptr, 0, 0, 0, nullptr, 0));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);                          // no geometry bound
    REQUIRE(observe(ctx) == before);
    CHECK(gv_pool_bind_geometry(ctx, kMain, f.ids.data(), 4, 4, kSlots - 1, kTable, 3));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);                          // an id column below a view's occupancy
    REQUIRE(observe(ctx) == before);
    CHECK(gv_pool_bind_geometry(ctx, kMain, f.ids.data(), 4, 4, kSlots, kTable, 3));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, GV_CLUSTERS_RUNS | GV_CLUSTERS_FRUSTUM_ONLY, kViews, 2, kEyes, 2, 0, target, sizeof(target)), GV_OK);
    REQUIRE(observe(ctx).commands == target);
    CHECK(gv_pool_bind_cluster_cones(ctx, kMain, nullptr, 0));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, kEyes, 2, 0, nullptr, 0), GV_E_STATE);                            // eyes, and the cones are gone
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_OK);
    const GvView views[2] = {make_view(-1), make_view(0)};
    CHECK(gv_cull(ctx, kMain, views, 2));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);                          // no emission since the last gv_cull
    REQUIRE(observe(ctx).code == GV_E_STATE);
    std::printf("cull: every row of the error lists under every flag combination, a refused call changes nothing: ok\n");
}

static void unbuilt_pyramid(std::vector<GvClusterLod>& lods)
{
    g_where = "a pyramid that is not built";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f, 1);
    CHECK(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 72));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_OK);
    const Observed before = observe(ctx);
    CHECK(gv_hiz_drop(ctx, 0));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);  // view 0 names pyramid 0, which is gone
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, GV_CLUSTERS_RUNS, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);
    REQUIRE(observe(ctx) == before);
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, GV_CLUSTERS_FRUSTUM_ONLY, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_OK);  // the flag asks for no pyramid
    std::printf("pyramid: a view that names a pyramid that is not built is refused without the frustum-only flag: ok\n");
}

static void dropped_by_a_cluster_bind(std::vector<GvClusterLod>& lods)
{
    g_where = "the LOD table dropped";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f);
    CHECK(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 72));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_OK);
    CHECK(gv_pool_bind_clusters(ctx, kMain, kRanges, 3, f.clusters.data(), 72));                          // a new table, of the same size
    REQUIRE(observe(ctx).code == GV_E_STATE);
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);   // ... drops the LOD table
    EXPECT(gv_pool_cull_clusters(ctx, kMain, 0, 0, nullptr, 0), GV_OK);
    CHECK(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 72));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_OK);
    CHECK(gv_pool_bind_clusters(ctx, kMain, nullptr, 0, nullptr, 0));                                     // removal
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 72), GV_E_STATE);                           // no cluster binding
    CHECK(gv_pool_bind_clusters(ctx, kMain, kRanges, 3, f.clusters.data(), 80));
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_STATE);   // ... and the table did not come back
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 72), GV_E_ARG);                             // the table now has 80 entries
    EXPECT(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 80), GV_OK);
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_OK);
    std::printf("dropped: gv_pool_bind_clusters, a new table or removal, drops the LOD table: ok\n");
}

static void lifetimes(std::vector<GvClusterLod>& lods, std::vector<GvClusterCone>& cones)
{
    g_where = "lifetimes";
    Fixture f;
    GvCtx* ctx = f.ctx;
    stand_up(f, 1);
    CHECK(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 72));
    CHECK(gv_pool_bind_cluster_cones(ctx, kMain, cones.data(), 72));
    const GvView views[2] = {make_view(-1, 1), make_view(0)};
    const uint32_t listed[2] = {0, 1};
    auto again = [&](uint32_t flags, bool eyes) {
        const uint64_t launches = emit_launches(ctx);
        const uint32_t plain = lod_launches, with_cones = lod_cone_launches;
        std::memset(last_views, 0, sizeof(last_views));
        std::memset(last_eyes, 0, sizeof(last_eyes));
        CHECK(gv_pool_cull_cluster_lods(ctx, kMain, flags, kViews, 2, eyes ? kEyes : nullptr, eyes ? 2u : 0u, 0, nullptr, 0));
        REQUIRE(emit_launches(ctx) - launches == ((flags & GV_CLUSTERS_RUNS) ? 6u : 5u));  // ... one of them the test with the LOD cut in it
        REQUIRE(lod_launches - plain == (eyes ? 0u : 1u) && lod_cone_launches - with_cones == (eyes ? 1u : 0u));
        REQUIRE(std::memcmp(last_views, kViews, sizeof(kViews)) == 0 && last_table != nullptr);
        REQUIRE(!eyes || std::memcmp(last_eyes, kEyes, sizeof(kEyes)) == 0);
        REQUIRE(observe(ctx).code == GV_OK);
    };
    again(0, false);
    again(0, true);
    // what does not end it
    CHECK(gv_pool_emit_draw_commands(ctx, kMain, 0, 0, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_OK);
    CHECK(gv_hiz_build(ctx, f.depth.data(), 16, 8, GV_MEM_HOST));
    REQUIRE(observe(ctx).code == GV_OK);
    // what ends it: where a cluster result ends
    CHECK(gv_cull(ctx, kMain, views, 2));
    REQUIRE(observe(ctx).code == GV_E_STATE);
    CHECK(gv_pool_emit_instances(ctx, kMain, listed, 2, nullptr, 0));
    again(GV_CLUSTERS_RUNS, false);
    again(GV_CLUSTERS_RUNS | GV_CLUSTERS_FRUSTUM_ONLY, true);
    CHECK(gv_pool_emit_instances(ctx, kMain, listed, 1, nullptr, 0));
    REQUIRE(observe(ctx).code == GV_E_STATE);
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 2, nullptr, 0, 0, nullptr, 0), GV_E_ARG);   // that emission has one view
    EXPECT(gv_pool_cull_cluster_lods(ctx, kMain, 0, kViews, 1, nullptr, 0, 0, nullptr, 0), GV_OK);
    CHECK(gv_pool_emit_instances(ctx, kMain, listed, 2, nullptr, 0));
    // the second phase behind it carries the LOD test, with the views (and eyes) the cull kept (the caller's copies may be gone)
    const void *second = nullptr, *second_counts = nullptr;
    for (int with_eyes = 0; with_eyes < 2; with_eyes++) {
        {
            std::vector<GvClusterLodView> gone(kViews, kViews + 2);
            std::vector<GvClusterEye> gone_eyes(kEyes, kEyes + 2);
            CHECK(gv_pool_cull_cluster_lods(ctx, kMain, 0, gone.data(), 2, with_eyes ? gone_eyes.data() : nullptr, with_eyes ? 2u : 0u, 0, nullptr, 0));
            gone.assign(2, lod_view(9.0f, 9.0f, 9.0f));
            gone_eyes.assign(2, GvClusterEye{{9.0f, 9.0f, 9.0f, 9.0f}});
        }
        std::memset(last_views, 0, sizeof(last_views));
        std::memset(last_eyes, 0, sizeof(last_eyes));
        const uint32_t plain = lod_second_launches, with_cones = lod_cone_second_launches, older = cone_second_launches;
        const uint64_t launches = emit_launches(ctx);
        CHECK(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0));
        REQUIRE(emit_launches(ctx) - launches == 5u && cone_second_launches == older);
        REQUIRE(lod_second_launches - plain == (with_eyes ? 0u : 1u) && lod_cone_second_launches - with_cones == (with_eyes ? 1u : 0u));
        REQUIRE(std::memcmp(last_views, kViews, sizeof(kViews)) == 0);
        REQUIRE(!with_eyes || std::memcmp(last_eyes, kEyes, sizeof(kEyes)) == 0);
        REQUIRE(gv_pool_cluster_second_commands_device(ctx, kMain, &second, &second_counts) == GV_OK);
    }
    // a cluster cull of an older form replaces it, and the second phase behind that one carries no LOD test; a second-phase result
    // behind the replaced one ends with it
    alignas(16) static uint8_t target[8192];
    for (int form = 0; form < 3; form++) {
        if (form == 0)
            CHECK(gv_pool_cull_clusters(ctx, kMain, 0, 0, target, sizeof(target)));
        else if (form == 1)
            CHECK(gv_pool_cull_cluster_runs(ctx, kMain, 0, 0, target, sizeof(target)));
        else
            CHECK(gv_pool_cull_cluster_cones(ctx, kMain, 0, kEyes, 2, 0, target, sizeof(target)));
        REQUIRE(observe(ctx).commands == target);
        REQUIRE(gv_pool_cluster_second_commands_device(ctx, kMain, &second, &second_counts) == GV_E_STATE);
        const uint32_t plain = lod_second_launches, with_cones = lod_cone_second_launches, older = cone_second_launches;
        CHECK(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0));
        REQUIRE(lod_second_launches == plain && lod_cone_second_launches == with_cones && cone_second_launches - older == (form == 2 ? 1u : 0u));
        again(form == 1 ? GV_CLUSTERS_RUNS : 0u, form == 2);
        REQUIRE(observe(ctx).commands != target);
        REQUIRE(gv_pool_cluster_second_commands_device(ctx, kMain, &second, &second_counts) == GV_E_STATE);
    }
    CHECK(gv_pool_bind_cluster_lods(ctx, kMain, lods.data(), 72));  // a bind of the LOD table ends it, and a second phase has nothing to follow
    REQUIRE(observe(ctx).code == GV_E_STATE);
    EXPECT(gv_pool_cull_clusters_second_phase(ctx, kMain, 0, 0, nullptr, 0), GV_E_STATE);
    std::printf("lifetimes: the pool's one cluster result, ended where it ends and by a LOD bind, replaced by any form; five and six launches; "
                "the second phase carries the kept views and eyes: ok\n");
}

int main()
{
    static_assert(sizeof(GvClusterLod) == 48 && sizeof(GvClusterLodView) == 32, "the header's sizes");
    std::vector<GvClusterLod> lods(80, GvClusterLod{{0.0f, 0.0f, 0.0f}, 1.0f, {0.0f, 0.0f, 0.0f}, 2.0f, 0.0f, 1.0f, {0u, 0u}});
    std::vector<GvClusterCone> cones(80, GvClusterCone{{0.0f, 0.0f, 0.0f}, 0.5f, {0.0f, 0.0f, 1.0f}, 0u});
    bind_errors(lods);
    cull_errors(lods, cones);
    unbuilt_pyramid(lods);
    dropped_by_a_cluster_bind(lods);
    lifetimes(lods, cones);
    std::printf("error list: %u rows as pinned\n", rows);
    std::printf("cluster lods: ok\n");
    return 0;
}
