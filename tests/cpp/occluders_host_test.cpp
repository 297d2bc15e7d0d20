// occluders_host_test.cpp — TEST driver of gv_pool_bind_occluders / gv_occluder_begin / gv_pool_draw_occluders / gv_occluder_depth_device /
// gv_occluder_depth_fetch / gv_hiz_build_from_occluders through include/garden_vis.h alone. It pins:
//   1. the code of every row of the header's error lists, and that a refused call changes nothing;
//   2. the two-image rule: a begin never hands out the image the current pyramid reads, whatever the sizes and however often it is
//      called; (stub build) a sentinel written into the pyramid's image survives every begin;
//   3. the box mirror's bookkeeping through GvStats::upload_bytes: the first draw uploads the column, a draw without marks nothing,
//      GV_DIRTY_OCCLUDER and GV_DIRTY_MESH marks their rows, gv_sync consumes marks too, a rebind uploads everything again, marks in
//      front of the first draw are not kept;
//   4. (stub build) every allocation of a frame failing once, in turn: GV_E_OOM, the open image stays usable or is reported gone,
//      and the same context completes the frame.
// Built two ways from this file, as view_delta_host_test.cpp: against tests/cpp/hip_stub with every host source under
// AddressSanitizer + UBSan (tests/test_occluders_host.py; the kernels are no-ops there), and against libgarden_vis.so for the device
// (tests/cpp/occluders_host.mk). Every step prints a line ending in "ok"; the last line is "occluders: ok".
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/garden_vis.h"
#ifdef GV_HIP_STUB
#include <hip/hip_runtime.h>  // tests/cpp/hip_stub: the fault-injection counters
#include "gv_occluder_kernels.hpp"
namespace gv {  // the three launches as no-ops (the generated stubs cover the headers make_kernel_stubs.py lists)
hipError_t launch_occluder_setup(const OccluderLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_occluder_scan(const OccluderLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_occluder_raster(const OccluderLaunch&, hipStream_t) { return hipSuccess; }
}  // namespace gv
constexpr bool kDevice = false;
#else
constexpr bool kDevice = true;
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

// a sheet of 64 boxes in front of a camera that looks down -z, each with an occluder box half the size of its AABB
constexpr uint32_t kSlots = 64;
constexpr uint32_t kMain = 0, kUnbound = 5;
constexpr uint32_t kCountOnly = 1, kLater = 2, kNever = 6;  // views of cull_all: 0 emitted, 1 count-only, 2 emitted

struct Fixture {
    GvCtx* ctx = nullptr;
    std::vector<Transform> xf;
    std::vector<uint32_t> e2t;
    std::vector<Mesh> main;
    std::vector<float> lo, hi;  // 4 floats a slot
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
            Mesh m{};
            m.entity = i + 1;
            m.isEnabled = 1;
            for (int k = 0; k < 3; k++)
                m.aabbMin[k] = -0.5f, m.aabbMax[k] = 0.5f;
            main.push_back(m);
        }
        lo.assign(4 * kSlots, -0.25f);
        hi.assign(4 * kSlots, 0.25f);
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

static GvView make_view(uint8_t emit)
{
    GvView v{};
    v.view_proj[0] = 9.0f / 16.0f;  // infinite reversed-Z perspective, camera looking down -z
    v.view_proj[5] = 1.0f;
    v.view_proj[11] = -1.0f;
    v.view_proj[14] = 0.01f;
    v.shadow_pass = -1;
    v.emit_records = emit;
    return v;
}

static const GvMeshLayout kMeshLayout = {(uint32_t)offsetof(Mesh, entity), (uint32_t)offsetof(Mesh, isEnabled), (uint32_t)offsetof(Mesh, isVisible),
                                         (uint32_t)offsetof(Mesh, aabbMin), (uint32_t)offsetof(Mesh, aabbMax)};

static int bind_pools(Fixture& f)
{
    GvCtx* ctx = f.ctx;
    const GvTransformLayout tl = {(uint32_t)offsetof(Transform, entity), (uint32_t)offsetof(Transform, parent), (uint32_t)offsetof(Transform, position),
                                  (uint32_t)offsetof(Transform, scale), (uint32_t)offsetof(Transform, rotation), (uint32_t)offsetof(Transform, selfActive),
                                  (uint32_t)offsetof(Transform, ancestorsActive), (uint32_t)offsetof(Transform, modelWithAncestors)};
    TRY(gv_transform_bind(ctx, f.xf.data(), sizeof(Transform), (uint32_t)f.xf.size(), &tl, f.e2t.data(), (uint32_t)f.e2t.size()));
    TRY(gv_pool_bind(ctx, kMain, f.main.data(), sizeof(Mesh), kSlots, &kMeshLayout));
    return GV_OK;
}

static int bind_boxes(Fixture& f, uint32_t slots = kSlots) { return gv_pool_bind_occluders(f.ctx, kMain, f.lo.data(), f.hi.data(), 16, slots); }

static int cull_all(Fixture& f, uint32_t views = 3)
{
    const GvView v[3] = {make_view(1), make_view(0), make_view(1)};
    return gv_cull(f.ctx, kMain, v, views);
}

struct Image {
    const void *depth = nullptr, *counts = nullptr;
    uint32_t width = 0, height = 0;
};
static Image image_of(GvCtx* ctx)
{
    Image i;
    CHECK(gv_occluder_depth_device(ctx, &i.depth, &i.width, &i.height, &i.counts));
    return i;
}

static uint64_t uploaded(GvCtx* ctx)
{
    GvStats s{};
    CHECK(gv_stats(ctx, &s));
    return s.upload_bytes;
}

// ---- 1. the error lists ------------------------------------------------------------------------------------------------------------
static void error_list()
{
    g_where = "error list";
    uint32_t rows = 0;
    Image i;
    GvOccluderCounts counts{};
    std::vector<float> pixels(16 * 16);
    {
        GvCtx* ctx = nullptr;
        EXPECT(gv_pool_bind_occluders(nullptr, kMain, nullptr, nullptr, 0, 0), GV_E_ARG);
        EXPECT(gv_occluder_begin(nullptr, 16, 16), GV_E_ARG);
        EXPECT(gv_pool_draw_occluders(nullptr, kMain, 0, 1), GV_E_ARG);
        EXPECT(gv_occluder_depth_device(nullptr, &i.depth, &i.width, &i.height, &i.counts), GV_E_ARG);
        EXPECT(gv_occluder_depth_fetch(nullptr, pixels.data(), pixels.size() * 4, &counts), GV_E_ARG);
        EXPECT(gv_hiz_build_from_occluders(nullptr), GV_E_ARG);
        rows += 6;
    }
    Fixture f;
    GvCtx* ctx = f.ctx;
    // nothing begun, nothing bound
    EXPECT(gv_occluder_depth_device(ctx, &i.depth, &i.width, &i.height, &i.counts), GV_E_STATE);
    EXPECT(gv_occluder_depth_fetch(ctx, pixels.data(), pixels.size() * 4, &counts), GV_E_STATE);
    EXPECT(gv_hiz_build_from_occluders(ctx), GV_E_STATE);
    EXPECT(gv_pool_draw_occluders(ctx, kMain, 0, 1), GV_E_ARG);  // (the pool is not bound)
    EXPECT(gv_occluder_begin(ctx, 0, 16), GV_E_ARG);
    EXPECT(gv_occluder_begin(ctx, 16, 0), GV_E_ARG);
    EXPECT(gv_occluder_begin(ctx, 32769, 16), GV_E_ARG);
    EXPECT(gv_occluder_begin(ctx, 16, 32769), GV_E_ARG);
    EXPECT(gv_occluder_depth_device(ctx, &i.depth, &i.width, &i.height, &i.counts), GV_E_STATE);  // (a refused begin opened nothing)
    rows += 9;
    CHECK(bind_pools(f));
    EXPECT(gv_pool_bind_occluders(ctx, GV_MAX_POOLS, f.lo.data(), f.hi.data(), 16, kSlots), GV_E_ARG);
    EXPECT(gv_pool_bind_occluders(ctx, kMain, f.lo.data(), nullptr, 16, kSlots), GV_E_ARG);
    EXPECT(gv_pool_bind_occluders(ctx, kMain, nullptr, f.hi.data(), 16, kSlots), GV_E_ARG);
    EXPECT(gv_pool_bind_occluders(ctx, kMain, f.lo.data(), f.hi.data(), 11, kSlots), GV_E_ARG);
    EXPECT(gv_pool_bind_occluders(ctx, kMain, f.lo.data(), f.hi.data(), 16, 0x0FFFFFFFu), GV_E_ARG);
    CHECK(gv_pool_bind_occluders(ctx, kMain, nullptr, nullptr, 0, 0));  // (removing what is not there)
    rows += 6;
    EXPECT(gv_pool_draw_occluders(ctx, kUnbound, 0, 1), GV_E_ARG);
    EXPECT(gv_pool_draw_occluders(ctx, GV_MAX_POOLS, 0, 1), GV_E_ARG);
    EXPECT(gv_pool_draw_occluders(ctx, kMain, GV_MAX_VIEWS, 1), GV_E_ARG);
    EXPECT(gv_pool_draw_occluders(ctx, kMain, 0, 1), GV_E_ARG);  // (no cull of the pool has had a view yet)
    CHECK(cull_all(f));
    EXPECT(gv_pool_draw_occluders(ctx, kMain, kNever, 1), GV_E_ARG);
    EXPECT(gv_pool_draw_occluders(ctx, kMain, 0, 1), GV_E_STATE);  // no open image
    CHECK(gv_occluder_begin(ctx, 16, 16));
    EXPECT(gv_pool_draw_occluders(ctx, kMain, 0, 1), GV_E_STATE);  // no binding
    CHECK(bind_boxes(f, kSlots - 1));
    EXPECT(gv_pool_draw_occluders(ctx, kMain, 0, 1), GV_E_STATE);  // boxes below the view's occupancy
    CHECK(bind_boxes(f));
    EXPECT(gv_pool_draw_occluders(ctx, kMain, kCountOnly, 1), GV_E_STATE);
    rows += 9;
    // a refused call changes nothing: the image is still open, the same, and takes a draw
    const Image open = image_of(ctx);
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    CHECK(gv_pool_draw_occluders(ctx, kMain, kLater, 8));
    CHECK(cull_all(f, 1));
    EXPECT(gv_pool_draw_occluders(ctx, kMain, kLater, 1), GV_E_STATE);  // a later cull of fewer views ended it
    const Image still = image_of(ctx);
    if (still.depth != open.depth || still.counts != open.counts || still.width != 16 || still.height != 16)
        die(__FILE__, __LINE__, "a refused call replaced the image", 1, 0, ctx);
    rows += 3;
    EXPECT(gv_occluder_depth_device(ctx, nullptr, &i.width, &i.height, &i.counts), GV_E_ARG);
    EXPECT(gv_occluder_depth_device(ctx, &i.depth, nullptr, &i.height, &i.counts), GV_E_ARG);
    EXPECT(gv_occluder_depth_device(ctx, &i.depth, &i.width, nullptr, &i.counts), GV_E_ARG);
    EXPECT(gv_occluder_depth_device(ctx, &i.depth, &i.width, &i.height, nullptr), GV_E_ARG);
    EXPECT(gv_occluder_depth_fetch(ctx, nullptr, 0, nullptr), GV_E_ARG);
    pixels[0] = 42.0f;
    EXPECT(gv_occluder_depth_fetch(ctx, pixels.data(), pixels.size() * 4 - 1, &counts), GV_E_ARG);
    if (pixels[0] != 42.0f)
        die(__FILE__, __LINE__, "a refused fetch wrote", 1, 0, ctx);
    CHECK(gv_occluder_depth_fetch(ctx, pixels.data(), pixels.size() * 4, &counts));
    CHECK(gv_occluder_depth_fetch(ctx, nullptr, 0, &counts));
    CHECK(gv_occluder_depth_fetch(ctx, pixels.data(), pixels.size() * 4, nullptr));
    rows += 9;
    if (kDevice && (counts.drawn + counts.no_box + counts.behind + counts.range + counts.flat + counts.small != 2 * kSlots || counts.drawn == 0))
        die(__FILE__, __LINE__, "two draws of the sheet: records counted", counts.drawn, 2 * kSlots, ctx);
    // the build closes the image; it can still be read
    CHECK(gv_hiz_build_from_occluders(ctx));
    EXPECT(gv_hiz_build_from_occluders(ctx), GV_E_STATE);
    EXPECT(gv_pool_draw_occluders(ctx, kMain, 0, 1), GV_E_STATE);
    CHECK(gv_occluder_depth_fetch(ctx, pixels.data(), pixels.size() * 4, &counts));
    CHECK(gv_pool_bind_occluders(ctx, kMain, nullptr, nullptr, 0, 0));
    CHECK(gv_occluder_begin(ctx, 16, 16));
    EXPECT(gv_pool_draw_occluders(ctx, kMain, 0, 1), GV_E_STATE);  // the binding is gone
    rows += 7;
    std::printf("error list: %u rows as pinned, a refused call changes nothing: ok\n", rows);
}

// ---- 2. the two-image rule ------------------------------------------------------------------------------------------------------------
static void two_images()
{
    g_where = "two images";
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(bind_boxes(f));
    CHECK(cull_all(f));
    CHECK(gv_occluder_begin(ctx, 64, 48));
    const Image first = image_of(ctx);
    CHECK(gv_occluder_begin(ctx, 64, 48));  // starting over: the same image
    if (image_of(ctx).depth != first.depth)
        die(__FILE__, __LINE__, "a begin on an open image took another one", 1, 0, ctx);
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    CHECK(gv_hiz_build_from_occluders(ctx));
    const void* pyramid = first.depth;  // the pyramid's level 0 from here on
#ifdef GV_HIP_STUB
    uint32_t sentinel = 0;
    std::memcpy(const_cast<void*>(pyramid), "\x5a\x5a\x5a\x5a", 4);  // (the stub's device memory is host memory)
#endif
    uint32_t begins = 0;
    const uint32_t sizes[][2] = {{64, 48}, {64, 48}, {8, 8}, {512, 256}, {1, 1}, {513, 257}};
    for (const auto& s : sizes) {
        CHECK(gv_occluder_begin(ctx, s[0], s[1]));
        const Image now = image_of(ctx);
        if (now.depth == pyramid || now.width != s[0] || now.height != s[1])
            die(__FILE__, __LINE__, "a begin handed out the image the pyramid reads", (long)begins, 0, ctx);
        CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
        CHECK(gv_hiz_rebuild(ctx));  // (reads the pyramid's image)
        begins++;
    }
#ifdef GV_HIP_STUB
    std::memcpy(&sentinel, pyramid, 4);
    if (sentinel != 0x5a5a5a5au)
        die(__FILE__, __LINE__, "the pyramid's image was cleared or replaced under it", (long)sentinel, 0x5a5a5a5a, ctx);
#endif
    // the next build moves the pyramid over; the begin behind it takes the first image again, at another size
    CHECK(gv_hiz_build_from_occluders(ctx));
    const void* second = image_of(ctx).depth;
    CHECK(gv_occluder_begin(ctx, 700, 300));
    if (image_of(ctx).depth == second)
        die(__FILE__, __LINE__, "a begin handed out the image the second pyramid reads", 1, 0, ctx);
    CHECK(gv_hiz_rebuild(ctx));
    // a pyramid of the caller's own image frees both: the open one stays the open one
    std::vector<float> host(32 * 32, 0.5f);
    CHECK(gv_hiz_build(ctx, host.data(), 32, 32, GV_MEM_HOST));
    const void* open = image_of(ctx).depth;
    CHECK(gv_occluder_begin(ctx, 700, 300));
    if (image_of(ctx).depth != open)
        die(__FILE__, __LINE__, "a begin left an open image that no pyramid reads", 1, 0, ctx);
    // a caller who builds the pyramid of the open image himself closes it: no draw under the pyramid, the next begin takes the other
    const Image mine = image_of(ctx);
    CHECK(gv_hiz_build(ctx, static_cast<const float*>(mine.depth), mine.width, mine.height, GV_MEM_DEVICE));
    EXPECT(gv_pool_draw_occluders(ctx, kMain, 0, 1), GV_E_STATE);
    EXPECT(gv_hiz_build_from_occluders(ctx), GV_E_STATE);
    CHECK(gv_occluder_begin(ctx, 700, 300));
    if (image_of(ctx).depth == mine.depth)
        die(__FILE__, __LINE__, "a begin handed out the image the caller's own gv_hiz_build adopted", 1, 0, ctx);
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    std::printf("two images: %u begins at %zu sizes kept away from the pyramid's image, before and after it moved: ok\n", begins + 4, sizeof(sizes) / sizeof(sizes[0]));
}

// ---- 3. the mirror's bookkeeping ----------------------------------------------------------------------------------------------------
static void mirror_marks()
{
    g_where = "mirror marks";
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(bind_boxes(f));
    CHECK(cull_all(f));
    CHECK(gv_occluder_begin(ctx, 32, 32));
    constexpr uint64_t kRow = 32, kPacked = kRow + 4;  // a row; a row that travels in the packet with its slot word
    auto expect_upload = [&](const char* what, uint64_t lo, uint64_t hi, uint64_t& at) {
        const uint64_t now = uploaded(ctx);
        if (now - at < lo || now - at > hi)
            die(__FILE__, __LINE__, what, (long)(now - at), (long)lo, ctx);
        at = now;
    };
    CHECK(gv_mark_dirty(ctx, GV_DIRTY_OCCLUDER, (kMain << 28) | 3, 5));  // in front of the first draw: nobody wants the mirror yet
    uint64_t at = uploaded(ctx);
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    expect_upload("the first draw uploads the column", kSlots * kRow, kSlots * kPacked, at);
    CHECK(gv_pool_draw_occluders(ctx, kMain, kLater, 1));
    expect_upload("a draw without marks uploads nothing", 0, 0, at);
    CHECK(gv_mark_dirty(ctx, GV_DIRTY_OCCLUDER, (kMain << 28) | 7, 1));
    expect_upload("a mark alone uploads nothing", 0, 0, at);
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    expect_upload("one marked row", kPacked, kPacked, at);
    CHECK(gv_mark_dirty(ctx, GV_DIRTY_OCCLUDER, (kMain << 28) | 7, 1));
    CHECK(gv_mark_dirty(ctx, GV_DIRTY_OCCLUDER, (kMain << 28) | 7, 2));
    CHECK(gv_mark_dirty(ctx, GV_DIRTY_OCCLUDER, (kMain << 28) | 40, 3));
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    expect_upload("overlapping marks are uploaded once: 2 + 3 rows", 5 * kPacked, 5 * kPacked, at);
    CHECK(gv_mark_dirty(ctx, GV_DIRTY_OCCLUDER, (kMain << 28) | (kSlots - 1), 100));  // clamped to the occupancy
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    expect_upload("a mark beyond the occupancy is clamped", kPacked, kPacked, at);
    CHECK(gv_mark_dirty(ctx, GV_DIRTY_OCCLUDER, (kMain << 28) | 9, 1));
    CHECK(gv_sync(ctx));
    expect_upload("gv_sync consumes the mark", kPacked, kPacked, at);
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    expect_upload("... and the draw behind it finds none", 0, 0, at);
    CHECK(gv_mark_dirty(ctx, GV_DIRTY_OCCLUDER, ((kMain + 1) << 28) | 9, 1));  // another pool's mark
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    expect_upload("another pool's mark is not this pool's", 0, 0, at);
    // a slot filled anew has a new box: the pool's GV_DIRTY_MESH marks feed the set too (the mesh side of the mark waits for gv_sync)
    CHECK(gv_mark_dirty(ctx, GV_DIRTY_MESH, (kMain << 28) | 20, 2));
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    expect_upload("a mesh mark of two slots", 2 * kPacked, 2 * kPacked, at);
    CHECK(gv_sync(ctx));  // (the mesh side of that mark)
    at = uploaded(ctx);
    // a rebind uploads everything again, at the next draw
    CHECK(bind_boxes(f));
    expect_upload("a rebind alone uploads nothing", 0, 0, at);
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    expect_upload("the draw behind a rebind uploads the column", kSlots * kRow, kSlots * kPacked, at);
    // removed and bound again: the mirror starts over
    CHECK(gv_pool_bind_occluders(ctx, kMain, nullptr, nullptr, 0, 0));
    CHECK(gv_mark_dirty(ctx, GV_DIRTY_OCCLUDER, (kMain << 28) | 1, 1));
    CHECK(gv_sync(ctx));
    expect_upload("no binding: nothing to upload", 0, 0, at);
    CHECK(bind_boxes(f));
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    expect_upload("bound again", kSlots * kRow, kSlots * kPacked, at);
    std::printf("mirror marks: first draw, marks, overlaps, clamping, gv_sync, mesh marks, rebind and removal as pinned: ok\n");
}

// ---- 4. allocation failures -----------------------------------------------------------------------------------------------------------
#ifdef GV_HIP_STUB
static int frame(Fixture& f)
{
    GvCtx* ctx = f.ctx;
    TRY(gv_occluder_begin(ctx, 96, 64));
    TRY(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    GvOccluderCounts counts{};
    std::vector<float> pixels(96 * 64);
    TRY(gv_occluder_depth_fetch(ctx, pixels.data(), pixels.size() * 4, &counts));
    TRY(gv_hiz_build_from_occluders(ctx));
    TRY(gv_occluder_begin(ctx, 128, 64));  // the other image
    TRY(gv_pool_draw_occluders(ctx, kMain, kLater, 1));
    TRY(gv_hiz_build_from_occluders(ctx));
    return GV_OK;
}
static void allocation_failures()
{
    g_where = "allocation failures";
    long total = 0;
    {
        Fixture f;
        GvCtx* ctx = f.ctx;
        CHECK(bind_pools(f));
        CHECK(bind_boxes(f));
        CHECK(cull_all(f));
        const long before = gv_stub_allocations();
        CHECK(frame(f));
        total = gv_stub_allocations() - before;
    }
    if (total < 8)
        die(__FILE__, __LINE__, "allocations of a frame", total, 8, nullptr);
    for (long k = 1; k <= total; k++) {
        Fixture f;
        GvCtx* ctx = f.ctx;
        CHECK(bind_pools(f));
        CHECK(bind_boxes(f));
        CHECK(cull_all(f));
        gv_stub_fail_countdown() = k;
        const int rc = frame(f);
        gv_stub_fail_countdown() = 0;
        if (rc != GV_E_OOM)
            die(__FILE__, __LINE__, "a frame whose k-th allocation fails", rc, GV_E_OOM, ctx);
        // what the failed call left is either usable or reported gone: never a dangling image
        const void *depth = nullptr, *counts = nullptr;
        uint32_t w = 0, h = 0;
        const int held = gv_occluder_depth_device(ctx, &depth, &w, &h, &counts);
        if (held == GV_OK) {
            std::vector<float> pixels((size_t)w * h);
            CHECK(gv_occluder_depth_fetch(ctx, pixels.data(), pixels.size() * 4, nullptr));
        } else if (held != GV_E_STATE) {
            die(__FILE__, __LINE__, "the image behind a failed call", held, GV_E_STATE, ctx);
        }
        CHECK(frame(f));  // the same context completes the sequence
    }
    std::printf("allocation failures in the occluder frame: %ld allocations, each failed once, every context completed the sequence: ok\n", total);
}
#endif

int main()
{
    error_list();
    two_images();
    mirror_marks();
#ifdef GV_HIP_STUB
    allocation_failures();
#endif
    std::printf("occluders: ok\n");
    return 0;
}
