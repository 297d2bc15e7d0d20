// receivers_host_test.cpp — TEST driver of gv_receiver_begin / gv_pool_draw_receivers / gv_receiver_mask_device / gv_receiver_mask_fetch /
// gv_hiz_build_from_receivers through include/garden_vis.h alone. It pins:
//   1. the code of every row of the header's error lists, and that a refused call changes nothing;
//   2. the two-image rule, restated for the receiver pair: a begin never hands out the image the current pyramid reads, whatever the
//      sizes and however often it is called, before and after the pyramid moves, with an occluder image open alongside — which no
//      receiver call touches, closes or hands out; (stub build) a sentinel written into the pyramid's image survives every begin;
//   3. (stub build) every allocation of a frame failing once, in turn: GV_E_OOM, the open mask stays usable or is reported gone,
//      and the same context completes the frame.
// Built two ways from this file, as occluders_host_test.cpp: against tests/cpp/hip_stub with every host source under
// AddressSanitizer + UBSan (tests/test_receivers_host.py; the kernels are no-ops there), and against libgarden_vis.so for the device
// (tests/cpp/receivers_host.mk). Every step prints a line ending in "ok"; the last line is "receivers: ok".
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/garden_vis.h"
#ifdef GV_HIP_STUB
#include <hip/hip_runtime.h>  // tests/cpp/hip_stub: the fault-injection counters
#include "gv_receiver_kernels.hpp"
namespace gv {  // the launches as no-ops (the generated stubs cover the headers make_kernel_stubs.py lists)
hipError_t launch_occluder_setup(const OccluderLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_occluder_scan(const OccluderLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_occluder_raster(const OccluderLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_receiver_setup(const ReceiverLaunch&, hipStream_t) { return hipSuccess; }
hipError_t launch_receiver_raster(const ReceiverLaunch&, hipStream_t) { return hipSuccess; }
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

// a sheet of 64 boxes in front of a camera that looks down -z; the light looks down on it from above
constexpr uint32_t kSlots = 64;
constexpr uint32_t kMain = 0, kUnbound = 5;
constexpr uint32_t kCountOnly = 1, kLater = 2, kNever = 6;  // views of cull_all: 0 emitted, 1 count-only, 2 emitted

struct Fixture {
    GvCtx* ctx = nullptr;
    std::vector<Transform> xf;
    std::vector<uint32_t> e2t;
    std::vector<Mesh> main;
    std::vector<float> lo, hi;  // occluder boxes, 4 floats a slot
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

// an orthographic light looking down -y on the sheet: u = x / 12 + .5, v = (z + 22) / 12 + .5, depth = (y + 8) / 16
static const float kLight[16] = {1.0f / 6.0f, 0, 0, 0, 0, 0, 1.0f / 16.0f, 0, 0, 1.0f / 6.0f, 0, 0, 0, 22.0f / 6.0f, 0.5f, 1.0f};

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

static int cull_all(Fixture& f, uint32_t views = 3)
{
    const GvView v[3] = {make_view(1), make_view(0), make_view(1)};
    return gv_cull(f.ctx, kMain, v, views);
}

struct Image {
    const void *pixels = nullptr, *counts = nullptr;
    uint32_t width = 0, height = 0;
};
static Image mask_of(GvCtx* ctx)
{
    Image i;
    CHECK(gv_receiver_mask_device(ctx, &i.pixels, &i.width, &i.height, &i.counts));
    return i;
}
static Image occluders_of(GvCtx* ctx)
{
    Image i;
    CHECK(gv_occluder_depth_device(ctx, &i.pixels, &i.width, &i.height, &i.counts));
    return i;
}

// ---- 1. the error lists ------------------------------------------------------------------------------------------------------------
static void error_list()
{
    g_where = "error list";
    uint32_t rows = 0;
    Image i;
    GvReceiverCounts counts{};
    std::vector<float> pixels(16 * 16);
    {
        GvCtx* ctx = nullptr;
        EXPECT(gv_receiver_begin(nullptr, 16, 16), GV_E_ARG);
        EXPECT(gv_pool_draw_receivers(nullptr, kMain, 0, kLight), GV_E_ARG);
        EXPECT(gv_receiver_mask_device(nullptr, &i.pixels, &i.width, &i.height, &i.counts), GV_E_ARG);
        EXPECT(gv_receiver_mask_fetch(nullptr, pixels.data(), pixels.size() * 4, &counts), GV_E_ARG);
        EXPECT(gv_hiz_build_from_receivers(nullptr), GV_E_ARG);
        rows += 5;
    }
    Fixture f;
    GvCtx* ctx = f.ctx;
    // nothing begun, nothing bound
    EXPECT(gv_receiver_mask_device(ctx, &i.pixels, &i.width, &i.height, &i.counts), GV_E_STATE);
    EXPECT(gv_receiver_mask_fetch(ctx, pixels.data(), pixels.size() * 4, &counts), GV_E_STATE);
    EXPECT(gv_hiz_build_from_receivers(ctx), GV_E_STATE);
    EXPECT(gv_pool_draw_receivers(ctx, kMain, 0, kLight), GV_E_ARG);  // (the pool is not bound)
    EXPECT(gv_receiver_begin(ctx, 0, 16), GV_E_ARG);
    EXPECT(gv_receiver_begin(ctx, 16, 0), GV_E_ARG);
    EXPECT(gv_receiver_begin(ctx, 32769, 16), GV_E_ARG);
    EXPECT(gv_receiver_begin(ctx, 16, 32769), GV_E_ARG);
    EXPECT(gv_receiver_mask_device(ctx, &i.pixels, &i.width, &i.height, &i.counts), GV_E_STATE);  // (a refused begin opened nothing)
    rows += 9;
    CHECK(bind_pools(f));
    EXPECT(gv_pool_draw_receivers(ctx, kMain, 0, nullptr), GV_E_ARG);
    EXPECT(gv_pool_draw_receivers(ctx, kUnbound, 0, kLight), GV_E_ARG);
    EXPECT(gv_pool_draw_receivers(ctx, GV_MAX_POOLS, 0, kLight), GV_E_ARG);
    EXPECT(gv_pool_draw_receivers(ctx, kMain, GV_MAX_VIEWS, kLight), GV_E_ARG);
    EXPECT(gv_pool_draw_receivers(ctx, kMain, 0, kLight), GV_E_ARG);  // (no cull of the pool has had a view yet)
    CHECK(cull_all(f));
    EXPECT(gv_pool_draw_receivers(ctx, kMain, kNever, kLight), GV_E_ARG);
    EXPECT(gv_pool_draw_receivers(ctx, kMain, 0, kLight), GV_E_STATE);  // no open mask
    CHECK(gv_occluder_begin(ctx, 16, 16));
    EXPECT(gv_pool_draw_receivers(ctx, kMain, 0, kLight), GV_E_STATE);  // (an open occluder image is no open mask)
    CHECK(gv_receiver_begin(ctx, 16, 16));
    EXPECT(gv_pool_draw_receivers(ctx, kMain, kCountOnly, kLight), GV_E_STATE);
    rows += 9;
    // a refused call changes nothing: the mask is still open, the same, and takes a draw
    const Image open = mask_of(ctx);
    CHECK(gv_pool_draw_receivers(ctx, kMain, 0, kLight));
    CHECK(gv_pool_draw_receivers(ctx, kMain, kLater, kLight));
    CHECK(cull_all(f, 1));
    EXPECT(gv_pool_draw_receivers(ctx, kMain, kLater, kLight), GV_E_STATE);  // a later cull of fewer views ended it
    const Image still = mask_of(ctx);
    if (still.pixels != open.pixels || still.counts != open.counts || still.width != 16 || still.height != 16)
        die(__FILE__, __LINE__, "a refused call replaced the mask", 1, 0, ctx);
    rows += 3;
    EXPECT(gv_receiver_mask_device(ctx, nullptr, &i.width, &i.height, &i.counts), GV_E_ARG);
    EXPECT(gv_receiver_mask_device(ctx, &i.pixels, nullptr, &i.height, &i.counts), GV_E_ARG);
    EXPECT(gv_receiver_mask_device(ctx, &i.pixels, &i.width, nullptr, &i.counts), GV_E_ARG);
    EXPECT(gv_receiver_mask_device(ctx, &i.pixels, &i.width, &i.height, nullptr), GV_E_ARG);
    EXPECT(gv_receiver_mask_fetch(ctx, nullptr, 0, nullptr), GV_E_ARG);
    pixels[0] = 42.0f;
    EXPECT(gv_receiver_mask_fetch(ctx, pixels.data(), pixels.size() * 4 - 1, &counts), GV_E_ARG);
    if (pixels[0] != 42.0f)
        die(__FILE__, __LINE__, "a refused fetch wrote", 1, 0, ctx);
    CHECK(gv_receiver_mask_fetch(ctx, pixels.data(), pixels.size() * 4, &counts));
    CHECK(gv_receiver_mask_fetch(ctx, nullptr, 0, &counts));
    CHECK(gv_receiver_mask_fetch(ctx, pixels.data(), pixels.size() * 4, nullptr));
    rows += 9;
    if (kDevice && (counts.drawn + counts.flat + counts.behind + counts.range + counts.outside != 2 * kSlots || counts.drawn == 0 || counts.reserved != 0))
        die(__FILE__, __LINE__, "two draws of the sheet: records counted", counts.drawn, 2 * kSlots, ctx);
    if (kDevice) {  // (the light sees the whole sheet: some texel holds a receiver, and no word is negative)
        uint32_t finite = 0;
        for (float p : pixels) {
            uint32_t w;
            std::memcpy(&w, &p, 4);
            finite += w < 0x7F800000u;
            if (w > 0x7F800000u)
                die(__FILE__, __LINE__, "a word above +inf", (long)w, 0x7F800000, ctx);
        }
        if (!finite)
            die(__FILE__, __LINE__, "texels with a receiver", 0, 1, ctx);
    }
    // (the mirror-covers-fewer-slots row guards reads no sequence of public calls is known to reach, as gv_pool_view_bounds's: a cull
    // synchronises the mirror it reads; it is not pinned here)
    // the build closes the mask; it can still be read
    CHECK(gv_hiz_build_from_receivers(ctx));
    EXPECT(gv_hiz_build_from_receivers(ctx), GV_E_STATE);
    EXPECT(gv_pool_draw_receivers(ctx, kMain, 0, kLight), GV_E_STATE);
    CHECK(gv_receiver_mask_fetch(ctx, pixels.data(), pixels.size() * 4, &counts));
    rows += 4;
    std::printf("error list: %u rows as pinned, a refused call changes nothing: ok\n", rows);
}

// ---- 2. the two-image rule ------------------------------------------------------------------------------------------------------------
static void two_images()
{
    g_where = "two images";
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(gv_pool_bind_occluders(ctx, kMain, f.lo.data(), f.hi.data(), 16, kSlots));
    CHECK(cull_all(f));
    // an occluder image open alongside, all the way through: no receiver call closes it, moves it or hands it out
    CHECK(gv_occluder_begin(ctx, 40, 24));
    const Image occluders = occluders_of(ctx);
    auto occluders_untouched = [&](int line) {
        const Image now = occluders_of(ctx);
        if (now.pixels != occluders.pixels || now.width != 40 || now.height != 24)
            die(__FILE__, line, "a receiver call moved the open occluder image", 1, 0, ctx);
        CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));  // (still open)
    };
    CHECK(gv_receiver_begin(ctx, 64, 48));
    const Image first = mask_of(ctx);
    if (first.pixels == occluders.pixels)
        die(__FILE__, __LINE__, "the receiver pair shares an image with the occluder pair", 1, 0, ctx);
    CHECK(gv_receiver_begin(ctx, 64, 48));  // starting over: the same image
    if (mask_of(ctx).pixels != first.pixels)
        die(__FILE__, __LINE__, "a begin on an open mask took another one", 1, 0, ctx);
    CHECK(gv_pool_draw_receivers(ctx, kMain, 0, kLight));
    CHECK(gv_hiz_build_from_receivers(ctx));
    occluders_untouched(__LINE__);
    const void* pyramid = first.pixels;  // the pyramid's level 0 from here on
#ifdef GV_HIP_STUB
    uint32_t sentinel = 0;
    std::memcpy(const_cast<void*>(pyramid), "\x5a\x5a\x5a\x5a", 4);  // (the stub's device memory is host memory)
#endif
    uint32_t begins = 0;
    const uint32_t sizes[][2] = {{64, 48}, {64, 48}, {8, 8}, {512, 256}, {1, 1}, {513, 257}};
    for (const auto& s : sizes) {
        CHECK(gv_receiver_begin(ctx, s[0], s[1]));
        const Image now = mask_of(ctx);
        if (now.pixels == pyramid || now.pixels == occluders.pixels || now.width != s[0] || now.height != s[1])
            die(__FILE__, __LINE__, "a begin handed out the image the pyramid reads", (long)begins, 0, ctx);
        CHECK(gv_pool_draw_receivers(ctx, kMain, 0, kLight));
        CHECK(gv_hiz_rebuild(ctx));  // (reads the pyramid's image)
        begins++;
    }
    occluders_untouched(__LINE__);
#ifdef GV_HIP_STUB
    std::memcpy(&sentinel, pyramid, 4);
    if (sentinel != 0x5a5a5a5au)
        die(__FILE__, __LINE__, "the pyramid's image was cleared or replaced under it", (long)sentinel, 0x5a5a5a5a, ctx);
#endif
    // the next build moves the pyramid over; the begin behind it takes the first image again, at another size
    CHECK(gv_hiz_build_from_receivers(ctx));
    const void* second = mask_of(ctx).pixels;
    CHECK(gv_receiver_begin(ctx, 700, 300));
    if (mask_of(ctx).pixels == second)
        die(__FILE__, __LINE__, "a begin handed out the image the second pyramid reads", 1, 0, ctx);
    CHECK(gv_hiz_rebuild(ctx));
    // the pyramid moves to the occluder image: both receiver images are free, the open one stays the open one; the occluder image closes
    const void* open = mask_of(ctx).pixels;
    CHECK(gv_hiz_build_from_occluders(ctx));
    CHECK(gv_receiver_begin(ctx, 700, 300));
    if (mask_of(ctx).pixels != open)
        die(__FILE__, __LINE__, "a begin left an open mask that no pyramid reads", 1, 0, ctx);
    CHECK(gv_pool_draw_receivers(ctx, kMain, 0, kLight));  // (the occluder build did not close the mask)
    EXPECT(gv_pool_draw_occluders(ctx, kMain, 0, 1), GV_E_STATE);
    // a caller who builds the pyramid of the open mask himself closes it: no draw under the pyramid, the next begin takes the other
    const Image mine = mask_of(ctx);
    CHECK(gv_hiz_build(ctx, static_cast<const float*>(mine.pixels), mine.width, mine.height, GV_MEM_DEVICE));
    EXPECT(gv_pool_draw_receivers(ctx, kMain, 0, kLight), GV_E_STATE);
    EXPECT(gv_hiz_build_from_receivers(ctx), GV_E_STATE);
    CHECK(gv_receiver_begin(ctx, 700, 300));
    if (mask_of(ctx).pixels == mine.pixels)
        die(__FILE__, __LINE__, "a begin handed out the image the caller's own gv_hiz_build adopted", 1, 0, ctx);
    CHECK(gv_pool_draw_receivers(ctx, kMain, 0, kLight));
    // ... and an occluder begin under a receiver pyramid takes an occluder image, open beside the open mask
    CHECK(gv_occluder_begin(ctx, 40, 24));
    if (occluders_of(ctx).pixels == mine.pixels || occluders_of(ctx).pixels == mask_of(ctx).pixels)
        die(__FILE__, __LINE__, "an occluder begin handed out a receiver image", 1, 0, ctx);
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    CHECK(gv_pool_draw_receivers(ctx, kMain, 0, kLight));
    std::printf("two images: %u begins at %zu sizes kept away from the pyramid's image, before and after it moved, an occluder image open alongside: ok\n",
                begins + 4, sizeof(sizes) / sizeof(sizes[0]));
}

// ---- 3. allocation failures -----------------------------------------------------------------------------------------------------------
#ifdef GV_HIP_STUB
static int frame(Fixture& f)
{
    GvCtx* ctx = f.ctx;
    TRY(gv_receiver_begin(ctx, 96, 64));
    TRY(gv_pool_draw_receivers(ctx, kMain, 0, kLight));
    GvReceiverCounts counts{};
    std::vector<float> pixels(96 * 64);
    TRY(gv_receiver_mask_fetch(ctx, pixels.data(), pixels.size() * 4, &counts));
    TRY(gv_hiz_build_from_receivers(ctx));
    TRY(gv_receiver_begin(ctx, 128, 64));  // the other image
    TRY(gv_pool_draw_receivers(ctx, kMain, kLater, kLight));
    TRY(gv_hiz_build_from_receivers(ctx));
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
        CHECK(cull_all(f));
        gv_stub_fail_countdown() = k;
        const int rc = frame(f);
        gv_stub_fail_countdown() = 0;
        if (rc != GV_E_OOM)
            die(__FILE__, __LINE__, "a frame whose k-th allocation fails", rc, GV_E_OOM, ctx);
        // what the failed call left is either usable or reported gone: never a dangling image
        const void *mask = nullptr, *counts = nullptr;
        uint32_t w = 0, h = 0;
        const int held = gv_receiver_mask_device(ctx, &mask, &w, &h, &counts);
        if (held == GV_OK) {
            std::vector<float> pixels((size_t)w * h);
            CHECK(gv_receiver_mask_fetch(ctx, pixels.data(), pixels.size() * 4, nullptr));
        } else if (held != GV_E_STATE) {
            die(__FILE__, __LINE__, "the mask behind a failed call", held, GV_E_STATE, ctx);
        }
        CHECK(frame(f));  // the same context completes the sequence
    }
    std::printf("allocation failures in the receiver frame: %ld allocations, each failed once, every context completed the sequence: ok\n", total);
}
#endif

int main()
{
    error_list();
    two_images();
#ifdef GV_HIP_STUB
    allocation_failures();
#endif
    std::printf("receivers: ok\n");
    return 0;
}
