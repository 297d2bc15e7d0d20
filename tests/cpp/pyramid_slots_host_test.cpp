// pyramid_slots_host_test.cpp — TEST driver of gv_hiz_select / gv_hiz_drop and of views that name their pyramid (GvView::use_hiz =
// 1 + k) through include/garden_vis.h alone. It pins:
//   1. the code of every row of the two calls' error lists and of the "pyramid not built" rows of gv_cull and
//      gv_pool_cull_second_phase, and that a refused call changes nothing;
//   2. select / build / drop lifetimes: a build lands in the selected slot alone, a dropped slot is "not built" selected or parked,
//      a drop of a slot that was never built is GV_OK;
//   3. the image-taking rule: with one pyramid the images a begin takes are the two of old in the turn of old; with several, a begin
//      takes the image of the last begin unless a built pyramid reads it, then the lowest one no built pyramid reads — three masks
//      and an occluder image alive at once, four distinct images, a fourth mask beside them; (stub build) a sentinel written into
//      every image a pyramid reads survives every begin; a drop releases the reference, not the image;
//   4. (stub build) every allocation of a frame with three pyramids failing once, in turn: GV_E_OOM, and the same context completes
//      the frame; nothing leaks (LeakSanitizer at exit).
// Built two ways from this file, as receivers_host_test.cpp: against tests/cpp/hip_stub with every host source under AddressSanitizer +
// UBSan (tests/test_pyramid_slots_host.py; the kernels are no-ops there), and against libgarden_vis.so for the device
// (tests/cpp/pyramid_slots_host.mk). Every step prints a line ending in "ok"; the last line is "pyramid slots: ok".
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
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

constexpr uint32_t kSlots = 64, kMain = 0;

struct Fixture {  // a sheet of 64 boxes in front of a camera that looks down -z
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

static GvView make_view(uint8_t use_hiz, int8_t shadow_pass = -1)
{
    GvView v{};
    v.view_proj[0] = 9.0f / 16.0f;  // infinite reversed-Z perspective, camera looking down -z
    v.view_proj[5] = 1.0f;
    v.view_proj[11] = -1.0f;
    v.view_proj[14] = 0.01f;
    v.shadow_pass = shadow_pass;
    v.use_hiz = use_hiz;
    v.emit_records = 1;
    return v;
}

// an orthographic light looking down -y on the sheet: u = x / 12 + .5, v = (z + 22) / 12 + .5, depth = (y + 8) / 16
static const float kLight[16] = {1.0f / 6.0f, 0, 0, 0, 0, 0, 1.0f / 16.0f, 0, 0, 1.0f / 6.0f, 0, 0, 0, 22.0f / 6.0f, 0.5f, 1.0f};

static int bind_pools(Fixture& f)
{
    static const GvMeshLayout ml = {(uint32_t)offsetof(Mesh, entity), (uint32_t)offsetof(Mesh, isEnabled), (uint32_t)offsetof(Mesh, isVisible),
                                    (uint32_t)offsetof(Mesh, aabbMin), (uint32_t)offsetof(Mesh, aabbMax)};
    const GvTransformLayout tl = {(uint32_t)offsetof(Transform, entity), (uint32_t)offsetof(Transform, parent), (uint32_t)offsetof(Transform, position),
                                  (uint32_t)offsetof(Transform, scale), (uint32_t)offsetof(Transform, rotation), (uint32_t)offsetof(Transform, selfActive),
                                  (uint32_t)offsetof(Transform, ancestorsActive), (uint32_t)offsetof(Transform, modelWithAncestors)};
    TRY(gv_transform_bind(f.ctx, f.xf.data(), sizeof(Transform), (uint32_t)f.xf.size(), &tl, f.e2t.data(), (uint32_t)f.e2t.size()));
    TRY(gv_pool_bind(f.ctx, kMain, f.main.data(), sizeof(Mesh), kSlots, &ml));
    return GV_OK;
}

static const void* mask_of(GvCtx* ctx)
{
    const void *pixels = nullptr, *counts = nullptr;
    uint32_t w = 0, h = 0;
    CHECK(gv_receiver_mask_device(ctx, &pixels, &w, &h, &counts));
    return pixels;
}
static const void* occluders_of(GvCtx* ctx)
{
    const void *pixels = nullptr, *counts = nullptr;
    uint32_t w = 0, h = 0;
    CHECK(gv_occluder_depth_device(ctx, &pixels, &w, &h, &counts));
    return pixels;
}
static bool built(GvCtx* ctx, uint32_t* mips = nullptr)  // the selected pyramid
{
    uint32_t n = 0;
    const int rc = gv_hiz_mip_count(ctx, &n);
    if (rc != GV_OK && rc != GV_E_STATE)
        die(__FILE__, __LINE__, "gv_hiz_mip_count", rc, GV_E_STATE, ctx);
    if (mips)
        *mips = n;
    return rc == GV_OK;
}
static bool names(GvCtx* ctx, const char* a, const char* b)
{
    const char* text = gv_last_error(ctx);
    return std::strstr(text, a) && std::strstr(text, b);
}

// ---- 1. the error lists ------------------------------------------------------------------------------------------------------------
static void error_list()
{
    g_where = "error list";
    uint32_t rows = 0;
    {
        GvCtx* ctx = nullptr;
        EXPECT(gv_hiz_select(nullptr, 0), GV_E_ARG);
        EXPECT(gv_hiz_drop(nullptr, 0), GV_E_ARG);
        rows += 2;
    }
    Fixture f;
    GvCtx* ctx = f.ctx;
    std::vector<float> depth(64 * 32, 0.001f);
    uint32_t mips = 0;
    CHECK(gv_hiz_drop(ctx, 0));  // never built: GV_OK, selected ...
    CHECK(gv_hiz_drop(ctx, GV_MAX_PYRAMIDS - 1));  // ... or not
    CHECK(gv_hiz_select(ctx, 0));  // (a new context has 0 selected: selecting it is no change)
    CHECK(gv_hiz_build(ctx, depth.data(), 64, 32, GV_MEM_HOST));
    EXPECT(gv_hiz_select(ctx, GV_MAX_PYRAMIDS), GV_E_ARG);
    EXPECT(gv_hiz_select(ctx, 0xFFFFFFFFu), GV_E_ARG);
    EXPECT(gv_hiz_drop(ctx, GV_MAX_PYRAMIDS), GV_E_ARG);
    if (!built(ctx, &mips) || mips != 7)  // nothing changed: pyramid 0 is still the selected one, and built
        die(__FILE__, __LINE__, "a refused select or drop changed the selection", (long)mips, 7, ctx);
    rows += 5;
    CHECK(bind_pools(f));
    const GvView plain[2] = {make_view(0), make_view(0, 0)};
    CHECK(gv_cull(ctx, kMain, plain, 2));
    uint32_t before = 0, after = 0;
    CHECK(gv_pool_result_count(ctx, kMain, 1, &before));
    const GvView unbuilt[3] = {make_view(1), make_view(0, 0), make_view(4, 1)};
    EXPECT(gv_cull(ctx, kMain, unbuilt, 3), GV_E_STATE);
    if (!names(ctx, "view 2", "pyramid 3"))
        die(__FILE__, __LINE__, "the message names the view and the pyramid", 0, 1, ctx);
    const GvView last[1] = {make_view(GV_MAX_PYRAMIDS)};
    EXPECT(gv_cull(ctx, kMain, last, 1), GV_E_STATE);
    if (!names(ctx, "view 0", "pyramid 7"))
        die(__FILE__, __LINE__, "the message names the view and the pyramid", 0, 1, ctx);
    const GvView second = make_view(3);
    EXPECT(gv_pool_cull_second_phase(ctx, kMain, 0, 1, &second), GV_E_STATE);
    if (!names(ctx, "view 1", "pyramid 2"))
        die(__FILE__, __LINE__, "the message names the view and the pyramid", 0, 1, ctx);
    CHECK(gv_pool_result_count(ctx, kMain, 1, &after));  // the pool's previous results are still fetchable
    if (after != before)
        die(__FILE__, __LINE__, "a refused cull replaced the results", (long)after, (long)before, ctx);
    const GvView beyond[2] = {make_view(200), make_view(GV_MAX_PYRAMIDS + 1, 0)};  // any larger value: pyramid 0
    CHECK(gv_cull(ctx, kMain, beyond, 2));
    rows += 4;
    std::printf("error list: %u rows as pinned, a refused call changes nothing: ok\n", rows);
}

// ---- 2. lifetimes ----------------------------------------------------------------------------------------------------------------------
static void lifetimes()
{
    g_where = "lifetimes";
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    std::vector<float> a(64 * 32, 0.001f), b(20 * 9, 0.002f), c(1, 0.00001f);  // (c: an occluder 1000 units away, behind the sheet)
    uint32_t mips = 0;
    CHECK(gv_hiz_build(ctx, a.data(), 64, 32, GV_MEM_HOST));  // slot 0: 7 levels
    CHECK(gv_hiz_select(ctx, 2));
    if (built(ctx))
        die(__FILE__, __LINE__, "slot 2 before its first build", 1, 0, ctx);
    EXPECT(gv_hiz_rebuild(ctx), GV_E_STATE);
    CHECK(gv_hiz_build(ctx, b.data(), 20, 9, GV_MEM_HOST));  // slot 2: 5 levels
    CHECK(gv_hiz_select(ctx, 7));
    CHECK(gv_hiz_build(ctx, c.data(), 1, 1, GV_MEM_HOST));  // slot 7: 1 level
    const uint32_t want[GV_MAX_PYRAMIDS] = {7, 0, 5, 0, 0, 0, 0, 1};
    for (uint32_t round = 0; round < 2; round++)
        for (uint32_t k = 0; k < GV_MAX_PYRAMIDS; k++) {
            CHECK(gv_hiz_select(ctx, (k * 3) % GV_MAX_PYRAMIDS));  // (in another order than they were built in)
            const uint32_t slot = (k * 3) % GV_MAX_PYRAMIDS;
            if (built(ctx, &mips) != (want[slot] != 0) || mips != want[slot])
                die(__FILE__, __LINE__, "a slot's pyramid after other slots were selected and built", (long)mips, (long)want[slot], ctx);
            if (want[slot])
                CHECK(gv_hiz_rebuild(ctx));
        }
    // every view against the pyramid it names, batched (one camera position) and not; whichever slot is selected
    CHECK(gv_hiz_select(ctx, 4));
    GvView views[4] = {make_view(1), make_view(3, 0), make_view(0, 1), make_view(8, 2)};
    CHECK(gv_cull(ctx, kMain, views, 4));
    views[2].camera_position[0] = 1.0f;
    CHECK(gv_cull(ctx, kMain, views, 4));
    GvResult r{};
    CHECK(gv_pool_results_fetch(ctx, kMain, 3, 0, &r));
    if (kDevice && r.draw_count == 0)
        die(__FILE__, __LINE__, "draws of a view against a far pyramid", 0, 1, ctx);
    // drops: a parked slot, the selected slot; the others stay
    CHECK(gv_hiz_drop(ctx, 2));
    CHECK(gv_hiz_select(ctx, 2));
    if (built(ctx))
        die(__FILE__, __LINE__, "a dropped (parked) slot is still built", 1, 0, ctx);
    EXPECT(gv_cull(ctx, kMain, views, 4), GV_E_STATE);  // view 1 names it
    CHECK(gv_hiz_build(ctx, b.data(), 20, 9, GV_MEM_HOST));  // ... and it can be built again
    CHECK(gv_cull(ctx, kMain, views, 4));
    CHECK(gv_hiz_drop(ctx, 2));  // selected this time
    if (built(ctx))
        die(__FILE__, __LINE__, "a dropped (selected) slot is still built", 1, 0, ctx);
    CHECK(gv_hiz_drop(ctx, 2));  // twice: GV_OK
    CHECK(gv_hiz_select(ctx, 0));
    if (!built(ctx, &mips) || mips != 7)
        die(__FILE__, __LINE__, "slot 0 behind the drops of slot 2", (long)mips, 7, ctx);
    CHECK(gv_hiz_select(ctx, 7));
    if (!built(ctx, &mips) || mips != 1)
        die(__FILE__, __LINE__, "slot 7 behind the drops of slot 2", (long)mips, 1, ctx);
    // a batch: a recorded cull, then a select — which launches it first
    CHECK(gv_hiz_select(ctx, 0));
    CHECK(gv_cull_batch_begin(ctx));
    const GvView one[1] = {make_view(1)};
    CHECK(gv_cull(ctx, kMain, one, 1));
    CHECK(gv_hiz_select(ctx, 3));
    CHECK(gv_hiz_build(ctx, b.data(), 20, 9, GV_MEM_HOST));
    CHECK(gv_cull_batch_end(ctx));
    CHECK(gv_pool_results_fetch(ctx, kMain, 0, 0, &r));
    std::printf("lifetimes: builds land in the selected slot, drops leave the others, views name their pyramids: ok\n");  // (destroy frees slots 0, 3, 7)
}

// ---- 3. the image-taking rule -----------------------------------------------------------------------------------------------------------
#ifdef GV_HIP_STUB
static void mark(const void* image) { std::memcpy(const_cast<void*>(image), "\x5a\x5a\x5a\x5a", 4); }  // (the stub's device memory is host memory)
static bool marked(const void* image)
{
    uint32_t w = 0;
    std::memcpy(&w, image, 4);
    return w == 0x5a5a5a5au;
}
#else
static void mark(const void*) {}
static bool marked(const void*) { return true; }
#endif

static void images()
{
    g_where = "images";
    {  // one pyramid: the two images of old, in the turn of old
        Fixture f;
        GvCtx* ctx = f.ctx;
        CHECK(bind_pools(f));
        const GvView v[1] = {make_view(0)};
        CHECK(gv_cull(ctx, kMain, v, 1));
        CHECK(gv_receiver_begin(ctx, 32, 16));
        const void* first = mask_of(ctx);
        CHECK(gv_receiver_begin(ctx, 32, 16));  // starting over: the same image
        if (mask_of(ctx) != first)
            die(__FILE__, __LINE__, "a begin on an open mask took another one", 1, 0, ctx);
        CHECK(gv_pool_draw_receivers(ctx, kMain, 0, kLight));
        CHECK(gv_hiz_build_from_receivers(ctx));
        CHECK(gv_receiver_begin(ctx, 32, 16));
        const void* second = mask_of(ctx);
        if (second == first)
            die(__FILE__, __LINE__, "a begin handed out the image the pyramid reads", 1, 0, ctx);
        CHECK(gv_receiver_begin(ctx, 48, 16));  // (larger: the same image, reallocated or not, is never the pyramid's)
        if (mask_of(ctx) == first)
            die(__FILE__, __LINE__, "a begin handed out the image the pyramid reads", 2, 0, ctx);
        CHECK(gv_receiver_begin(ctx, 32, 16));
        second = mask_of(ctx);
        CHECK(gv_hiz_build_from_receivers(ctx));
        for (int turn = 0; turn < 6; turn++) {  // from here on the two alternate, as they always did
            CHECK(gv_receiver_begin(ctx, 32, 16));
            if (mask_of(ctx) != (turn % 2 ? second : first))
                die(__FILE__, __LINE__, "one pyramid: the two images in turn", turn, 0, ctx);
            CHECK(gv_hiz_build_from_receivers(ctx));
        }
    }
    Fixture f;
    GvCtx* ctx = f.ctx;
    CHECK(bind_pools(f));
    CHECK(gv_pool_bind_occluders(ctx, kMain, f.lo.data(), f.hi.data(), 16, kSlots));
    const GvView v[1] = {make_view(0)};
    CHECK(gv_cull(ctx, kMain, v, 1));
    std::set<const void*> read;  // the images some pyramid reads
    CHECK(gv_occluder_begin(ctx, 40, 24));
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    CHECK(gv_hiz_build_from_occluders(ctx));  // pyramid 0
    const void* occluders = occluders_of(ctx);
    read.insert(occluders), mark(occluders);
    const void* masks[3];
    for (uint32_t k = 0; k < 3; k++) {
        CHECK(gv_hiz_select(ctx, 1 + k));
        CHECK(gv_receiver_begin(ctx, 64 + 8 * k, 48));
        masks[k] = mask_of(ctx);
        if (read.count(masks[k]))
            die(__FILE__, __LINE__, "a begin handed out an image some pyramid reads", (long)k, 0, ctx);
        CHECK(gv_pool_draw_receivers(ctx, kMain, 0, kLight));
        CHECK(gv_hiz_build_from_receivers(ctx));
        EXPECT(gv_pool_draw_receivers(ctx, kMain, 0, kLight), GV_E_STATE);  // the build closed it
        read.insert(masks[k]), mark(masks[k]);
    }
    if (read.size() != 4)
        die(__FILE__, __LINE__, "three masks and an occluder image: distinct images", (long)read.size(), 4, ctx);
    // a fourth mask, three sizes, draws; and a second occluder image beside the one pyramid 0 reads
    CHECK(gv_hiz_select(ctx, 4));
    const uint32_t sizes[][2] = {{64, 48}, {512, 300}, {1, 1}};
    for (const auto& s : sizes) {
        CHECK(gv_receiver_begin(ctx, s[0], s[1]));
        if (read.count(mask_of(ctx)))
            die(__FILE__, __LINE__, "the fourth begin handed out an image some pyramid reads", (long)s[0], 0, ctx);
        CHECK(gv_pool_draw_receivers(ctx, kMain, 0, kLight));
    }
    CHECK(gv_occluder_begin(ctx, 700, 300));
    if (read.count(occluders_of(ctx)))
        die(__FILE__, __LINE__, "an occluder begin handed out an image some pyramid reads", 1, 0, ctx);
    CHECK(gv_pool_draw_occluders(ctx, kMain, 0, 1));
    for (const void* image : read)
        if (!marked(image))
            die(__FILE__, __LINE__, "an image a pyramid reads was cleared or replaced under it", 0, 1, ctx);
    for (uint32_t k = 0; k < 4; k++) {  // every pyramid still rebuilds from its image
        CHECK(gv_hiz_select(ctx, k));
        CHECK(gv_hiz_rebuild(ctx));
    }
    // a caller who builds slot 5 from the open mask's pointer himself closes it, as always
    CHECK(gv_hiz_select(ctx, 5));
    const void* fourth = mask_of(ctx);
    CHECK(gv_hiz_build(ctx, static_cast<const float*>(fourth), 1, 1, GV_MEM_DEVICE));
    EXPECT(gv_pool_draw_receivers(ctx, kMain, 0, kLight), GV_E_STATE);
    CHECK(gv_receiver_begin(ctx, 8, 8));
    const void* fifth = mask_of(ctx);
    if (fifth == fourth || read.count(fifth))
        die(__FILE__, __LINE__, "a begin handed out the image the caller's own gv_hiz_build adopted", 1, 0, ctx);
    // drops release the reference, not the image: the open mask stays the open one; once built, the next begin takes the LOWEST free image
    CHECK(gv_hiz_drop(ctx, 1));  // mask 0 is free (parked slot)
    CHECK(gv_hiz_drop(ctx, 5));  // the fourth is free (selected slot)
    CHECK(gv_receiver_begin(ctx, 8, 8));
    if (mask_of(ctx) != fifth)
        die(__FILE__, __LINE__, "a begin left an open mask that no pyramid reads", 1, 0, ctx);
    CHECK(gv_hiz_build_from_receivers(ctx));  // slot 5 reads the fifth
    CHECK(gv_receiver_begin(ctx, 64, 48));
    if (mask_of(ctx) != masks[0])
        die(__FILE__, __LINE__, "the lowest image no pyramid reads: the dropped pyramid's", 1, 0, ctx);
    if (!marked(masks[1]) || !marked(masks[2]) || !marked(occluders))
        die(__FILE__, __LINE__, "an image a pyramid reads was cleared or replaced under it", 0, 1, ctx);
    std::printf("images: one pyramid takes the two images of old in turn; three masks, an occluder image and a fourth mask alive at once, "
                "every image a pyramid reads untouched; a drop frees the reference alone: ok\n");
}

// ---- 4. allocation failures -----------------------------------------------------------------------------------------------------------
#ifdef GV_HIP_STUB
static int frame(Fixture& f)
{
    GvCtx* ctx = f.ctx;
    std::vector<float> depth(64 * 32, 0.001f);
    const GvView main_only[1] = {make_view(0)};
    TRY(gv_hiz_select(ctx, 0));
    TRY(gv_hiz_build(ctx, depth.data(), 64, 32, GV_MEM_HOST));
    TRY(gv_cull(ctx, kMain, main_only, 1));
    for (uint32_t k = 0; k < 2; k++) {
        TRY(gv_hiz_select(ctx, 1 + k));
        TRY(gv_receiver_begin(ctx, 96 + 32 * k, 64));
        TRY(gv_pool_draw_receivers(ctx, kMain, 0, kLight));
        TRY(gv_hiz_build_from_receivers(ctx));
    }
    TRY(gv_hiz_select(ctx, 0));
    const GvView all[3] = {make_view(1), make_view(2, 0), make_view(3, 1)};
    TRY(gv_cull(ctx, kMain, all, 3));
    GvResult r{};
    TRY(gv_pool_results_fetch(ctx, kMain, 2, 0, &r));
    TRY(gv_hiz_drop(ctx, 2));
    TRY(gv_hiz_drop(ctx, 1));
    TRY(gv_hiz_drop(ctx, 0));
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
        const long before = gv_stub_allocations();
        CHECK(frame(f));
        total = gv_stub_allocations() - before;
    }
    if (total < 12)
        die(__FILE__, __LINE__, "allocations of a frame", total, 12, nullptr);
    for (long k = 1; k <= total; k++) {
        Fixture f;
        GvCtx* ctx = f.ctx;
        CHECK(bind_pools(f));
        gv_stub_fail_countdown() = k;
        const int rc = frame(f);
        gv_stub_fail_countdown() = 0;
        if (rc != GV_E_OOM)
            die(__FILE__, __LINE__, "a frame whose k-th allocation fails", rc, GV_E_OOM, ctx);
        CHECK(frame(f));  // the same context completes the sequence
        CHECK(frame(f));  // ... and once more, over the buffers it kept
    }
    std::printf("allocation failures in the frame of three pyramids: %ld allocations, each failed once, every context completed the sequence: ok\n", total);
}
#endif

int main()
{
    error_list();
    lifetimes();
    images();
#ifdef GV_HIP_STUB
    allocation_failures();
#endif
    std::printf("pyramid slots: ok\n");
    return 0;
}
