// receivers.cpp — TEST driver of host/shadow_receivers.hpp (GpuShadowReceivers): HEADLESS ticks of an ecsm_lite world of one Opaque
// mesh system — small boxes around and over a floor slab — with the main pass and three shadow cascades (csm::cascade over the
// camera's slices, csm_lite.hpp). Per tick:
//   manager.update()                          the drop-in culls the main pass and the three cascades, frustum only, in one batch
//   per cascade k: begin, draw(p, main pass, cascade k), build, cull(p, k)
//                                             the main pass's receivers into a 256 x 256 mask on the device, its pyramid, and the
//                                             cascade culled again against it
// and the check, against the host path (the oracle's scalar cull, pyramid and Hi-Z query: gvo_prepare_meshes over the same pools,
// nothing of the library): the drop-in's frustum-only list of every cascade must be the host's, record for record; the mask fetched
// from the device is handed to the host path (gvo_hiz_build, the reference rule), which culls cascade k with the query on, and its
// list must be the shim's record for record (floats as bits; both sides ordered by component). Every record of the main pass's list
// must be counted in exactly one class of the mask; what the main pass and a cascade's frustum both hold must survive the masked cull;
// and over the run the masked culls must have dropped casters the frustum-only culls kept.
// Built by tests/cpp/receivers.mk (links the oracle: tests only), run by tests/test_receivers_host.py.
//
//   receivers [--entities N] [--ticks T]
// Prints one JSON line and, when everything held, "receivers ok".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/host/shadow_receivers.hpp"
#include "../../oracle/gv_oracle.h"

using namespace garden;

struct Rng {  // PCG32
    uint64_t state = 0x853c49e6748fea9bull, inc = 0xda3e39cb94b95bdbull;
    uint32_t next()
    {
        uint64_t old = state;
        state = old * 6364136223846793005ull + (inc | 1);
        uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u), rot = (uint32_t)(old >> 59u);
        return (xs >> rot) | (xs << ((-rot) & 31));
    }
    float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(next() >> 8) * (1.0f / 16777216.0f); }
};

static std::vector<UnsortedMesh> byComponent(std::vector<UnsortedMesh> list)
{
    std::sort(list.begin(), list.end(), [](const UnsortedMesh& a, const UnsortedMesh& b) { return a.componentOffset < b.componentOffset; });
    return list;
}

static bool sameRecord(const UnsortedMesh& a, const UnsortedMesh& b)
{
    return a.componentOffset == b.componentOffset && memcmp(a.bakedModel.m, b.bakedModel.m, 48) == 0 &&
           memcmp(&a.distanceSq, &b.distanceSq, 4) == 0;
}

// the host path: one prepareMeshes dispatch of the oracle over the system's pools, as oracle/cpu_mesh_render_system.hpp issues it
struct HostPath {
    GvoMeshPool mp{};
    GvoTransformPool tp{};
    std::vector<uint32_t> idx;
    std::vector<float> baked, dist;
    GvoHiz hiz{};
    std::vector<float> depth, mips;

    void bind(IMeshRenderSystem* meshSystem)
    {
        const auto& pool = meshSystem->getMeshComponentPool();
        mp.base = reinterpret_cast<uint8_t*>(pool.getData());
        mp.stride = meshSystem->getMeshComponentSize();
        mp.occupancy = pool.getOccupancy();
        mp.off_entity = offsetof(MeshRenderComponent, entity);
        mp.off_is_enabled = offsetof(MeshRenderComponent, isEnabled);
        mp.off_is_visible = offsetof(MeshRenderComponent, isVisible);
        mp.off_aabb_min = offsetof(MeshRenderComponent, aabb.min);
        mp.off_aabb_max = offsetof(MeshRenderComponent, aabb.max);
        auto transformSystem = TransformSystem::Instance::get();
        auto& tpool = transformSystem->getComponents();
        auto& emap = transformSystem->getEntityMap();
        tp.base = reinterpret_cast<const uint8_t*>(tpool.getData());
        tp.stride = sizeof(TransformComponent);
        tp.occupancy = tpool.getOccupancy();
        tp.off_entity = offsetof(TransformComponent, entity);
        tp.off_parent = offsetof(TransformComponent, parent);
        tp.off_position = offsetof(TransformComponent, posChildCount);
        tp.off_scale = offsetof(TransformComponent, scaleChildCap);
        tp.off_rotation = offsetof(TransformComponent, rotation);
        tp.off_self_active = offsetof(TransformComponent, selfActive);
        tp.off_ancestors_active = offsetof(TransformComponent, ancestorsActive);
        tp.off_model_with_ancestors = offsetof(TransformComponent, modelWithAncestors);
        tp.entity_to_transform = emap.data();
        tp.entity_capacity = (uint32_t)emap.size();
    }
    void setMask(const std::vector<float>& image, uint32_t width, uint32_t height)
    {
        depth = image;
        const uint64_t pairs = gvo_hiz_layout(width, height, &hiz);
        mips.assign((size_t)pairs * 2 + 2, 0.0f);
        hiz.depth = depth.data();
        hiz.mips = mips.data();
        gvo_hiz_build(&hiz, mips.data(), GVO_HIZ_RULE_REFERENCE);
    }
    // the cull of `view` as the library was given it; shadow passes leave isVisible alone (mesh.cpp:121)
    std::vector<UnsortedMesh> cull(const GvView& view, bool masked)
    {
        GvoView v{};
        memcpy(v.view_proj, view.view_proj, sizeof(v.view_proj));
        memcpy(v.camera_position, view.camera_position, sizeof(v.camera_position));
        memcpy(v.camera_offset, view.camera_offset, sizeof(v.camera_offset));
        v.shadow_pass = view.shadow_pass;
        v.use_hiz = masked ? 1 : 0;
        const size_t n = mp.occupancy ? mp.occupancy : 1;
        idx.resize(n), baked.resize(n * 12), dist.resize(n);
        GvoCullOut out{idx.data(), baked.data(), dist.data(), 0, 0};
        gvo_prepare_meshes(&mp, &tp, &v, masked ? &hiz : nullptr, 1, &out);
        std::vector<UnsortedMesh> list(out.draw_count);
        for (uint32_t k = 0; k < out.draw_count; k++) {
            list[k].componentOffset = (size_t)idx[k] * mp.stride;
            memcpy(list[k].bakedModel.m, baked.data() + (size_t)k * 12, 48);
            list[k].distanceSq = dist[k];
        }
        return list;
    }
};

#define FAIL(...)                              \
    do {                                       \
        printf("{\"ok\": false, \"why\": \""); \
        printf(__VA_ARGS__);                   \
        printf("\"}\n");                       \
        return 1;                              \
    } while (0)

int main(int argc, char** argv)
{
    uint32_t entities = 20000, ticks = 5;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--entities" && i + 1 < argc) entities = (uint32_t)atoi(argv[++i]);
        else if (a == "--ticks" && i + 1 < argc) ticks = (uint32_t)atoi(argv[++i]);
    }
    try {
        Manager manager;
        auto transformSystem = manager.createSystem<TransformSystem>();
        manager.registerComponents<TransformComponent>(transformSystem);
        auto graphicsSystem = manager.createSystem<GraphicsSystem>();
        manager.createSystem<DeferredRenderSystem>();
        auto opaque = manager.createSystem<OpaqueMeshSystem>();
        manager.registerComponents<MeshRenderComponent>(opaque);
        GpuVisibilitySystem* gpu = manager.createSystem<GpuVisibilitySystem>(0);
        manager.initialize();

        // entities of 1 - 6 units in x -320 .. 320, y 0.5 .. 40, z -40 .. 320; entity 0 is the floor slab: x -150 .. 150, y -2 .. 0, z -20 .. 280
        Rng rng;
        std::vector<ID<Entity>> ents;
        for (uint32_t i = 0; i < entities; i++) {
            auto e = manager.createEntity();
            ents.push_back(e);
            auto t = transformSystem->add(e);
            if (i == 0) {
                t->setPosition(0.0f, -1.0f, 130.0f);
                t->setScale(150.0f, 1.0f, 150.0f);
            } else {
                t->setPosition(rng.uniform(-320.0f, 320.0f), rng.uniform(0.5f, 40.0f), rng.uniform(-40.0f, 320.0f));
                t->setScale(rng.uniform(1.0f, 6.0f), rng.uniform(1.0f, 6.0f), rng.uniform(1.0f, 6.0f));
            }
            t->uid = i + 1;
            MeshRenderComponent* m = *opaque->add(e);
            const float h = i == 0 ? 1.0f : rng.uniform(0.25f, 1.0f);
            m->aabb.min = f32x4(-h, -h, -h);
            m->aabb.max = f32x4(h, h, h);
            if (i && rng.next() % 100 == 0) m->isEnabled = false;
        }

        // camera: at (0, 8, -20), looks down +z, FOV 60, 16:9, near 0.1, infinite reversed-Z (camera.hpp:111-121)
        const float fov = 1.0471975512f, aspect = 16.0f / 9.0f, nearPlane = 0.1f;
        const float f = 1.0f / std::tan(0.5f * fov);
        f32x4x4 viewProj;
        memset(viewProj.m, 0, sizeof(viewProj.m));
        viewProj.m[0] = f / aspect; viewProj.m[5] = -f; viewProj.m[11] = 1.0f; viewProj.m[14] = nearPlane;
        graphicsSystem->setCamera(viewProj, f32x4(0.0f, 8.0f, -20.0f));

        // three cascades over the slices of the first 300 units (csm.cpp:318-324), the view's translation zeroed (graphics.cpp:201)
        const uint32_t cascadeCount = 3;
        const float splits[2] = {0.15f, 0.45f};
        f32x4x4 view;  // identity: the camera looks down +z
        std::vector<csm::Cascade> cascades;
        std::vector<GpuVisibilitySystem::ShadowPass> shadowPasses;
        for (uint32_t k = 0; k < cascadeCount; k++) {
            cascades.push_back(csm::cascade(k, cascadeCount, splits, 300.0f, view, f32x4(0.1f, -1.0f, 0.3f), fov, aspect, nearPlane, 10.0f, 2048));
            GpuVisibilitySystem::ShadowPass pass;
            pass.viewProj = cascades[k].viewProj;
            pass.cameraOffset = cascades[k].cameraOffset;
            shadowPasses.push_back(pass);
        }
        gpu->setShadowPasses(shadowPasses);

        GpuShadowReceivers receivers(gpu);
        if (!receivers.isSupported())
            FAIL("one context reported as unsupported");
        const uint32_t width = 256, height = 256;
        HostPath host;
        uint64_t dropped = 0, keptPlain = 0, keptMasked = 0, receiversDrawn = 0, selfKept = 0, emptyTexels = 0;
        uint64_t plainOf[3] = {0, 0, 0}, maskedOf[3] = {0, 0, 0};  // per cascade, over the run
        for (uint32_t tick = 0; tick < ticks; tick++) {
            if (tick) {  // movers, reported one by one
                for (uint32_t k = 1 + tick % 7; k < entities; k += 7)
                    if (auto t = transformSystem->tryGetOf(ents[k])) {
                        t->posChildCount.x += 0.75f;
                        transformSystem->markMoved(ents[k]);
                    }
            }
            manager.update();  // the main pass and the three cascades, frustum only
            if (gpu->getMeshSystems().size() != 1)
                FAIL("%zu mesh systems", gpu->getMeshSystems().size());
            const uint32_t p = 0;
            auto meshSystem = gpu->getMeshSystems()[p];
            const size_t componentSize = meshSystem->getMeshComponentSize();
            const uint32_t occupancy = meshSystem->getMeshComponentPool().getOccupancy();
            host.bind(meshSystem);
            const uint32_t mainView = receivers.passView(p, -1);
            const std::vector<UnsortedMesh> mainWanted = byComponent(host.cull(gpu->getSystemView(p, mainView), false));
            std::vector<UnsortedMesh> mainList(gpu->getUnsortedBuffers()[0]->meshes(), gpu->getUnsortedBuffers()[0]->meshes() + gpu->getUnsortedBuffers()[0]->drawCount);
            mainList = byComponent(mainList);
            if (mainList.size() != mainWanted.size())
                FAIL("tick %u: the main pass holds %zu records, the host path's %zu", tick, mainList.size(), mainWanted.size());
            for (size_t k = 0; k < mainList.size(); k++)
                if (!sameRecord(mainList[k], mainWanted[k]))
                    FAIL("tick %u: record %zu of the main pass differs from the host path's", tick, k);
            std::vector<uint8_t> inMain(occupancy, 0);
            for (const UnsortedMesh& m : mainList)
                inMain[m.componentOffset / componentSize] = 1;

            for (uint32_t k = 0; k < cascadeCount; k++) {
                const uint32_t cascadeView = receivers.passView(p, (int8_t)k);
                const GvView systemView = gpu->getSystemView(p, cascadeView);
                if (memcmp(systemView.view_proj, cascades[k].viewProj.m, 64) != 0 || memcmp(systemView.camera_position, gpu->getSystemView(p, mainView).camera_position, 12) != 0)
                    FAIL("tick %u: cascade %u is not culled with its own matrix and the main camera's position", tick, k);
                // the drop-in's frustum-only list of the cascade against the host path's
                const std::vector<UnsortedMesh> plainWanted = byComponent(host.cull(systemView, false));
                const UnsortedBuffer* shadowBuffer = gpu->getShadowBuffers(0).at(k);
                const std::vector<UnsortedMesh> plain = byComponent(std::vector<UnsortedMesh>(shadowBuffer->meshes(), shadowBuffer->meshes() + shadowBuffer->drawCount));
                if (plain.size() != plainWanted.size())
                    FAIL("tick %u: cascade %u holds %zu records frustum only, the host path's %zu", tick, k, plain.size(), plainWanted.size());
                for (size_t i = 0; i < plain.size(); i++)
                    if (!sameRecord(plain[i], plainWanted[i]))
                        FAIL("tick %u: record %zu of cascade %u, frustum only, differs from the host path's", tick, i, k);

                receivers.begin(width, height);
                receivers.draw(p, receivers.passView(p, -1), cascades[k]);
                uint32_t w = 0, h = 0;
                const std::vector<float> mask = receivers.fetch(w, h);
                if (w != width || h != height)
                    FAIL("tick %u: a %ux%u mask", tick, w, h);
                const GvReceiverCounts counts = receivers.counts();
                if ((uint64_t)counts.drawn + counts.flat + counts.behind + counts.range + counts.outside != mainList.size() || counts.reserved)
                    FAIL("tick %u: cascade %u: %u + %u + %u + %u + %u records classed, the main pass holds %zu", tick, k, counts.drawn, counts.flat,
                         counts.behind, counts.range, counts.outside, mainList.size());
                receiversDrawn += counts.drawn;
                for (float d : mask)
                    emptyTexels += std::isinf(d) ? 1 : 0;
                receivers.build();
                receivers.cull(p, (int8_t)k);
                const std::vector<UnsortedMesh> got = byComponent(std::vector<UnsortedMesh>(receivers.meshes(), receivers.meshes() + receivers.drawCount()));

                host.setMask(mask, width, height);  // the host path, fed the fetched mask
                const std::vector<UnsortedMesh> wanted = byComponent(host.cull(systemView, true));
                if (got.size() != wanted.size())
                    FAIL("tick %u: cascade %u holds %zu records against the mask, the host path's %zu", tick, k, got.size(), wanted.size());
                std::vector<uint8_t> inMasked(occupancy, 0);
                for (size_t i = 0; i < got.size(); i++) {
                    if (!sameRecord(got[i], wanted[i]))
                        FAIL("tick %u: record %zu of cascade %u against the mask differs from the host path's", tick, i, k);
                    inMasked[got[i].componentOffset / componentSize] = 1;
                }
                for (const UnsortedMesh& m : plain) {  // self-keeping
                    const size_t slot = m.componentOffset / componentSize;
                    if (inMain[slot] && !inMasked[slot])
                        FAIL("tick %u: cascade %u dropped component %zu, which the main pass sees", tick, k, slot);
                    selfKept += inMain[slot];
                }
                plainOf[k] += plain.size(), maskedOf[k] += got.size();
                keptPlain += plain.size();
                keptMasked += got.size();
                dropped += plain.size() - got.size();
            }
        }
        const bool ok = dropped && keptMasked && receiversDrawn && selfKept && emptyTexels;
        printf("{\"ok\": %s, \"ticks\": %u, \"cascades\": %u, \"kept_frustum_only\": %llu, \"kept_masked\": %llu, \"dropped\": %llu, "
               "\"receivers_drawn\": %llu, \"kept_because_the_main_pass_sees_them\": %llu, \"texels_without_receiver\": %llu, "
               "\"kept_frustum_only_per_cascade\": [%llu, %llu, %llu], \"kept_masked_per_cascade\": [%llu, %llu, %llu]}\n",
               ok ? "true" : "false", ticks, cascadeCount, (unsigned long long)keptPlain, (unsigned long long)keptMasked, (unsigned long long)dropped,
               (unsigned long long)receiversDrawn, (unsigned long long)selfKept, (unsigned long long)emptyTexels, (unsigned long long)plainOf[0],
               (unsigned long long)plainOf[1], (unsigned long long)plainOf[2], (unsigned long long)maskedOf[0], (unsigned long long)maskedOf[1],
               (unsigned long long)maskedOf[2]);
        if (ok)
            printf("receivers ok\n");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        printf("{\"ok\": false, \"why\": \"%s\"}\n", e.what());
        return 1;
    }
}
