// pick_select.cpp — TEST driver of host/mesh_selector.hpp: an ecsm_lite world of Opaque, Translucent and UI mesh systems with a
// hierarchy, one tick of the GpuVisibilitySystem drop-in, then GpuMeshSelector::select for many cursor positions, with no selection
// and with the entity just selected, each against a CPU restatement of the selector's loop (mesh-selector.cpp:78-122) through the
// picking twin (tests/pick_twin.h) and the oracle's calcModel. Built and run by tests/test_gpu_pick.py.
//
//   pick_select [--entities N] [--ranks R] [--cursors K]
// Prints one JSON line: ok, the number of cursors that selected something, and a checksum of every selection made.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/host/mesh_selector.hpp"
#include "../../oracle/gv_oracle.h"
#include "../pick_twin.h"

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

// One non-UI mesh entry as the selector's loop sees it, after the loop's filters (:95-100) and the cull's empty-box filter
// (DESIGN.md §4 item 8): camera-relative model (float4x3 order), box, slot, entity.
struct Entry {
    float model[12], box[6];
    uint32_t slot;
    ID<Entity> entity;
};

int main(int argc, char** argv)
{
    uint32_t entities = 30000, ranks = 1, cursors = 300;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--entities" && i + 1 < argc) entities = (uint32_t)atoi(argv[++i]);
        else if (a == "--ranks" && i + 1 < argc) ranks = (uint32_t)atoi(argv[++i]);
        else if (a == "--cursors" && i + 1 < argc) cursors = (uint32_t)atoi(argv[++i]);
    }
    try {
        Manager manager;
        auto transformSystem = manager.createSystem<TransformSystem>();
        manager.registerComponents<TransformComponent>(transformSystem);
        auto graphicsSystem = manager.createSystem<GraphicsSystem>();
        manager.createSystem<DeferredRenderSystem>();
        auto opaque = manager.createSystem<OpaqueMeshSystem>();
        manager.registerComponents<MeshRenderComponent>(opaque);
        auto translucent = manager.createSystem<TranslucentMeshSystem>();
        manager.registerComponents<TranslucentMeshComponent>(translucent);
        auto ui = manager.createSystem<UiMeshSystem>();
        manager.registerComponents<UiMeshComponent>(ui);
        // a dense world: rays from the camera cross several boxes
        const float side = 8.0f * std::cbrt((float)entities);
        GpuVisibilitySystem* gpu = ranks > 1 ? manager.createSystem<GpuVisibilitySystem>(std::vector<int>(ranks, 0), (double)side)
                                             : manager.createSystem<GpuVisibilitySystem>(0);
        manager.initialize();

        Rng rng;
        std::vector<ID<Entity>> ents;
        for (uint32_t i = 0; i < entities; i++) {
            auto e = manager.createEntity();
            ents.push_back(e);
            auto t = transformSystem->add(e);
            t->setPosition(rng.uniform(-0.5f * side, 0.5f * side), rng.uniform(-0.5f * side, 0.5f * side), rng.uniform(-0.5f * side, 0.5f * side));
            t->setScale(rng.uniform(0.5f, 2.0f), rng.uniform(0.5f, 2.0f), rng.uniform(0.5f, 2.0f));
            float q[4] = {rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1)};
            const float inv = 1.0f / std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] + 1e-12f);
            t->setRotation(quat(q[0] * inv, q[1] * inv, q[2] * inv, q[3] * inv));
            t->uid = i + 1;
            // UI components in the same space, in front of the camera too: the selector must skip them (:84-85)
            MeshRenderComponent* m = i % 3 == 0 ? *opaque->add(e) : (i % 3 == 1 ? static_cast<MeshRenderComponent*>(*translucent->add(e))
                                                                             : static_cast<MeshRenderComponent*>(*ui->add(e)));
            const float hx = rng.uniform(0.25f, 1.0f), hy = rng.uniform(0.25f, 1.0f), hz = rng.uniform(0.25f, 1.0f);
            m->aabb.min = f32x4(-hx, -hy, -hz);
            m->aabb.max = f32x4(hx, hy, hz);
            const uint32_t r = rng.next() % 100;
            if (r == 0) m->isEnabled = false;
            if (r == 1) m->aabb.max = m->aabb.min;
        }
        for (uint32_t i = entities / 10; i < entities; i++) {  // a hierarchy: parents among earlier entities, small local offsets
            auto t = transformSystem->tryGetOf(ents[i]);
            t->setPosition(rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3, 3));
            transformSystem->setParent(ents[i], ents[rng.next() % (i / 4 + 1)]);
        }
        for (uint32_t i = 0; i < entities; i += 37)
            transformSystem->setActive(ents[i], false);

        // camera: looks down +z, FOV 90, 16:9, near 0.01, infinite reversed-Z (camera.hpp:111-121); invViewProj its inverse
        f32x4x4 viewProj, invViewProj;
        memset(viewProj.m, 0, sizeof(viewProj.m));
        viewProj.m[0] = 9.0f / 16.0f; viewProj.m[5] = -1.0f; viewProj.m[11] = 1.0f; viewProj.m[14] = 0.01f;
        memset(invViewProj.m, 0, sizeof(invViewProj.m));
        invViewProj.m[0] = 16.0f / 9.0f; invViewProj.m[5] = -1.0f; invViewProj.m[11] = 100.0f; invViewProj.m[14] = 1.0f;
        const f32x4 cameraPosition(3.0f, -2.0f, 5.0f);
        graphicsSystem->setCamera(viewProj, cameraPosition);
        manager.update();  // one tick: the drop-in binds and culls the pools

        // the CPU restatement's candidates, in the selector's system order (meshSystems minus UI)
        auto& tpool = transformSystem->getComponents();
        auto& emap = transformSystem->getEntityMap();
        GvoTransformPool tp{};
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
        const float cam[3] = {cameraPosition.x, cameraPosition.y, cameraPosition.z};
        std::vector<std::vector<Entry>> lists;
        for (auto meshSystem : gpu->getMeshSystems()) {
            if (meshSystem->getMeshRenderType() == MeshRenderType::UI)
                continue;
            lists.emplace_back();
            const uint32_t occupancy = meshSystem->getMeshComponentPool().getOccupancy();
            for (uint32_t i = 0; i < occupancy; i++) {
                const MeshRenderComponent* c = GpuMeshSelector::componentAt(meshSystem, i);
                if (!c->getEntity() || !c->isEnabled)  // :95-96
                    continue;
                auto t = transformSystem->tryGetOf(c->getEntity());
                if (!t || !t->isActive())  // :98-100
                    continue;
                const Aabb& b = c->aabb;
                if (b.max.x - b.min.x <= 0.0f && b.max.y - b.min.y <= 0.0f && b.max.z - b.min.z <= 0.0f)
                    continue;  // the cull's filter: nothing to hit
                Entry e;
                float m[16];
                gvo_transform_calc_model(&tp, (uint32_t)(*t - tpool.getData()), cam, m);  // calcModel(cameraPosition), :102
                const int cols[4] = {0, 4, 8, 12};
                for (int k = 0; k < 4; k++)
                    for (int r = 0; r < 3; r++)
                        e.model[3 * k + r] = m[cols[k] + r];
                const float box[6] = {b.min.x, b.min.y, b.min.z, b.max.x, b.max.y, b.max.z};
                memcpy(e.box, box, sizeof(box));
                e.slot = i;
                e.entity = c->getEntity();
                lists.back().push_back(e);
            }
        }
        // :104-116 over those candidates: the smallest (distanceSq, system, slot) that is not the selected entity
        auto cpuSelect = [&](const GvPickRay& r, ID<Entity> selected) {
            const float ray[6] = {r.origin[0], r.origin[1], r.origin[2], r.direction[0], r.direction[1], r.direction[2]};
            uint64_t best = PICK_TWIN_MISS;
            ID<Entity> chosen;
            for (uint32_t k = 0; k < lists.size(); k++)
                for (const Entry& e : lists[k]) {
                    if (e.entity == selected)
                        continue;
                    const uint64_t key = pick_twin_key(e.model, e.box, ray, (k << 28) | e.slot);
                    if (key < best)
                        best = key, chosen = e.entity;
                }
            return chosen;
        };

        GpuMeshSelector selector(gpu);
        const f32x4 window(1280.0f, 720.0f, 0.0f);
        Rng cursorRng;
        uint32_t hits = 0, reselected = 0;
        uint64_t checksum = 1469598103934665603ull;
        for (uint32_t k = 0; k < cursors; k++) {
            const f32x4 cursor((float)(cursorRng.next() % 1280), (float)(cursorRng.next() % 720), 0.0f);
            const GvPickRay ray = GpuMeshSelector::cursorRay(cursor, window, invViewProj);
            const ID<Entity> first = selector.select(cursor, window, invViewProj, cameraPosition, ID<Entity>());
            const ID<Entity> expect = cpuSelect(ray, ID<Entity>());
            if (first != expect) {
                printf("{\"ok\": false, \"why\": \"cursor %u: selected entity %u, the loop selects %u\"}\n", k, *first, *expect);
                return 1;
            }
            // clicking again with that entity selected: the next one behind it in the ordering
            const ID<Entity> second = selector.select(cursor, window, invViewProj, cameraPosition, first);
            const ID<Entity> expectSecond = cpuSelect(ray, first);
            if (second != expectSecond) {
                printf("{\"ok\": false, \"why\": \"cursor %u, %u selected: selected entity %u, the loop selects %u\"}\n", k, *first, *second,
                       *expectSecond);
                return 1;
            }
            hits += first ? 1u : 0u;
            reselected += second ? 1u : 0u;
            checksum = (checksum ^ *first) * 1099511628211ull;
            checksum = (checksum ^ *second) * 1099511628211ull;
        }
        printf("{\"ok\": true, \"ranks\": %u, \"cursors\": %u, \"hits\": %u, \"reselected\": %u, \"checksum\": \"%016llx\"}\n", ranks, cursors,
               hits, reselected, (unsigned long long)checksum);
        return 0;
    } catch (const std::exception& e) {
        printf("{\"ok\": false, \"why\": \"%s\"}\n", e.what());
        return 1;
    }
}
