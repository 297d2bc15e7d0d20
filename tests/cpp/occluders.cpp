// occluders.cpp — TEST driver of host/occluders.hpp (GpuOccluders) with host/second_phase.hpp: one HEADLESS frame per tick of an
// ecsm_lite world of an Opaque (unsorted) mesh system and a Translucent one, a hundredth of the opaque meshes being wide slabs with an
// occluder box at 0.9 of their aabb. Nobody hands the drop-in a depth image; per tick:
//   manager.update()                       1. cull: the drop-in delivers list 1 (tick 0: frustum only; later: last tick's pyramid)
//   begin, draw(opaque, light pass)        2. the occluders among list 1 into a 256 x 128 image on the device
//   build()                                3. the pyramid of that image
//   GpuSecondPhase::run(p, true)           4. the newly visible records against the new pyramid, isVisible = the union
// and the check, against the CPU reference-path system (oracle/cpu_mesh_render_system.hpp: the oracle's scalar cull, pyramid and
// Hi-Z query, nothing of the library): in front of step 1 it culls the same world against the pyramid it was handed last tick, and
// its list must be list 1 record for record; behind step 4 the fetched image is handed to it (CpuMeshRenderSystem::setHizDepth), it
// culls again — nothing moved — and delivers list 2, and a host loop over the two lists must give the shim's records field by field
// (floats as bits; both sides ordered by component) and the union in the isVisible bytes. Over the run the image must hold depth,
// the pyramid must cull something the frustum keeps, and some components must be new, some gone and some in both lists.
// Built by tests/cpp/occluders.mk (links the oracle: tests only), run by tests/test_occluders_host.py.
//
//   occluders [--entities N] [--ticks T]
// Prints one JSON line and, when everything held, "occluders ok".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/host/occluders.hpp"
#include "../../garden_amd/csrc/host/second_phase.hpp"
#include "../../oracle/cpu_mesh_render_system.hpp"

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

static std::vector<UnsortedMesh> listOf(const UnsortedBuffer* buffer)
{
    return std::vector<UnsortedMesh>(buffer->meshes(), buffer->meshes() + buffer->drawCount);
}

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
        auto translucent = manager.createSystem<TranslucentMeshSystem>();
        manager.registerComponents<TranslucentMeshComponent>(translucent);
        const float side = 8.0f * std::cbrt((float)entities);
        CpuMeshRenderSystem* cpu = manager.createSystem<CpuMeshRenderSystem>();
        GpuVisibilitySystem* gpu = manager.createSystem<GpuVisibilitySystem>(0);
        manager.initialize();

        Rng rng;
        std::vector<ID<Entity>> ents;
        for (uint32_t i = 0; i < entities; i++) {
            auto e = manager.createEntity();
            ents.push_back(e);
            auto t = transformSystem->add(e);
            t->setPosition(rng.uniform(-0.5f * side, 0.5f * side), rng.uniform(-0.5f * side, 0.5f * side), rng.uniform(-0.5f * side, 0.5f * side));
            const bool slab = i % 100 == 0;  // (opaque: i % 4 == 0)
            if (slab)
                t->setScale(1.0f, 1.0f, 1.0f);
            else
                t->setScale(rng.uniform(0.5f, 2.0f), rng.uniform(0.5f, 2.0f), rng.uniform(0.5f, 2.0f));
            t->uid = i + 1;
            MeshRenderComponent* m = i % 4 != 3 ? *opaque->add(e) : static_cast<MeshRenderComponent*>(*translucent->add(e));
            const float hx = slab ? 14.0f : rng.uniform(0.25f, 1.0f), hy = slab ? 10.0f : rng.uniform(0.25f, 1.0f), hz = slab ? 0.5f : rng.uniform(0.25f, 1.0f);
            m->aabb.min = f32x4(-hx, -hy, -hz);
            m->aabb.max = f32x4(hx, hy, hz);
            if (rng.next() % 100 == 0) m->isEnabled = false;
        }

        // camera: looks down +z, FOV 90, 16:9, near 0.01, infinite reversed-Z (camera.hpp:111-121)
        f32x4x4 viewProj;
        memset(viewProj.m, 0, sizeof(viewProj.m));
        viewProj.m[0] = 9.0f / 16.0f; viewProj.m[5] = -1.0f; viewProj.m[11] = 1.0f; viewProj.m[14] = 0.01f;
        graphicsSystem->setCamera(viewProj, f32x4(3.0f, -2.0f, 5.0f));

        GpuSecondPhase second(gpu);
        GpuOccluders occluders(gpu);
        if (!second.isSupported() || !occluders.isSupported()) {
            printf("{\"ok\": false, \"why\": \"one context reported as unsupported\"}\n");
            return 1;
        }
        const uint32_t width = 256, height = 128;
        uint64_t fresh = 0, gone = 0, both = 0, drawn = 0, covered = 0, culledByPyramid = 0;
        std::vector<float> boxMin, boxMax;  // 4 floats a component: the slabs' boxes, everybody else's empty
        for (uint32_t tick = 0; tick < ticks; tick++) {
            if (tick) {  // movers, reported one by one
                for (uint32_t k = tick % 7; k < entities; k += 7)
                    if (auto t = transformSystem->tryGetOf(ents[k])) {
                        t->posChildCount.x += 0.75f;
                        transformSystem->markMoved(ents[k]);
                    }
            }
            cpu->isEnabled = true, gpu->isEnabled = false;
            manager.update();  // the reference's list 1: frustum only on tick 0, against last tick's image afterwards
            const std::vector<UnsortedMesh> firstWanted = byComponent(listOf(cpu->getUnsortedBuffers()[0]));
            cpu->isEnabled = false, gpu->isEnabled = true;
            manager.update();  // 1. cull
            const auto& meshSystems = gpu->getMeshSystems();
            if (meshSystems.size() != 2) {
                printf("{\"ok\": false, \"why\": \"%zu mesh systems\"}\n", meshSystems.size());
                return 1;
            }
            uint32_t p = 0;
            for (uint32_t q = 0; q < 2; q++)
                if (meshSystems[q]->getMeshRenderType() == MeshRenderType::Opaque)
                    p = q;
            auto meshSystem = meshSystems[p];
            const size_t componentSize = meshSystem->getMeshComponentSize();
            const uint32_t occupancy = meshSystem->getMeshComponentPool().getOccupancy();
            const uint8_t* components = reinterpret_cast<const uint8_t*>(meshSystem->getMeshComponentPool().getData());
            if (tick == 0) {
                boxMin.assign((size_t)4 * occupancy, 0.0f);
                boxMax.assign((size_t)4 * occupancy, 0.0f);
                for (uint32_t i = 0; i < occupancy; i++) {
                    const auto* m = reinterpret_cast<const MeshRenderComponent*>(components + (size_t)i * componentSize);
                    if (m->aabb.max.x < 5.0f)
                        continue;
                    const float lo[3] = {m->aabb.min.x, m->aabb.min.y, m->aabb.min.z}, hi[3] = {m->aabb.max.x, m->aabb.max.y, m->aabb.max.z};
                    for (int k = 0; k < 3; k++)
                        boxMin[4 * i + k] = 0.9f * lo[k], boxMax[4 * i + k] = 0.9f * hi[k];
                }
                occluders.setBoxes(p, boxMin.data(), boxMax.data(), 16, occupancy);
            }
            const std::vector<UnsortedMesh> first = byComponent(listOf(gpu->getUnsortedBuffers()[0]));
            if (first.size() != firstWanted.size()) {
                printf("{\"ok\": false, \"why\": \"tick %u: list 1 holds %zu records, the CPU system's %zu\"}\n", tick, first.size(), firstWanted.size());
                return 1;
            }
            for (size_t k = 0; k < first.size(); k++)
                if (!sameRecord(first[k], firstWanted[k])) {
                    printf("{\"ok\": false, \"why\": \"tick %u: record %zu of list 1 differs from the CPU system's\"}\n", tick, k);
                    return 1;
                }
            std::vector<uint8_t> inFirst(occupancy, 0), inNew(occupancy, 0);
            for (const UnsortedMesh& m : first)
                inFirst[m.componentOffset / componentSize] = 1;
            const auto& passes = gpu->getSystemPasses(p);
            uint32_t light = 0;
            for (uint32_t v = 0; v < passes.size(); v++)
                if (passes[v] < 0)
                    light = v;

            occluders.begin(width, height);  // 2. draw
            occluders.draw(p, light);
            uint32_t w = 0, h = 0;
            const std::vector<float> image = occluders.fetch(w, h);
            if (w != width || h != height) {
                printf("{\"ok\": false, \"why\": \"tick %u: a %ux%u image\"}\n", tick, w, h);
                return 1;
            }
            drawn += occluders.counts().drawn;
            for (float d : image)
                covered += d > 0.0f;
            occluders.build();       // 3. build
            second.run(p, true);     // 4. the second phase against the new pyramid
            const std::vector<UnsortedMesh> got = byComponent(std::vector<UnsortedMesh>(second.meshes(p), second.meshes(p) + second.drawCount(p)));
            std::vector<uint8_t> visible(occupancy);
            for (uint32_t i = 0; i < occupancy; i++)
                visible[i] = reinterpret_cast<const MeshRenderComponent*>(components + (size_t)i * componentSize)->isVisible ? 1 : 0;

            cpu->setHizDepth(image.data(), width, height);  // the CPU path, fed the fetched image
            cpu->isEnabled = true, gpu->isEnabled = false;
            manager.update();                               // nothing moved: its full cull against that image
            cpu->isEnabled = false, gpu->isEnabled = true;
            const std::vector<UnsortedMesh> full = byComponent(listOf(cpu->getUnsortedBuffers()[0]));
            std::vector<UnsortedMesh> expected;
            for (const UnsortedMesh& m : full) {
                const size_t slot = m.componentOffset / componentSize;
                if (inFirst[slot]) {
                    both++;
                } else {
                    expected.push_back(m);
                    inNew[slot] = 1;
                    fresh++;
                }
            }
            gone += first.size() - (full.size() - expected.size());
            if (tick == 0)
                culledByPyramid = first.size() - full.size();  // (list 1 was frustum only)
            if (got.size() != expected.size() || second.instanceCount(p) != expected.size()) {
                printf("{\"ok\": false, \"why\": \"tick %u: %zu new records, the host loop has %zu\"}\n", tick, got.size(), expected.size());
                return 1;
            }
            for (size_t k = 0; k < got.size(); k++)
                if (!sameRecord(got[k], expected[k])) {
                    printf("{\"ok\": false, \"why\": \"tick %u: record %zu differs from the host loop\"}\n", tick, k);
                    return 1;
                }
            for (uint32_t i = 0; i < occupancy; i++)
                if (visible[i] != (inFirst[i] | inNew[i])) {
                    printf("{\"ok\": false, \"why\": \"tick %u: isVisible of component %u is %u, the union says %u\"}\n", tick, i, visible[i],
                           inFirst[i] | inNew[i]);
                    return 1;
                }
        }
        const bool ok = drawn && covered && culledByPyramid && fresh && gone && both;
        printf("{\"ok\": %s, \"ticks\": %u, \"occluders_drawn\": %llu, \"covered_pixels\": %llu, \"culled_by_the_pyramid\": %llu, \"new\": %llu, "
               "\"gone\": %llu, \"both\": %llu}\n", ok ? "true" : "false", ticks, (unsigned long long)drawn, (unsigned long long)covered,
               (unsigned long long)culledByPyramid, (unsigned long long)fresh, (unsigned long long)gone, (unsigned long long)both);
        if (ok)
            printf("occluders ok\n");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        printf("{\"ok\": false, \"why\": \"%s\"}\n", e.what());
        return 1;
    }
}
