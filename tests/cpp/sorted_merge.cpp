// sorted_merge.cpp — TEST driver of GpuVisibilitySystem::mergeOnDevice: an ecsm_lite world of two Translucent systems, two UI
// systems and one Opaque system with a main pass and two cascades (translucent shadow casters), animated for some ticks, goes
// through TWO GpuVisibilitySystems — one assembling the shared sorted arrays on the host (append + bufferIndex fix-up + mergeRuns),
// one on the device (gv_merge_sorted + one gv_merge_fetch per array). The world is built twice from the same seed, one system
// each (a system consumes the world's change reports, so two cannot share a world). After every tick: the draw indices, every
// buffer's counters, isVisible, and the shared arrays [0, drawIndex) must be the same bytes in both modes; and what
// prepareSortedMeshes / sortMeshes leave behind (headless_tick's sortedArraysHold, restated) holds in both.
// Built and run by tests/test_gpu_sorted_merge_shim.py.
//
//   sorted_merge [--entities N] [--ticks T] [--time]
// Prints one JSON line: ok, systems, passes, ticks, records compared. --time: the host side of the sorted delivery per tick
// (GpuVisibilitySystem::TickSeconds::sortedDelivery) and the whole prepare phase, both modes, median over the ticks after warm-up.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/host/gpu_visibility_system.hpp"

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

// five component types of different sizes, one per system
struct alignas(16) OpaqueC final : public MeshRenderComponent {};
struct alignas(16) TransA final : public MeshRenderComponent { float own[4] = {}; };
struct alignas(16) TransB final : public MeshRenderComponent { float own[8] = {}; };
struct alignas(16) UiA final : public MeshRenderComponent { float own[12] = {}; };
struct alignas(16) UiB final : public MeshRenderComponent { float own[16] = {}; };
using OpaqueSystem = MeshSystemOf<OpaqueC, MeshRenderType::Opaque>;
using TransASystem = MeshSystemOf<TransA, MeshRenderType::Translucent>;
using TransBSystem = MeshSystemOf<TransB, MeshRenderType::Translucent>;
using UiASystem = MeshSystemOf<UiA, MeshRenderType::UI>;
using UiBSystem = MeshSystemOf<UiB, MeshRenderType::UI>;

static constexpr uint32_t kPasses = 2;

// headless_tick's sortedArraysHold, restated for the shared sorted arrays: bufferIndex ownership (mesh.cpp:252,414-421), direction
// (mesh.hpp:204, mesh.cpp:296-326), sum of drawCount == the array's draw index (mesh.cpp:255-259). Empty string: holds.
static std::string sortedArraysHold(const GpuVisibilitySystem* system)
{
    auto owns = [](const MeshBuffer* buffer, size_t componentOffset, bool mustBeVisible) -> const char* {
        if (!buffer || !buffer->meshSystem)
            return "the buffer names no mesh system";
        const size_t size = buffer->meshSystem->getMeshComponentSize();
        const auto& pool = buffer->meshSystem->getMeshComponentPool();
        if (componentOffset % size != 0 || componentOffset / size >= pool.getOccupancy())
            return "componentOffset is not a component of the system the bufferIndex names";
        const auto* c = reinterpret_cast<const MeshRenderComponent*>(reinterpret_cast<const uint8_t*>(pool.getData()) + componentOffset);
        if (!*c->entity || !c->isEnabled)
            return "componentOffset names a free or disabled component";
        if (mustBeVisible && !c->isVisible)
            return "a record of the light pass names a component whose isVisible is false";
        return nullptr;
    };
    for (int ui = 0; ui < 2; ui++) {
        const auto& list = ui ? system->getUiSortedMeshes() : system->getTransSortedMeshes();
        const uint32_t n = ui ? system->getUiDrawCount() : system->getTransDrawCount();
        const std::string name = ui ? "uiSortedMeshes" : "transSortedMeshes";
        uint64_t sum = 0;
        for (uint32_t b = 0; b < system->getSortedBufferCount(); b++)
            if ((system->getSortedBuffers()[b]->meshSystem->getMeshRenderType() == MeshRenderType::UI) == (ui != 0))
                sum += system->getSortedBuffers()[b]->drawCount;
        if (sum != n || list.size() < n)
            return name + ": the buffers' drawCounts sum to " + std::to_string(sum) + ", the array's draw index is " + std::to_string(n);
        std::vector<uint32_t> perBuffer(system->getSortedBufferCount(), 0);
        for (uint32_t k = 0; k < n; k++) {
            const SortedMesh& m = list[k];
            if (m.bufferIndex >= system->getSortedBufferCount())
                return name + ": a record's bufferIndex is past sortedBuffers";
            const auto buffer = system->getSortedBuffers()[m.bufferIndex];
            if ((buffer->meshSystem->getMeshRenderType() == MeshRenderType::UI) != (ui != 0))
                return name + ": a record's bufferIndex names a system of the other kind";
            if (const char* why = owns(buffer, m.componentOffset, true))
                return name + ": record " + std::to_string(k) + ": " + why;
            perBuffer[m.bufferIndex]++;
            if (k > 0 && list[k - 1].distanceSq < m.distanceSq)
                return name + ": not in descending distanceSq order at record " + std::to_string(k);
        }
        for (uint32_t b = 0; b < system->getSortedBufferCount(); b++) {
            const auto buffer = system->getSortedBuffers()[b];
            if ((buffer->meshSystem->getMeshRenderType() == MeshRenderType::UI) == (ui != 0) && perBuffer[b] != buffer->drawCount)
                return name + ": sortedBuffers[" + std::to_string(b) + "] does not count the records that carry its index";
        }
    }
    for (uint32_t s = 0; s < kPasses; s++) {
        const auto& buffers = system->getShadowSortedBuffers(s);
        const auto& list = system->getShadowTransMeshes(s);
        const uint32_t n = system->getShadowTransDrawCount(s);
        const std::string name = "shadow pass " + std::to_string(s);
        uint64_t sum = 0;
        std::vector<uint32_t> perBuffer(buffers.size(), 0);
        for (auto buffer : buffers) {
            if (buffer->meshSystem->getMeshRenderType() != MeshRenderType::Translucent)
                return name + ": its sortedBuffers hold a system that is not Translucent";
            sum += buffer->drawCount;
        }
        if (sum != n || list.size() < n)
            return name + ": the buffers' drawCounts sum to " + std::to_string(sum) + ", the array's draw index is " + std::to_string(n);
        for (uint32_t k = 0; k < n; k++) {
            const SortedMesh& m = list[k];
            if (m.bufferIndex >= buffers.size())
                return name + ": a record's bufferIndex counts more than the Translucent systems";
            if (const char* why = owns(buffers[m.bufferIndex], m.componentOffset, false))
                return name + ": record " + std::to_string(k) + ": " + why;
            perBuffer[m.bufferIndex]++;
            if (k > 0 && list[k - 1].distanceSq < m.distanceSq)
                return name + ": not in descending distanceSq order at record " + std::to_string(k);
        }
        for (size_t b = 0; b < buffers.size(); b++)
            if (perBuffer[b] != buffers[b]->drawCount)
                return name + ": sortedBuffers[" + std::to_string(b) + "] does not count the records that carry its index";
    }
    return "";
}

// everything a tick leaves behind that the two modes must agree on, section by section
struct Snapshot {
    std::vector<std::pair<std::string, std::vector<uint8_t>>> sections;
    void add(const std::string& name, const void* data, size_t bytes)
    {
        const uint8_t* p = static_cast<const uint8_t*>(data);
        sections.emplace_back(name, std::vector<uint8_t>(p, p + bytes));
    }
    void counters(const std::string& name, const MeshBuffer* b)
    {
        const uint32_t c[2] = {b->drawCount, b->instanceCount};
        add(name, c, sizeof(c));
    }
};

static Snapshot snapshot(const GpuVisibilitySystem* gpu, uint64_t& records)
{
    Snapshot s;
    uint32_t indices[2 + kPasses] = {gpu->getTransDrawCount(), gpu->getUiDrawCount()};
    for (uint32_t p = 0; p < kPasses; p++)
        indices[2 + p] = gpu->getShadowTransDrawCount(p);
    s.add("the draw indices", indices, sizeof(indices));
    for (uint32_t b = 0; b < gpu->getSortedBufferCount(); b++)
        s.counters("sortedBuffers[" + std::to_string(b) + "]", gpu->getSortedBuffers()[b]);
    for (uint32_t b = 0; b < gpu->getUnsortedBufferCount(); b++) {
        const UnsortedBuffer* u = gpu->getUnsortedBuffers()[b];
        s.counters("unsortedBuffers[" + std::to_string(b) + "]", u);
        s.add("unsortedBuffers[" + std::to_string(b) + "] records", u->meshes(), (size_t)u->drawCount * sizeof(UnsortedMesh));
        for (uint32_t p = 0; p < kPasses; p++) {
            const UnsortedBuffer* sb = gpu->getShadowBuffers(b)[p];
            s.counters("shadowBuffers[" + std::to_string(b) + "][" + std::to_string(p) + "]", sb);
            s.add("shadowBuffers[" + std::to_string(b) + "][" + std::to_string(p) + "] records", sb->meshes(), (size_t)sb->drawCount * sizeof(UnsortedMesh));
        }
    }
    for (uint32_t p = 0; p < kPasses; p++)
        for (size_t b = 0; b < gpu->getShadowSortedBuffers(p).size(); b++)
            s.counters("shadowSortedBuffers[" + std::to_string(p) + "][" + std::to_string(b) + "]", gpu->getShadowSortedBuffers(p)[b]);
    for (size_t m = 0; m < gpu->getMeshSystems().size(); m++) {
        auto meshSystem = gpu->getMeshSystems()[m];
        const auto& pool = meshSystem->getMeshComponentPool();
        const size_t size = meshSystem->getMeshComponentSize();
        std::vector<uint8_t> visible(pool.getOccupancy());
        for (uint32_t i = 0; i < pool.getOccupancy(); i++)
            visible[i] = reinterpret_cast<const MeshRenderComponent*>(reinterpret_cast<const uint8_t*>(pool.getData()) + i * size)->isVisible ? 1 : 0;
        s.add("isVisible of mesh system " + std::to_string(m), visible.data(), visible.size());
    }
    s.add("transSortedMeshes", gpu->getTransSortedMeshes().data(), (size_t)indices[0] * sizeof(SortedMesh));
    s.add("uiSortedMeshes", gpu->getUiSortedMeshes().data(), (size_t)indices[1] * sizeof(SortedMesh));
    for (uint32_t p = 0; p < kPasses; p++)
        s.add("shadowTransMeshes[" + std::to_string(p) + "]", gpu->getShadowTransMeshes(p).data(), (size_t)indices[2 + p] * sizeof(SortedMesh));
    records += (uint64_t)indices[0] + indices[1] + indices[2] + indices[3];
    return s;
}

struct Timing {
    std::vector<double> delivery, total;  // seconds per tick
};

// one world, one system, `ticks` animated ticks; false: a check of its own failed (the JSON line has been printed)
static bool run(bool mergeOnDevice, uint32_t entities, uint32_t ticks, std::vector<Snapshot>& out, uint64_t& records, Timing& timing)
{
    Manager manager;
    auto transformSystem = manager.createSystem<TransformSystem>();
    manager.registerComponents<TransformComponent>(transformSystem);
    auto graphicsSystem = manager.createSystem<GraphicsSystem>();
    manager.createSystem<DeferredRenderSystem>();
    auto opaque = manager.createSystem<OpaqueSystem>();
    manager.registerComponents<OpaqueC>(opaque);
    auto transA = manager.createSystem<TransASystem>();
    manager.registerComponents<TransA>(transA);
    auto uiA = manager.createSystem<UiASystem>();
    manager.registerComponents<UiA>(uiA);
    auto transB = manager.createSystem<TransBSystem>();
    manager.registerComponents<TransB>(transB);
    auto uiB = manager.createSystem<UiBSystem>();
    manager.registerComponents<UiB>(uiB);
    const float side = 8.0f * std::cbrt((float)entities);
    GpuVisibilitySystem* gpu = manager.createSystem<GpuVisibilitySystem>(0);
    gpu->mergeOnDevice = mergeOnDevice;
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
        MeshRenderComponent* m;
        switch (i % 7) {  // translucent systems of unequal size, so that the runs interleave unevenly
        case 0: m = *opaque->add(e); break;
        case 1: case 2: case 3: m = *transA->add(e); break;
        case 4: m = *transB->add(e); break;
        case 5: m = *uiA->add(e); break;
        default: m = *uiB->add(e); break;
        }
        const float hx = rng.uniform(0.25f, 1.0f), hy = rng.uniform(0.25f, 1.0f), hz = rng.uniform(0.25f, 1.0f);
        m->aabb.min = f32x4(-hx, -hy, -hz);
        m->aabb.max = f32x4(hx, hy, hz);
        if (rng.next() % 100 == 0) m->isEnabled = false;
    }
    for (uint32_t i = entities / 10; i < entities; i += 2) {  // a hierarchy under half of the entities
        auto t = transformSystem->tryGetOf(ents[i]);
        t->setPosition(rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3, 3));
        transformSystem->setParent(ents[i], ents[rng.next() % (i / 4 + 1)]);
    }

    // camera: looks down +z, FOV 90, 16:9, near 0.01, infinite reversed-Z (camera.hpp:111-121)
    f32x4x4 viewProj;
    memset(viewProj.m, 0, sizeof(viewProj.m));
    viewProj.m[0] = 9.0f / 16.0f; viewProj.m[5] = -1.0f; viewProj.m[11] = 1.0f; viewProj.m[14] = 0.01f;
    graphicsSystem->setCamera(viewProj, f32x4(3.0f, -2.0f, 5.0f));
    gpu->setUiSize(side, side);
    std::vector<GpuVisibilitySystem::ShadowPass> passes;
    for (uint32_t c = 0; c < kPasses; c++) {
        const float size = side * (0.3f + 0.4f * (float)c), nearPlane = -side, farPlane = side;
        f32x4x4 vp;
        memset(vp.m, 0, sizeof(vp.m));
        vp.m[0] = 2.0f / size; vp.m[5] = -2.0f / size; vp.m[10] = -1.0f / (farPlane - nearPlane);
        vp.m[14] = farPlane / (farPlane - nearPlane); vp.m[15] = 1.0f;
        passes.push_back({vp, f32x4(3.0f * (float)(c + 1), -7.0f, 11.0f), (int8_t)c});
    }
    gpu->setShadowPasses(passes);

    for (uint32_t tick = 0; tick < ticks; tick++) {
        if (tick)
            for (uint32_t k = tick % 7; k < entities; k += 7)  // movers, reported one by one
                if (auto t = transformSystem->tryGetOf(ents[k])) {
                    t->posChildCount.x += 0.75f;
                    transformSystem->markMoved(ents[k]);
                }
        gpu->tickSeconds = {};
        manager.update();  // the prepare phase: the drop-in binds, culls, sorts and fills the engine's buffers
        timing.delivery.push_back(gpu->tickSeconds.sortedDelivery);
        timing.total.push_back(gpu->tickSeconds.total);
        if (gpu->getMeshSystems().size() != 5 || gpu->getSortedBufferCount() != 4) {
            printf("{\"ok\": false, \"why\": \"%zu mesh systems, %u sorted buffers\"}\n", gpu->getMeshSystems().size(), gpu->getSortedBufferCount());
            return false;
        }
        const std::string held = sortedArraysHold(gpu);
        if (!held.empty()) {
            printf("{\"ok\": false, \"why\": \"tick %u, mergeOnDevice %d: %s\"}\n", tick, mergeOnDevice ? 1 : 0, held.c_str());
            return false;
        }
        out.push_back(snapshot(gpu, records));
    }
    return true;
}

static double median(std::vector<double> v, size_t skip)
{
    v.erase(v.begin(), v.begin() + std::min(skip, v.size() - 1));
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv)
{
    uint32_t entities = 30000, ticks = 20;
    bool timed = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--entities" && i + 1 < argc) entities = (uint32_t)atoi(argv[++i]);
        else if (a == "--ticks" && i + 1 < argc) ticks = (uint32_t)atoi(argv[++i]);
        else if (a == "--time") timed = true;
    }
    try {
        std::vector<Snapshot> host, device;
        uint64_t hostRecords = 0, deviceRecords = 0;
        Timing hostTiming, deviceTiming;
        if (!run(false, entities, ticks, host, hostRecords, hostTiming) || !run(true, entities, ticks, device, deviceRecords, deviceTiming))
            return 1;
        for (uint32_t tick = 0; tick < ticks; tick++) {
            const auto &a = host[tick].sections, &b = device[tick].sections;
            if (a.size() != b.size()) {
                printf("{\"ok\": false, \"why\": \"tick %u: %zu sections against %zu\"}\n", tick, a.size(), b.size());
                return 1;
            }
            for (size_t k = 0; k < a.size(); k++)
                if (a[k].first != b[k].first || a[k].second != b[k].second) {
                    printf("{\"ok\": false, \"why\": \"tick %u: %s differs between the host merge and the device merge (%zu / %zu bytes)\"}\n", tick,
                           a[k].first.c_str(), a[k].second.size(), b[k].second.size());
                    return 1;
                }
        }
        if (hostRecords == 0) {
            printf("{\"ok\": false, \"why\": \"no sorted record in any tick\"}\n");
            return 1;
        }
        printf("{\"ok\": true, \"systems\": 5, \"passes\": %u, \"ticks\": %u, \"entities\": %u, \"sorted_records\": %llu", kPasses + 1, ticks, entities,
               (unsigned long long)hostRecords);
        if (timed) {
            const size_t skip = ticks / 4;
            printf(", \"host_delivery_us\": %.1f, \"device_delivery_us\": %.1f, \"host_tick_us\": %.1f, \"device_tick_us\": %.1f",
                   1e6 * median(hostTiming.delivery, skip), 1e6 * median(deviceTiming.delivery, skip), 1e6 * median(hostTiming.total, skip),
                   1e6 * median(deviceTiming.total, skip));
        }
        printf("}\n");
        return 0;
    } catch (const std::exception& e) {
        printf("{\"ok\": false, \"why\": \"%s\"}\n", e.what());
        return 1;
    }
}
