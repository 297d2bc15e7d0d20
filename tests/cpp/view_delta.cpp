// view_delta.cpp — TEST driver of host/visible_delta.hpp (GpuVisibleDelta): an ecsm_lite world of one Opaque mesh system, a camera
// that steps every tick, the CPU reference-path system (oracle/cpu_mesh_render_system.hpp) and the GpuVisibilitySystem drop-in with
// its own write-back switched off (writeBackVisible = false). Per tick:
//   the CPU system alone            MeshRenderComponent::isVisible of every component as the reference computes it
//   the drop-in alone, then         GpuVisibleDelta::run + writeBack over the bytes the delta path itself left last tick
// and the component bytes must then be the CPU system's, byte for byte; the appeared / vanished spans must be what a host loop over
// the CPU bytes of two consecutive ticks finds (on a tick whose write-back is the whole column: everything visible, nothing
// vanished). Half way entities are added (the occupancy changes) and later TransformSystem::hierarchyVersion is bumped: both ticks
// must rewrite the whole column, which the driver fills with ones beforehand. Built by tests/cpp/view_delta.mk, run by
// tests/test_gpu_view_delta.py.
//
//   view_delta [--entities N] [--ticks T]           the check; prints one JSON line and, when everything held, "view_delta ok"
//   view_delta --bench R [--entities N] [--ticks T]  R alternated rounds of  full: fetch + whole-column write-back (the drop-in as it
//                                                   is)  and  delta: fetch without + GpuVisibleDelta::run / writeBack, us per tick
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/host/visible_delta.hpp"
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

struct World {
    Manager manager;
    TransformSystem* transformSystem = nullptr;
    GraphicsSystem* graphicsSystem = nullptr;
    OpaqueMeshSystem* opaque = nullptr;
    Rng rng;
    float side = 1.0f;
    uint64_t uids = 0;
    void add(uint32_t count)
    {
        for (uint32_t i = 0; i < count; i++) {
            auto e = manager.createEntity();
            auto t = transformSystem->add(e);
            t->setPosition(rng.uniform(-0.5f * side, 0.5f * side), rng.uniform(-0.5f * side, 0.5f * side), rng.uniform(-0.5f * side, 0.5f * side));
            t->setScale(rng.uniform(0.5f, 2.0f), rng.uniform(0.5f, 2.0f), rng.uniform(0.5f, 2.0f));
            t->uid = ++uids;
            MeshRenderComponent* m = *opaque->add(e);
            const float hx = rng.uniform(0.25f, 1.0f), hy = rng.uniform(0.25f, 1.0f), hz = rng.uniform(0.25f, 1.0f);
            m->aabb.min = f32x4(-hx, -hy, -hz);
            m->aabb.max = f32x4(hx, hy, hz);
            if (rng.next() % 100 == 0) m->isEnabled = false;
        }
    }
    // camera: looks down +z, FOV 90, 16:9, near 0.01, infinite reversed-Z (camera.hpp:111-121), `step` world units along x and z per tick
    void camera(uint32_t tick, float step)
    {
        f32x4x4 viewProj;
        memset(viewProj.m, 0, sizeof(viewProj.m));
        viewProj.m[0] = 9.0f / 16.0f; viewProj.m[5] = -1.0f; viewProj.m[11] = 1.0f; viewProj.m[14] = 0.01f;
        graphicsSystem->setCamera(viewProj, f32x4(3.0f + step * (float)tick, -2.0f, 5.0f - 0.5f * step * (float)tick));
    }
    uint32_t occupancy() { return opaque->getMeshComponentPool().getOccupancy(); }
    MeshRenderComponent* component(uint32_t i)
    {
        uint8_t* base = reinterpret_cast<uint8_t*>(opaque->getMeshComponentPool().getData());
        return reinterpret_cast<MeshRenderComponent*>(base + (size_t)i * opaque->getMeshComponentSize());
    }
    std::vector<uint8_t> bytes()
    {
        std::vector<uint8_t> out(occupancy());
        for (uint32_t i = 0; i < out.size(); i++)
            out[i] = component(i)->isVisible ? 1 : 0;
        return out;
    }
    void setBytes(const std::vector<uint8_t>& from, uint8_t beyond)
    {
        for (uint32_t i = 0; i < occupancy(); i++)
            component(i)->isVisible = (i < from.size() ? from[i] : beyond) != 0;
    }
};

static int fail(const char* why, uint32_t tick, long a = 0, long b = 0)
{
    printf("{\"ok\": false, \"why\": \"tick %u: %s (%ld, %ld)\"}\n", tick, why, a, b);
    return 1;
}

static int check(uint32_t entities, uint32_t ticks)
{
    World w;
    Manager& manager = w.manager;
    w.transformSystem = manager.createSystem<TransformSystem>();
    manager.registerComponents<TransformComponent>(w.transformSystem);
    w.graphicsSystem = manager.createSystem<GraphicsSystem>();
    manager.createSystem<DeferredRenderSystem>();
    w.opaque = manager.createSystem<OpaqueMeshSystem>();
    manager.registerComponents<MeshRenderComponent>(w.opaque);
    w.side = 8.0f * std::cbrt((float)entities);
    CpuMeshRenderSystem* cpu = manager.createSystem<CpuMeshRenderSystem>();
    GpuVisibilitySystem* gpu = manager.createSystem<GpuVisibilitySystem>(0);
    gpu->writeBackVisible = false;
    manager.initialize();
    w.add(entities);
    GpuVisibleDelta delta(gpu);
    if (!delta.isSupported())
        return fail("one context reported as unsupported", 0);
    const size_t componentSize = w.opaque->getMeshComponentSize();
    std::vector<uint8_t> mine, previous;  // the bytes the delta path left / the CPU system's bytes of the previous tick
    uint64_t appearedTotal = 0, vanishedTotal = 0;
    uint32_t fullWriteBacks = 0;
    for (uint32_t tick = 0; tick < ticks; tick++) {
        w.camera(tick, 0.02f * w.side);
        bool wantFull = tick == 0;
        if (tick == ticks / 2) {  // the occupancy changes
            w.add(entities / 16 + 1);
            wantFull = true;
        }
        if (tick == ticks / 2 + 2) {  // a structural change nobody itemised
            w.transformSystem->hierarchyVersion++;
            wantFull = true;
        }
        cpu->isEnabled = true, gpu->isEnabled = false;
        manager.update();
        const std::vector<uint8_t> reference = w.bytes();
        // the drop-in's turn, over the bytes its own path left — or, where the whole column must be rewritten, over ones
        if (wantFull)
            mine.assign(w.occupancy(), 1);
        w.setBytes(mine, 1);
        cpu->isEnabled = false, gpu->isEnabled = true;
        manager.update();
        if (wantFull && w.bytes() != std::vector<uint8_t>(w.occupancy(), 1))
            return fail("the drop-in wrote isVisible although writeBackVisible is off", tick);
        delta.run(0);
        if (delta.wroteWholeColumn(0) != wantFull)
            return fail("whole-column write-back expected / decided", tick, wantFull, delta.wroteWholeColumn(0));
        const std::vector<size_t> appeared = delta.appeared(0), vanished = delta.vanished(0);
        delta.writeBack(0);
        mine = w.bytes();
        for (uint32_t i = 0; i < mine.size(); i++)
            if (mine[i] != reference[i])
                return fail("isVisible of a component differs from the CPU system's", tick, i, mine[i]);
        std::vector<size_t> wantAppeared, wantVanished;
        for (uint32_t i = 0; i < reference.size(); i++) {
            const uint8_t before = (wantFull || i >= previous.size()) ? 0 : previous[i];
            if (reference[i] && !before)
                wantAppeared.push_back((size_t)i * componentSize);
            if (!reference[i] && before)
                wantVanished.push_back((size_t)i * componentSize);
        }
        if (appeared != wantAppeared || vanished != wantVanished)
            return fail("the spans differ from the host loop over two ticks' bytes", tick, (long)appeared.size(), (long)wantAppeared.size());
        if (delta.visibleCount(0) != (uint32_t)std::count(reference.begin(), reference.end(), 1))
            return fail("visibleCount", tick, delta.visibleCount(0));
        if (wantFull)
            fullWriteBacks++;
        else
            appearedTotal += appeared.size(), vanishedTotal += vanished.size();
        previous = reference;
    }
    const bool ok = appearedTotal && vanishedTotal && fullWriteBacks >= 1;
    printf("{\"ok\": %s, \"ticks\": %u, \"appeared\": %llu, \"vanished\": %llu, \"full_write_backs\": %u}\n", ok ? "true" : "false", ticks,
           (unsigned long long)appearedTotal, (unsigned long long)vanishedTotal, fullWriteBacks);
    if (ok)
        printf("view_delta ok\n");
    return ok ? 0 : 1;
}

static int bench(uint32_t entities, uint32_t ticks, uint32_t rounds)
{
    World w;
    Manager& manager = w.manager;
    w.transformSystem = manager.createSystem<TransformSystem>();
    manager.registerComponents<TransformComponent>(w.transformSystem);
    w.graphicsSystem = manager.createSystem<GraphicsSystem>();
    manager.createSystem<DeferredRenderSystem>();
    w.opaque = manager.createSystem<OpaqueMeshSystem>();
    manager.registerComponents<MeshRenderComponent>(w.opaque);
    w.side = 8.0f * std::cbrt((float)entities);
    GpuVisibilitySystem* gpu = manager.createSystem<GpuVisibilitySystem>(0);
    manager.initialize();
    w.add(entities);
    GpuVisibleDelta delta(gpu);
    const float step = 0.002f * w.side;
    uint32_t tick = 0;
    auto run = [&](bool useDelta, uint32_t count, double& us, double& changed, double& visible) {
        gpu->writeBackVisible = !useDelta;
        const auto start = std::chrono::steady_clock::now();
        uint64_t lists = 0, seen = 0;
        for (uint32_t k = 0; k < count; k++) {
            w.camera(tick++, step);
            manager.update();
            if (useDelta) {
                delta.run(0);
                delta.writeBack(0);
                lists += delta.appeared(0).size() + delta.vanished(0).size();
                seen += delta.visibleCount(0);
            }
        }
        us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - start).count() / count;
        changed = (double)lists / count, visible = (double)seen / count;
    };
    double us, changed, visible;
    run(false, 20, us, changed, visible);  // warm-up of both paths (the delta path's first tick writes the whole column)
    run(true, 20, us, changed, visible);
    for (uint32_t r = 0; r < rounds; r++) {
        run(false, ticks, us, changed, visible);
        printf("full  --entities %u --ticks %u :: us/tick: total %.1f (fetch + whole-column write-back)\n", entities, ticks, us);
        delta.restart(0);                    // (somebody else wrote the bytes meanwhile: one whole-column tick, not timed)
        run(true, 1, us, changed, visible);
        run(true, ticks, us, changed, visible);
        printf("delta --entities %u --ticks %u :: us/tick: total %.1f (fetch + view delta + listed bytes; %.0f of %u bytes change per tick, %.0f visible)\n",
               entities, ticks, us, changed, w.occupancy(), visible);
    }
    return 0;
}

int main(int argc, char** argv)
{
    uint32_t entities = 10000, ticks = 8, rounds = 0;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--entities" && i + 1 < argc) entities = (uint32_t)atoi(argv[++i]);
        else if (a == "--ticks" && i + 1 < argc) ticks = (uint32_t)atoi(argv[++i]);
        else if (a == "--bench" && i + 1 < argc) rounds = (uint32_t)atoi(argv[++i]);
    }
    try {
        return rounds ? bench(entities, ticks, rounds) : check(entities, ticks);
    } catch (const std::exception& e) {
        printf("{\"ok\": false, \"why\": \"%s\"}\n", e.what());
        return 1;
    }
}
