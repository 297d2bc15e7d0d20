// motion_history.cpp — TEST driver of host/motion_history.hpp: an ecsm_lite world of one opaque mesh system with movers under a camera
// that moves every tick, the GpuVisibilitySystem drop-in, and after every tick GpuInstanceWriter::write followed by
// GpuMotionHistory::write into the same base instance array {mvp, prevMvp, hasHistory}: every byte of the array against the draw loop
// restated over the buffers the drop-in filled, mvp through the instance twin and prevMvp / hasHistory through the previous-frame twin
// (tests/previous_twin.h), whose history is kept here by the same rule. Tick 0 has no history, ticks 1 - 2 a moving camera and movers,
// tick 3 a camera cut, tick 4 a forgotten range of slots. Built by motion_history.mk, run by tests/test_gpu_previous.py.
//
//   motion_history [--entities N]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/host/instance_writer.hpp"
#include "../../garden_amd/csrc/host/motion_history.hpp"
#include "../previous_twin.h"

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

struct Instance {  // the plugin's struct: the two matrices, the flag, bytes of its own behind them
    float mvp[16];
    float prevMvp[16];
    uint32_t hasHistory;
    uint32_t own[3];
};
static_assert(sizeof(Instance) == 144, "a multiple of 16");

static constexpr uint8_t kPattern = 0x5A;  // the plugin's bytes before the writers run
static constexpr uint32_t kTicks = 5, kCutTick = 3, kForgetTick = 4, kForgetFirst = 100;

static int fail(const char* why, uint32_t tick, long a = 0, long b = 0)
{
    printf("motion history: tick %u: %s (%ld, %ld)\n", tick, why, a, b);
    return 1;
}

int main(int argc, char** argv)
{
    uint32_t entities = 20000;
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--entities" && i + 1 < argc)
            entities = (uint32_t)atoi(argv[++i]);
    try {
        Manager manager;
        auto transformSystem = manager.createSystem<TransformSystem>();
        manager.registerComponents<TransformComponent>(transformSystem);
        auto graphicsSystem = manager.createSystem<GraphicsSystem>();
        manager.createSystem<DeferredRenderSystem>();
        auto opaque = manager.createSystem<OpaqueMeshSystem>();
        manager.registerComponents<MeshRenderComponent>(opaque);
        const float side = 8.0f * std::cbrt((float)entities);
        GpuVisibilitySystem* gpu = manager.createSystem<GpuVisibilitySystem>(0);
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
            MeshRenderComponent* m = *opaque->add(e);
            const float hx = rng.uniform(0.25f, 1.0f), hy = rng.uniform(0.25f, 1.0f), hz = rng.uniform(0.25f, 1.0f);
            m->aabb.min = f32x4(-hx, -hy, -hz);
            m->aabb.max = f32x4(hx, hy, hz);
        }
        // camera: looks down +z, FOV 90, 16:9, near 0.01, infinite reversed-Z (camera.hpp:111-121)
        f32x4x4 viewProj;
        memset(viewProj.m, 0, sizeof(viewProj.m));
        viewProj.m[0] = 9.0f / 16.0f; viewProj.m[5] = -1.0f; viewProj.m[11] = 1.0f; viewProj.m[14] = 0.01f;
        gpu->setUiSize(side, side);

        GpuInstanceWriter writer(gpu);
        GpuMotionHistory history(gpu);
        if (!writer.isSupported() || !history.isSupported())
            return fail("one context reported as unsupported", 0);
        const GvInstanceLayout instanceLayout{sizeof(Instance), offsetof(Instance, mvp), GV_NONE, GV_NONE, GV_NONE};
        const GvPreviousLayout previousLayout{sizeof(Instance), offsetof(Instance, prevMvp), offsetof(Instance, hasHistory)};
        history.setLayout(0, previousLayout);

        std::vector<uint32_t> rows;  // the twin's history
        PreviousTwinHistory twin{};
        std::vector<Instance> base, expected;
        std::vector<uint32_t> slots;
        std::vector<float> models;
        uint64_t compared = 0;
        for (uint32_t tick = 0; tick < kTicks; tick++) {
            if (tick) {  // movers, reported one by one
                for (uint32_t k = tick % 7; k < entities; k += 7)
                    if (auto t = transformSystem->tryGetOf(ents[k])) {
                        t->posChildCount.x += 0.75f;
                        transformSystem->markMoved(ents[k]);
                    }
            }
            graphicsSystem->setCamera(viewProj, f32x4(3.0f + 15.0f * (float)tick, -2.0f, 5.0f - 6.5f * (float)tick));  // (strides that bring fresh draws)
            manager.update();  // the prepare phase: the drop-in binds, culls and fills the engine's buffers
            const auto& meshSystems = gpu->getMeshSystems();
            if (meshSystems.size() != 1)
                return fail("mesh systems", tick, (long)meshSystems.size(), 1);
            if (tick == 0)
                writer.setLayout(0, instanceLayout);
            const auto& cc = graphicsSystem->getCommonConstants();
            const float camera[3] = {cc.cameraPos.x, cc.cameraPos.y, cc.cameraPos.z};
            const size_t componentSize = meshSystems[0]->getMeshComponentSize();
            const uint32_t occupancy = meshSystems[0]->getMeshComponentPool().getOccupancy();
            const std::vector<int8_t>& passes = gpu->getSystemPasses(0);
            uint32_t lightView = GV_MAX_VIEWS;
            for (uint32_t v = 0; v < passes.size(); v++)
                if (passes[v] < 0)
                    lightView = v;
            if (lightView == GV_MAX_VIEWS)
                return fail("no light pass", tick);
            base.resize(occupancy), expected.resize(occupancy);
            memset(static_cast<void*>(base.data()), kPattern, occupancy * sizeof(Instance));
            memset(static_cast<void*>(expected.data()), kPattern, occupancy * sizeof(Instance));
            if (tick == kCutTick)
                history.cut();
            if (tick == kForgetTick) {
                history.forget(0, kForgetFirst, occupancy / 4);
                previous_twin_forget(&twin, kForgetFirst, occupancy / 4);
            }
            const auto w = writer.write(0, base.data(), base.size() * sizeof(Instance), nullptr, 0, 0);
            const auto h = history.write(0, lightView, base.data(), base.size() * sizeof(Instance));

            // the draw loop restated (renderUnsorted, mesh.cpp:589-601), with the velocity plugin's second matrix
            const UnsortedBuffer* buffer = gpu->getUnsortedBuffers()[0];
            const uint32_t n = buffer->drawCount;
            slots.resize(n), models.resize((size_t)n * 12);
            twin.rows = rows.data();
            uint32_t kept = 0, forgotten = 0;
            for (uint32_t k = 0; k < n; k++) {
                const UnsortedMesh& m = buffer->meshes()[k];
                slots[k] = (uint32_t)(m.componentOffset / componentSize);
                memcpy(&models[(size_t)k * 12], m.bakedModel.m, 48);
                instance_twin_mvp(cc.viewProj.m, m.bakedModel.m, expected[k].mvp);
                expected[k].hasHistory = previous_twin_draw(&twin, cc.viewProj.m, camera, nullptr, tick == kCutTick, slots[k], m.bakedModel.m,
                                                            expected[k].prevMvp);
                kept += expected[k].hasHistory;
                forgotten += tick == kForgetTick && slots[k] >= kForgetFirst && slots[k] < kForgetFirst + occupancy / 4;
                if (tick == kForgetTick && slots[k] >= kForgetFirst && slots[k] < kForgetFirst + occupancy / 4 && expected[k].hasHistory)
                    return fail("a forgotten slot has a history", tick, (long)slots[k]);
            }
            if (w.baseCount != n || h.drawCount != n || h.keptCount != kept || h.epoch != twin.epoch)
                return fail("counts", tick, (long)h.drawCount, (long)h.keptCount);
            if (memcmp(base.data(), expected.data(), occupancy * sizeof(Instance)) != 0)
                return fail("the base array differs from the draw loop", tick, (long)n, (long)kept);
            if (n < 1000)
                return fail("too few draws to mean anything", tick, (long)n);
            if ((tick == 0 || tick == kCutTick) ? kept != 0 : (kept < 64 || n - kept < 64))
                return fail("kept draws", tick, (long)kept, (long)n);
            if (tick == kForgetTick && forgotten < 64)
                return fail("forgotten draws", tick, (long)forgotten);
            if (tick == 0 || tick == kCutTick)  // no history, a cut: prevMvp is mvp
                for (uint32_t k = 0; k < n; k++)
                    if (memcmp(base[k].mvp, base[k].prevMvp, 64) != 0)
                        return fail("prevMvp is not mvp under a cut", tick, (long)k);
            // the twin keeps what the library keeps
            if (occupancy > twin.slots) {
                rows.resize((size_t)occupancy * 16, 0);
                twin.rows = rows.data();
                twin.slots = occupancy;
            }
            previous_twin_keep(&twin, cc.viewProj.m, camera, slots.data(), models.data(), n, 0);
            compared += n;
        }
        printf("motion history: %u ticks, every prevMvp equal to the twin's: ok (%llu instances)\n", kTicks, (unsigned long long)compared);
        return 0;
    } catch (const std::exception& e) {
        printf("motion history: %s\n", e.what());
        return 1;
    }
}
