// group_commands.cpp — TEST driver of the grouping side of host/draw_commands.hpp (setGrouping): an ecsm_lite world of Opaque (unsorted,
// 40 geometries, a byte column, no levels), Refracted (unsorted, 4 base geometries of 4 levels, a uint32 column) and Translucent
// (sorted) mesh systems with movers and a few geometry switches and size edits per tick, the GpuVisibilitySystem drop-in with a
// main pass and three cascades, and after every tick GpuInstanceWriter::write + GpuDrawCommands with setGrouping(true) for the two
// unsorted systems against a host loop that takes the records as the drop-in delivered them (ungrouped), stable-sorts every pass's
// records by min(id, table size) — the id is the base id of the record's slot plus, for the system with levels, the level the C
// twin of the rule (tests/lod_twin.h) picks for that pass's scale — and writes the commands a CPU would record over that order: per
// run of one id within a pass (three ticks of four) or per draw (every fourth tick). Every command array byte for byte, and the
// per-pass counts. setGrouping(true) of the sorted system must throw. Built and run by tests/test_gpu_group_draws.py.
//
//   group_commands [--entities N] [--ticks T]
// Prints one JSON line: ok, ticks, passes, geometries (ids + levels in use per pass at most), the run-mode commands compared, the
// draws behind them, and whether the sorted system threw.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/host/instance_writer.hpp"
#include "../lod_twin.h"

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

struct Instance {
    float mvp[16];
};
struct Command {  // the indexed indirect command
    uint32_t indexCount, instanceCount, firstIndex;
    int32_t vertexOffset;
    uint32_t firstInstance;
};
static_assert(sizeof(Command) == 20, "packed");

// what the host alternative writes: one command per draw, or per run of one geometry id within a pass
struct HostLoop {
    const std::vector<GvGeometry>& table;
    bool merge;
    std::vector<Command> out;
    std::vector<uint32_t> perPass;
    bool open = false;
    uint32_t previous = 0;
    void beginPass()
    {
        open = false;
        perPass.push_back(0);
    }
    void draw(uint32_t id, uint32_t instanceIndex)
    {
        const bool known = id < table.size();
        if (merge && open && id == previous) {
            out.back().instanceCount += known ? 1u : 0u;
            return;
        }
        const GvGeometry g = known ? table[id] : GvGeometry{0, 0, 0};
        out.push_back({g.count, known ? 1u : 0u, g.first, g.vertex_offset, instanceIndex});
        perPass.back()++;
        open = true;
        previous = id;
    }
    // one pass: the draws' ids in delivery order, stable-sorted by min(id, table size), drawn in that order
    void pass(const std::vector<uint32_t>& ids, uint32_t& instanceIndex)
    {
        beginPass();
        std::vector<uint32_t> order(ids.size());
        std::iota(order.begin(), order.end(), 0u);
        const uint32_t K = (uint32_t)table.size();
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return std::min(ids[a], K) < std::min(ids[b], K); });
        for (uint32_t k : order)
            draw(ids[k], instanceIndex++);
    }
};

static bool same(const GpuDrawCommands::Emitted& got, const HostLoop& exp, const char* what, uint32_t tick, bool merge)
{
    if (got.counts == exp.perPass && got.commands.size() == exp.out.size() * sizeof(Command) &&
        (exp.out.empty() || memcmp(got.commands.data(), exp.out.data(), got.commands.size()) == 0))
        return true;
    printf("{\"ok\": false, \"why\": \"tick %u: %s (%s) differs from the host loop (%zu commands against %zu)\"}\n", tick, what,
           merge ? "runs" : "per draw", got.commands.size() / sizeof(Command), exp.out.size());
    return false;
}

int main(int argc, char** argv)
{
    uint32_t entities = 30000, ticks = 20;
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
        auto refracted = manager.createSystem<RefractedMeshSystem>();
        manager.registerComponents<RefractedMeshComponent>(refracted);
        auto translucent = manager.createSystem<TranslucentMeshSystem>();
        manager.registerComponents<TranslucentMeshComponent>(translucent);
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
            t->uid = i + 1;
            MeshRenderComponent* m = i % 3 == 0 ? *opaque->add(e) : (i % 3 == 1 ? static_cast<MeshRenderComponent*>(*refracted->add(e))
                                                                             : static_cast<MeshRenderComponent*>(*translucent->add(e)));
            const float hx = rng.uniform(0.25f, 1.0f), hy = rng.uniform(0.25f, 1.0f), hz = rng.uniform(0.25f, 1.0f);
            m->aabb.min = f32x4(-hx, -hy, -hz);
            m->aabb.max = f32x4(hx, hy, hz);
            if (rng.next() % 100 == 0) m->isEnabled = false;
        }

        // camera: looks down +z, FOV 90, 16:9, near 0.01, infinite reversed-Z (camera.hpp:111-121)
        f32x4x4 viewProj;
        memset(viewProj.m, 0, sizeof(viewProj.m));
        viewProj.m[0] = 9.0f / 16.0f; viewProj.m[5] = -1.0f; viewProj.m[11] = 1.0f; viewProj.m[14] = 0.01f;
        graphicsSystem->setCamera(viewProj, f32x4(3.0f, -2.0f, 5.0f));
        const uint32_t passCount = 3;
        std::vector<GpuVisibilitySystem::ShadowPass> passes;
        for (uint32_t c = 0; c < passCount; c++) {
            const float size = side * (0.2f + 0.3f * (float)c), nearPlane = -side, farPlane = side;
            f32x4x4 vp;
            memset(vp.m, 0, sizeof(vp.m));
            vp.m[0] = 2.0f / size; vp.m[5] = -2.0f / size; vp.m[10] = -1.0f / (farPlane - nearPlane);
            vp.m[14] = farPlane / (farPlane - nearPlane); vp.m[15] = 1.0f;
            passes.push_back({vp, f32x4(3.0f * (float)(c + 1), -7.0f, 11.0f), (int8_t)c});
        }
        gpu->setShadowPasses(passes);

        GpuInstanceWriter writer(gpu);
        GpuDrawCommands commands(gpu);
        writer.setCommands(&commands);
        if (!writer.isSupported() || !commands.isSupported()) {
            printf("{\"ok\": false, \"why\": \"one context reported as unsupported\"}\n");
            return 1;
        }
        const GvInstanceLayout instanceLayout{sizeof(Instance), 0, GV_NONE, GV_NONE, GV_NONE};
        const GvCommandLayout commandLayout{sizeof(Command), offsetof(Command, indexCount), offsetof(Command, instanceCount),
                                            offsetof(Command, firstIndex), offsetof(Command, firstInstance), offsetof(Command, vertexOffset), GV_NONE};
        // by kind: 0 opaque (40 geometries, no levels), 1 refracted (4 bases of 4 levels)
        std::vector<uint8_t> opaqueIds;
        std::vector<uint32_t> refractedIds;
        std::vector<float> sizes;
        std::vector<GvGeometry> tables[2];
        std::vector<GvLodGeometry> lods;
        const uint32_t tableSize[2] = {40, 16};
        for (uint32_t k = 0; k < 2; k++)
            for (uint32_t g = 0; g < tableSize[k]; g++)
                tables[k].push_back({36u * (g + 1), 1000u * k + 36u * g * (g + 1) / 2u, (int32_t)(g * 24u) - 100});
        for (uint32_t g = 0; g < 16; g++) {
            GvLodGeometry e{};
            e.levels = g % 4 == 0 ? 4u : 1u;  // (the entries between the bases are never a base id)
            for (uint32_t i = 0; i + 1 < e.levels; i++)
                e.switch_at[i] = 40.0f * (float)(i + 1) + (float)g;
            lods.push_back(e);
        }
        const float baseScale = 1.5f, shadowScale = 0.5f;
        std::vector<Instance> base, shadow;
        uint64_t compared = 0, draws = 0;
        bool sortedThrows = false;
        for (uint32_t tick = 0; tick < ticks; tick++) {
            if (tick) {  // movers, reported one by one
                for (uint32_t k = tick % 7; k < entities; k += 7)
                    if (auto t = transformSystem->tryGetOf(ents[k])) {
                        t->posChildCount.x += 0.75f;
                        transformSystem->markMoved(ents[k]);
                    }
            }
            manager.update();  // the prepare phase: the drop-in binds, culls, sorts and fills the engine's buffers
            const auto& meshSystems = gpu->getMeshSystems();
            if (meshSystems.size() != 3) {
                printf("{\"ok\": false, \"why\": \"%zu mesh systems\"}\n", meshSystems.size());
                return 1;
            }
            auto kindOf = [](MeshRenderType type) { return type == MeshRenderType::Opaque ? 0u : (type == MeshRenderType::Refracted ? 1u : 2u); };
            for (uint32_t p = 0; p < 3; p++) {
                const uint32_t kind = kindOf(meshSystems[p]->getMeshRenderType());
                const uint32_t occupancy = meshSystems[p]->getMeshComponentPool().getOccupancy();
                if (kind == 2) {
                    if (tick == 0) {
                        try {
                            commands.setGrouping(p, true);
                        } catch (const GardenError&) {
                            sortedThrows = true;
                        }
                    }
                    continue;
                }
                if (tick == 0) {
                    writer.setLayout(p, instanceLayout);
                    commands.setLayout(p, commandLayout);
                    if (kind == 0) {
                        opaqueIds.resize(occupancy);
                        for (auto& id : opaqueIds) id = (uint8_t)(rng.next() % 40u);
                        commands.setGeometry(p, opaqueIds.data(), 1, 1, occupancy, tables[0].data(), 40);
                    } else {
                        refractedIds.resize(occupancy);
                        for (auto& id : refractedIds) id = 4u * (rng.next() % 4u);
                        commands.setGeometry(p, refractedIds.data(), 4, 4, occupancy, tables[1].data(), 16);
                        sizes.resize(occupancy);
                        for (auto& r : sizes) r = rng.uniform(0.5f, 2.0f);
                        commands.setLods(p, sizes.data(), 4, occupancy, lods.data(), 16);
                        commands.setLodScale(p, baseScale, shadowScale);
                    }
                    commands.setGrouping(p, true);
                } else {  // a few geometry switches and size edits between the cull and the grouping, reported one by one
                    for (uint32_t k = 0; k < 5; k++) {
                        const uint32_t slot = rng.next() % occupancy, other = rng.next() % occupancy;
                        if (kind == 0) opaqueIds[slot] = (uint8_t)(rng.next() % 40u);
                        else refractedIds[slot] = 4u * (rng.next() % 4u);
                        bool ok = gv_mark_dirty(gpu->getContext(), GV_DIRTY_GEOMETRY, (p << 28) | slot, 1) == GV_OK;
                        if (kind == 1) {
                            sizes[other] = rng.uniform(0.25f, 4.0f);
                            ok = ok && gv_mark_dirty(gpu->getContext(), GV_DIRTY_LOD, (p << 28) | other, 1) == GV_OK;
                        }
                        if (!ok) {
                            printf("{\"ok\": false, \"why\": \"gv_mark_dirty failed\"}\n");
                            return 1;
                        }
                    }
                }
            }
            uint32_t unsortedIndex = 0;
            for (uint32_t p = 0; p < 3; p++) {
                auto meshSystem = meshSystems[p];
                const uint32_t kind = kindOf(meshSystem->getMeshRenderType());
                if (kind == 2)
                    continue;
                const uint32_t bufferIndex = unsortedIndex++;
                const size_t componentSize = meshSystem->getMeshComponentSize();
                const uint32_t occupancy = meshSystem->getMeshComponentPool().getOccupancy();
                auto idOf = [&](const UnsortedMesh& record, bool shadowPass) {
                    const size_t slot = record.componentOffset / componentSize;
                    if (kind == 0)
                        return (uint32_t)opaqueIds[slot];
                    const uint32_t b = refractedIds[slot];
                    const GvLodGeometry one{1u, {}};
                    const GvLodGeometry& e = b < lods.size() ? lods[b] : one;
                    return lod_twin_effective(b, lod_twin_level(record.bakedModel.m, sizes[slot], shadowPass ? shadowScale : baseScale, e.levels, e.switch_at));
                };
                auto idsOf = [&](const UnsortedBuffer* buffer, bool shadowPass) {
                    std::vector<uint32_t> ids(buffer->drawCount);
                    for (uint32_t k = 0; k < buffer->drawCount; k++)
                        ids[k] = idOf(buffer->meshes()[k], shadowPass);
                    return ids;
                };
                base.resize(occupancy);
                shadow.resize((size_t)occupancy * passCount);
                const bool merge = tick % 4 != 3;
                // the host loop first: over the records as the drop-in delivered them, before write() groups them on the device
                HostLoop light{tables[kind], merge, {}, {}}, dark{tables[kind], merge, {}, {}};
                uint32_t n = 0, shadowIndex = 0;
                light.pass(idsOf(gpu->getUnsortedBuffers()[bufferIndex], false), n);
                for (int8_t pass : gpu->getSystemPasses(p))
                    if (pass >= 0)
                        dark.pass(idsOf(gpu->getShadowBuffers(bufferIndex)[(uint32_t)pass], true), shadowIndex);
                commands.setMode(p, merge ? GV_COMMANDS_MERGE_RUNS : 0u, 0);
                writer.write(p, base.data(), base.size() * sizeof(Instance), shadow.data(), shadow.size() * sizeof(Instance), passCount);
                if (!same(commands.getBase(p), light, kind == 0 ? "the opaque base commands" : "the refracted base commands", tick, merge) ||
                    !same(commands.getShadow(p), dark, kind == 0 ? "the opaque shadow commands" : "the refracted shadow commands", tick, merge))
                    return 1;
                if (merge) {
                    compared += light.out.size() + dark.out.size();
                    draws += n + shadowIndex;
                }
            }
        }
        printf("{\"ok\": true, \"ticks\": %u, \"passes\": %u, \"geometries\": %u, \"commands\": %llu, \"draws\": %llu, \"sorted_throws\": %s}\n", ticks,
               passCount + 1, tableSize[0] + tableSize[1], (unsigned long long)compared, (unsigned long long)draws, sortedThrows ? "true" : "false");
        return 0;
    } catch (const std::exception& e) {
        printf("{\"ok\": false, \"why\": \"%s\"}\n", e.what());
        return 1;
    }
}
