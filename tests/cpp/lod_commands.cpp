// lod_commands.cpp — TEST driver of the level-of-detail side of host/draw_commands.hpp (setLods / setLodScale): an ecsm_lite world
// of Opaque (4 base geometries of 4 levels, a byte column), Translucent (sorted, 2 base geometries of 8 levels, a uint32 column) and
// UI (sorted, one geometry, no column, NO levels) mesh systems with movers, a few geometry switches and a few size edits per tick,
// the GpuVisibilitySystem drop-in with a main pass and three cascades, and after every tick GpuInstanceWriter::write +
// GpuDrawCommands for each system, in both modes, against a host loop that walks the records in draw order as mesh.cpp:589-601
// does, picks each draw's level with the C twin of the rule (tests/lod_twin.h) from the record's bakedModel, and writes the struct
// a CPU would record per draw — or, merged, per run of consecutive draws of one EFFECTIVE geometry within a pass. Every command
// array byte for byte, and the per-pass counts. Built and run by tests/test_gpu_lod_select.py.
//
//   lod_commands [--entities N] [--ticks T]
// Prints one JSON line: ok, systems, passes, ticks, the number of commands compared and the draws per level.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
        auto translucent = manager.createSystem<TranslucentMeshSystem>();
        manager.registerComponents<TranslucentMeshComponent>(translucent);
        auto ui = manager.createSystem<UiMeshSystem>();
        manager.registerComponents<UiMeshComponent>(ui);
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
            MeshRenderComponent* m = i % 3 == 0 ? *opaque->add(e) : (i % 3 == 1 ? static_cast<MeshRenderComponent*>(*translucent->add(e))
                                                                             : static_cast<MeshRenderComponent*>(*ui->add(e)));
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
        gpu->setUiSize(side, side);
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
        // geometry: base ids per POOL slot of each system (kept by this driver, as a component field would be), the geometry tables
        // (the levels of a base geometry are consecutive entries), the LOD tables the base ids index, and a size per slot
        std::vector<uint8_t> opaqueIds;
        std::vector<uint32_t> transIds;
        std::vector<float> sizes[2];
        std::vector<GvGeometry> tables[3];
        std::vector<GvLodGeometry> lods[2];
        const uint32_t tableSize[3] = {16, 16, 1};  // by system kind: opaque 4 x 4 levels, translucent 2 x 8 levels, UI
        const uint32_t levelsOf[2] = {4, 8};
        for (uint32_t k = 0; k < 3; k++)
            for (uint32_t g = 0; g < tableSize[k]; g++)
                tables[k].push_back({36u * (g + 1), 1000u * k + 36u * g * (g + 1) / 2u, (int32_t)(g * 24u) - 100});
        for (uint32_t k = 0; k < 2; k++)
            for (uint32_t g = 0; g < tableSize[k]; g++) {
                GvLodGeometry e{};
                e.levels = g % levelsOf[k] == 0 ? levelsOf[k] : 1u;  // (the entries between the bases are never a base id)
                for (uint32_t i = 0; i + 1 < e.levels; i++)
                    e.switch_at[i] = (k == 0 ? 40.0f : 18.0f) * (float)(i + 1) + (float)g;
                lods[k].push_back(e);
            }
        const float baseScale[2] = {1.5f, 1.0f}, shadowScale[2] = {0.5f, 2.0f};
        uint64_t perLevel[GV_MAX_LOD_LEVELS] = {};
        auto kindOf = [](MeshRenderType type) { return type == MeshRenderType::UI ? 2u : (type == MeshRenderType::Translucent ? 1u : 0u); };
        std::vector<Instance> base, shadow;
        uint64_t compared = 0;
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
            for (uint32_t p = 0; p < 3; p++) {
                const uint32_t kind = kindOf(meshSystems[p]->getMeshRenderType());
                const uint32_t occupancy = meshSystems[p]->getMeshComponentPool().getOccupancy();
                if (tick == 0) {
                    writer.setLayout(p, instanceLayout);
                    commands.setLayout(p, commandLayout);
                    if (kind == 0) {
                        opaqueIds.resize(occupancy);
                        for (auto& id : opaqueIds) id = (uint8_t)(4u * (rng.next() % 4u));
                        commands.setGeometry(p, opaqueIds.data(), 1, 1, occupancy, tables[0].data(), 16);
                    } else if (kind == 1) {
                        transIds.resize(occupancy);
                        for (auto& id : transIds) id = 8u * (rng.next() % 2u);
                        commands.setGeometry(p, transIds.data(), 4, 4, occupancy, tables[1].data(), 16);
                    } else {
                        commands.setGeometry(p, nullptr, 0, 0, 0, tables[2].data(), 1);
                    }
                    if (kind != 2) {
                        sizes[kind].resize(occupancy);
                        for (auto& r : sizes[kind]) r = rng.uniform(0.5f, 2.0f);
                        commands.setLods(p, sizes[kind].data(), 4, occupancy, lods[kind].data(), 16);
                        commands.setLodScale(p, baseScale[kind], shadowScale[kind]);
                    }
                } else if (kind != 2) {  // a few geometry switches and size edits between the cull and the emission, reported one by one
                    for (uint32_t k = 0; k < 5; k++) {
                        const uint32_t slot = rng.next() % occupancy, other = rng.next() % occupancy;
                        if (kind == 0) opaqueIds[slot] = (uint8_t)(4u * (rng.next() % 4u));
                        else transIds[slot] = 8u * (rng.next() % 2u);
                        sizes[kind][other] = rng.uniform(0.25f, 4.0f);
                        if (gv_mark_dirty(gpu->getContext(), GV_DIRTY_GEOMETRY, (p << 28) | slot, 1) != GV_OK ||
                            gv_mark_dirty(gpu->getContext(), GV_DIRTY_LOD, (p << 28) | other, 1) != GV_OK) {
                            printf("{\"ok\": false, \"why\": \"gv_mark_dirty failed\"}\n");
                            return 1;
                        }
                    }
                }
            }
            for (uint32_t p = 0; p < 3; p++) {
                auto meshSystem = meshSystems[p];
                const uint32_t kind = kindOf(meshSystem->getMeshRenderType());
                const size_t componentSize = meshSystem->getMeshComponentSize();
                const uint32_t occupancy = meshSystem->getMeshComponentPool().getOccupancy();
                // the effective id of a record's draw: the base id of its slot plus the level the twin picks for this pass
                auto idOf = [&](const auto& record, bool shadowPass) {
                    const size_t slot = record.componentOffset / componentSize;
                    const uint32_t b = kind == 0 ? (uint32_t)opaqueIds[slot] : (kind == 1 ? transIds[slot] : 0u);
                    if (kind == 2)
                        return b;
                    const GvLodGeometry one{1u, {}};
                    const GvLodGeometry& e = b < lods[kind].size() ? lods[kind][b] : one;
                    const uint32_t level = lod_twin_level(record.bakedModel.m, sizes[kind][slot], shadowPass ? shadowScale[kind] : baseScale[kind],
                                                          e.levels, e.switch_at);
                    perLevel[level]++;
                    return lod_twin_effective(b, level);
                };
                base.resize(occupancy);
                shadow.resize((size_t)occupancy * passCount);
                for (uint32_t merge = 0; merge < 2; merge++) {
                    commands.setMode(p, merge ? GV_COMMANDS_MERGE_RUNS : 0u, 0);
                    writer.write(p, base.data(), base.size() * sizeof(Instance), kind == 2 ? nullptr : shadow.data(),
                                 kind == 2 ? 0 : shadow.size() * sizeof(Instance), passCount);
                    HostLoop light{tables[kind], merge != 0, {}, {}}, dark{tables[kind], merge != 0, {}, {}};
                    uint32_t n = 0;
                    light.beginPass();
                    if (kind == 2) {
                        for (uint32_t k = 0; k < gpu->getUiDrawCount(); k++)
                            light.draw(idOf(gpu->getUiSortedMeshes()[k], false), n++);
                    } else if (kind == 1) {
                        for (uint32_t k = 0; k < gpu->getTransDrawCount(); k++)
                            light.draw(idOf(gpu->getTransSortedMeshes()[k], false), n++);
                    } else {
                        const UnsortedBuffer* buffer = gpu->getUnsortedBuffers()[0];
                        for (uint32_t k = 0; k < buffer->drawCount; k++)
                            light.draw(idOf(buffer->meshes()[k], false), n++);
                    }
                    if (!same(commands.getBase(p), light, kind == 2 ? "the UI system's commands" : (kind == 1 ? "the translucent base commands" : "the opaque base commands"),
                              tick, merge != 0))
                        return 1;
                    compared += light.out.size();
                    if (kind == 2)
                        continue;
                    uint32_t shadowIndex = 0;  // shadowInstanceIndex: pass after pass
                    for (int8_t pass : gpu->getSystemPasses(p)) {
                        if (pass < 0)
                            continue;
                        dark.beginPass();
                        const uint32_t s = (uint32_t)pass;
                        if (kind == 1) {
                            for (uint32_t k = 0; k < gpu->getShadowTransDrawCount(s); k++)
                                dark.draw(idOf(gpu->getShadowTransMeshes(s)[k], true), shadowIndex++);
                        } else {
                            const UnsortedBuffer* sb = gpu->getShadowBuffers(0)[s];
                            for (uint32_t k = 0; k < sb->drawCount; k++)
                                dark.draw(idOf(sb->meshes()[k], true), shadowIndex++);
                        }
                    }
                    if (!same(commands.getShadow(p), dark, kind == 1 ? "the translucent shadow commands" : "the opaque shadow commands", tick, merge != 0))
                        return 1;
                    compared += dark.out.size();
                }
            }
        }
        printf("{\"ok\": true, \"systems\": 3, \"passes\": %u, \"ticks\": %u, \"commands\": %llu, \"levels\": [%llu, %llu, %llu, %llu, %llu, %llu, %llu, %llu]}\n",
               passCount + 1, ticks, (unsigned long long)compared, (unsigned long long)perLevel[0], (unsigned long long)perLevel[1],
               (unsigned long long)perLevel[2], (unsigned long long)perLevel[3], (unsigned long long)perLevel[4], (unsigned long long)perLevel[5],
               (unsigned long long)perLevel[6], (unsigned long long)perLevel[7]);
        return 0;
    } catch (const std::exception& e) {
        printf("{\"ok\": false, \"why\": \"%s\"}\n", e.what());
        return 1;
    }
}
