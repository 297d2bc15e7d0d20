// cluster_lods.cpp — TEST driver of GpuClusterCommands::setClusterLods / setLodViews / lodScale (host/cluster_commands.hpp): the world
// of cluster_cones.cpp — one Opaque mesh system, 2 base geometries of 3 levels, one geometry drawn whole, a camera that moves every
// tick, movers, a main pass and ONE cascade, LODs on — where every level's clusters are a binary cluster DAG over the 4^3, 2^3 and 1
// cells of the model's box (127, 15 and 1 clusters: nested spheres, self error 0 at the leaves and doubling per level, the root's
// parent error +inf). The main pass has the camera's LOD view; the cascade names the camera's eye with half its scale, so that a
// pass that got the other's view shows. Five ticks, every command byte of gv_pool_cull_cluster_lods against a host path that walks
// the delivered records in draw order, decides frustum and pyramid with the oracle (tests/cluster_twin.h), the cut with the rule
// restated in tests/cluster_lod_twin.h and the cone with tests/cluster_cone_twin.h. Odd ticks write runs (setRuns); from tick 3 on
// outward cones are bound on the leaves (setCones, setEyes), so the calls carry eyes too. Built by cluster_lods.mk, run by
// tests/test_gpu_cluster_lods_shim.py.
//
//   cluster_lods [--entities N] [--ticks T]
// Prints one JSON line: ok, passes, ticks, commands compared, clusters tested, on the cut (all, main pass, cascade), kept by the
// unchanged test, survivors, cone-rejected on the cut.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/host/instance_writer.hpp"
#include "../cluster_lod_twin.h"
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

constexpr uint32_t kLevels = 3, kBases = 2, kTable = kLevels * kBases + 1;  // ids 0-2 and 3-5: two models; id 6: no clusters
constexpr float kHalf[3] = {9.0f, 6.0f, 12.0f};                              // every model's box
static const uint32_t kGrid[kLevels] = {4, 2, 1};

// one pass of the host path: the twin over the pass's records
struct HostPass {
    std::vector<float> models;
    std::vector<uint32_t> ids, first;
};

static bool same(const GpuClusterCommands::Emitted& got, const std::vector<Command>& exp, const std::vector<uint32_t>& counts,
                 const std::vector<uint32_t>& tested, const char* what, uint32_t tick)
{
    if (got.counts == counts && got.tested == tested && got.commands.size() == exp.size() * sizeof(Command) &&
        (exp.empty() || memcmp(got.commands.data(), exp.data(), got.commands.size()) == 0))
        return true;
    printf("{\"ok\": false, \"why\": \"tick %u: %s differ from the host path (%zu commands against %zu)\"}\n", tick, what,
           got.commands.size() / sizeof(Command), exp.size());
    return false;
}

int main(int argc, char** argv)
{
    uint32_t entities = 3000, ticks = 5;
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
        const float side = 40.0f * std::cbrt((float)entities);
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
            MeshRenderComponent* m = *opaque->add(e);
            m->aabb.min = f32x4(-kHalf[0], -kHalf[1], -kHalf[2]);
            m->aabb.max = f32x4(kHalf[0], kHalf[1], kHalf[2]);
        }

        // camera: looks down +z, FOV 90, 16:9, near 0.01, infinite reversed-Z (camera.hpp:111-121); it moves every tick
        f32x4x4 viewProj;
        memset(viewProj.m, 0, sizeof(viewProj.m));
        viewProj.m[0] = 9.0f / 16.0f; viewProj.m[5] = -1.0f; viewProj.m[11] = 1.0f; viewProj.m[14] = 0.01f;
        const uint32_t passCount = 1;
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
        GpuClusterCommands clusterCommands(gpu);
        writer.setCommands(&commands);
        commands.setClusterCommands(&clusterCommands);
        if (!writer.isSupported() || !commands.isSupported() || !clusterCommands.isSupported()) {
            printf("{\"ok\": false, \"why\": \"one context reported as unsupported\"}\n");
            return 1;
        }
        const GvInstanceLayout instanceLayout{sizeof(Instance), 0, GV_NONE, GV_NONE, GV_NONE};
        const GvCommandLayout commandLayout{sizeof(Command), offsetof(Command, indexCount), offsetof(Command, instanceCount),
                                            offsetof(Command, firstIndex), offsetof(Command, firstInstance), offsetof(Command, vertexOffset), GV_NONE};
        // the geometry table (the levels of a model are consecutive entries), the LOD table the base ids index, the clusters of
        // every level: a regular sub-grid of the model's box
        std::vector<GvGeometry> table;
        std::vector<GvLodGeometry> lods;
        std::vector<GvClusterRange> ranges;
        std::vector<GvCluster> clusters;
        std::vector<GvClusterCone> cones;
        std::vector<GvClusterLod> lodTable;
        for (uint32_t g = 0; g < kTable; g++) {
            table.push_back({3000u * (g + 1), 100000u * g, (int32_t)(g * 24u) - 100});
            GvLodGeometry e{};
            e.levels = g < kLevels * kBases && g % kLevels == 0 ? kLevels : 1u;
            for (uint32_t i = 0; i + 1 < e.levels; i++)
                e.switch_at[i] = 0.25f * side * (float)(i + 1) + (float)g;
            lods.push_back(e);
            if (g == kTable - 1)
                break;  // (no range for the last geometry: beyond range_count, drawn whole)
            // a binary DAG over cells^3 leaves in bit-interleaved order (bit b of the leaf index goes to axis b % 3): the levels one
            // behind the other, leaves first
            const uint32_t cells = kGrid[g % kLevels], leaves = cells * cells * cells;
            uint32_t depth = 1;
            while ((1u << (depth - 1)) < leaves)
                depth++;
            const uint32_t firstCluster = (uint32_t)clusters.size();
            ranges.push_back({firstCluster, 2u * leaves - 1u});
            std::vector<uint32_t> levelStart;
            uint32_t index = 0;
            for (uint32_t level = 0; level < depth; level++) {
                levelStart.push_back((uint32_t)clusters.size());
                for (uint32_t i = 0; i < (leaves >> level); i++) {
                    GvCluster c{};
                    GvClusterLod l{};
                    if (level == 0) {
                        uint32_t at[3] = {0, 0, 0};
                        for (uint32_t b = 0; b + 1 < depth; b++)
                            at[b % 3] |= ((i >> b) & 1u) << (b / 3);
                        float diagonal = 0.0f;
                        for (int a = 0; a < 3; a++) {
                            c.box_min[a] = -kHalf[a] + 2.0f * kHalf[a] * (float)at[a] / (float)cells;
                            c.box_max[a] = -kHalf[a] + 2.0f * kHalf[a] * (float)(at[a] + 1) / (float)cells;
                            l.self_center[a] = 0.5f * (c.box_min[a] + c.box_max[a]);
                            diagonal += (c.box_max[a] - c.box_min[a]) * (c.box_max[a] - c.box_min[a]);
                        }
                        l.self_radius = 0.5f * std::sqrt(diagonal) * 1.03f;
                        l.self_error = 0.0f;
                    } else {
                        const GvCluster &c0 = clusters[levelStart[level - 1] + 2 * i], &c1 = clusters[levelStart[level - 1] + 2 * i + 1];
                        const GvClusterLod &l0 = lodTable[levelStart[level - 1] + 2 * i], &l1 = lodTable[levelStart[level - 1] + 2 * i + 1];
                        for (int a = 0; a < 3; a++) {
                            c.box_min[a] = std::min(c0.box_min[a], c1.box_min[a]);
                            c.box_max[a] = std::max(c0.box_max[a], c1.box_max[a]);
                            l.self_center[a] = 0.5f * (c.box_min[a] + c.box_max[a]);
                        }
                        float reach = 0.0f;  // the radius that holds both children's spheres
                        for (const GvClusterLod* child : {&l0, &l1}) {
                            float d = 0.0f;
                            for (int a = 0; a < 3; a++)
                                d += (l.self_center[a] - child->self_center[a]) * (l.self_center[a] - child->self_center[a]);
                            reach = std::max(reach, std::sqrt(d) + child->self_radius);
                        }
                        l.self_radius = reach * 1.03f;
                        l.self_error = 0.02f * kHalf[1] * (float)(1u << (level - 1));
                    }
                    c.first = 30u * index + 5u * (index / 11u) + g;  // back to back, a hole of 5 indices behind every 11th cluster
                    c.count = 30u;
                    index++;
                    clusters.push_back(c);
                    lodTable.push_back(l);
                    // an outward cone on a leaf (none for a cell around the origin), a zero axis — never rejected — on an inner cluster
                    GvClusterCone cone{};
                    if (level == 0) {
                        float length = 0.0f;
                        for (int a = 0; a < 3; a++)
                            length += l.self_center[a] * l.self_center[a];
                        length = std::sqrt(length);
                        for (int a = 0; a < 3; a++) {
                            cone.axis[a] = length > 0.0f ? l.self_center[a] / length : 0.0f;
                            cone.apex[a] = l.self_center[a] - cone.axis[a] * (l.self_radius / 1.03f);
                        }
                    }
                    cone.cutoff = rng.uniform(0.1f, 0.8f);
                    cones.push_back(cone);
                }
            }
            for (uint32_t level = 0; level < depth; level++)  // the parent triple: the parent cluster's self triple; the root's own, +inf
                for (uint32_t i = 0; i < (leaves >> level); i++) {
                    GvClusterLod& l = lodTable[levelStart[level] + i];
                    const GvClusterLod& parent = level + 1 < depth ? lodTable[levelStart[level + 1] + i / 2] : l;
                    for (int a = 0; a < 3; a++)
                        l.parent_center[a] = parent.self_center[a];
                    l.parent_radius = parent.self_radius;
                    l.parent_error = level + 1 < depth ? parent.self_error : INFINITY;
                }
        }
        const float baseScale = 1.5f, shadowScale = 0.5f;
        std::vector<uint8_t> ids;
        std::vector<float> sizes;
        std::vector<Instance> base, shadow;
        uint64_t compared = 0, testedTotal = 0, baseKept = 0, survivors = 0, lodKept = 0, mainKept = 0, cascadeKept = 0, coneRejected = 0;
        const f32x4 lightDir(0.0f, 0.0f, 1.0f);  // the cascade's rays travel down +z: its projection puts z = -side nearest (reversed Z)
        const GvClusterEye cameraEye{{0.0f, 0.0f, 0.0f, 1.0f}}, cascadeEye = GpuClusterCommands::cascadeEye(lightDir);
        // the camera's LOD view: 1080 rows, 90 degrees, an error of 5 pixels; the cascade names the camera's eye, with half the scale
        const float k = GpuClusterCommands::lodScale(1.57079632679f, 1080.0f, 5.0f);
        const GvClusterLodView cameraLod{{0.0f, 0.0f, 0.0f, 1.0f}, k, 0.01f, {0.0f, 0.0f}}, cascadeLod{{0.0f, 0.0f, 0.0f, 1.0f}, 0.5f * k, 0.01f, {0.0f, 0.0f}};
        for (uint32_t tick = 0; tick < ticks; tick++) {
            graphicsSystem->setCamera(viewProj, f32x4(3.0f + 17.0f * (float)tick, -2.0f, 5.0f - 9.0f * (float)tick));
            if (tick) {  // movers, reported one by one
                for (uint32_t k = tick % 7; k < entities; k += 7)
                    if (auto t = transformSystem->tryGetOf(ents[k])) {
                        t->posChildCount.x += 0.75f;
                        transformSystem->markMoved(ents[k]);
                    }
            }
            manager.update();  // the prepare phase: the drop-in binds, culls and fills the engine's buffers
            const auto& meshSystems = gpu->getMeshSystems();
            if (meshSystems.size() != 1) {
                printf("{\"ok\": false, \"why\": \"%zu mesh systems\"}\n", meshSystems.size());
                return 1;
            }
            const uint32_t p = 0;
            auto meshSystem = meshSystems[p];
            const size_t componentSize = meshSystem->getMeshComponentSize();
            const uint32_t occupancy = meshSystem->getMeshComponentPool().getOccupancy();
            if (tick == 0) {
                writer.setLayout(p, instanceLayout);
                commands.setLayout(p, commandLayout);
                ids.resize(occupancy);
                for (auto& id : ids) {
                    const uint32_t r = rng.next() % 8u;
                    id = (uint8_t)(r == 7u ? kTable - 1 : kLevels * (r % kBases));
                }
                sizes.resize(occupancy);
                for (auto& r : sizes) r = rng.uniform(0.5f, 2.0f);
                commands.setGeometry(p, ids.data(), 1, 1, occupancy, table.data(), kTable);
                commands.setLods(p, sizes.data(), 4, occupancy, lods.data(), kTable);
                commands.setLodScale(p, baseScale, shadowScale);
                clusterCommands.setClusters(p, ranges.data(), (uint32_t)ranges.size(), clusters.data(), (uint32_t)clusters.size());
                clusterCommands.setClusterLods(p, lodTable.data(), (uint32_t)lodTable.size());
                clusterCommands.setLodViews(p, cameraLod, &cascadeLod, 1);
            }
            const bool withCones = tick >= 3u;
            if (tick == 3u) {
                clusterCommands.setCones(p, cones.data(), (uint32_t)cones.size());
                clusterCommands.setEyes(p, cameraEye, &cascadeEye, 1);
            }
            const bool asRuns = tick % 2u == 1u;
            clusterCommands.setRuns(p, asRuns);
            base.resize(occupancy);
            shadow.resize((size_t)occupancy * passCount);
            writer.write(p, base.data(), base.size() * sizeof(Instance), shadow.data(), shadow.size() * sizeof(Instance), passCount);

            // the host path, pass by pass
            auto idOf = [&](const auto& record, bool shadowPass) {
                const size_t slot = record.componentOffset / componentSize;
                const uint32_t b = ids[slot];
                const GvLodGeometry& e = lods[b];
                return lod_twin_effective(b, lod_twin_level(record.bakedModel.m, sizes[slot], shadowPass ? shadowScale : baseScale, e.levels, e.switch_at));
            };
            auto hostPass = [&](const UnsortedBuffer* buffer, bool shadowPass, uint32_t firstInstance, const float* vp, const GvClusterEye& eye, const GvClusterLodView& lodView,
                                std::vector<Command>& out, std::vector<uint32_t>& counts, std::vector<uint32_t>& tested) {
                HostPass h;
                size_t room = 1;
                for (uint32_t k = 0; k < buffer->drawCount; k++) {
                    const auto& record = buffer->meshes()[k];
                    h.models.insert(h.models.end(), record.bakedModel.m, record.bakedModel.m + 12);
                    h.ids.push_back(idOf(record, shadowPass));
                    h.first.push_back(firstInstance + k);
                    room += h.ids.back() < ranges.size() ? std::max(1u, ranges[h.ids.back()].count) : 1u;
                }
                h.first.push_back(firstInstance + buffer->drawCount);
                std::vector<ClusterTwinCommand> twin(room);
                uint32_t t = 0;
                ClusterLodCensus census;
                const uint32_t n = cluster_lod_twin_view(h.models.data(), h.ids.data(), h.first.data(), buffer->drawCount,
                                                         reinterpret_cast<const ClusterTwinGeometry*>(table.data()), kTable,
                                                         reinterpret_cast<const ClusterTwinRange*>(ranges.data()), (uint32_t)ranges.size(),
                                                         reinterpret_cast<const ClusterTwinCluster*>(clusters.data()),
                                                         reinterpret_cast<const ClusterLodTwinLod*>(lodTable.data()),
                                                         reinterpret_cast<const ClusterLodTwinView*>(&lodView),
                                                         withCones ? reinterpret_cast<const ClusterConeTwinCone*>(cones.data()) : nullptr,
                                                         withCones ? eye.eye : nullptr, vp, nullptr, nullptr,
                                                         asRuns ? CLUSTER_CONE_TWIN_RUNS : CLUSTER_CONE_TWIN_PLAIN, twin.data(), &t, nullptr, &census);
                baseKept += census.base_kept;
                survivors += census.survivors;
                lodKept += census.lod_kept;
                (shadowPass ? cascadeKept : mainKept) += census.lod_kept;
                coneRejected += census.lod_cone;
                for (uint32_t c = 0; c < n; c++)
                    out.push_back({twin[c].count, twin[c].instance_count, twin[c].first, twin[c].vertex_offset, twin[c].first_instance});
                counts.push_back(n);
                tested.push_back(t);
                testedTotal += t;
                return (uint32_t)buffer->drawCount;
            };
            std::vector<Command> light, dark;
            std::vector<uint32_t> lightCounts, lightTested, darkCounts, darkTested;
            hostPass(gpu->getUnsortedBuffers()[0], false, 0, viewProj.m, cameraEye, cameraLod, light, lightCounts, lightTested);
            if (!same(clusterCommands.getBase(p), light, lightCounts, lightTested, "the base cluster commands", tick))
                return 1;
            uint32_t shadowIndex = 0;  // shadowInstanceIndex: pass after pass
            for (int8_t pass : gpu->getSystemPasses(p)) {
                if (pass < 0)
                    continue;
                shadowIndex += hostPass(gpu->getShadowBuffers(0)[(uint32_t)pass], true, shadowIndex, passes[(uint32_t)pass].viewProj.m, cascadeEye, cascadeLod, dark,
                                        darkCounts, darkTested);
            }
            if (!same(clusterCommands.getShadow(p), dark, darkCounts, darkTested, "the shadow cluster commands", tick))
                return 1;
            compared += light.size() + dark.size();
            if (commands.getShadow(p).counts.size() != darkCounts.size() || commands.getBase(p).counts.size() != 1) {  // the per-draw commands stand beside them
                printf("{\"ok\": false, \"why\": \"tick %u: the per-draw commands are gone\"}\n", tick);
                return 1;
            }
        }
        printf("{\"ok\": true, \"passes\": %u, \"ticks\": %u, \"commands\": %llu, \"tested\": %llu, \"base_kept\": %llu, \"survivors\": %llu, "
               "\"lod_kept\": %llu, \"main_kept\": %llu, \"cascade_kept\": %llu, \"cone_rejected\": %llu}\n", passCount + 1, ticks,
               (unsigned long long)compared, (unsigned long long)testedTotal, (unsigned long long)baseKept, (unsigned long long)survivors,
               (unsigned long long)lodKept, (unsigned long long)mainKept, (unsigned long long)cascadeKept, (unsigned long long)coneRejected);
        return 0;
    } catch (const std::exception& e) {
        printf("{\"ok\": false, \"why\": \"%s\"}\n", e.what());
        return 1;
    }
}
