// cluster_second.cpp — TEST driver of GpuClusterCommands::cullSecond (host/cluster_commands.hpp): an ecsm_lite world of one Opaque
// mesh system whose geometries have 4^3, 2^3 or no clusters, boxes large against the frustum, a camera that moves every tick, the
// GpuVisibilitySystem drop-in with Hi-Z, and per tick two depth images of random walls, A (the old pyramid) and B (the new one):
//   setHizDepth(A), manager.update(), GpuInstanceWriter::write   phase 1: the draws, their commands, the cluster cull K1 against A
//   setHizDepth(B), GpuClusterCommands::cullSecond               the clusters K1 left out, against B
//   GpuSecondPhase::run, an emission of its view, cull()         the draws phase 1 left out, and THEIR clusters against B
// and a host path over the fetched records that decides every cluster with the oracle against the pyramids the oracle builds from A
// and B (tests/cluster_twin.h, tests/cluster_second_twin.h). Every command byte and every count of the three cluster results; K1's
// host copy is fetched again behind the second phase and must not have changed. Built by cluster_second.mk, run by
// tests/test_gpu_clusters_second.py.
//
//   cluster_second [--entities N] [--ticks T]
// Prints one JSON line: ok, ticks, K1's commands, pending clusters, second-phase commands, late draws and their cluster commands.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/host/instance_writer.hpp"
#include "../../garden_amd/csrc/host/second_phase.hpp"
#include "../cluster_second_twin.h"

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

constexpr uint32_t kTable = 3;                   // id 0: 4^3 clusters, id 1: 2^3, id 2: none (drawn whole)
constexpr float kHalf[3] = {9.0f, 6.0f, 12.0f};  // every model's box
static const uint32_t kGrid[2] = {4, 2};

// background 0 (far, reversed-Z) and `rects` walls at mid-scene depths: what lies behind one is occluded, what stands in front is not
static std::vector<float> walls(Rng& rng, uint32_t w, uint32_t h, uint32_t rects, float side)
{
    std::vector<float> d((size_t)w * h, 0.0f);
    for (uint32_t r = 0; r < rects; r++) {
        const uint32_t rw = w / 16 + rng.next() % (w / 4), rh = h / 16 + rng.next() % (h / 4);
        const uint32_t x = rng.next() % (w - rw), y = rng.next() % (h - rh);
        const float z = 0.01f / rng.uniform(0.05f * side, 0.4f * side);
        for (uint32_t j = y; j < y + rh; j++)
            for (uint32_t i = x; i < x + rw; i++)
                d[(size_t)j * w + i] = std::fmax(d[(size_t)j * w + i], z);
    }
    return d;
}

// the oracle's pyramid of one depth image
struct HostHiz {
    std::vector<float> depth, mips;
    GvoHiz hiz{};
    void build(const std::vector<float>& image, uint32_t width, uint32_t height)
    {
        depth = image;
        hiz = GvoHiz{};
        hiz.width = width, hiz.height = height;
        const uint64_t pairs = gvo_hiz_layout(width, height, &hiz);
        mips.assign((size_t)pairs * 2 + 2, 0.0f);
        hiz.depth = depth.data();
        hiz.mips = mips.data();
        gvo_hiz_build(&hiz, mips.data(), GVO_HIZ_RULE_REFERENCE);
    }
};

static std::vector<Command> laid(const std::vector<ClusterTwinCommand>& twin, uint32_t n)
{
    std::vector<Command> out;
    for (uint32_t c = 0; c < n; c++)
        out.push_back({twin[c].count, twin[c].instance_count, twin[c].first, twin[c].vertex_offset, twin[c].first_instance});
    return out;
}

static bool same(const GpuClusterCommands::Emitted& got, const std::vector<Command>& exp, uint32_t second_count, const char* what, uint32_t tick)
{
    if (got.counts.size() == 1 && got.counts[0] == exp.size() && got.tested.size() == 1 && got.tested[0] == second_count &&
        got.commands.size() == exp.size() * sizeof(Command) && (exp.empty() || memcmp(got.commands.data(), exp.data(), got.commands.size()) == 0))
        return true;
    printf("{\"ok\": false, \"why\": \"tick %u: %s differ from the host path (%zu commands and a second count of %u against %zu and %u)\"}\n", tick, what,
           got.commands.size() / sizeof(Command), got.tested.empty() ? 0u : got.tested[0], exp.size(), second_count);
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
        for (uint32_t i = 0; i < entities; i++) {
            auto e = manager.createEntity();
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

        GpuInstanceWriter writer(gpu);
        GpuDrawCommands commands(gpu);
        GpuClusterCommands clusterCommands(gpu);
        GpuSecondPhase second(gpu);
        writer.setCommands(&commands);
        commands.setClusterCommands(&clusterCommands);
        if (!writer.isSupported() || !commands.isSupported() || !clusterCommands.isSupported() || !second.isSupported()) {
            printf("{\"ok\": false, \"why\": \"one context reported as unsupported\"}\n");
            return 1;
        }
        const GvInstanceLayout instanceLayout{sizeof(Instance), 0, GV_NONE, GV_NONE, GV_NONE};
        const GvCommandLayout commandLayout{sizeof(Command), offsetof(Command, indexCount), offsetof(Command, instanceCount),
                                            offsetof(Command, firstIndex), offsetof(Command, firstInstance), offsetof(Command, vertexOffset), GV_NONE};
        std::vector<GvGeometry> table;
        std::vector<GvClusterRange> ranges;
        std::vector<GvCluster> clusters;
        for (uint32_t g = 0; g < kTable; g++) {
            table.push_back({3000u * (g + 1), 100000u * g, (int32_t)(g * 24u) - 100});
            if (g == kTable - 1)
                break;  // (no range for the last geometry: beyond range_count, drawn whole)
            const uint32_t cells = kGrid[g];
            ranges.push_back({(uint32_t)clusters.size(), cells * cells * cells});
            for (uint32_t j = 0; j < cells * cells * cells; j++) {
                const uint32_t at[3] = {j % cells, j / cells % cells, j / (cells * cells)};
                GvCluster c{};
                for (int a = 0; a < 3; a++) {
                    c.box_min[a] = -kHalf[a] + 2.0f * kHalf[a] * (float)at[a] / (float)cells;
                    c.box_max[a] = -kHalf[a] + 2.0f * kHalf[a] * (float)(at[a] + 1) / (float)cells;
                }
                c.first = 30u * j + g;
                c.count = 30u;
                clusters.push_back(c);
            }
        }
        const uint32_t width = 256, height = 128;
        std::vector<uint8_t> ids;
        std::vector<Instance> base;
        HostHiz hizA, hizB;
        uint64_t firstTotal = 0, pendingTotal = 0, secondTotal = 0, lateDraws = 0, lateCommands = 0;
        for (uint32_t tick = 0; tick < ticks; tick++) {
            graphicsSystem->setCamera(viewProj, f32x4(3.0f + 17.0f * (float)tick, -2.0f, 5.0f - 9.0f * (float)tick));
            const std::vector<float> a = walls(rng, width, height, 40, side), b = walls(rng, width, height, 40, side);
            hizA.build(a, width, height);
            hizB.build(b, width, height);
            gpu->setHizDepth(a.data(), width, height);
            manager.update();  // phase 1: the drop-in binds, culls against A and fills the engine's buffers
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
                for (auto& id : ids)
                    id = (uint8_t)(rng.next() % kTable);
                commands.setGeometry(p, ids.data(), 1, 1, occupancy, table.data(), kTable);
                clusterCommands.setClusters(p, ranges.data(), (uint32_t)ranges.size(), clusters.data(), (uint32_t)clusters.size());
            }
            base.resize(occupancy);
            writer.write(p, base.data(), base.size() * sizeof(Instance), nullptr, 0, 0);  // emission, commands, K1 against A
            const GpuClusterCommands::Emitted firstCopy = clusterCommands.getBase(p);

            // the host path over a list of records: K1-style (hiz1 alone) or the second phase (hiz1 then hiz2)
            struct HostList {
                std::vector<float> models;
                std::vector<uint32_t> ids, first;
                size_t room = 1;
            };
            auto listOf = [&](const UnsortedMesh* meshes, uint32_t count) {
                HostList h;
                for (uint32_t k = 0; k < count; k++) {
                    h.models.insert(h.models.end(), meshes[k].bakedModel.m, meshes[k].bakedModel.m + 12);
                    h.ids.push_back(ids[meshes[k].componentOffset / componentSize]);
                    h.first.push_back(k);
                    h.room += h.ids.back() < ranges.size() ? ranges[h.ids.back()].count : 1u;
                }
                h.first.push_back(count);
                return h;
            };
            auto firstPhase = [&](const HostList& h, const GvoHiz* hiz, uint32_t* tested) {
                std::vector<ClusterTwinCommand> twin(h.room);
                const uint32_t n = cluster_twin_view(h.models.data(), h.ids.data(), h.first.data(), (uint32_t)h.ids.size(),
                                                     reinterpret_cast<const ClusterTwinGeometry*>(table.data()), kTable,
                                                     reinterpret_cast<const ClusterTwinRange*>(ranges.data()), (uint32_t)ranges.size(),
                                                     reinterpret_cast<const ClusterTwinCluster*>(clusters.data()), viewProj.m, hiz, twin.data(), tested,
                                                     nullptr, nullptr);
                return laid(twin, n);
            };
            const UnsortedBuffer* buffer = gpu->getUnsortedBuffers()[0];
            const HostList drawn = listOf(buffer->meshes(), buffer->drawCount);
            uint32_t tested = 0;
            const std::vector<Command> first = firstPhase(drawn, &hizA.hiz, &tested);
            if (!same(clusterCommands.getBase(p), first, tested, "the first phase's cluster commands", tick))
                return 1;
            firstTotal += first.size();

            // the pyramid is rebuilt; the clusters K1 left out
            gpu->setHizDepth(b.data(), width, height);
            clusterCommands.cullSecond(p, false, sizeof(Command));
            std::vector<ClusterTwinCommand> twin(drawn.room);
            ClusterSecondTwinStats stats;
            const uint32_t n = cluster_second_twin_view(drawn.models.data(), drawn.ids.data(), drawn.first.data(), (uint32_t)drawn.ids.size(),
                                                        reinterpret_cast<const ClusterTwinGeometry*>(table.data()), kTable,
                                                        reinterpret_cast<const ClusterTwinRange*>(ranges.data()), (uint32_t)ranges.size(),
                                                        reinterpret_cast<const ClusterTwinCluster*>(clusters.data()), viewProj.m, &hizA.hiz, &hizB.hiz,
                                                        twin.data(), &stats);
            if (!same(clusterCommands.getBaseSecond(p), laid(twin, n), stats.pending, "the second phase's cluster commands", tick))
                return 1;
            pendingTotal += stats.pending;
            secondTotal += n;
            // K1's result stands: fetched again, byte for byte
            {
                GvCtx* ctx = gpu->getContext();
                uint32_t counts[2 * GV_MAX_VIEWS] = {};
                std::vector<uint8_t> again(firstCopy.commands.size());
                if (gv_pool_cluster_commands_fetch(ctx, p, again.data(), again.size(), counts, 2 * GV_MAX_VIEWS) != GV_OK || again != firstCopy.commands ||
                    counts[0] != firstCopy.counts[0] || counts[1] != firstCopy.tested[0]) {
                    printf("{\"ok\": false, \"why\": \"tick %u: the first phase's cluster commands changed behind the second phase\"}\n", tick);
                    return 1;
                }
            }

            // the draw-level second phase, its own emission and cluster cull: an ordinary view against B
            second.run(p);
            const uint32_t spare = second.viewIndex(p);
            GvCtx* ctx = gpu->getContext();
            if (gv_pool_emit_instances(ctx, p, &spare, 1, nullptr, 0) != GV_OK) {
                printf("{\"ok\": false, \"why\": \"tick %u: %s\"}\n", tick, gv_last_error(ctx));
                return 1;
            }
            clusterCommands.cull(p, false, sizeof(Command));
            const HostList late = listOf(second.meshes(p), second.drawCount(p));
            const std::vector<Command> lateExpected = firstPhase(late, &hizB.hiz, &tested);
            if (!same(clusterCommands.getBase(p), lateExpected, tested, "the cluster commands of the late draws", tick))
                return 1;
            lateDraws += second.drawCount(p);
            lateCommands += lateExpected.size();
        }
        printf("{\"ok\": true, \"ticks\": %u, \"first\": %llu, \"pending\": %llu, \"second\": %llu, \"late_draws\": %llu, \"late_commands\": %llu}\n", ticks,
               (unsigned long long)firstTotal, (unsigned long long)pendingTotal, (unsigned long long)secondTotal, (unsigned long long)lateDraws,
               (unsigned long long)lateCommands);
        return 0;
    } catch (const std::exception& e) {
        printf("{\"ok\": false, \"why\": \"%s\"}\n", e.what());
        return 1;
    }
}
