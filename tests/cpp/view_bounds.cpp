// view_bounds.cpp — TEST driver of host/view_bounds.hpp (GpuViewBounds): an ecsm_lite world of an Opaque mesh system with movers and
// the GpuVisibilitySystem drop-in. Per tick: manager.update() delivers the light pass's list; GpuViewBounds::request asks for the
// bounds of that pass in two bases (a rotation with a translation, and the identity) and fetch() brings 32 bytes each; a host loop
// over the delivered list — eight corners per record through the record's own bakedModel and the component's box, projected, folded
// in the order of the key — must give the same 32 bytes. Built by tests/cpp/view_bounds.mk, run by tests/test_gpu_view_bounds.py.
//
//   view_bounds [--entities N] [--ticks T]
// Prints one JSON line and, when everything held, "view_bounds ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../garden_amd/csrc/host/view_bounds.hpp"

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

static uint32_t keyOf(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
static float row(const float* m, int r, float x, float y, float z) { return fmaf(m[r], x, fmaf(m[3 + r], y, fmaf(m[6 + r], z, m[9 + r]))); }

// the host alternative: every record, every corner
static GvViewBounds hostBounds(const UnsortedMesh* meshes, uint32_t count, const uint8_t* components, const float* basis)
{
    GvViewBounds out;
    bool haveLo[3] = {false, false, false}, haveHi[3] = {false, false, false};
    for (int r = 0; r < 3; r++) {
        out.lo[r] = INFINITY;
        out.hi[r] = -INFINITY;
    }
    out.draw_count = count;
    out.nan_records = 0;
    for (uint32_t k = 0; k < count; k++) {
        const auto* component = reinterpret_cast<const MeshRenderComponent*>(components + meshes[k].componentOffset);
        const float* m = meshes[k].bakedModel.m;
        const float lo[3] = {component->aabb.min.x, component->aabb.min.y, component->aabb.min.z};
        const float hi[3] = {component->aabb.max.x, component->aabb.max.y, component->aabb.max.z};
        bool nan = false;
        for (int c = 0; c < 8; c++) {
            const float x = (c & 1) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 4) ? hi[2] : lo[2];
            const float px = row(m, 0, x, y, z), py = row(m, 1, x, y, z), pz = row(m, 2, x, y, z);
            for (int r = 0; r < 3; r++) {
                const float q = row(basis, r, px, py, pz);
                if (q != q) {
                    nan = true;
                    continue;
                }
                if (!haveLo[r] || keyOf(q) < keyOf(out.lo[r])) {
                    out.lo[r] = q;
                    haveLo[r] = true;
                }
                if (!haveHi[r] || keyOf(q) > keyOf(out.hi[r])) {
                    out.hi[r] = q;
                    haveHi[r] = true;
                }
            }
        }
        out.nan_records += nan ? 1u : 0u;
    }
    return out;
}

int main(int argc, char** argv)
{
    uint32_t entities = 20000, ticks = 4;
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
            MeshRenderComponent* m = *opaque->add(e);
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

        GpuViewBounds bounds(gpu);
        if (!bounds.isSupported()) {
            printf("{\"ok\": false, \"why\": \"one context reported as unsupported\"}\n");
            return 1;
        }
        // a rotation about (1, 2, 3) by 0.7 rad with a translation, and the identity
        const float ax = 1.0f / std::sqrt(14.0f), ay = 2.0f * ax, az = 3.0f * ax, cs = std::cos(0.7f), sn = std::sin(0.7f), t = 1.0f - cs;
        const float rotated[12] = {t * ax * ax + cs, t * ax * ay + sn * az, t * ax * az - sn * ay,
                                   t * ax * ay - sn * az, t * ay * ay + cs, t * ay * az + sn * ax,
                                   t * ax * az + sn * ay, t * ay * az - sn * ax, t * az * az + cs,
                                   12.5f, -7.25f, 100.0f};
        const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        uint64_t draws = 0;
        for (uint32_t tick = 0; tick < ticks; tick++) {
            if (tick) {  // movers, reported one by one
                for (uint32_t k = tick % 7; k < entities; k += 7)
                    if (auto tr = transformSystem->tryGetOf(ents[k])) {
                        tr->posChildCount.x += 0.75f;
                        transformSystem->markMoved(ents[k]);
                    }
            }
            manager.update();
            const auto& meshSystems = gpu->getMeshSystems();
            if (meshSystems.size() != 1) {
                printf("{\"ok\": false, \"why\": \"%zu mesh systems\"}\n", meshSystems.size());
                return 1;
            }
            const auto& passes = gpu->getSystemPasses(0);
            uint32_t light = GV_NONE;
            for (uint32_t v = 0; v < passes.size(); v++)
                if (passes[v] < 0)
                    light = v;
            if (light == GV_NONE) {
                printf("{\"ok\": false, \"why\": \"no light pass\"}\n");
                return 1;
            }
            GpuViewBounds::Item items[2];
            items[0].view = items[1].view = light;
            memcpy(items[0].basis, rotated, sizeof(rotated));
            memcpy(items[1].basis, identity, sizeof(identity));
            bounds.request(0, {items[0], items[1]});
            const std::vector<GvViewBounds> got = bounds.fetch(0);
            const UnsortedBuffer* buffer = gpu->getUnsortedBuffers()[0];
            const uint32_t count = buffer->drawCount;
            const uint8_t* components = reinterpret_cast<const uint8_t*>(meshSystems[0]->getMeshComponentPool().getData());
            draws += count;
            for (uint32_t i = 0; i < 2; i++) {
                const GvViewBounds expected = hostBounds(buffer->meshes(), count, components, items[i].basis);
                if (got.size() != 2 || memcmp(&got[i], &expected, sizeof(expected)) != 0) {
                    printf("{\"ok\": false, \"why\": \"tick %u item %u: lo %g %g %g hi %g %g %g count %u, the host loop has lo %g %g %g hi %g %g %g "
                           "count %u\"}\n", tick, i, got[i].lo[0], got[i].lo[1], got[i].lo[2], got[i].hi[0], got[i].hi[1], got[i].hi[2],
                           got[i].draw_count, expected.lo[0], expected.lo[1], expected.lo[2], expected.hi[0], expected.hi[1], expected.hi[2],
                           expected.draw_count);
                    return 1;
                }
            }
        }
        const bool ok = draws > 0;
        printf("{\"ok\": %s, \"ticks\": %u, \"draws\": %llu}\n", ok ? "true" : "false", ticks, (unsigned long long)draws);
        if (ok)
            printf("view_bounds ok\n");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        printf("{\"ok\": false, \"why\": \"%s\"}\n", e.what());
        return 1;
    }
}
