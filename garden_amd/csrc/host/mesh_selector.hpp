// mesh_selector.hpp — the editor's click selection over the drop-in: MeshSelectorEditorSystem::render
// (source/editor/system/render/mesh-selector.cpp:67-122) with its per-entity loop (:78-122) replaced by gv_pick on every context
// of a GpuVisibilitySystem. The pools are the ones the drop-in bound for its last frame (pool p of every context = mesh system p),
// so select() belongs after a tick, where the editor's render() runs.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "gpu_visibility_system.hpp"

namespace garden {

class GpuMeshSelector {
    GpuVisibilitySystem* system;
    // where the last selection came from: resolves the selected entity to its slot without a scan when it still sits there
    uint32_t lastPool = GV_NONE, lastSlot = GV_NONE;

    static void transform(const f32x4x4& m, float x, float y, float z, float w, float out[4])
    {
        for (int r = 0; r < 4; r++)
            out[r] = m.m[r] * x + m.m[4 + r] * y + m.m[8 + r] * z + m.m[12 + r] * w;
    }
    // the slot of `entity` in pool p (GV_NONE: it has no component there) — getEntity() != selectedEntity, :110
    uint32_t slotOf(uint32_t p, IMeshRenderSystem* meshSystem, ID<Entity> entity) const
    {
        const uint32_t occupancy = meshSystem->getMeshComponentPool().getOccupancy();
        if (lastPool == p && lastSlot < occupancy && componentAt(meshSystem, lastSlot)->getEntity() == entity)
            return lastSlot;
        for (uint32_t i = 0; i < occupancy; i++)
            if (componentAt(meshSystem, i)->getEntity() == entity)
                return i;
        return GV_NONE;
    }

public:
    explicit GpuMeshSelector(GpuVisibilitySystem* system) : system(system) {}

    // mesh.cpp:120,139: base + i * componentSize
    static MeshRenderComponent* componentAt(IMeshRenderSystem* meshSystem, uint32_t slot)
    {
        return reinterpret_cast<MeshRenderComponent*>(reinterpret_cast<uint8_t*>(meshSystem->getMeshComponentPool().getData()) +
                                                      (size_t)slot * meshSystem->getMeshComponentSize());
    }

    // :72-76 — cursorPosition and windowSize in pixels (x, y used), invViewProj of the camera-relative viewProj
    static GvPickRay cursorRay(f32x4 cursorPosition, f32x4 windowSize, const f32x4x4& invViewProj)
    {
        const float nx = ((cursorPosition.x + 0.5f) / windowSize.x) * 2.0f - 1.0f;
        const float ny = ((cursorPosition.y + 0.5f) / windowSize.y) * 2.0f - 1.0f;
        float o[4], d[4];
        transform(invViewProj, nx, -ny, 1.0f, 1.0f, o);
        transform(invViewProj, nx, -ny, 0.0001f, 1.0f, d);
        GvPickRay ray{};
        for (int c = 0; c < 3; c++) {
            ray.origin[c] = o[c] / o[3];
            ray.direction[c] = d[c] / d[3] - ray.origin[c];
        }
        return ray;
    }

    // :67-122: the entity under the cursor whose pivot lies nearest the ray origin, never `selectedEntity`; a null ID if none.
    // Mesh systems in the drop-in's order, UI systems skipped (:84-85). Several ranks: every rank picks in its share (the index
    // maps give the engine's slots) and the smallest (distanceSq, system, slot) wins — the key each rank minimised.
    ID<Entity> select(f32x4 cursorPosition, f32x4 windowSize, const f32x4x4& invViewProj, f32x4 cameraPosition, ID<Entity> selectedEntity)
    {
        const auto& meshSystems = system->getMeshSystems();
        std::vector<uint32_t> pools, exclude;
        for (uint32_t p = 0; p < meshSystems.size(); p++) {
            if (meshSystems[p]->getMeshRenderType() == MeshRenderType::UI)
                continue;
            pools.push_back(p);
            exclude.push_back(selectedEntity ? slotOf(p, meshSystems[p], selectedEntity) : GV_NONE);
        }
        lastPool = lastSlot = GV_NONE;
        if (pools.empty())
            return {};
        const GvPickRay ray = cursorRay(cursorPosition, windowSize, invViewProj);
        const float camera[4] = {cameraPosition.x, cameraPosition.y, cameraPosition.z, 0.0f};
        uint64_t best = UINT64_MAX;
        GvPickHit found{GV_NONE, GV_NONE, 0.0f, 0};
        for (uint32_t r = 0; r < system->getRankCount(); r++) {
            GvPickHit hit;
            if (gv_pick(system->getContext(r), pools.data(), (uint32_t)pools.size(), exclude.data(), camera, &ray, 1, &hit) != GV_OK)
                throw GardenError(std::string("gv_pick failed: ") + gv_last_error(system->getContext(r)));
            if (hit.pool_id == GV_NONE)
                continue;
            uint32_t bits, order = 0;
            memcpy(&bits, &hit.distance_sq, 4);
            while (pools[order] != hit.pool_id)
                order++;
            const uint64_t key = ((uint64_t)bits << 32) | ((uint64_t)order << 28) | hit.slot;
            if (key < best)
                best = key, found = hit;
        }
        if (found.pool_id == GV_NONE)
            return {};
        lastPool = found.pool_id;
        lastSlot = found.slot;
        return componentAt(meshSystems[found.pool_id], found.slot)->getEntity();
    }
};

}  // namespace garden
