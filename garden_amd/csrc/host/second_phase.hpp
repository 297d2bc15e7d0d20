// second_phase.hpp — the second phase of two-phase occlusion culling for the drop-in's unsorted mesh systems. The pyramid the light
// pass queries is built behind the PREVIOUS frame's depth pass (HizRenderSystem::preHdrRender), so a box that has just come into view
// stays "occluded" for a frame. With this object a renderer draws what the frame's prepare phase delivered, hands the depth of those
// draws to GpuVisibilitySystem::setHizDepth, and calls run(p): mesh system p's light pass is re-tested against the new pyramid on the
// device (gv_pool_cull_second_phase) and what the first phase left out comes back as UnsortedMesh records in the system's own record
// layout — draw them behind the first list. MeshRenderComponent::isVisible is written back as the UNION of both phases: the frame's
// final answer, which the light pass and the next frame's logic read.
//
// The result lives in a spare view of the pool (the index behind the system's culled passes), so an instance or command emission
// can list it like any view; the system's next cull ends it.
//
// A sorted system (Translucent, UI) throws: its order is the distance order of the whole list, which two lists drawn one behind
// the other do not have. One context only, like the writer: with ranks no device holds a view's records — isSupported() is false.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "gpu_visibility_system.hpp"

namespace garden {

class GpuSecondPhase {
    GpuVisibilitySystem* system;
    struct PerSystem {
        std::vector<UnsortedMesh> meshes;  // grown, never shrunk
        uint32_t drawCount = 0, instanceCount = 0;
        uint32_t view = GV_NONE;           // the pool's view that holds the result (GV_NONE: run(p) has not been called)
    } per[GV_MAX_POOLS];

    void check(int rc, const char* what) const
    {
        if (rc != GV_OK)
            throw GardenError(std::string(what) + " failed: " + gv_last_error(system->getContext()));
    }
    PerSystem& of(uint32_t p)
    {
        if (p >= GV_MAX_POOLS)
            throw GardenError("GpuSecondPhase: mesh system out of range");
        return per[p];
    }

public:
    explicit GpuSecondPhase(GpuVisibilitySystem* system) : system(system) {}

    bool isSupported() const noexcept { return system->getRankCount() == 1; }

    // Mesh system p (unsorted, its light pass culled this tick) against the pyramid as it stands now. Afterwards meshes(p)[0,
    // drawCount(p)) are the newly visible records — in the order of the system's own list: front to back when the drop-in sorts on
    // the device — and the components' isVisible bytes hold the union of both phases.
    // withHiz: query the pyramid even though the first phase did not — a headless frame, whose first phase had no pyramid and whose
    // occluders were drawn from its result (GpuOccluders).
    void run(uint32_t p, bool withHiz = false)
    {
        PerSystem& s = of(p);
        if (!isSupported())
            throw GardenError("GpuSecondPhase: unsupported with several ranks (no device holds a view's records)");
        if (p >= system->getMeshSystems().size())
            throw GardenError("GpuSecondPhase: mesh system " + std::to_string(p) + " was not part of the last frame");
        if (system->isSystemSorted(p))
            throw GardenError("GpuSecondPhase: a sorted mesh system's order is the distance order of the whole list");
        if (!system->emitRecords)
            throw GardenError("GpuSecondPhase: the second phase is defined by the first phase's records (emitRecords is off)");
        const auto& passes = system->getSystemPasses(p);
        uint32_t light = GV_NONE;
        for (uint32_t v = 0; v < passes.size(); v++)
            if (passes[v] < 0)
                light = v;
        if (light == GV_NONE)
            throw GardenError("GpuSecondPhase: the light pass of mesh system " + std::to_string(p) + " was not culled this tick");
        const uint32_t spare = (uint32_t)passes.size();
        if (spare >= GV_MAX_VIEWS)
            throw GardenError("GpuSecondPhase: mesh system " + std::to_string(p) + " has no spare view");
        GvCtx* ctx = system->getContext();
        IMeshRenderSystem* meshSystem = system->getMeshSystems()[p];
        GvView view = system->getSystemView(p, light);
        if (withHiz)
            view.use_hiz = 1;
        // (a frame with more passes may have left a record target at this index: the result must not land in that pass's array)
        check(gv_pool_set_record_target(ctx, p, spare, nullptr, 0), "gv_pool_set_record_target");
        check(gv_pool_cull_second_phase(ctx, p, light, spare, &view), "gv_pool_cull_second_phase");
        if (system->sortOnDevice && meshSystem->getMeshRenderType() != MeshRenderType::OIT)  // as the system's own list (sortMeshes, mesh.cpp:270-295)
            check(gv_pool_sort(ctx, p, spare, 0), "gv_pool_sort");
        GvResult r{};
        check(gv_pool_results_fetch(ctx, p, spare, 1, &r), "gv_pool_results_fetch");  // write-back: isVisible = the union
        s.view = spare;
        s.drawCount = r.draw_count;
        s.instanceCount = r.instance_count;
        if (s.meshes.size() < r.draw_count)
            s.meshes.resize(r.draw_count);
        if (r.draw_count && !r.visible_idx) {  // the pool has a record layout: the structs arrive as they are
            const void* records = nullptr;
            uint32_t count = 0;
            check(gv_pool_results_records(ctx, p, spare, &records, &count), "gv_pool_results_records");
            memcpy(static_cast<void*>(s.meshes.data()), records, (size_t)count * sizeof(UnsortedMesh));
            return;
        }
        const size_t componentSize = meshSystem->getMeshComponentSize();
        for (uint32_t k = 0; k < r.draw_count; k++) {
            s.meshes[k].componentOffset = (size_t)r.visible_idx[k] * componentSize;
            memcpy(s.meshes[k].bakedModel.m, r.baked_model + (size_t)k * 12, 48);
            s.meshes[k].distanceSq = r.distance_sq[k];
        }
    }

    const UnsortedMesh* meshes(uint32_t p) { return of(p).meshes.data(); }
    uint32_t drawCount(uint32_t p) { return of(p).drawCount; }
    uint32_t instanceCount(uint32_t p) { return of(p).instanceCount; }
    uint32_t viewIndex(uint32_t p) { return of(p).view; }  // for GpuInstanceWriter-style emissions of the result
};

}  // namespace garden
