// occluders.hpp — a depth image for the Hi-Z query without a renderer: the drop-in's mesh systems give a few hundred large meshes a
// conservative inner box (a wall's slab, a building's core), and this object draws those boxes — of the draws a pass delivered —
// into a small depth image on the device and builds the pyramid from it (gv_pool_draw_occluders). A headless
// server, a shadow cascade or a pass nobody has drawn yet gets occlusion culling that way:
//   manager.update()                      the prepare phase: the first list, frustum only (or against last frame's pyramid)
//   begin(w, h); draw(p, view) ...        every system and pass whose occluders should count
//   build()                               the pyramid of the image; the next tick's light pass queries it (adoptPyramid)
//   GpuSecondPhase::run(p, true)          what the new pyramid lets through besides the first list
// setBoxes hands over one box per component of mesh system p, in the space its aabb lives in. THE BINDER'S CONTRACT: a box lies
// inside what the component draws; nobody checks it, and a box that sticks out culls what is visible. A component without an
// occluder gets an empty box (min == max). Edited boxes are reported with markBoxes.
//
// One context only, like the other readers of a view's records: isSupported() is false with several ranks.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "gpu_visibility_system.hpp"

namespace garden {

class GpuOccluders {
    GpuVisibilitySystem* system;
    std::vector<float> image;
    GvOccluderCounts held{};

    void check(int rc, const char* what) const
    {
        if (rc != GV_OK)
            throw GardenError(std::string(what) + " failed: " + gv_last_error(system->getContext()));
    }
    void checkSystem(uint32_t p) const
    {
        if (!isSupported())
            throw GardenError("GpuOccluders: unsupported with several ranks (no device holds a view's records)");
        if (p >= GV_MAX_POOLS || p >= system->getMeshSystems().size())
            throw GardenError("GpuOccluders: mesh system " + std::to_string(p) + " was not part of the last frame");
    }

public:
    explicit GpuOccluders(GpuVisibilitySystem* system) : system(system) {}

    bool isSupported() const noexcept { return system->getRankCount() == 1; }

    // Mesh system p's boxes: 3 floats each at boxMin + i * stride and boxMax + i * stride for component i < count. The arrays stay the
    // caller's and stay where they are until the next setBoxes of the system (NULL, NULL removes them).
    void setBoxes(uint32_t p, const float* boxMin, const float* boxMax, uint32_t stride, uint32_t count)
    {
        checkSystem(p);
        check(gv_pool_bind_occluders(system->getContext(), p, boxMin, boxMax, stride, count), "gv_pool_bind_occluders");
    }
    void markBoxes(uint32_t p, uint32_t first, uint32_t count)
    {
        checkSystem(p);
        check(gv_mark_dirty(system->getContext(), GV_DIRTY_OCCLUDER, (p << 28) | first, count), "gv_mark_dirty");
    }

    void begin(uint32_t width, uint32_t height) { check(gv_occluder_begin(system->getContext(), width, height), "gv_occluder_begin"); }

    // The occluders among the draws of pass `view` (an index among mesh system p's culled passes) into the open image. Asynchronous.
    void draw(uint32_t p, uint32_t view, uint32_t minPixels = 1)
    {
        checkSystem(p);
        if (!system->emitRecords)
            throw GardenError("GpuOccluders: occluders are the records' (emitRecords is off)");
        check(gv_pool_draw_occluders(system->getContext(), p, view, minPixels), "gv_pool_draw_occluders");
    }

    // The pyramid of the image; the light pass of the next tick queries it. Closes the image.
    void build()
    {
        check(gv_hiz_build_from_occluders(system->getContext()), "gv_hiz_build_from_occluders");
        system->adoptPyramid();
    }

    // Waits; the image of the last begin (rows of `width` floats) and its counts — for a debug view, or a host-side consumer.
    const std::vector<float>& fetch(uint32_t& width, uint32_t& height)
    {
        const void *depth = nullptr, *counts = nullptr;
        check(gv_occluder_depth_device(system->getContext(), &depth, &width, &height, &counts), "gv_occluder_depth_device");
        image.resize((size_t)width * height);
        check(gv_occluder_depth_fetch(system->getContext(), image.data(), image.size() * sizeof(float), &held), "gv_occluder_depth_fetch");
        return image;
    }
    const GvOccluderCounts& counts() const noexcept { return held; }
};

}  // namespace garden
