// visible_delta.hpp — what came into view and what left it since last frame, for the drop-in's mesh systems (gv_pool_view_delta).
// Streaming, animation and audio want the components that came into view (load, wake) and those that left it (release, sleep):
// run(p) lists mesh system p's light pass — and the GpuSecondPhase view when one is named, so that the set is the frame's final
// answer — and appeared(p) / vanished(p) hand out their componentOffsets, ascending. writeBack(p) stores 1 / 0 into
// MeshRenderComponent::isVisible of exactly those components instead of the whole column (every store of the column is a cache line
// of its own: DESIGN.md §9); switch the drop-in's own write-back off with GpuVisibilitySystem::writeBackVisible = false.
//
// The delta write-back is right only over bytes that hold what the previous call saw. So writeBack(p) writes the whole column —
// and run(p) restarts the channel — on a system's first frame, after TransformSystem::hierarchyVersion changed (nobody itemised
// what moved where) and whenever the pool's occupancy changed (components came, went or were moved into freed slots).
//
// One context only, like the other emitters: with ranks no device holds a view's records — isSupported() is false.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "gpu_visibility_system.hpp"

namespace garden {

class GpuVisibleDelta {
    GpuVisibilitySystem* system;
    uint32_t channel;
    struct PerSystem {
        std::vector<size_t> appeared, vanished;  // componentOffsets, ascending; grown, never shrunk in capacity
        uint32_t visibleCount = 0;
        uint32_t views[2] = {GV_NONE, GV_NONE};  // the light pass and, when named, the second-phase view
        uint32_t viewCount = 0;                  // 0: run(p) has not been called
        bool full = false;                       // this frame's write-back is the whole column
        bool fetched = false, written = false;
        uint32_t seenOccupancy = GV_NONE;        // of the previous run (GV_NONE: none)
        uint64_t seenHierarchy = ~0ull;
    } per[GV_MAX_POOLS];

    void check(int rc, const char* what) const
    {
        if (rc != GV_OK)
            throw GardenError(std::string(what) + " failed: " + gv_last_error(system->getContext()));
    }
    PerSystem& of(uint32_t p)
    {
        if (p >= GV_MAX_POOLS)
            throw GardenError("GpuVisibleDelta: mesh system out of range");
        return per[p];
    }
    PerSystem& ran(uint32_t p)
    {
        PerSystem& s = of(p);
        if (!s.viewCount)
            throw GardenError("GpuVisibleDelta: run(" + std::to_string(p) + ") has not been called");
        return s;
    }
    // the one wait of the frame: the four counts, then the two lists; with `store` the library writes the listed bytes on the way
    void fetch(uint32_t p, PerSystem& s, bool store)
    {
        GvViewDelta d{};
        check(gv_pool_view_delta_fetch(system->getContext(), p, channel, store ? 1 : 0, &d), "gv_pool_view_delta_fetch");
        const size_t componentSize = system->getMeshSystems()[p]->getMeshComponentSize();
        s.appeared.resize(d.appeared_count);
        s.vanished.resize(d.vanished_count);
        for (uint32_t k = 0; k < d.appeared_count; k++)
            s.appeared[k] = (size_t)d.appeared[k] * componentSize;
        for (uint32_t k = 0; k < d.vanished_count; k++)
            s.vanished[k] = (size_t)d.vanished[k] * componentSize;
        s.visibleCount = d.visible_count;
        s.fetched = true;
    }

public:
    // channel: one of the pool's GV_MAX_DELTA_CHANNELS — two objects with different channels do not disturb each other
    explicit GpuVisibleDelta(GpuVisibilitySystem* system, uint32_t channel = 0) : system(system), channel(channel) {}

    bool isSupported() const noexcept { return system->getRankCount() == 1; }

    // Behind the frame's culls (and GpuSecondPhase::run(p), when secondView = its viewIndex(p) is named): asynchronous, the device
    // takes the difference against what the previous run saw and keeps this frame's set for the next.
    void run(uint32_t p, uint32_t secondView = GV_NONE)
    {
        PerSystem& s = of(p);
        if (!isSupported())
            throw GardenError("GpuVisibleDelta: unsupported with several ranks (no device holds a view's records)");
        if (p >= system->getMeshSystems().size())
            throw GardenError("GpuVisibleDelta: mesh system " + std::to_string(p) + " was not part of the last frame");
        const auto& passes = system->getSystemPasses(p);
        uint32_t light = GV_NONE;
        for (uint32_t v = 0; v < passes.size(); v++)
            if (passes[v] < 0)
                light = v;
        if (light == GV_NONE)
            throw GardenError("GpuVisibleDelta: the light pass of mesh system " + std::to_string(p) + " was not culled this tick");
        const uint32_t occupancy = system->getMeshSystems()[p]->getMeshComponentPool().getOccupancy();
        const uint64_t hierarchy = TransformSystem::Instance::get()->hierarchyVersion;
        s.full = s.seenOccupancy != occupancy || s.seenHierarchy != hierarchy;
        s.viewCount = 0;
        s.views[0] = light, s.views[1] = secondView;
        const uint32_t count = secondView == GV_NONE ? 1u : 2u;
        check(gv_pool_view_delta(system->getContext(), p, channel, s.views, count, s.full ? GV_DELTA_RESTART : 0u), "gv_pool_view_delta");
        s.viewCount = count;
        s.fetched = s.written = false;
        s.seenOccupancy = occupancy;
        s.seenHierarchy = hierarchy;
    }

    // Somebody else has written the isVisible bytes of mesh system p (or they were never written): the next run(p) restarts the
    // channel and its write-back is the whole column.
    void restart(uint32_t p) { of(p).seenOccupancy = GV_NONE; }

    // The componentOffsets (MeshRenderComponent of mesh system p at pool data + offset) that came into view / left it, ascending.
    // On a frame whose write-back is the whole column everything visible has "appeared". Valid until the next run(p).
    const std::vector<size_t>& appeared(uint32_t p)
    {
        PerSystem& s = ran(p);
        if (!s.fetched)
            fetch(p, s, false);
        return s.appeared;
    }
    const std::vector<size_t>& vanished(uint32_t p)
    {
        PerSystem& s = ran(p);
        if (!s.fetched)
            fetch(p, s, false);
        return s.vanished;
    }
    uint32_t visibleCount(uint32_t p)
    {
        appeared(p);
        return per[p].visibleCount;
    }
    bool wroteWholeColumn(uint32_t p) { return ran(p).full; }

    // MeshRenderComponent::isVisible of mesh system p brought up to date: the listed bytes only, or — see above — the whole column
    // (the final view's bytes: with a second phase the union, as GpuSecondPhase writes them).
    void writeBack(uint32_t p)
    {
        PerSystem& s = ran(p);
        if (s.written)
            return;
        if (s.full) {
            GvResult r{};
            check(gv_pool_results_fetch(system->getContext(), p, s.views[s.viewCount - 1], 1, &r), "gv_pool_results_fetch");
            if (!s.fetched)
                fetch(p, s, false);
        } else {
            fetch(p, s, true);
        }
        s.written = true;
    }
};

}  // namespace garden
