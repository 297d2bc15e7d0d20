// view_bounds.hpp — the bounds of what a mesh system's passes actually drew, for the code that fits a projection to it. The
// reference fits a shadow cascade to its slice of the camera frustum and stretches the light's depth range by zCoeff because it
// does not know where the casters are (csm.cpp:294-295); with this object a CSM system asks, behind the cascade's cull and in front
// of beginShadowRender: request(p, {{view, basis}, ...}) with csm::casterBasis(fit) as the basis, then fetch(p) — 32 bytes per
// item — and csm::tightenedDepth(fit, bounds) (csm_lite.hpp). The records stay on the device (gv_pool_view_bounds).
//
// One context only: with ranks a rank's device holds the records of its own share alone, so its bounds would be those of a part
// of the view — isSupported() is false, and folding the ranks' answers is not built.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "gpu_visibility_system.hpp"

namespace garden {

class GpuViewBounds {
    GpuVisibilitySystem* system;
    uint32_t requested[GV_MAX_POOLS] = {};  // items of the pool's last request (0: none)
    std::vector<GvViewBounds> fetched[GV_MAX_POOLS];

    void check(int rc, const char* what) const
    {
        if (rc != GV_OK)
            throw GardenError(std::string(what) + " failed: " + gv_last_error(system->getContext()));
    }

public:
    struct Item {
        uint32_t view;    // index among the mesh system's culled passes
        float basis[12];  // affine 3x4 in the layout of bakedModel: c0.xyz c1.xyz c2.xyz c3.xyz
    };

    explicit GpuViewBounds(GpuVisibilitySystem* system) : system(system) {}

    bool isSupported() const noexcept { return system->getRankCount() == 1; }

    // Asynchronous: queued behind the culls of mesh system p on the context's stream.
    void request(uint32_t p, const std::vector<Item>& items)
    {
        if (!isSupported())
            throw GardenError("GpuViewBounds: unsupported with several ranks (a rank sees only its own share's records)");
        if (p >= GV_MAX_POOLS || p >= system->getMeshSystems().size())
            throw GardenError("GpuViewBounds: mesh system " + std::to_string(p) + " was not part of the last frame");
        if (items.empty() || items.size() > GV_MAX_BOUNDS_ITEMS)
            throw GardenError("GpuViewBounds: " + std::to_string(items.size()) + " items (1 to " + std::to_string(GV_MAX_BOUNDS_ITEMS) + ")");
        uint32_t views[GV_MAX_BOUNDS_ITEMS];
        float bases[GV_MAX_BOUNDS_ITEMS * 12];
        for (size_t i = 0; i < items.size(); i++) {
            views[i] = items[i].view;
            memcpy(bases + 12 * i, items[i].basis, sizeof(items[i].basis));
        }
        requested[p] = 0;
        check(gv_pool_view_bounds(system->getContext(), p, views, bases, (uint32_t)items.size()), "gv_pool_view_bounds");
        requested[p] = (uint32_t)items.size();
    }

    // Waits for the request of mesh system p; one GvViewBounds per item, in the order requested.
    const std::vector<GvViewBounds>& fetch(uint32_t p)
    {
        if (p >= GV_MAX_POOLS || !requested[p])
            throw GardenError("GpuViewBounds: no request for mesh system " + std::to_string(p));
        fetched[p].resize(requested[p]);
        check(gv_pool_view_bounds_fetch(system->getContext(), p, fetched[p].data(), requested[p]), "gv_pool_view_bounds_fetch");
        return fetched[p];
    }
};

}  // namespace garden
