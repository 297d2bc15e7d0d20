// motion_history.hpp — last frame's mvp beside this frame's in the drop-in's instance buffers: what a velocity pass needs so that
// objects that MOVE get a motion vector too (the renderer's velocity.frag reprojects depth with cc.prevViewProj, which is right for
// the camera's own motion only). For a mesh system whose instance struct has a prevMvp field (and optionally a uint32 "had a
// history"), write() — behind GpuInstanceWriter::write for the same system and into the same base instance array — fills those
// fields for the light pass's draws on the device (gv_pool_emit_previous) and then keeps this frame's models
// as the next frame's history (gv_pool_keep_models). A draw nobody saw last frame is taken as static in the world. No host loop
// over the records, no second fetch of last frame's results, no join by slot.
//
// One context only, as the instance writer: with ranks no device holds a view's records in draw order — isSupported() is false
// and write() throws.
#pragma once
#include <cstdint>
#include <string>

#include "gpu_visibility_system.hpp"

namespace garden {

class GpuMotionHistory {
    GpuVisibilitySystem* system;
    GvPreviousLayout layouts[GV_MAX_POOLS];
    bool cutPending[GV_MAX_POOLS];

    void check(int rc, const char* what) const
    {
        if (rc != GV_OK)
            throw GardenError(std::string(what) + " failed: " + gv_last_error(system->getContext()));
    }

public:
    // what one write() left behind: the light pass's draws, how many of them had a history, the history's epoch before the keep
    struct Written {
        uint32_t drawCount = 0, keptCount = 0, epoch = 0;
    };

    explicit GpuMotionHistory(GpuVisibilitySystem* system) : system(system)
    {
        for (uint32_t p = 0; p < GV_MAX_POOLS; p++) {
            layouts[p] = GvPreviousLayout{0, 0, GV_NONE};
            cutPending[p] = false;
        }
    }

    bool isSupported() const noexcept { return system->getRankCount() == 1; }

    // where prevMvp (and the flag) lie in the instance struct of mesh system p: see GvPreviousLayout. The stride is the instance
    // struct's; keeping the fields apart from the instance layout's is the caller's business.
    void setLayout(uint32_t p, const GvPreviousLayout& layout)
    {
        if (p >= GV_MAX_POOLS)
            throw GardenError("GpuMotionHistory::setLayout: bad argument");
        layouts[p] = layout;
    }

    // a camera cut: the next write() of every system takes every draw as fresh against the frame's own viewProj (prevMvp == mvp)
    void cut() noexcept
    {
        for (bool& pending : cutPending)
            pending = true;
    }

    // slots [first, first + count) of mesh system p are fresh at its next write(): a teleported entity, a slot filled anew (the
    // history is not fed by dirty marks); count == 0 forgets the whole system
    void forget(uint32_t p, uint32_t first, uint32_t count) { check(gv_pool_forget_models(system->getContext(), p, first, count), "gv_pool_forget_models"); }

    // view: the system's light-pass view (the index at which getSystemPasses(p) holds a negative pass); dst: the system's mapped base
    // instance array, as handed to GpuInstanceWriter::write — only the layout's fields are written, draw k at instance k
    Written write(uint32_t p, uint32_t view, void* dst, size_t dstBytes)
    {
        if (!isSupported())
            throw GardenError("GpuMotionHistory: unsupported with several ranks (the merged draw order is made on the host)");
        if (p >= GV_MAX_POOLS || !layouts[p].stride)
            throw GardenError("GpuMotionHistory::write: no layout for this system (setLayout)");
        GvCtx* ctx = system->getContext();
        check(gv_pool_emit_previous(ctx, p, view, &layouts[p], nullptr, cutPending[p] ? GV_PREVIOUS_CUT : 0u, nullptr, 0), "gv_pool_emit_previous");
        cutPending[p] = false;
        check(gv_pool_keep_models(ctx, p, view, 0), "gv_pool_keep_models");  // (stream order: behind the emission that reads the old rows)
        uint32_t counts[4] = {};
        check(gv_pool_previous_fetch(ctx, p, dst, dstBytes, counts), "gv_pool_previous_fetch");
        Written out;
        out.drawCount = counts[0], out.keptCount = counts[1], out.epoch = counts[3];
        return out;
    }
};

}  // namespace garden
