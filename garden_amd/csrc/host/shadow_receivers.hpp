// shadow_receivers.hpp — shadow-caster culling against what the main pass sees: the reference culls every cascade as a plain frustum
// cull of the whole pool (mesh.cpp:795-847), and a cascade's box, long towards the light, holds many casters whose shadows fall on
// nothing the main camera sees. This object draws the cull AABBs of the main pass's draws into a receiver mask in a cascade's clip
// space on the device and builds the pyramid from it (gv_pool_draw_receivers); a cull of that cascade with
// use_hiz then drops every caster that lies behind all visible receivers under its footprint, or over none. Per cascade:
//   begin(w, h)                               a mask, cleared to "no receiver"
//   draw(p, view, cascade.viewProj) ...       every mesh system that receives shadows; `view`: the main pass among p's culled passes
//   build()                                   the pyramid of the mask; the cascade's cull queries it
//   cull(p, shadowPass)                       the cascade's pass again with use_hiz = 1: one gv_cull per cascade, the system's other
//                                             views where they were, so the main pass's records stay for the next cascade's mask
// The cascade comes from csm::cascade / csm::fit (csm_lite.hpp): the matrix the mask is drawn with is the one the cascade is culled
// with, and both passes share the main camera's position — a slot's record model is then the same in both, so a caster the main
// pass sees keeps itself. The context has ONE pyramid: the main pass's depth pyramid is gone once a mask is built and is rebuilt next
// frame, as it is every frame anyway; cascades culled this way leave the batched multi-view pass.
//
// One context only, like the other readers of a view's records: isSupported() is false with several ranks.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "csm_lite.hpp"
#include "gpu_visibility_system.hpp"

namespace garden {

class GpuShadowReceivers {
    GpuVisibilitySystem* system;
    std::vector<float> image;
    GvReceiverCounts held{};
    std::vector<UnsortedMesh> list;  // cull(): the cascade's records
    uint32_t count = 0;

    void check(int rc, const char* what) const
    {
        if (rc != GV_OK)
            throw GardenError(std::string(what) + " failed: " + gv_last_error(system->getContext()));
    }
    void checkSystem(uint32_t p) const
    {
        if (!isSupported())
            throw GardenError("GpuShadowReceivers: unsupported with several ranks (no device holds a view's records)");
        if (p >= GV_MAX_POOLS || p >= system->getMeshSystems().size())
            throw GardenError("GpuShadowReceivers: mesh system " + std::to_string(p) + " was not part of the last frame");
    }

public:
    explicit GpuShadowReceivers(GpuVisibilitySystem* system) : system(system) {}

    bool isSupported() const noexcept { return system->getRankCount() == 1; }

    void begin(uint32_t width, uint32_t height) { check(gv_receiver_begin(system->getContext(), width, height), "gv_receiver_begin"); }

    // The draws of pass `view` (an index among mesh system p's culled passes: the main pass) into the open mask, as the cascade whose
    // viewProj is given sees them. Asynchronous.
    void draw(uint32_t p, uint32_t view, const f32x4x4& cascadeViewProj)
    {
        checkSystem(p);
        if (!system->emitRecords)
            throw GardenError("GpuShadowReceivers: receivers are the records' (emitRecords is off)");
        check(gv_pool_draw_receivers(system->getContext(), p, view, cascadeViewProj.m), "gv_pool_draw_receivers");
    }
    void draw(uint32_t p, uint32_t view, const csm::Cascade& cascade) { draw(p, view, cascade.viewProj); }

    // The pyramid of the mask; the cascade's cull queries it. Closes the mask. (Not adoptPyramid: the pyramid is in the CASCADE's clip
    // space, and the light pass of the next tick must not query it — the renderer's depth, or an occluder image, is built again first.)
    void build() { check(gv_hiz_build_from_receivers(system->getContext()), "gv_hiz_build_from_receivers"); }

    // The cascade as the view to cull against the pyramid just built: its own viewProj and cameraOffset, the main camera's position
    // (the records of both passes are relative to it), use_hiz on.
    static GvView cascadeView(const csm::Cascade& cascade, const f32x4& cameraPosition, int32_t shadowPass, bool emitRecords = true)
    {
        GvView v{};
        for (int k = 0; k < 16; k++)
            v.view_proj[k] = cascade.viewProj.m[k];
        v.camera_position[0] = cameraPosition.x, v.camera_position[1] = cameraPosition.y, v.camera_position[2] = cameraPosition.z;
        v.camera_offset[0] = cascade.cameraOffset.x, v.camera_offset[1] = cascade.cameraOffset.y, v.camera_offset[2] = cascade.cameraOffset.z;
        v.shadow_pass = shadowPass;
        v.use_hiz = 1;
        v.emit_records = emitRecords ? 1 : 0;
        return v;
    }

    // The view index of the main (light) pass among mesh system p's culled passes, and of shadow pass `shadowPass`.
    uint32_t passView(uint32_t p, int8_t shadowPass) const
    {
        checkSystem(p);
        const auto& passes = system->getSystemPasses(p);
        for (uint32_t v = 0; v < passes.size(); v++)
            if (shadowPass < 0 ? passes[v] < 0 : passes[v] == shadowPass)
                return v;
        throw GardenError("GpuShadowReceivers: pass " + std::to_string(shadowPass) + " of mesh system " + std::to_string(p) + " was not culled this tick");
    }

    // Culls shadow pass `shadowPass` of mesh system p again, against the pyramid just built: the system's own views of this tick,
    // every one where it was — so the main pass's records stay at their index for the next cascade's mask — with that pass's view
    // querying the pyramid. One gv_cull per cascade: cascades culled this way leave the one batched pass. Waits; afterwards
    // meshes()[0, drawCount()) are the cascade's records (unsorted mesh systems; in the order of delivery).
    void cull(uint32_t p, int8_t shadowPass)
    {
        const uint32_t target = passView(p, shadowPass);
        const auto& passes = system->getSystemPasses(p);
        std::vector<GvView> views;
        for (uint32_t v = 0; v < passes.size(); v++)
            views.push_back(system->getSystemView(p, v));
        views[target].use_hiz = 1;
        for (uint32_t v = 0; v < passes.size(); v++)
            if (v != target && passes[v] < 0)
                views[v].use_hiz = 0;  // (the pyramid is the cascade's: the main pass is culled again by its frustum alone — a superset)
        GvCtx* ctx = system->getContext();
        check(gv_pool_set_record_target(ctx, p, target, nullptr, 0), "gv_pool_set_record_target");  // (the result is this object's)
        check(gv_cull(ctx, p, views.data(), (uint32_t)views.size()), "gv_cull");
        GvResult r{};
        check(gv_pool_results_fetch(ctx, p, target, 0, &r), "gv_pool_results_fetch");
        count = r.draw_count;
        if (list.size() < r.draw_count)
            list.resize(r.draw_count);
        if (r.draw_count && !r.visible_idx) {  // the pool has a record layout: the structs arrive as they are
            const void* records = nullptr;
            uint32_t n = 0;
            check(gv_pool_results_records(ctx, p, target, &records, &n), "gv_pool_results_records");
            memcpy(static_cast<void*>(list.data()), records, (size_t)n * sizeof(UnsortedMesh));
            return;
        }
        const size_t componentSize = system->getMeshSystems()[p]->getMeshComponentSize();
        for (uint32_t k = 0; k < r.draw_count; k++) {
            list[k].componentOffset = (size_t)r.visible_idx[k] * componentSize;
            memcpy(list[k].bakedModel.m, r.baked_model + (size_t)k * 12, 48);
            list[k].distanceSq = r.distance_sq[k];
        }
    }
    const UnsortedMesh* meshes() const noexcept { return list.data(); }
    uint32_t drawCount() const noexcept { return count; }

    // Waits; the counts of the last begin's draws: every record in exactly one of drawn, flat, behind, range, outside.
    const GvReceiverCounts& counts()
    {
        check(gv_receiver_mask_fetch(system->getContext(), nullptr, 0, &held), "gv_receiver_mask_fetch");
        return held;
    }

    // Waits; the mask of the last begin (rows of `width` floats, +inf where no receiver lies) — for a debug view, or a host-side consumer.
    const std::vector<float>& fetch(uint32_t& width, uint32_t& height)
    {
        const void *mask = nullptr, *counts = nullptr;
        check(gv_receiver_mask_device(system->getContext(), &mask, &width, &height, &counts), "gv_receiver_mask_device");
        image.resize((size_t)width * height);
        check(gv_receiver_mask_fetch(system->getContext(), image.data(), image.size() * sizeof(float), &held), "gv_receiver_mask_fetch");
        return image;
    }
};

}  // namespace garden
