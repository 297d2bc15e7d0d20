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
// pass sees keeps itself. In this order the context has ONE pyramid: the main pass's depth pyramid is gone once a mask is built and is
// rebuilt next frame, as it is every frame anyway; cascades culled this way leave the batched multi-view pass.
//
// With pyramid slots (gv_hiz_select) every cascade's mask gets a pyramid of its own and the cascades stay in ONE cull:
//   per cascade k: begin(w, h, 1 + k), draw(...), build()      the mask's pyramid lands in slot 1 + k; slot 0 is selected again
//   cullCascades(p, {0, 1, 2}, {1, 2, 3})                     ONE gv_cull of the system's views: the main pass as the system set it
//                                                             (its own use_hiz, pyramid 0 untouched), shadow pass k against slot 1 + k
// The main pass's depth pyramid — slot 0, what GpuVisibilitySystem::setHizDepth / adoptPyramid and the next tick mean — is never
// touched, so GpuSecondPhase of the main pass may run after the masked cascades of the same tick. cull() stays the default.
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
    struct CascadeList {             // cullCascades(): the records of one listed cascade
        std::vector<UnsortedMesh> meshes;  // grown, never shrunk
        uint32_t count = 0;
    };
    std::vector<CascadeList> lists;

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

    // Waits; the records of view `target` of mesh system p into `out[0, n)`
    void fetchList(uint32_t p, uint32_t target, std::vector<UnsortedMesh>& out, uint32_t& n)
    {
        GvCtx* ctx = system->getContext();
        GvResult r{};
        check(gv_pool_results_fetch(ctx, p, target, 0, &r), "gv_pool_results_fetch");
        n = r.draw_count;
        if (out.size() < r.draw_count)
            out.resize(r.draw_count);
        if (r.draw_count && !r.visible_idx) {  // the pool has a record layout: the structs arrive as they are
            const void* records = nullptr;
            uint32_t held_records = 0;
            check(gv_pool_results_records(ctx, p, target, &records, &held_records), "gv_pool_results_records");
            memcpy(static_cast<void*>(out.data()), records, (size_t)held_records * sizeof(UnsortedMesh));
            return;
        }
        const size_t componentSize = system->getMeshSystems()[p]->getMeshComponentSize();
        for (uint32_t k = 0; k < r.draw_count; k++) {
            out[k].componentOffset = (size_t)r.visible_idx[k] * componentSize;
            memcpy(out[k].bakedModel.m, r.baked_model + (size_t)k * 12, 48);
            out[k].distanceSq = r.distance_sq[k];
        }
    }

public:
    explicit GpuShadowReceivers(GpuVisibilitySystem* system) : system(system) {}

    bool isSupported() const noexcept { return system->getRankCount() == 1; }

    void begin(uint32_t width, uint32_t height) { check(gv_receiver_begin(system->getContext(), width, height), "gv_receiver_begin"); }
    // ... whose pyramid build() will put into slot `pyramid` (1 .. GV_MAX_PYRAMIDS - 1: slot 0 is the main pass's depth pyramid)
    // Slot `pyramid` stays selected until build(), which selects slot 0 again — so does abandon(), for a caller who gives the mask up
    // (a draw() that threw, a cascade dropped half way), and so does GpuVisibilitySystem::setHizDepth before its own build: the next
    // tick's depth pyramid lands in slot 0 whatever was left selected. A caller who builds pyramids through the C-ABI himself in
    // between (gv_hiz_build, gv_hiz_build_from_occluders) builds into the slot selected then: call abandon() or build() first.
    void begin(uint32_t width, uint32_t height, uint32_t pyramid)
    {
        check(gv_hiz_select(system->getContext(), pyramid), "gv_hiz_select");
        try {
            begin(width, height);
        } catch (...) {
            (void)gv_hiz_select(system->getContext(), 0);
            throw;
        }
    }
    // Gives up the mask of the last begin(w, h, pyramid) without building it: slot 0 is selected again. (The open mask stays open
    // until the next begin; the slot keeps whatever pyramid it held.)
    void abandon() { check(gv_hiz_select(system->getContext(), 0), "gv_hiz_select"); }

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
    // Into the slot begin() selected; slot 0 is selected again afterwards, whether the build succeeded or not (what the system builds
    // next — setHizDepth, an occluder image — is the main pass's).
    void build()
    {
        const int rc = gv_hiz_build_from_receivers(system->getContext());
        const std::string why = rc != GV_OK ? gv_last_error(system->getContext()) : "";
        check(gv_hiz_select(system->getContext(), 0), "gv_hiz_select");
        if (rc != GV_OK)
            throw GardenError("gv_hiz_build_from_receivers failed: " + why);
    }

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

    // ... against the pyramid of slot `pyramid` (cullCascades)
    static GvView cascadeView(const csm::Cascade& cascade, const f32x4& cameraPosition, int32_t shadowPass, bool emitRecords, uint32_t pyramid)
    {
        GvView v = cascadeView(cascade, cameraPosition, shadowPass, emitRecords);
        v.use_hiz = (uint8_t)(1 + pyramid);
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
        fetchList(p, target, list, count);
    }
    const UnsortedMesh* meshes() const noexcept { return list.data(); }
    uint32_t drawCount() const noexcept { return count; }

    // The shadow passes `shadowPasses` of mesh system p again, pass k against the pyramid of slot pyramids[k] (begin(w, h, slot) ...
    // build() per cascade), in ONE gv_cull of the system's own views of this tick: the main pass exactly as the system set it — its own
    // use_hiz, against pyramid 0, which no mask has touched — and every pass that is not listed as it was. Views that share the camera
    // position (a main pass and its cascades do) are culled in one pass over the pool. Waits; afterwards meshes(k)[0, drawCount(k))
    // are the records of the k-th listed cascade (unsorted mesh systems; in the order of delivery).
    void cullCascades(uint32_t p, const std::vector<int8_t>& shadowPasses, const std::vector<uint32_t>& pyramids)
    {
        if (shadowPasses.size() != pyramids.size())
            throw GardenError("GpuShadowReceivers: one pyramid per listed shadow pass");
        const auto& passes = system->getSystemPasses(p);
        std::vector<GvView> views;
        for (uint32_t v = 0; v < passes.size(); v++)
            views.push_back(system->getSystemView(p, v));
        GvCtx* ctx = system->getContext();
        std::vector<uint32_t> targets;
        for (size_t k = 0; k < shadowPasses.size(); k++) {
            if (shadowPasses[k] < 0 || pyramids[k] >= GV_MAX_PYRAMIDS)
                throw GardenError("GpuShadowReceivers: cullCascades takes shadow passes and pyramid slots below GV_MAX_PYRAMIDS");
            targets.push_back(passView(p, shadowPasses[k]));
            views[targets[k]].use_hiz = (uint8_t)(1 + pyramids[k]);
            check(gv_pool_set_record_target(ctx, p, targets[k], nullptr, 0), "gv_pool_set_record_target");  // (the result is this object's)
        }
        check(gv_cull(ctx, p, views.data(), (uint32_t)views.size()), "gv_cull");
        if (lists.size() < shadowPasses.size())
            lists.resize(shadowPasses.size());
        for (size_t k = 0; k < shadowPasses.size(); k++)
            fetchList(p, targets[k], lists[k].meshes, lists[k].count);
    }
    const UnsortedMesh* meshes(size_t k) const { return lists.at(k).meshes.data(); }
    uint32_t drawCount(size_t k) const { return lists.at(k).count; }

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
