// draw_commands.hpp — the indirect draw commands of the drop-in's mesh systems, built on the device: for a mesh system that has
// declared its geometry (setGeometry), its command struct (setLayout) and how its commands are merged and placed (setMode),
// GpuInstanceWriter::write() — given this object through setCommands — follows each of its two instance emissions with a command
// emission (gv_pool_emit_draw_commands): one for the light pass behind the system's base instance array, one for the shadow passes,
// in pass order, behind its shadow array. A command emission belongs to the instance emission in front of it: first_instance
// indexes the array that emission filled. What the reference's draw loops would record as one drawAsync per record
// (mesh.cpp:589-601) is then a buffer a renderer submits as one indirect draw per pass (DrawIndexedIndirectCommand with offset,
// drawCount and stride, graphics/command-buffer.hpp:210-229), with drawCount from getBase / getShadow (packed) or the region size
// (regions: no count has to be read back).
//
// The commands land in caller-owned device memory when setTargets names some (a renderer's indirect buffers), else in the
// library's own buffer; either way they are fetched into host copies (getBase / getShadow) unless setFetch(false) — the library's
// buffer is reused by the next emission of the pool, so without device targets the host copies are what survives a write().
//
// Levels of detail: a system that has declared them (setLods: a size per component and, per BASE geometry, how many consecutive
// entries of the geometry table are its levels and where they switch) gets a selection (gv_pool_select_lods) in front of each
// command emission: every draw then takes the entry of its level, chosen per pass on the device from the record's distance
// (DESIGN.md §4 item 11). setLodScale gives the light pass and the shadow passes their view scales.
//
// Grouping: run mode merges CONSECUTIVE draws of one id, and an unsorted system's records arrive in space order. setGrouping(p, true)
// makes GpuInstanceWriter::write() group every view it is about to emit by geometry (gv_pool_group_draws; with LODs by geometry +
// level, GV_GROUP_BY_LOD with that pass's scale) in front of its emissions: run mode then writes one command per geometry (or
// level) and pass. The records delivered to the host afterwards are in the grouped order too. A sorted system's order is the
// distance order: it cannot be grouped, and asking for it throws.
//
// One context only, like the writer: with ranks no device holds a view's records in draw order — isSupported() is false.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "cluster_commands.hpp"
#include "gpu_visibility_system.hpp"

namespace garden {

class GpuDrawCommands {
public:
    // what one command emission left behind
    struct Emitted {
        std::vector<uint8_t> commands;  // the command positions, stride bytes each (empty with setFetch(false))
        std::vector<uint32_t> counts;   // commands per listed view: the light pass, or the culled shadow passes in pass order
        uint32_t stride = 0, region = 0;
    };

private:
    GpuVisibilitySystem* system;
    struct PerSystem {
        bool enabled = false;  // a layout is set
        uint32_t flags = 0, region = 0;
        void *baseDevice = nullptr, *shadowDevice = nullptr;
        size_t baseBytes = 0, shadowBytes = 0;
        uint32_t stride = 0;
        bool lods = false;     // an LOD table is bound: emit() selects in front of the commands
        bool grouping = false; // group() reorders the views by geometry in front of the instance emissions
        float baseScale = 1.0f, shadowScale = 1.0f;
        Emitted base, shadow;
    } per[GV_MAX_POOLS];
    bool fetch = true;
    GpuClusterCommands* clusters = nullptr;

    void check(int rc, const char* what) const
    {
        if (rc != GV_OK)
            throw GardenError(std::string(what) + " failed: " + gv_last_error(system->getContext()));
    }
    PerSystem& of(uint32_t p)
    {
        if (p >= GV_MAX_POOLS)
            throw GardenError("GpuDrawCommands: mesh system out of range");
        return per[p];
    }

public:
    explicit GpuDrawCommands(GpuVisibilitySystem* system) : system(system) {}

    bool isSupported() const noexcept { return system->getRankCount() == 1; }

    // the geometry ids of mesh system p's components (element i at ids + i * stride, 1, 2 or 4 bytes wide; NULL: every draw takes
    // table[0]) and the table they index (gv_pool_bind_geometry; re-issue when the pool's storage may have moved, report edits with
    // GV_DIRTY_GEOMETRY or GV_DIRTY_MESH)
    void setGeometry(uint32_t p, const void* ids, uint32_t stride, uint32_t width, uint32_t occupancy, const GvGeometry* table, uint32_t tableCount)
    {
        check(gv_pool_bind_geometry(system->getContext(), p, ids, stride, width, occupancy, table, tableCount), "gv_pool_bind_geometry");
    }
    // the levels of detail of mesh system p: the sizes of its components (element i at sizes + i * stride, fp32; NULL: every size is 1)
    // and the table the BASE geometry ids index (gv_pool_bind_lod; both NULL: no LODs; report size edits with GV_DIRTY_LOD or
    // GV_DIRTY_MESH). ModelRenderComponent::lods[L] of a model is entry base + L of the geometry table.
    void setLods(uint32_t p, const void* sizes, uint32_t stride, uint32_t occupancy, const GvLodGeometry* table, uint32_t tableCount)
    {
        check(gv_pool_bind_lod(system->getContext(), p, sizes, stride, occupancy, table, tableCount), "gv_pool_bind_lod");
        of(p).lods = table != nullptr;
    }
    // view_scale of the light pass and of every shadow pass (for example (tan(fov / 2) / height)^2, or a quality bias; default 1)
    void setLodScale(uint32_t p, float baseScale, float shadowScale)
    {
        of(p).baseScale = baseScale;
        of(p).shadowScale = shadowScale;
    }
    // the command struct of mesh system p: see GvCommandLayout
    void setLayout(uint32_t p, const GvCommandLayout& layout)
    {
        check(gv_pool_set_command_layout(system->getContext(), p, &layout), "gv_pool_set_command_layout");
        of(p).enabled = true;
        of(p).stride = layout.stride;
    }
    // flags: 0 or GV_COMMANDS_MERGE_RUNS; region: 0 packs the passes' commands, R > 0 gives every pass R positions
    void setMode(uint32_t p, uint32_t flags, uint32_t region)
    {
        of(p).flags = flags;
        of(p).region = region;
    }
    // caller-owned, 16-byte aligned device memory for the two command arrays of mesh system p (NULL: the library's buffer)
    void setTargets(uint32_t p, void* baseDevice, size_t baseBytes, void* shadowDevice, size_t shadowBytes)
    {
        PerSystem& s = of(p);
        s.baseDevice = baseDevice, s.baseBytes = baseBytes, s.shadowDevice = shadowDevice, s.shadowBytes = shadowBytes;
    }
    void setFetch(bool on) noexcept { fetch = on; }
    // optional: emit() then follows each command emission with the cluster cull of the systems that have declared clusters
    // (cluster_commands.hpp); NULL: none, every tick runs as before
    void setClusterCommands(GpuClusterCommands* clusterCommands) noexcept { clusters = clusterCommands; }
    // on: the views of mesh system p are grouped by geometry in front of the writer's emissions (see above). Unsorted systems only:
    // GardenError for a sorted one, here when the last frame already knows the system, otherwise at the write().
    void setGrouping(uint32_t p, bool on)
    {
        PerSystem& s = of(p);
        if (on && p < system->getMeshSystems().size() && system->isSystemSorted(p))
            throw GardenError("GpuDrawCommands::setGrouping: a sorted mesh system's order is the distance order");
        s.grouping = on;
    }

    // GpuInstanceWriter::write calls this in front of its emissions for mesh system p with the views it is about to emit (shadow: those
    // of the shadow array). Both calls come in front of the FIRST emission: gv_pool_group_draws refuses a pool that holds one.
    void group(uint32_t p, const uint32_t* views, uint32_t count, bool shadow)
    {
        PerSystem& s = of(p);
        if (!s.grouping || !count)
            return;
        if (!isSupported())
            throw GardenError("GpuDrawCommands: unsupported with several ranks (the merged draw order is made on the host)");
        if (system->isSystemSorted(p))
            throw GardenError("GpuDrawCommands: grouping a sorted mesh system (its order is the distance order)");
        for (uint32_t k = 0; k < count; k++)
            check(gv_pool_group_draws(system->getContext(), p, views[k], s.lods ? GV_GROUP_BY_LOD : 0u, shadow ? s.shadowScale : s.baseScale),
                  "gv_pool_group_draws");
    }

    // GpuInstanceWriter::write calls this behind each of its emissions for mesh system p (shadow: the one into the shadow array)
    void emit(uint32_t p, bool shadow)
    {
        PerSystem& s = of(p);
        if (!s.enabled)
            return;
        if (!isSupported())
            throw GardenError("GpuDrawCommands: unsupported with several ranks (the merged draw order is made on the host)");
        GvCtx* ctx = system->getContext();
        if (s.lods) {  // the levels of this emission's draws first: the commands take the selected ids
            uint32_t listed = 0;
            float scales[GV_MAX_VIEWS];
            check(gv_pool_instances_info(ctx, p, &listed, nullptr, nullptr), "gv_pool_instances_info");
            std::fill(scales, scales + GV_MAX_VIEWS, shadow ? s.shadowScale : s.baseScale);
            check(gv_pool_select_lods(ctx, p, scales, listed), "gv_pool_select_lods");
        }
        check(gv_pool_emit_draw_commands(ctx, p, s.flags, s.region, shadow ? s.shadowDevice : s.baseDevice, shadow ? s.shadowBytes : s.baseBytes),
              "gv_pool_emit_draw_commands");
        if (clusters)  // (behind the selection, if any: the cluster cull takes the same ids)
            clusters->cull(p, shadow, s.stride);
        Emitted& out = shadow ? s.shadow : s.base;
        out.stride = s.stride;
        out.region = s.region;
        out.commands.clear();
        if (!fetch) {
            out.counts.clear();
            return;
        }
        uint32_t views = 0, counts[GV_MAX_VIEWS];
        check(gv_pool_instances_info(ctx, p, &views, nullptr, nullptr), "gv_pool_instances_info");
        check(gv_pool_draw_commands_fetch(ctx, p, nullptr, 0, counts, GV_MAX_VIEWS), "gv_pool_draw_commands_fetch");
        out.counts.assign(counts, counts + views);
        size_t positions = (size_t)views * s.region;
        if (!s.region)
            for (uint32_t c : out.counts)
                positions += c;
        const size_t room = (shadow ? s.shadowDevice : s.baseDevice) ? (shadow ? s.shadowBytes : s.baseBytes) / s.stride : positions;
        out.commands.resize(std::min(positions, room) * s.stride);
        check(gv_pool_draw_commands_fetch(ctx, p, out.commands.data(), out.commands.size(), counts, GV_MAX_VIEWS), "gv_pool_draw_commands_fetch");
    }

    const Emitted& getBase(uint32_t p) { return of(p).base; }
    const Emitted& getShadow(uint32_t p) { return of(p).shadow; }
};

}  // namespace garden
