// instance_writer.hpp — the instance buffers of the drop-in's mesh systems, filled on the device: what prepareDraw / drawAsync /
// finalizeDraw leave in a system's instanceMap (source/system/render/instance.cpp:120-230) when every draw writes
// instanceData[instanceIndex].mvp = viewProj * model first (sprite.cpp:107-108,122-126). For a mesh system that declares its
// instance layout, write() — after the frame's prepare phase (preRender), where the render passes would start — emits the light
// pass into the system's base instance array and the shadow passes, in pass order, into its shadow array, which the reference
// fills pass after pass behind shadowInstanceIndex (instance.cpp:164,215), and returns the per-pass starts.
//
// A system whose instances carry fields of the draw's own component next to mvp (SpriteRenderSystem: color, uvSize, uvOffset,
// sprite.cpp:127-129) binds them as the pool's payload (setPayload) and says where they go in the base and in the shadow struct
// (setPayloadLayout; the two differ, instance.hpp:82-86): write() then produces the whole instance, in draw order, and no host loop
// over the records is left. The bytes are copied verbatim — srgbToRgb(color) is NOT applied (see gv_pool_bind_payload): bind a
// column that already holds the value the buffer should hold.
//
// One context only. With ranks (GpuVisibilitySystem(devices, ...)) every context holds the records of its own share and the
// frame's draw order is merged on the host (mergeRanks): no device holds a view's records in draw order, so there is nothing
// to emit from — isSupported() is false and write() throws.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "draw_commands.hpp"
#include "gpu_visibility_system.hpp"

namespace garden {

class GpuInstanceWriter {
    GpuVisibilitySystem* system;
    GpuDrawCommands* commands = nullptr;

    struct PayloadAt {
        uint32_t count = 0;  // 0: no payload destinations for this system
        uint32_t base[GV_MAX_PAYLOAD_FIELDS], shadow[GV_MAX_PAYLOAD_FIELDS];
    } payloadAt[GV_MAX_POOLS];

    void check(int rc, const char* what) const
    {
        if (rc != GV_OK)
            throw GardenError(std::string(what) + " failed: " + gv_last_error(system->getContext()));
    }

public:
    // what one write() left behind
    struct Written {
        uint32_t baseCount = 0;             // instances [0, baseCount) of the base array: the light pass's draws
        std::vector<uint32_t> shadowStart;  // [shadow passes + 1]: pass s took instances [shadowStart[s], shadowStart[s + 1]) of the
                                            // shadow array (a pass that was not culled for this system: an empty range)
    };

    explicit GpuInstanceWriter(GpuVisibilitySystem* system) : system(system) {}

    bool isSupported() const noexcept { return system->getRankCount() == 1; }

    // optional: write() then follows each of its emissions with the system's indirect draw commands (draw_commands.hpp); NULL: none
    void setCommands(GpuDrawCommands* drawCommands) noexcept { commands = drawCommands; }

    // the instance struct of mesh system p (pool p of the context): see GvInstanceLayout
    void setLayout(uint32_t p, const GvInstanceLayout& layout) { check(gv_pool_set_instance_layout(system->getContext(), p, &layout), "gv_pool_set_instance_layout"); }

    // the component fields mesh system p's instances carry (gv_pool_bind_payload: element i of field f at fields[f].data + i *
    // fields[f].stride; re-issue when the pool's storage may have moved, report edits with GV_DIRTY_PAYLOAD or GV_DIRTY_MESH);
    // count == 0 removes them. Every call leaves the destinations unset: setPayloadLayout follows it.
    void setPayload(uint32_t p, const GvPayloadField* fields, uint32_t count, uint32_t occupancy)
    {
        check(gv_pool_bind_payload(system->getContext(), p, fields, count, occupancy), "gv_pool_bind_payload");
        if (p < GV_MAX_POOLS && count == 0)
            payloadAt[p].count = 0;
    }
    // where field f goes in the base struct and in the shadow struct (GV_NONE: not written there; shadowAt NULL: nowhere in the shadow
    // struct, the usual case); `count` as in setPayload. Checked against the instance layout when write() emits.
    void setPayloadLayout(uint32_t p, const uint32_t* baseAt, const uint32_t* shadowAt, uint32_t count)
    {
        if (p >= GV_MAX_POOLS || count > GV_MAX_PAYLOAD_FIELDS || !baseAt)
            throw GardenError("GpuInstanceWriter::setPayloadLayout: bad argument");
        payloadAt[p].count = count;
        for (uint32_t f = 0; f < count; f++) {
            payloadAt[p].base[f] = baseAt[f];
            payloadAt[p].shadow[f] = shadowAt ? shadowAt[f] : GV_NONE;
        }
    }

    // base / shadow: the system's mapped instance arrays (NULL: that array is not wanted); only the layout's fields and the payload
    // destinations are written
    Written write(uint32_t p, void* base, size_t baseBytes, void* shadow, size_t shadowBytes, uint32_t shadowPassCount)
    {
        if (!isSupported())
            throw GardenError("GpuInstanceWriter: unsupported with several ranks (the merged draw order is made on the host)");
        GvCtx* ctx = system->getContext();
        const std::vector<int8_t>& passes = system->getSystemPasses(p);
        Written out;
        out.shadowStart.assign((size_t)shadowPassCount + 1, 0);
        std::vector<uint32_t> shadowViews;
        uint32_t starts[GV_MAX_VIEWS + 1];
        const PayloadAt& at = payloadAt[p < GV_MAX_POOLS ? p : 0];
        const bool payload = p < GV_MAX_POOLS && at.count != 0;
        if (commands) {  // setGrouping: the views about to be emitted, grouped by geometry in front of the emissions (both of them
                         // here: a pool that holds an emission is no longer grouped)
            std::vector<uint32_t> light, cascades;
            for (uint32_t v = 0; v < passes.size(); v++)
                (passes[v] >= 0 ? cascades : light).push_back(v);
            if (base)
                commands->group(p, light.data(), (uint32_t)light.size(), false);
            if (shadow)
                commands->group(p, cascades.data(), (uint32_t)cascades.size(), true);
        }
        for (uint32_t v = 0; v < passes.size(); v++) {
            if (passes[v] >= 0) {
                shadowViews.push_back(v);
            } else if (base) {
                if (payload)
                    check(gv_pool_set_payload_layout(ctx, p, at.base, at.count), "gv_pool_set_payload_layout");
                check(gv_pool_emit_instances(ctx, p, &v, 1, nullptr, 0), "gv_pool_emit_instances");
                check(gv_pool_instances_fetch(ctx, p, base, baseBytes, starts, GV_MAX_VIEWS + 1), "gv_pool_instances_fetch");
                out.baseCount = starts[1];
                if (commands)
                    commands->emit(p, false);
            }
        }
        if (shadow && !shadowViews.empty()) {
            if (payload)
                check(gv_pool_set_payload_layout(ctx, p, at.shadow, at.count), "gv_pool_set_payload_layout");
            check(gv_pool_emit_instances(ctx, p, shadowViews.data(), (uint32_t)shadowViews.size(), nullptr, 0), "gv_pool_emit_instances");
            check(gv_pool_instances_fetch(ctx, p, shadow, shadowBytes, starts, GV_MAX_VIEWS + 1), "gv_pool_instances_fetch");
            // the listed views are the culled passes in pass order: spread their starts over all passes
            uint32_t k = 0;
            for (uint32_t s = 0; s < shadowPassCount; s++) {
                out.shadowStart[s] = starts[k];
                if (k < shadowViews.size() && (uint32_t)passes[shadowViews[k]] == s)
                    k++;
            }
            out.shadowStart[shadowPassCount] = starts[shadowViews.size()];
            if (commands)
                commands->emit(p, true);
        }
        return out;
    }
};

}  // namespace garden
