// cluster_commands.hpp — the cluster commands of the drop-in's mesh systems, built on the device: for a mesh system that has declared
// its clusters (setClusters) — per geometry id a range of model-space boxes with index ranges — GpuDrawCommands::emit(), given this
// object through GpuDrawCommands::setClusterCommands, follows each of its command emissions with a cluster cull
// (gv_pool_cull_clusters): every cluster of every delivered draw tested with the draw's own matrix against the pass's frustum and,
// where the pass named a pyramid, against that pyramid; one indirect command per surviving cluster — or, with setRuns, per run of
// adjacent surviving clusters (gv_pool_cull_cluster_runs) — a draw without clusters drawn whole. The per-draw commands stand beside them (a depth pre-pass may still take those). Geometry, command struct, LODs and
// grouping are the ones declared to GpuDrawCommands: the cluster cull takes the same ids — the selected ones behind a selection.
//
// The commands land in caller-owned device memory when setTargets names some, else in the library's own buffer; either way they
// are fetched into host copies (getBase / getShadow) unless setFetch(false). A renderer submits them as one indirect draw per pass:
// drawCount from counts[] (packed) or the region size (regions: no count has to be read back).
//
// With setCones a system's cluster culls also reject the clusters whose normal cone faces away from the pass's eye
// (gv_pool_cull_cluster_cones): the light pass is seen from the camera — the point eye (0, 0, 0, 1) of the camera-relative records —
// and a cascade along its light's direction (cascadeEye). setRuns, setMode and the targets combine with it.
// With setClusterLods a system's cluster culls are made over the CUT through the bound cluster DAG (gv_pool_cull_cluster_lods): a
// cluster is drawn when its own error is small enough on screen for the pass's LOD view (setLodViews, lodScale) and its parent's is
// not. It combines with setCones, setRuns, setMode and the targets; cullSecond takes nothing new, the library keeps the views.
//
// In a two-phase frame cullSecond(p, ...) re-tests what a system's last cluster cull left out against the rebuilt pyramid
// (gv_pool_cull_clusters_second_phase), into host copies of its own (getBaseSecond / getShadowSecond).
//
// Opt-in: a tick that sets no clusters runs exactly as before. One context only, like the writer: isSupported() is false with ranks.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "gpu_visibility_system.hpp"

namespace garden {

class GpuClusterCommands {
public:
    // what one cluster cull left behind
    struct Emitted {
        std::vector<uint8_t> commands;  // the command positions, stride bytes each (empty with setFetch(false))
        std::vector<uint32_t> counts;   // commands per listed view: the light pass, or the culled shadow passes in pass order
        std::vector<uint32_t> tested;   // clusters tested per listed view (draws drawn whole are not tested)
        uint32_t stride = 0, region = 0;
    };

private:
    GpuVisibilitySystem* system;
    struct PerSystem {
        bool enabled = false;  // clusters are bound
        bool runs = false;     // adjacent surviving clusters are merged into one command (gv_pool_cull_cluster_runs)
        bool cones = false;    // normal cones are bound: the culls are gv_pool_cull_cluster_cones
        GvClusterEye baseEye{{0.0f, 0.0f, 0.0f, 1.0f}};  // the camera, in the camera-relative space of the records
        std::vector<GvClusterEye> shadowEyes;            // by the shadow system's pass number; a pass beyond them: all zero, no cone test
        bool lods = false;     // a LOD table is bound: the culls are gv_pool_cull_cluster_lods, over the cut through the cluster DAG
        GvClusterLodView baseLod{{0.0f, 0.0f, 0.0f, 1.0f}, 0.0f, 1.0f, {0.0f, 0.0f}};  // scale 0: no LOD test until setLodViews
        std::vector<GvClusterLodView> shadowLods;        // by the shadow system's pass number; a pass beyond them: scale 0, no LOD test
        uint32_t flags = 0, region = 0;
        void *baseDevice = nullptr, *shadowDevice = nullptr;
        size_t baseBytes = 0, shadowBytes = 0;
        void *baseSecondDevice = nullptr, *shadowSecondDevice = nullptr;
        size_t baseSecondBytes = 0, shadowSecondBytes = 0;
        Emitted base, shadow, baseSecond, shadowSecond;
    } per[GV_MAX_POOLS];
    bool fetch = true;

    void check(int rc, const char* what) const
    {
        if (rc != GV_OK)
            throw GardenError(std::string(what) + " failed: " + gv_last_error(system->getContext()));
    }
    PerSystem& of(uint32_t p)
    {
        if (p >= GV_MAX_POOLS)
            throw GardenError("GpuClusterCommands: mesh system out of range");
        return per[p];
    }

public:
    explicit GpuClusterCommands(GpuVisibilitySystem* system) : system(system) {}

    bool isSupported() const noexcept { return system->getRankCount() == 1; }

    // the clusters of mesh system p: ranges[g] names the clusters of geometry id g (count 0, or g beyond rangeCount: drawn whole);
    // both tables are copied (gv_pool_bind_clusters). Both NULL: no clusters, the system's ticks run as before.
    void setClusters(uint32_t p, const GvClusterRange* ranges, uint32_t rangeCount, const GvCluster* clusters, uint32_t clusterCount)
    {
        check(gv_pool_bind_clusters(system->getContext(), p, ranges, rangeCount, clusters, clusterCount), "gv_pool_bind_clusters");
        of(p).enabled = ranges != nullptr;
        of(p).cones = false;  // (the library drops the cones with the table they belonged to)
        of(p).lods = false;   // (... and the LOD table)
    }
    // the LOD table of mesh system p's clusters, one GvClusterLod per entry of the cluster table and in its order (meshoptimizer
    // clusterlod bounds as they are); copied (gv_pool_bind_cluster_lods). NULL: no table, the culls run as before. Call it behind
    // setClusters.
    void setClusterLods(uint32_t p, const GvClusterLod* table, uint32_t count)
    {
        check(gv_pool_bind_cluster_lods(system->getContext(), p, table, count), "gv_pool_bind_cluster_lods");
        of(p).lods = table != nullptr;
    }
    // the LOD views of mesh system p's passes: the light pass's and one per shadow pass, indexed by the shadow system's pass number (a
    // cascade that wants the camera's cut names the camera's eye and scale; a pass without one gets no LOD test)
    void setLodViews(uint32_t p, const GvClusterLodView& baseView, const GvClusterLodView* shadowViews, uint32_t shadowViewCount)
    {
        of(p).baseLod = baseView;
        of(p).shadowLods.assign(shadowViews, shadowViews + shadowViewCount);
    }
    // k of a perspective view: the projection factor (height / 2) / tan(fovy / 2) divided by the pixel threshold
    static float lodScale(float fovy, float height, float pixels) { return 0.5f * height / std::tan(0.5f * fovy) / pixels; }
    // the normal cones of mesh system p's clusters, one per entry of the cluster table and in its order (meshopt_Bounds' cone_apex /
    // cone_axis / cone_cutoff as they are); copied (gv_pool_bind_cluster_cones). NULL: no cones, the culls run as before. Call it
    // behind setClusters.
    void setCones(uint32_t p, const GvClusterCone* cones, uint32_t count)
    {
        check(gv_pool_bind_cluster_cones(system->getContext(), p, cones, count), "gv_pool_bind_cluster_cones");
        of(p).cones = cones != nullptr;
    }
    // the eyes of mesh system p's passes: the light pass's (default: the camera, (0, 0, 0, 1)) and one per shadow pass, indexed by the
    // shadow system's pass number (cascadeEye of the pass's light direction; a pass without one gets no cone test)
    void setEyes(uint32_t p, const GvClusterEye& baseEye, const GvClusterEye* shadowEyes, uint32_t shadowEyeCount)
    {
        of(p).baseEye = baseEye;
        of(p).shadowEyes.assign(shadowEyes, shadowEyes + shadowEyeCount);
    }
    // the eye of a cascade: parallel rays that travel along the light direction given to csm::calcLightViewProj (csm_lite.hpp looks
    // from center - lightDir to center)
    static GvClusterEye cascadeEye(const f32x4& lightDir) { return GvClusterEye{{lightDir.x, lightDir.y, lightDir.z, 0.0f}}; }
    // flags: 0 or GV_CLUSTERS_FRUSTUM_ONLY; region: 0 packs the passes' commands, R > 0 gives every pass R positions
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
    // on: mesh system p's cluster culls write one command per RUN of adjacent surviving clusters (gv_pool_cull_cluster_runs) — for
    // a cluster table that lays a geometry's clusters out back to back in the index buffer, the same indices in far fewer commands.
    // Default off. The second phase (cullSecond) is unchanged and writes one command per cluster.
    void setRuns(uint32_t p, bool on) { of(p).runs = on; }
    void setFetch(bool on) noexcept { fetch = on; }

    // GpuDrawCommands::emit calls this behind each of its command emissions for mesh system p (shadow: the one behind the shadow
    // array) with the stride of the system's command struct; also callable behind an instance emission of one's own. eyes (with
    // setCones only): one eye per view of that emission, in its order, in place of the ones setEyes declared.
    void cull(uint32_t p, bool shadow, uint32_t stride, const GvClusterEye* eyes = nullptr, uint32_t eyeCount = 0)
    {
        PerSystem& s = of(p);
        if (!s.enabled)
            return;
        if (!isSupported())
            throw GardenError("GpuClusterCommands: unsupported with several ranks (the merged draw order is made on the host)");
        GvCtx* ctx = system->getContext();
        void* const device = shadow ? s.shadowDevice : s.baseDevice;
        const size_t bytes = shadow ? s.shadowBytes : s.baseBytes;
        std::vector<GvClusterEye> declared;
        if (s.cones || s.lods) {
            if (!eyes && s.cones) {  // the light pass, or the system's culled shadow passes in pass order
                if (!shadow)
                    declared.push_back(s.baseEye);
                else
                    for (int8_t pass : system->getSystemPasses(p))
                        if (pass >= 0)
                            declared.push_back((size_t)pass < s.shadowEyes.size() ? s.shadowEyes[(size_t)pass] : GvClusterEye{{0.0f, 0.0f, 0.0f, 0.0f}});
                eyes = declared.data();
                eyeCount = (uint32_t)declared.size();
            }
        }
        if (s.lods) {  // (eyes NULL without cones: no cone test)
            std::vector<GvClusterLodView> views;
            if (!shadow)
                views.push_back(s.baseLod);
            else
                for (int8_t pass : system->getSystemPasses(p))
                    if (pass >= 0)
                        views.push_back((size_t)pass < s.shadowLods.size() ? s.shadowLods[(size_t)pass]
                                                                           : GvClusterLodView{{0.0f, 0.0f, 0.0f, 0.0f}, 0.0f, 1.0f, {0.0f, 0.0f}});
            check(gv_pool_cull_cluster_lods(ctx, p, s.flags | (s.runs ? GV_CLUSTERS_RUNS : 0u), views.data(), (uint32_t)views.size(),
                                            s.cones ? eyes : nullptr, s.cones ? eyeCount : 0u, s.region, device, bytes),
                  "gv_pool_cull_cluster_lods");
        } else if (s.cones) {
            check(gv_pool_cull_cluster_cones(ctx, p, s.flags | (s.runs ? GV_CLUSTERS_RUNS : 0u), eyes, eyeCount, s.region, device, bytes),
                  "gv_pool_cull_cluster_cones");
        } else if (s.runs)
            check(gv_pool_cull_cluster_runs(ctx, p, s.flags, s.region, device, bytes), "gv_pool_cull_cluster_runs");
        else
            check(gv_pool_cull_clusters(ctx, p, s.flags, s.region, device, bytes), "gv_pool_cull_clusters");
        Emitted& out = shadow ? s.shadow : s.base;
        out.stride = stride;
        out.region = s.region;
        out.commands.clear();
        out.counts.clear();
        out.tested.clear();
        if (!fetch)
            return;
        uint32_t views = 0, counts[2 * GV_MAX_VIEWS];
        check(gv_pool_instances_info(ctx, p, &views, nullptr, nullptr), "gv_pool_instances_info");
        check(gv_pool_cluster_commands_fetch(ctx, p, nullptr, 0, counts, 2 * GV_MAX_VIEWS), "gv_pool_cluster_commands_fetch");
        out.counts.assign(counts, counts + views);
        out.tested.assign(counts + views, counts + 2 * views);
        size_t positions = (size_t)views * s.region;
        if (!s.region)
            for (uint32_t c : out.counts)
                positions += c;
        const size_t room = device ? bytes / stride : positions;
        out.commands.resize(std::min(positions, room) * stride);
        check(gv_pool_cluster_commands_fetch(ctx, p, out.commands.data(), out.commands.size(), counts, 2 * GV_MAX_VIEWS), "gv_pool_cluster_commands_fetch");
    }

    // The second phase of mesh system p's LAST cluster cull (gv_pool_cull_clusters_second_phase), for a renderer that has drawn that
    // cull's commands and handed the new depth to GpuVisibilitySystem::setHizDepth: the clusters the cull tested and did not keep,
    // where its pass queried a pyramid, tested again against the pyramid as it stands now — draw the survivors behind the first
    // list. shadow: the last cull was the one behind the shadow array (it picks the targets of setSecondTargets and the host copy).
    // Nothing of the first cull changes. The newly visible DRAWS of GpuSecondPhase::run are an ordinary view: emit it and call
    // cull(). Opt-in: a tick that does not call this runs as before. Emitted::tested holds the pending clusters re-tested per view.
    // Behind a cull with cones the library applies the same cone test with that cull's eyes — it kept them, none is passed here — and
    // the cone-rejected clusters of a queried pass are among the pending ones: re-tested, rejected again, counted in tested.
    void cullSecond(uint32_t p, bool shadow, uint32_t stride)
    {
        PerSystem& s = of(p);
        if (!s.enabled)
            return;
        if (!isSupported())
            throw GardenError("GpuClusterCommands: unsupported with several ranks (the merged draw order is made on the host)");
        GvCtx* ctx = system->getContext();
        void* const device = shadow ? s.shadowSecondDevice : s.baseSecondDevice;
        const size_t bytes = shadow ? s.shadowSecondBytes : s.baseSecondBytes;
        check(gv_pool_cull_clusters_second_phase(ctx, p, 0, s.region, device, bytes), "gv_pool_cull_clusters_second_phase");
        Emitted& out = shadow ? s.shadowSecond : s.baseSecond;
        out.stride = stride;
        out.region = s.region;
        out.commands.clear();
        out.counts.clear();
        out.tested.clear();
        if (!fetch)
            return;
        uint32_t views = 0, counts[2 * GV_MAX_VIEWS];
        check(gv_pool_instances_info(ctx, p, &views, nullptr, nullptr), "gv_pool_instances_info");
        check(gv_pool_cluster_second_commands_fetch(ctx, p, nullptr, 0, counts, 2 * GV_MAX_VIEWS), "gv_pool_cluster_second_commands_fetch");
        out.counts.assign(counts, counts + views);
        out.tested.assign(counts + views, counts + 2 * views);
        size_t positions = (size_t)views * s.region;
        if (!s.region)
            for (uint32_t c : out.counts)
                positions += c;
        const size_t room = device ? bytes / stride : positions;
        out.commands.resize(std::min(positions, room) * stride);
        check(gv_pool_cluster_second_commands_fetch(ctx, p, out.commands.data(), out.commands.size(), counts, 2 * GV_MAX_VIEWS),
              "gv_pool_cluster_second_commands_fetch");
    }
    // caller-owned, 16-byte aligned device memory for the second phase's two command arrays (NULL: the library's buffer)
    void setSecondTargets(uint32_t p, void* baseDevice, size_t baseBytes, void* shadowDevice, size_t shadowBytes)
    {
        PerSystem& s = of(p);
        s.baseSecondDevice = baseDevice, s.baseSecondBytes = baseBytes, s.shadowSecondDevice = shadowDevice, s.shadowSecondBytes = shadowBytes;
    }

    // device pointers of mesh system p's last cluster cull: the commands and uint32 counts[2 * views]
    void getDevice(uint32_t p, const void** commands, const void** counts)
    {
        check(gv_pool_cluster_commands_device(system->getContext(), p, commands, counts), "gv_pool_cluster_commands_device");
    }
    // ... and of its last second phase
    void getSecondDevice(uint32_t p, const void** commands, const void** counts)
    {
        check(gv_pool_cluster_second_commands_device(system->getContext(), p, commands, counts), "gv_pool_cluster_second_commands_device");
    }
    const Emitted& getBase(uint32_t p) { return of(p).base; }
    const Emitted& getShadow(uint32_t p) { return of(p).shadow; }
    const Emitted& getBaseSecond(uint32_t p) { return of(p).baseSecond; }
    const Emitted& getShadowSecond(uint32_t p) { return of(p).shadowSecond; }
};

}  // namespace garden
