// gv_second.cpp — gv_pool_cull_second_phase of include/garden_vis.h: the second phase of two-phase occlusion culling (DESIGN.md §4
// item 13). The first phase is gv_cull as it stands, against last frame's pyramid; once the pyramid has been rebuilt from what was
// drawn, this call culls the pool again and leaves in `second_view` the records of that cull whose slot the first view does not
// hold: an ordinary emitted view. Its own launches (gv_second.hip) are the seen set, the masked cull and the union of the isVisible
// bytes; compaction and records are the cull's (begin_view and emit_view of gv_context.cpp), on the second view's own ViewState; what the
// call ends is what a cull ends (end_derived of gv_ctx.hpp).
#include "gv_ctx.hpp"

using namespace gv;

extern "C" {

int gv_pool_cull_second_phase(GvCtx* ctx, uint32_t pool_id, uint32_t first_view, uint32_t second_view, const GvView* view)
{
    if (!ctx)
        return GV_E_ARG;
    if (!view)
        return ctx->fail(GV_E_ARG, "gv_pool_cull_second_phase: view is NULL");
    if (!bound_pool(ctx, "gv_pool_cull_second_phase", pool_id))
        return GV_E_ARG;
    if (first_view >= GV_MAX_VIEWS || second_view >= GV_MAX_VIEWS || first_view == second_view)
        return ctx->fail(GV_E_ARG, "gv_pool_cull_second_phase: views %u and %u (two different indices below %u)", first_view, second_view,
                         (uint32_t)GV_MAX_VIEWS);
    if (!view->emit_records)
        return ctx->fail(GV_E_ARG, "gv_pool_cull_second_phase: the second view is defined by its records (emit_records must be 1)");
    if (!view_of(ctx, pool_id, first_view) || !view_of(ctx, pool_id, first_view)->emitted)
        return ctx->fail(GV_E_ARG, "gv_pool_cull_second_phase: pool %u view %u has no emitted records", pool_id, first_view);
    PoolState& p = ctx->pools[pool_id];
    ViewState& vs1 = *view_of(ctx, pool_id, first_view);
    ViewState& vs2 = ctx->views[pool_id][second_view];
    if (!ctx->xf.bound)
        return ctx->fail(GV_E_STATE, "gv_pool_cull_second_phase: pools not bound");
    if (view->use_hiz && !ctx->pyramid_built(Context::pyramid_of(view->use_hiz)))
        return ctx->fail(GV_E_STATE, "gv_pool_cull_second_phase: the view asks for Hi-Z but gv_hiz_build has not run (view %u, pyramid %u is not built)",
                         second_view, Context::pyramid_of(view->use_hiz));
    if (p.occupancy != vs1.occupancy)
        return ctx->fail(GV_E_STATE, "gv_pool_cull_second_phase: pool %u holds %u slots, view %u was culled with %u (cull again first)", pool_id,
                         p.occupancy, first_view, vs1.occupancy);
    ZoneScope zone("Meshes Prepare Second");
    if (int rc = flush_sorts(ctx))  // a read of the first view: recorded culls and deferred sorts first (as the emissions and the grouping)
        return rc;
    if (int rc = sync_mirror(ctx))  // ... and a cull: it sees the pools as they are
        return rc;
    GV_HIP(ctx, hipSetDevice(ctx->device));
    ViewParams vp;  // (the masked cull writes the ballot words: the mask form of this view carries the new entries only)
    if (int rc = begin_view(ctx, vs2, pool_id, *view, &vp))
        return rc;
    // what a gv_cull of the pool ends, this call ends too; the pool's other views stay (invalidate_views_beyond is gv_cull's)
    end_derived(ctx, p, Ends::ViewsReplaced);
    if (p.occupancy == 0) {
        GV_HIP(ctx, hipMemsetAsync(vs2.draw_count.ptr, 0, 4, ctx->stream));
        return GV_OK;
    }
    const MeshMirror mesh = mesh_mirror(p);
    const TransformMirror xf = xf_mirror(ctx);
    const HizDevice hz = hiz_device(ctx, vp.hiz_index);  // the pyramid the view names
    // the seen set: bit entry(s) for every slot s in the first view's records, whatever order they are in by now
    const size_t words = second_seen_words(p.occupancy);
    GV_HIP(ctx, vs2.seen.reserve(words));
    GV_HIP(ctx, hipMemsetAsync(vs2.seen.ptr, 0, words * sizeof(unsigned long long), ctx->stream));
    GV_LAUNCH(ctx, GV_K_CULL, launch_second_seen(records_of(vs1).count, records_of(vs1).idx, vs1.occupancy, p.inv.empty() ? nullptr : p.d_inv.ptr,
                                                 p.occupancy, p.occupancy, vs2.seen.ptr, ctx->stream));
    const ViewBuffers vb = view_buffers(vs2);
    ViewParams cvp = vp;  // as the cull kernel sees the view: the isVisible bytes are left to the emit that follows
    cvp.write_is_visible = 0;
    GV_LAUNCH(ctx, GV_K_CULL, launch_second_cull(mesh, xf, hz, cvp, vb, vs2.seen.ptr, ctx->stream));
    const bool self_prefix = (p.occupancy + kEmitChunk - 1) / kEmitChunk <= kSelfPrefixMaxChunks;
    if (int rc = emit_view(ctx, vs2, mesh, xf, vp, vb, self_prefix, nullptr, nullptr))  // no seeds, no resident world
        return rc;
    if (vs2.main_pass) {
        // isVisible is the frame's final answer: the first view's records or the new ones
        GV_LAUNCH(ctx, GV_K_EMIT, launch_second_union(vs2.seen.ptr, p.occupancy, vs2.is_visible.ptr, ctx->stream));
        vs2.vis_flags_current = false;  // the self-prefixing emit trusts its flags to skip chunks it believes are zero
    }
    return GV_OK;
}

}  // extern "C"
