"""Test helpers of the mirror sync: which upload form brings each side of the device mirror up to date (sync_mirror and its steps
in garden_amd/csrc/gv_mirror.cpp, the rules of gv_dirty_ranges.hpp), restated in plain Python (sync_plan over a MirrorState), and the
table of GPU cases (CASES) that tests/test_mirror_sync_census.py proves to hold every reachable cell and
tests/test_gpu_mirror_sync_forms.py runs against the oracle. TEST INFRASTRUCTURE ONLY.

A CELL is (side, form, order, binding, flagging, cache):
  side      xf (the transform mirror) or mesh (a mesh pool's)
  form      xf:   rebuild, grow, device_dense (upload_dense_transforms by upload_transforms_device), pipelined
                  (regather_transforms_pipelined), device (every range of an itemised sync gathered on the device), packet (ONE
                  scattered packet), ranged (plain ranged copies), mixed+packet / mixed+ranged (device gathers AND a host form)
            mesh: rebuild, grow, device (upload_meshes_device for every range), whole ("most of a permuted pool goes up whole"),
                  packet, ranged, mixed+whole / mixed+packet / mixed+ranged
  order     permuted or slot: whether the side's mirror has an order table (a spatially ordered context, two slots or more)
  binding   aos, columns, or (mesh side) ready: an AoS pool with a ready column
  flagging  what the sync does for the pools that record changed blocks (PoolState::recording): none (nobody records), packet
            (the packet flags the blocks itself), marks (a mark_dirty_blocks launch), both, stopped (the sync ended a recording)
  cache     xf side: tracked (the world-matrix cache is valid: every re-mirrored entry gets its dirty byte) or invalid; mesh: "-"
A second, small dimension is the hand-over between two syncs (HANDOVER cells): (side, form of sync 2, "refreshed" or "gathered")
when the ranges of sync 2 lie in staging that an earlier sync left stale — refreshed: refresh_stale_staging /
refresh_stale_mesh_staging re-read the stale range; gathered: the form re-reads its own ranges only.

Unlike the results delivery, the route is observable: GvStats.upload_bytes grows by an amount the source fixes per form (Step.bytes),
which the GPU tests assert as an equality for every sync; bounds_blocks_total shows whether the block boxes survived."""
import collections
import functools
import itertools

from garden_amd.pools import MESH_DTYPE, TRANSFORM_DTYPE
from hiz_paths_support import header_constant, source_text  # noqa: F401  (source_text: for the census)

DEVICE_GATHER_MIN = header_constant("gv_dirty_ranges.hpp", "kDeviceGatherMinSlots")
CULL_BLOCK = header_constant("gv_kernels.hpp", "kCullBlock")
HOT_MIN = header_constant("gv_kernels.hpp", "kHotMinSlots")
AUTO_BOUNDS_MIN = header_constant("gv_kernels.hpp", "kAutoBoundsMinSlots")
# (not `constexpr uint32_t`: LITERAL_LINES holds the lines these are read from)
RANGED_COPY_MAX = 32      # kRangedCopyMaxRanges
RANGES_MAX = 16384        # DirtyRanges::kMax
XF_COPY_BYTES, MESH_COPY_BYTES, XF_PACKET_BYTES, MESH_PACKET_BYTES = 45, 28, 64, 32
MESH_GATHER_ENTITY_SHARE = 12  # count * 12 < entity_capacity: the device gather is not worth the entity table
FEW_SHARE, FEW_FREE = 16, 16 * 64
MIN_SMALL_STREAK = 4

# Lines that the restatement below follows (test_mirror_sync_census.py checks that the library still holds them).
LITERAL_LINES = {
    "gv_dirty_ranges.hpp": [
        "return occupancy > mirrored && ((uint64_t)appended + (occupancy - mirrored)) * 8 > occupancy && occupancy >= 1024;",
        "inline bool few_enough_to_patch_blocks(uint64_t total, uint64_t nblocks) { return total * 16 <= nblocks + 16 * 64; }",
        "inline bool most_of_pool(uint64_t total, uint32_t occupancy) { return total * 2 > occupancy; }",
        "return own == candidates ? kPairedExact : (own * 10 >= candidates * 9 ? kPairedSpeculate : kPairedGeneral);",
        "static constexpr size_t kMax = 16384;",
        # normalise
        "r.hi = std::min(r.hi, limit);",
        "if (!merged.empty() && (uint64_t)r.lo <= (uint64_t)merged.back().hi + gap)",
        "if (items.size() <= kMax || gap >= (1u << 30))",
        "gap = gap ? gap * 2 : 1;",
    ],
    "gv_mirror.cpp": [
        # the bytes every form adds to GvStats.upload_bytes
        "ctx->stats.upload_bytes += n * 45;",
        "ctx->stats.upload_bytes += n * 28;",
        "ctx->stats.upload_bytes += (size_t)n * sizeof(XfPacket);",
        "ctx->stats.upload_bytes += (size_t)n * sizeof(MeshPacket);",
        "const size_t bytes = (size_t)(count - 1) * L.stride + extent;",
        "ctx->stats.upload_bytes += bytes;",
        "ctx->stats.upload_bytes += bytes + (size_t)cap * 4;",
        "constexpr size_t kRangedCopyMaxRanges = 32;  // dirty ranges of a slot-order mirror sent as plain copies; more go as one scattered packet",
        # upload_transforms_device, upload_meshes_device
        "if (hi <= lo || !aos_transform_layout(ctx->xf, &base, &L, &extent))",
        "ctx->staging_stale.add(lo, count);",
        "if (count < kDeviceGatherMinSlots || (uint64_t)count * 12 < ctx->xf.entity_capacity || p.ready.ptr ||",
        "if (ctx->h_flag.ptr[0] && p.mapping == kMapExact)",
        "p.staging_stale.add(lo, count);",
        # refresh_stale_staging, refresh_stale_mesh_staging, regather_transforms_pipelined
        "const uint32_t lo = ctx->staging_stale.lo, hi = std::min(ctx->staging_stale.hi, ctx->xf.occupancy);",
        "const uint32_t lo = p.staging_stale.lo, hi = std::min(p.staging_stale.hi, p.occupancy);",
        "const int rc = upload_transforms(ctx, j0, j1);",
        # grow_transforms, grow_meshes
        "q.stop_recording();  // (appended entries: the blocks change; rebuilt once the pools are at rest)",
        "ctx->xf_appended += n1 - n0;",
        "p.appended += n1 - n0;",
        # pools_that_keep_flagging
        "const bool few = !dense && !ctx->xf_links_dirty && few_enough_to_patch_blocks(total, blocks_of(q.occupancy));",
        "q.small_streak = few ? std::min(q.small_streak + 1u, 1000u) : 0u;",
        "if (!few || ctx->max_depth != 0 || q.mapping != kMapExact || !q.d_blk_dirty.ptr) {",
        # upload_dense_transforms
        "if (!ctx->xf_links_dirty)\n        rc = upload_transforms_device(ctx, lo, hi);",
        "refresh_stale_staging(ctx);  // this path re-uploads every entry from the staging arrays",
        "rc = regather_transforms_pipelined(ctx, lo, hi);  // dense, chunked, DMA under gather",
        # upload_itemised_transforms
        "if (!ctx->xf_links_dirty && r.hi - r.lo >= kDeviceGatherMinSlots)",
        "if (!ctx->xinv.empty() || host.size() > kRangedCopyMaxRanges) {",
        "bits_current = unflagged.empty();",
        "GV_HIP(ctx, hipMemsetAsync(ctx->d_xdirty.ptr + r.lo, 1, r.hi - r.lo, ctx->stream));",
        # after_transform_upload
        "if (track_world_dirty(ctx) && !dense)",
        "return ctx->world_valid && ctx->d_xdirty.ptr && ctx->d_xdirty.cap >= ctx->xf.occupancy;",
        # remirror_dirty_transforms
        "ctx->xf_dirty.normalise(n, 0);  // exact: a re-mirrored slot is a flagged slot (its whole subtree is re-swept)",
        "const bool dense = most_of_pool(total, n);",
        "if (int rc = dense ? upload_dense_transforms(ctx, ranges.front().lo, ranges.back().hi)",
        "if (!bits_current)",
        "if (flagging && !unflagged.empty())",
        "if (int rc = mark_dirty_blocks(ctx, ctx->pools[k], unflagged, ctx->xinv.empty() ? nullptr : ctx->d_xinv.ptr, ctx->xf.occupancy))",
        # remirror_dirty_meshes
        "p.dirty.normalise(p.occupancy, 0);",
        "const int one = upload_meshes_device(ctx, p, r.lo, r.hi);",
        "const bool most = !left.empty() && !p.inv.empty() && most_of_pool(left_total, p.occupancy);",
        # upload_meshes_from_host
        "refresh_stale_mesh_staging(ctx, p);  // (it re-uploads every entry from the staging arrays)",
        "gather_meshes(ctx, p, left.front().lo, left.back().hi);",
        "return upload_meshes(ctx, p, 0, p.occupancy);",
        "if (p.inv.empty() && left.size() <= kRangedCopyMaxRanges) {",
        "packet_flagged = p.recording() && p.d_blk_dirty.ptr && few_enough_to_patch_blocks(total, blocks_of(p.occupancy));",
        # flag_dirty_mesh_blocks
        "const bool few = few_enough_to_patch_blocks(total, blocks_of(p.occupancy));",
        "p.small_streak = 0;  // (small mesh edits leave the streak to the transform side: no double count)",
        "if (most || p.mapping != kMapExact || !few) {",
        "return unflagged.empty() ? GV_OK : mark_dirty_blocks(ctx, p, unflagged, p.inv.empty() ? nullptr : p.d_inv.ptr, p.occupancy);",
        # sync_mirror
        "pass.spatial = !(ctx->config.flags & GV_CONFIG_KEEP_SLOT_ORDER);",
        "if (!ctx->xf_need_full && pass.spatial && tail_due_for_reorder(n, ctx->xf_mirrored, ctx->xf_appended)) {",
        "if (n > ctx->xf_mirrored) {",
        "if (ctx->xf_dirty.any())",
        "if (!p.need_full && pass.spatial && tail_due_for_reorder(p.occupancy, p.mirrored, p.appended)) {",
        "if (!p.need_full && p.occupancy > p.mirrored) {",
        "} else if (p.dirty.any()) {",
        "p.need_full = true;",  # rebuild_transforms: every bound pool follows
        # when a mirror is permuted
        "if ((ctx->config.flags & GV_CONFIG_KEEP_SLOT_ORDER) || n < 2)",
        "if (ctx->xinv.empty() || n < 2)",
        # the device re-order: stale staging, recordings ended, tails back in order
        "ctx->staging_stale.add(0, n);",
        "p.staging_stale.add(0, n);",
        "ctx->xf_appended = 0;",
    ],
    "gv_context.cpp": [  # what a cull of a pool at rest leaves for the next sync to keep current (cull_at_rest)
        "bool batched = view_count > 1 && view_count <= kMaxBatchViews && p.occupancy > 0;",  # (cull(): views with cameras of their own, never batched)
        "batched = memcmp(views[v].camera_position, views[0].camera_position, 12) == 0 && !views[v].use_hiz;",
        "plan.patchable = paired && flat;",
        "((ctx->config.flags & GV_CONFIG_BLOCK_BOUNDS) || (!(ctx->config.flags & GV_CONFIG_LINEAR_SCAN) && p.occupancy > kAutoBoundsMinSlots));",
        "plan.hot_wanted = !plan.batched && !plan.fused && !plan.bounds_wanted && p.occupancy > kHotMinSlots && exact && flat;",
        "p.hot_patch_valid = true;  // from here on every sync flags what it re-mirrors (gv_mirror.cpp); stale kDirtyHot bits only cost a re-derivation",
        "p.patch_valid = patchable;  // from here on every sync records what it re-mirrors (gv_mirror.cpp mark_dirty_blocks)",
        "const bool may_rebuild = !(changed && p.changed_prev) || (patchable && changed && p.small_streak >= kMinSmallStreak);",
        "ctx->xf_dirty.add(first, count);  // re-parented slots: links re-gathered in place, order kept",
    ],
    "gv_ctx.hpp": ["inline uint32_t blocks_of(uint32_t occupancy) { return (occupancy + kCullBlock - 1) / kCullBlock; }  // cull workgroups of a pool"],
    "gv_sort_kernels.hpp": ['static_assert(sizeof(XfPacket) == 64, "one sector per entry");', 'static_assert(sizeof(MeshPacket) == 32, "half a sector per entry");'],
}

MAP_GENERAL, MAP_SPECULATE, MAP_EXACT = 0, 1, 2


# ---- the four rules and normalise (gv_dirty_ranges.hpp) ----

def tail_due_for_reorder(occupancy, mirrored, appended):
    return occupancy > mirrored and (appended + (occupancy - mirrored)) * 8 > occupancy and occupancy >= 1024


def few_enough_to_patch_blocks(total, nblocks):
    return total * FEW_SHARE <= nblocks + FEW_FREE


def most_of_pool(total, occupancy):
    return total * 2 > occupancy


def mesh_mapping_of(own, candidates):
    return MAP_EXACT if own == candidates else (MAP_SPECULATE if own * 10 >= candidates * 9 else MAP_GENERAL)


def blocks_of(occupancy):
    return (occupancy + CULL_BLOCK - 1) // CULL_BLOCK


def add_marks(marks):
    """DirtyRanges::add over (first, count) marks: [(lo, hi)] as the library holds them before a sync"""
    items = []
    for first, count in marks:
        if count == 0:
            continue
        hi = min(first + count, 0xFFFFFFFF)
        if items and first <= items[-1][1] and hi >= items[-1][0]:
            items[-1] = (min(items[-1][0], first), max(items[-1][1], hi))
        else:
            items.append((first, hi))
    return items


def normalise(items, limit, gap=0, kmax=RANGES_MAX):
    """DirtyRanges::normalise: sorted, clamped to [0, limit), merged; beyond kmax ranges merged across a growing gap"""
    items = sorted(((lo, min(hi, limit)) for lo, hi in items if lo < min(hi, limit)), key=lambda r: r[0])
    while True:
        merged = []
        for lo, hi in items:
            if merged and lo <= merged[-1][1] + gap:
                merged[-1] = (merged[-1][0], max(merged[-1][1], hi))
            else:
                merged.append((lo, hi))
        items = merged
        if len(items) <= kmax or gap >= 1 << 30:
            return items
        gap = gap * 2 if gap else 1


@functools.lru_cache(maxsize=4096)
def dirty_ranges(marks, limit):
    """what a sync finds of (first, count) marks (a tuple): add, then normalise(limit, 0)"""
    return tuple(normalise(add_marks(marks), limit))


def aos_extent(dtype, fields):
    """(stride, extent) as aos_transform_layout / aos_mesh_layout derive them: extent = bytes from the lowest bound field to the end of
    the last one"""
    offs = [(dtype.fields[name][1], width) for name, width in fields]
    base = min(o for o, _ in offs)
    return dtype.itemsize, max(o - base + w for o, w in offs)


XF_STRIDE, XF_EXTENT = aos_extent(TRANSFORM_DTYPE, [("entity", 4), ("position", 12), ("scale", 12), ("rotation", 16), ("selfActive", 1),
                                                    ("ancestorsActive", 1), ("modelWithAncestors", 1)])
MESH_STRIDE, MESH_EXTENT = aos_extent(MESH_DTYPE, [("entity", 4), ("isEnabled", 1), ("aabbMin", 12), ("aabbMax", 12)])


# ---- the model ----
# stale: None or the covering (lo, hi) of the staging entries written on the device only (DirtyRange)
Xf = collections.namedtuple("Xf", "occupancy mirrored appended permuted binding need_full stale world_valid chained entity_capacity")
# binding: aos / columns / ready; has_flags: the pool's d_blk_dirty exists
# changed: the mirror the pool's culls read changed since its last cull; changed_prev: ... and so it had at the cull before
# (may_rebuild_at); boxes / hot: the last cull used block boxes / the sphere stream
Pool = collections.namedtuple("Pool", "occupancy mirrored appended permuted binding mapping need_full patch_valid hot_patch_valid has_flags small_streak stale "
                              "changed changed_prev boxes hot")
# context: (keep_slot_order, block_bounds, linear_scan)
MirrorState = collections.namedtuple("MirrorState", "context xf pools")
# xf / pools[k]: (first, count) marks; links: the transform marks are GV_DIRTY_HIERARCHY (chained: whether chains exist afterwards);
# demotes: pools in whose marked ranges a candidate no longer pairs with its own index
Marks = collections.namedtuple("Marks", "xf links pools demotes chained", defaults=((), False, {}, (), None))
# side: "xf" or the pool's index; reread: [(lo, hi)] of the caller's pool read by the step — the slots exactly, or (exact False) a
# covering range of which the step may read less; bytes: what the step adds to GvStats.upload_bytes
Step = collections.namedtuple("Step", "side name reread exact bytes")
Plan = collections.namedtuple("Plan", "steps cells handovers state reorder")


def bound(context, n_xf, pools, chained=False, xf_binding="aos", entity_capacity=None):
    """the state behind gv_transform_bind and gv_pool_bind of fresh pools: everything waits for its rebuild.
    pools: [(occupancy, binding, mapping the rebuild will find)]"""
    xf = Xf(n_xf, 0, 0, False, xf_binding, True, None, False, chained, n_xf + 1 if entity_capacity is None else entity_capacity)
    return MirrorState(context, xf, tuple(Pool(n, 0, 0, False, b, m, True, False, False, False, 0, None, True, False, False, False) for n, b, m in pools))


def _cover(stale, lo, hi):
    return (lo, hi) if stale is None else (min(stale[0], lo), max(stale[1], hi))


def _overlaps(stale, ranges):
    return stale is not None and any(lo < stale[1] and stale[0] < hi for lo, hi in ranges)


def _size(ranges):
    return sum(hi - lo for lo, hi in ranges)


def sync_plan(state, marks=Marks()):
    """one gv_sync: Plan(steps in the order sync_mirror takes them, the cells of the sync, its hand-over cells, the state after it,
    whether a device re-order ran behind it)"""
    spatial = not state.context[0]
    xf, pools = state.xf, list(state.pools)
    steps, cells, handovers = [], [], []
    n = xf.occupancy

    def xf_cell(form, flagging, tracked):
        for f in (flagging or ["none"]):
            cells.append(("xf", form, "permuted" if xf.permuted else "slot", xf.binding, f, "tracked" if tracked else "invalid"))

    # ---- the transform side ----
    reorder_xf = False
    if not xf.need_full and spatial and tail_due_for_reorder(n, xf.mirrored, xf.appended):
        if xf.permuted:
            reorder_xf = True
        else:
            xf = xf._replace(need_full=True)
    if xf.need_full:
        if n:
            steps.append(Step("xf", "rebuild_transforms", [(0, n)], False, XF_COPY_BYTES * n))
        xf = xf._replace(permuted=spatial and n >= 2)
        xf_cell("rebuild", ["stopped"] if any(p.patch_valid or p.hot_patch_valid for p in pools) else None, False)
        xf = xf._replace(need_full=False, stale=None, world_valid=False, mirrored=n, appended=0,
                         chained=xf.chained if marks.chained is None else marks.chained)
        pools = [p._replace(need_full=True, changed=True) for p in pools]
    else:
        if n > xf.mirrored:
            steps.append(Step("xf", "grow_transforms", [(xf.mirrored, n)], True, XF_COPY_BYTES * (n - xf.mirrored)))
            xf_cell("grow", ["stopped"] if any(p.patch_valid or p.hot_patch_valid for p in pools) else None, False)
            pools = [p._replace(patch_valid=False, hot_patch_valid=False, small_streak=0, changed=True) for p in pools]
            xf = xf._replace(appended=xf.appended + n - xf.mirrored, mirrored=n, world_valid=False)
        ranges = dirty_ranges(tuple(marks.xf), n)
        total = _size(ranges)
        if total:
            dense = most_of_pool(total, n)
            tracked = xf.world_valid
            links = marks.links
            # pools_that_keep_flagging
            targets, stopped = [], []
            for k, q in enumerate(pools):
                few = not dense and not links and few_enough_to_patch_blocks(total, blocks_of(q.occupancy))
                q = q._replace(small_streak=min(q.small_streak + 1, 1000) if few else 0, changed=True)
                if q.patch_valid or q.hot_patch_valid:
                    if not few or xf.chained or q.mapping != MAP_EXACT or not q.has_flags:
                        q = q._replace(patch_valid=False, hot_patch_valid=False)
                        stopped.append(k)
                    else:
                        targets.append(k)
                pools[k] = q
            aos = xf.binding == "aos"
            if dense:
                lo, hi = ranges[0][0], ranges[-1][1]
                if not links and aos:
                    steps.append(Step("xf", "xf_device_dense", [(lo, hi)], False, (hi - lo - 1) * XF_STRIDE + XF_EXTENT))
                    xf = xf._replace(stale=_cover(xf.stale, lo, hi))
                    form = "device_dense"
                else:
                    if xf.stale is not None:
                        slo, shi = xf.stale[0], min(xf.stale[1], n)
                        if slo < shi:
                            steps.append(Step("xf", "refresh_stale_staging", [(slo, shi)], False, 0))
                        handovers.append(("xf", "pipelined", "refreshed"))
                        xf = xf._replace(stale=None)
                    steps.append(Step("xf", "regather_transforms_pipelined", [(lo, hi)], False, XF_COPY_BYTES * n))
                    form = "pipelined"
                flagging = ["stopped"] if stopped else None  # (dense: nobody goes on recording)
            else:
                unflagged, host = [], []
                for r in ranges:
                    if not links and r[1] - r[0] >= DEVICE_GATHER_MIN and aos:
                        steps.append(Step("xf", "xf_device", [r], True, (r[1] - r[0] - 1) * XF_STRIDE + XF_EXTENT))
                        xf = xf._replace(stale=_cover(xf.stale, *r))
                        unflagged.append(r)
                    else:
                        host.append(r)
                device = bool(unflagged)
                packet = False
                if host:
                    over_stale = _overlaps(state.xf.stale, host)
                    if xf.permuted or len(host) > RANGED_COPY_MAX:
                        steps.append(Step("xf", "xf_packet", host, True, XF_PACKET_BYTES * _size(host)))
                        packet, hostform = True, "packet"
                    else:
                        for r in host:
                            steps.append(Step("xf", "xf_ranged_copy", [r], True, XF_COPY_BYTES * (r[1] - r[0])))
                        unflagged += host
                        hostform = "ranged"
                    form = "mixed+" + hostform if device else hostform
                    if over_stale:
                        handovers.append(("xf", form, "gathered"))
                else:
                    form = "device"
                marked = bool(targets) and bool(unflagged)
                flagging = []
                if targets:
                    flagging.append("both" if packet and marked else ("packet" if packet else "marks"))
                if stopped:
                    flagging.append("stopped")
            xf_cell(form, flagging, tracked)
            if links and marks.chained is not None:
                xf = xf._replace(chained=marks.chained)
            if not (tracked and not dense):
                xf = xf._replace(world_valid=False)

    # ---- the mesh side, pool by pool ----
    reorder_pools = []
    for k, p in enumerate(pools):
        order = lambda: "permuted" if p.permuted else "slot"  # noqa: E731
        recording = lambda: p.patch_valid or p.hot_patch_valid  # noqa: E731
        if not p.need_full and spatial and tail_due_for_reorder(p.occupancy, p.mirrored, p.appended):
            if p.permuted:
                reorder_pools.append(k)
            else:
                p = p._replace(need_full=True)
        if not p.need_full and p.occupancy > p.mirrored:
            steps.append(Step(k, "grow_meshes", [(p.mirrored, p.occupancy)], True, MESH_COPY_BYTES * (p.occupancy - p.mirrored)))
            cells.append(("mesh", "grow", order(), p.binding, "stopped" if recording() else "none", "-"))
            p = p._replace(appended=p.appended + p.occupancy - p.mirrored, mirrored=p.occupancy, patch_valid=False, hot_patch_valid=False, changed=True)
        my = dirty_ranges(tuple(marks.pools.get(k, ())), p.occupancy)
        if p.need_full:
            if p.occupancy:
                steps.append(Step(k, "rebuild_meshes", [(0, p.occupancy)], False, MESH_COPY_BYTES * p.occupancy))
            p = p._replace(permuted=xf.permuted and p.occupancy >= 2)
            cells.append(("mesh", "rebuild", order(), p.binding, "stopped" if recording() else "none", "-"))
            p = p._replace(need_full=False, patch_valid=False, hot_patch_valid=False, stale=None, mirrored=p.occupancy, appended=0, changed=True)
        elif my:
            total = _size(my)
            p = p._replace(changed=True)
            stale_before = p.stale
            left = []
            for r in my:
                count = r[1] - r[0]
                if count < DEVICE_GATHER_MIN or count * MESH_GATHER_ENTITY_SHARE < xf.entity_capacity or p.binding != "aos":
                    left.append(r)
                else:
                    steps.append(Step(k, "mesh_device", [r], True, (count - 1) * MESH_STRIDE + MESH_EXTENT + 4 * xf.entity_capacity))
                    p = p._replace(stale=_cover(p.stale, *r))
            device = len(left) < len(my)
            demoted = k in marks.demotes and p.mapping == MAP_EXACT
            if demoted:
                p = p._replace(mapping=MAP_SPECULATE)
            most = bool(left) and p.permuted and most_of_pool(_size(left), p.occupancy)
            packet_flagged = False
            form = "device"
            if left:
                if most:
                    if p.stale is not None:
                        slo, shi = p.stale[0], min(p.stale[1], p.occupancy)
                        if slo < shi:
                            steps.append(Step(k, "refresh_stale_mesh_staging", [(slo, shi)], False, 0))
                        if stale_before is not None:
                            handovers.append(("mesh", "mixed+whole" if device else "whole", "refreshed"))
                        p = p._replace(stale=None)
                    steps.append(Step(k, "mesh_whole", [(left[0][0], left[-1][1])], False, MESH_COPY_BYTES * p.occupancy))
                    hostform = "whole"
                elif not p.permuted and len(left) <= RANGED_COPY_MAX:
                    for r in left:
                        steps.append(Step(k, "mesh_ranged_copy", [r], True, MESH_COPY_BYTES * (r[1] - r[0])))
                    hostform = "ranged"
                else:
                    # (the demotion of this sync's own gathers does not reach p.recording(): a packet may flag for a pool that stops below)
                    packet_flagged = recording() and p.has_flags and few_enough_to_patch_blocks(total, blocks_of(p.occupancy))
                    steps.append(Step(k, "mesh_packet", left, True, MESH_PACKET_BYTES * _size(left)))
                    hostform = "packet"
                form = "mixed+" + hostform if device else hostform
                if not most and _overlaps(stale_before, left):
                    handovers.append(("mesh", form, "gathered"))
            # flag_dirty_mesh_blocks
            few = few_enough_to_patch_blocks(total, blocks_of(p.occupancy))
            if not few:
                p = p._replace(small_streak=0)
            if not recording():
                flagging = "none"
            elif most or p.mapping != MAP_EXACT or not few:
                p = p._replace(patch_valid=False, hot_patch_valid=False)
                flagging = "stopped"
            else:
                kept = set(left)
                unflagged = my if not packet_flagged else [r for r in my if r not in kept]
                flagging = ("both" if unflagged else "packet") if packet_flagged else "marks"
            cells.append(("mesh", form, order(), p.binding, flagging, "-"))
        pools[k] = p

    # ---- the device re-order, behind everything that went up in the old order ----
    reorder = reorder_xf or bool(reorder_pools)
    if reorder_xf:
        xf = xf._replace(stale=_cover(xf.stale, 0, xf.mirrored), world_valid=False, appended=0)
        pools = [p._replace(changed=True) for p in pools]
    for k, p in enumerate(pools):
        if reorder_xf or k in reorder_pools:
            assert p.permuted and p.occupancy >= 2  # (a pool without an order table is rebuilt on the host: not modelled)
            pools[k] = p._replace(stale=_cover(p.stale, 0, p.mirrored), patch_valid=False, hot_patch_valid=False, appended=0, changed=True)
    return Plan(steps, cells, handovers, MirrorState(state.context, xf, tuple(pools)), reorder)


def cull(state, k=0):
    """the state after a gv_cull of pool k whose views each have a camera position of their own (not batched) (plan_cull, may_rebuild_at, hot_stream_ready, block_bounds_ready): block boxes
    and the sphere stream are patched from a recording, (re)built when the pool is at rest or has just changed after a quiet frame, or
    gone without. Pool.boxes afterwards says whether GvStats.bounds_blocks_total reads blocks_of(occupancy) or stays 0."""
    keep_slot_order, block_bounds, linear_scan = state.context
    p, xf = state.pools[k], state.xf
    exact, flat = p.mapping == MAP_EXACT, not xf.chained
    patchable = exact and p.occupancy <= xf.occupancy and flat
    bounds_wanted = p.occupancy != 0 and (block_bounds or (not linear_scan and p.occupancy > AUTO_BOUNDS_MIN))
    hot_wanted = not bounds_wanted and p.occupancy > HOT_MIN and exact and flat
    changed = p.changed
    may_rebuild = not (changed and p.changed_prev) or (patchable and changed and p.small_streak >= MIN_SMALL_STREAK)
    boxes, hot = False, False
    if hot_wanted:
        hot = p.hot and not changed
        if not hot and p.hot_patch_valid and p.has_flags:
            hot = True
        if not hot and may_rebuild:
            p = p._replace(has_flags=True, hot_patch_valid=True)  # (a fresh flag array would end patch_valid: no pool here has both)
            hot = True
    if bounds_wanted:
        boxes = p.boxes and not changed
        if not boxes and p.patch_valid and patchable and p.has_flags:
            boxes = True
        if not boxes and may_rebuild:
            p = p._replace(has_flags=True, hot_patch_valid=False, patch_valid=patchable)
            boxes = True
    pools = list(state.pools)
    pools[k] = p._replace(changed=False, changed_prev=changed, boxes=boxes, hot=hot)
    return state._replace(pools=tuple(pools))


def swept(state):
    """after gv_sweep: the world-matrix cache is valid"""
    return state._replace(xf=state.xf._replace(world_valid=True))


def resized(state, n_xf=None, pools=None):
    """pools re-bound in place with more slots in use (gv_transform_bind / gv_pool_bind of the same address: growth, no rebuild)"""
    xf = state.xf if n_xf is None else state.xf._replace(occupancy=n_xf, entity_capacity=max(state.xf.entity_capacity, n_xf + 1))
    ps = list(state.pools)
    for k, n in (pools or {}).items():
        ps[k] = ps[k]._replace(occupancy=n)
    return MirrorState(state.context, xf, tuple(ps))


def upload_bytes(plan):
    return sum(s.bytes for s in plan.steps)


def reread(plan, side):
    """[(lo, hi)], merged: every slot of `side`'s pool that the sync may have read"""
    return normalise([r for s in plan.steps if s.side == side for r in s.reread], 0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------------
# The GPU cases: ONE transform pool and ONE mesh pool of `n` slots each (scene.flat_scene, or scene.hierarchy_scene under
# `chained`), bound to a context of `context`, brought to rest by `prep`, then `syncs`: per sync the marks of each side.
#   context  spatial / slot, + "+bounds" (GV_CONFIG_BLOCK_BOUNDS: small pools get block boxes)
#   binding  aos / columns (both sides bound as columns) / ready (AoS with a ready column on the mesh pool)
#   prep     a string of  c (a cull: builds boxes / the sphere stream where the plan wants them; a second c is the quiet frame)
#                         s (a sweep: the world cache becomes valid)
#   Sync     xf / mesh: (first, count) marks; links: the transform marks are GV_DIRTY_HIERARCHY (slots re-parented, chains
#            afterwards); demote: entities change hands inside the mesh marks; grow: slots appended to both pools before the sync
#   cells    what the case claims, per sync — checked against sync_plan by the census
# Sizes are never a multiple of 256.
# ---------------------------------------------------------------------------------------------------------------------------
#   quiet: one more cull, without a change in front, behind the sync and its decoys (a pool at rest gets its boxes back and records again)
#   claim: the (side, form, flagging) of the sync's cells, in the order sync_plan gives them
Sync = collections.namedtuple("Sync", "xf mesh links demote grow quiet claim", defaults=((), (), False, False, 0, False, ()))
# sweeps: a sweep behind every sync and behind its decoys (the world cache is tracked from then on); without, ONE sweep ends the case
Case = collections.namedtuple("Case", "name context n syncs binding chained prep sweeps", defaults=("aos", False, "ccs", True))


def context_flags(context):
    return ("slot" in context, "+bounds" in context, False)


def case_start(c):
    """the state behind the case's bind, its first sync and its prep; and the slots bound at first"""
    n0 = c.n - sum(s.grow for s in c.syncs)
    state = bound(context_flags(c.context), n0, [(n0, c.binding, MAP_EXACT)], chained=c.chained, xf_binding="columns" if c.binding == "columns" else "aos",
                  entity_capacity=c.n + 1)
    state = sync_plan(state).state
    for step in c.prep:
        state = cull(state) if step == "c" else swept(state)
    return state, n0


def case_bind(c):
    """the Plan of the sync behind the case's binds (gv_hierarchy_rebuild): both sides rebuilt"""
    n0 = c.n - sum(s.grow for s in c.syncs)
    return sync_plan(bound(context_flags(c.context), n0, [(n0, c.binding, MAP_EXACT)], chained=c.chained,
                           xf_binding="columns" if c.binding == "columns" else "aos", entity_capacity=c.n + 1))


def case_states(c):
    """[(state before, Marks, Plan, the state behind the cull that follows)] of the case's syncs, as the GPU test runs them: the
    sync, a cull, a sweep (c.sweeps), the sync of the decoys, a cull, a sweep, a quiet cull where the Sync asks for one"""
    state, n = case_start(c)
    out = []
    for s in c.syncs:
        if s.grow:
            n += s.grow
            state = resized(state, n, {0: n})
        marks = case_marks(s)
        plan = sync_plan(state, marks)
        after = cull(plan.state)
        out.append((state, marks, plan, after))
        state = swept(after) if c.sweeps else after
        decoy = sync_plan(state, decoy_marks(plan, n))
        state = cull(decoy.state)
        state = swept(state) if c.sweeps else state
        if s.quiet:
            state = cull(state)
    return out


def case_marks(s):
    return Marks(tuple(s.xf), s.links, {0: tuple(s.mesh)}, (0,) if s.demote else (), True if s.links else None)


def decoy_slots(plan, side, n, allowed=None, count=2):
    """`count` isolated slots of `side`'s pool that the sync did not read (outside the covering ranges of its steps), from the middle
    of the widest gap outwards; allowed: a boolean array that narrows the choice (the GPU tests: slots whose edit shows in a record)"""
    edges = [0] + [min(x, n) for r in reread(plan, side) for x in r] + [n]
    gaps = [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2)]
    lo, hi = max(gaps, key=lambda g: g[1] - g[0])
    out, s = [], lo + (hi - lo) // 2
    while len(out) < count and s < hi:
        if (allowed is None or allowed[s]) and (not out or s >= out[-1] + 2):
            out.append(s)
        s += 1
    assert len(out) == count or hi - lo < 8, f"no room for {count} decoys in [{lo}, {hi})"
    return out if len(out) == count else []  # (a sync that re-reads the whole pool leaves no slot for a decoy)


def decoy_marks(plan, n, allowed_xf=None, allowed_mesh=None):
    return Marks(tuple((s, 1) for s in decoy_slots(plan, "xf", n, allowed_xf)), False, {0: tuple((s, 1) for s in decoy_slots(plan, 0, n, allowed_mesh))})


def every(first, step, count, width=1):
    """`count` marks of `width` slots, `step` apart"""
    return tuple((first + k * step, width) for k in range(count))


def few_limit(n):
    """the largest total for which few_enough_to_patch_blocks holds on a pool of n slots"""
    return (blocks_of(n) + FEW_FREE) // FEW_SHARE


# ---- the table ----
# A program is written for what each sync is MEANT to take (the claims: plain rules of thumb, stated here once more and apart from
# sync_plan, which the census holds them against): a host range of a permuted mirror, or more than 32 of them, travel as the packet,
# else as ranged copies; AoS ranges of 2048 slots (meshes: and 1/12 of the entity capacity) are gathered on the device; a recording
# pool goes on recording through a sync of at most few_limit slots, flagged by the packet or by marks, and stops otherwise.
G = DEVICE_GATHER_MIN
N_FORMS = 12 * G + 257      # 24 833 slots: the mesh device gather exists (1/12 of 24 834 entities: 2 070 slots, above 2 048)
N_HOT = HOT_MIN + 7         # 65 543 slots: just above kHotMinSlots, the sphere stream records


def _host(order, ranges):
    return "packet" if order == "permuted" or ranges > RANGED_COPY_MAX else "ranged"


def program(order, binding, recording, n, tracked=True, sides=("xf", "mesh")):
    """the syncs of one case: every form the binding has in this order, each on both sides of its threshold, and — where the pool
    records — each once while it goes on recording (where it can) and once as the sync that ends the recording. Between two syncs
    that end a recording stand a quiet frame (the boxes come back) and a small sync (so that the cull behind the next one sees a pool
    that changed twice in a row and may NOT rebuild: bounds_blocks_total then tells a recording that stopped from one that went on)."""
    xa, ma = binding != "columns", binding == "aos"   # the device gathers exist: transforms / meshes
    few, share = few_limit(n), -(-(n + 1) // MESH_GATHER_ENTITY_SHARE)
    h1 = _host(order, 1)
    out = []
    live = [recording]   # the pool records when the next sync begins
    warm = [True]        # the cull in front of the next sync saw a change
    small = [0]

    def add(xf=(), mesh=(), forms=(None, None), keeps=False, ends_for_good=False, extra=(), **kw):
        if ("xf" not in sides and xf and not mesh) or ("mesh" not in sides and mesh and not xf):
            return
        if live[0] and not keeps and not warm[0]:
            warm_up()
        rec, claim = live[0], list(extra)
        for side, form in zip(("xf", "mesh"), forms):
            if form is None:
                continue
            flag = "none" if not rec else (("packet" if form == "packet" else "marks") if keeps else "stopped")
            rec = rec and keeps
            claim.append((side, form, flag))
        ended = live[0] and not rec
        out.append(Sync(tuple(xf), tuple(mesh), quiet=ended and not ends_for_good, claim=tuple(claim), **kw))
        live[0] = recording and not ends_for_good and (live[0] or ended)
        warm[0] = not (ended and not ends_for_good)
        if ends_for_good:
            live[0] = False

    def warm_up():
        k = small[0] = small[0] + 1
        add(every(6101 + k, 7, 5), every(7 + k, 7, 5), (h1 if order == "slot" else "packet",) * 2, keeps=True)

    # small syncs on both sides: 32 ranges, 33 ranges (a mirror in slot order changes over to the packet). (Every flagging sync
    # marks blocks of its own: the entity that the GPU test brings into view widens its block's box for good.)
    add(every(6101, 7, 32), every(9, 7, 32), (_host(order, 32),) * 2, keeps=True)
    add(every(7201, 7, 33), every(1033, 7, 33), ("packet", "packet"), keeps=True)
    if recording:  # few_limit slots go on recording, one more ends it: as scattered slots (the packet) and as one range
        add(xf=every(2561, 3, few), forms=("packet", None), keeps=True)
        add(xf=every(2561, 3, few + 1), forms=("packet", None))
        add(mesh=every(3585, 3, few), forms=(None, "packet"), keeps=True)
        add(mesh=every(3585, 3, few + 1), forms=(None, "packet"))
        add(xf=((4610, few),), forms=(h1, None), keeps=True)
        add(xf=((4610, few + 1),), forms=(h1, None))
        add(mesh=((5130, few),), forms=(None, h1), keeps=True)
        add(mesh=((5130, few + 1),), forms=(None, h1))
    # one slot below the device gather, and at it
    add(xf=((6000, G - 1),), forms=(h1, None))
    add(xf=((5000, G),), forms=("device" if xa else h1, None))
    add(mesh=((7, share - 1),), forms=(None, h1))
    add(mesh=((7, share),), forms=(None, "device" if ma else h1))
    # small ranges inside what the device gathers left stale in the staging
    add(every(6101, 7, 5), every(9, 7, 5), (h1, h1), keeps=True)
    # a device gather and a host form in one sync, the host ranges inside the stale staging
    add(xf=((7100, G), (5500, 3)), forms=("mixed+" + h1 if xa else _host(order, 2), None))
    if order == "slot":
        add(xf=((300, G),) + every(5200, 7, 33), forms=("mixed+packet" if xa else "packet", None))
        add(mesh=((7, share),) + every(share + 40, 7, 33), forms=(None, "mixed+packet" if ma else "packet"))
    # half of the pool (itemised) and one slot more (dense)
    add(xf=((1, n // 2),), forms=("device" if xa else h1, None))
    add(xf=((1, n // 2 + 1),), forms=("device_dense" if xa else "pipelined", None))
    wide = (n // 2 + 1) // 7 + 1  # seven ranges, each too short for the device gather, that together are most of the pool ...
    last = n // 2 + 1 - 6 * wide
    assert wide < min(G, share) and 1 < last <= wide and most_of_pool(6 * wide + last, n) and not most_of_pool(6 * wide + last - 1, n)
    add(mesh=every(0, 3200, 6, wide) + ((19200, last - 1),), forms=(None, _host(order, 7)))   # ... but for one slot
    if order == "permuted" and ma:  # (the staging is stale from the device gathers above: refreshed; and stale again behind this one)
        add(mesh=((7, share),) + every(2200, 3200, 6, wide) + ((21400, last),), forms=(None, "mixed+whole"))
    add(mesh=((7, share), (share + 40, 2)), forms=(None, "mixed+" + h1 if ma else _host(order, 2)))
    add(mesh=every(0, 3200, 6, wide) + ((19200, last),), forms=(None, "whole" if order == "permuted" else "ranged"))
    # growth by three slots, with a small edit of old slots in the same sync: the appended slots end every recording
    if live[0] and not warm[0]:
        warm_up()
    out.append(Sync(((n // 3, 1),), ((n // 3, 1),), grow=3, quiet=recording,
                    claim=(("xf", "grow", "stopped" if recording else "none"), ("xf", h1, "none"), ("mesh", "grow", "none"), ("mesh", h1, "none"))))
    live[0], warm[0] = recording, not recording
    # re-parented slots go through the host, dense and itemised; chains from here on, so nothing records any more
    add(xf=((1, n // 2 + 4),), forms=("pipelined", None), links=True, ends_for_good=True)
    add(xf=((9000, 5),), forms=(h1, None), links=True, ends_for_good=True)
    # entities change hands: inside a device-gathered range (aos_meshes_kernel reports it) and inside a host-gathered one
    if ma:
        add(mesh=((7, share),), forms=(None, "device"), demote=True, ends_for_good=True)
    add(mesh=((500, 12),), forms=(None, h1), demote=True, ends_for_good=True)
    return tuple(out)


def _table():
    cases = []
    for order, binding, recording, tracked in itertools.product(("permuted", "slot"), ("aos", "columns", "ready"), (False, True), (True, False)):
        if binding == "ready" and not tracked:
            continue  # (a ready column changes the mesh side alone, and the world cache the transform side alone)
        context = ("spatial" if order == "permuted" else "slot") + ("+bounds" if recording else "")
        sides = ("mesh",) if binding == "ready" else (("xf", "mesh") if tracked else ("xf",))
        name = f"{context}-{binding}-{'tracked' if tracked else 'invalid'}"
        cases.append(Case(name, context, N_FORMS + 3, program(order, binding, recording, N_FORMS, tracked, sides), binding,
                          prep="ccs" if tracked else "cc", sweeps=tracked))
    for order in ("permuted", "slot"):  # chains: the same forms over a hierarchy (nothing records: the pools are not flat)
        context = "spatial" if order == "permuted" else "slot"
        cases.append(Case(f"{context}-aos-chained", context, N_FORMS + 3, program(order, "aos", False, N_FORMS), chained=True))
    # the sphere stream records (no block boxes: exactness alone is the witness): a flat pool just above kHotMinSlots
    for order in ("permuted", "slot"):
        h1, few = _host(order, 1), few_limit(N_HOT)
        cases.append(Case(f"{'spatial' if order == 'permuted' else 'slot'}-sphere-stream", "spatial" if order == "permuted" else "slot", N_HOT, (
            Sync(every(30_001, 259, 20), every(11, 263, 20), claim=(("xf", "packet" if order == "permuted" else "ranged", "packet" if order == "permuted" else "marks"),
                                                                    ("mesh", "packet" if order == "permuted" else "ranged", "packet" if order == "permuted" else "marks"))),
            Sync(every(1, 257, few), claim=(("xf", "packet", "packet"),)),
            Sync(mesh=((40_000, few),), claim=(("mesh", h1, "packet" if order == "permuted" else "marks"),)),
            Sync(xf=((50_000, G),), claim=(("xf", "device", "stopped"),)),
        )))
    # dirty marks and a due re-order in one sync: the marks go up in the old order, the re-order runs behind them
    grown = N_FORMS // 7 + 2
    cases.append(Case("spatial-reorder-behind-marks", "spatial", N_FORMS + grown, (
        Sync(every(6101, 7, 5), every(9, 7, 5), claim=(("xf", "packet", "none"), ("mesh", "packet", "none"))),
        Sync(((4000, G), (9000, 3)), ((7, 2400), (3000, 2)), grow=grown,
             claim=(("xf", "grow", "none"), ("xf", "mixed+packet", "none"), ("mesh", "grow", "none"), ("mesh", "mixed+packet", "none"))),
        Sync(every(6101, 7, 5), every(9, 7, 5), claim=(("xf", "packet", "none"), ("mesh", "packet", "none"))),
        Sync(((1, (N_FORMS + grown) // 2 + 1),), every(0, 4000, 7, 2040), links=True, claim=(("xf", "pipelined", "none"), ("mesh", "whole", "none"))),
    )))
    return cases


CASES = _table()
