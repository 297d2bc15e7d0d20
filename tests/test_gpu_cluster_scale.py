"""The cluster cull family on the device AT SCALE: the index machinery of garden_amd/csrc/gv_clusters.hip taken past its first
iteration. Expected values come from where the cluster tests take them — the C twins (cluster_twin.h, cluster_second_twin.h,
cluster_runs_twin.h, cluster_lod_twin.h over cluster_cone_twin.h) calling the oracle's gvo_is_behind_frustum / gvo_hiz_occluded over
the FETCHED records (order="raw") and the pyramids the oracle builds from the same depth images; the placement is
cluster_scale_support.place. Every comparison is exact: every command byte over a 0xA5 background on the device and through the
fetch, the rows behind the last written position, counts, tested and pending, and the launch count. The two worlds are
cluster_scale_support's, held to their conditions on the oracle alone by tests/test_cluster_scale_census.py.

What each test is the first in the suite to take past its first iteration:

  test                                   loop
  -------------------------------------  ----------------------------------------------------------------------------------------
  world_a_plain_packed                   scan_table over block_total: second turn, non-zero carry, scalar tail; the per-view
                                         block_tested sums' second stride; the tile_block fill's second stride and its skip of count
                                         workgroups without candidates; locate over 32 and more count workgroups
  world_a_plain_regions_library_owned    the same through the library's own target, a region cut in one view and padded in another
  world_a_runs_packed                    the same tables under cluster_run_test / heads / run_write
  world_a_second_phase                   cluster_second_scan<0> and find_pending behind a scan of two turns on the count side
  world_b_plain_packed_regions_held      scan_table over tile_count: second turn; second and third pass of cluster_test_kernel (its
                                         wave_count barrier pair) and cluster_write_kernel (its `continue`s); survivors_before behind
                                         tile 4096; the padding loop's second stride (2 R > 524 288 positions)
  world_b_runs_packed_and_regions        scan_table over head_count: second turn; second and third pass of cluster_run_test,
                                         cluster_run_heads' neighbours across passes, cluster_run_write and its padding loop
  world_b_second_phase_dense             scan_table over pending_count and kept_count: second turn; the pending_tile fill's strides;
                                         second and third pass of cluster_second_count / test / write and the padding loop
  world_b_second_phase_sparse            find_pending over 50 and more candidate tiles
  world_b_lods_cones_runs_and_second     the widest instantiations: cluster_lod_cone_run_test on its third pass,
                                         cluster_lod_cone_second_test on its second
  world_b_two_calls_identical            (none: two calls at this size give the same bytes)"""
import numpy as np
import pytest

import cluster_lods_support as lsup
import cluster_runs_support as rsup
import cluster_scale_support as xsup
import clusters_second_support as ssup
import clusters_support as ksup
import commands_support as csup
import test_gpu_clusters_second as second
from garden_amd.lib import GpuVisibility

pytestmark = pytest.mark.gpu

PLAIN_LAUNCHES, RUN_LAUNCHES, SECOND_LAUNCHES = 5, 6, 5


def walk_grid():
    """workgroups of a walk on this device; the worlds must give more than two passes of it"""
    import torch
    return xsup.GRID_PER_CU * int(torch.cuda.get_device_properties(0).multi_processor_count)


def stand_up(vis, world, wide=None):
    """binds the world (tables= of test_gpu_clusters_second.bind; wide: with cones and LOD entries), culls it under the far image — every
    view's draws are then the frustum's — and emits the instances of every view. Returns the views."""
    views = xsup.views_of(world)
    second.bind(vis, world.scene, world.ids, (wide[0], wide[1], wide[2]) if wide else world.tables)
    if wide:
        vis.bind_cluster_cones(0, wide[3])
        vis.bind_cluster_lods(0, wide[4])
    vis.hiz_build(xsup.image("far"))
    vis.cull(0, views)
    vis.emit_instances(0, list(range(len(views))))
    return views


class Frame:
    """what the twins need of the emission, fetched once: the records of every view as delivered, g_k, first_k"""

    def __init__(self, vis, world, views, tables):
        self.vis, self.world, self.views, self.tables = vis, world, views, tables
        self.fetched = second.fetch_all(vis, 0, list(range(len(views))), world.occupancy)
        self.starts = second.instance_starts(vis, 0)
        self.first = xsup.firsts(self.fetched, self.starts, None)
        self.n = [int(f["draw_count"]) for f in self.fetched]
        self.models = [np.asarray(f["baked_model"]).reshape(-1, 12)[:n] for f, n in zip(self.fetched, self.n)]
        self.g = [world.ids[f["visible_idx"][:n].astype(np.int64)].astype(np.uint32) for f, n in zip(self.fetched, self.n)]

    def _views(self):
        return zip(self.models, self.g, self.first, self.views)

    def plain(self, hizzes):
        t, r, c = self.tables[:3]
        got = [ksup.view_commands(m, g, first, view["view_proj"], hizzes[v], table=t, ranges=r, clusters=c) for v, (m, g, first, view) in enumerate(self._views())]
        return [x[0] for x in got], np.array([len(x[0]) for x in got], np.uint32), np.array([x[1] for x in got], np.uint32)

    def runs(self, hizzes):
        t, r, c = self.tables[:3]
        per_view, tested, base = [], [], 0
        for v, (m, g, first, view) in enumerate(self._views()):
            commands, n, census = rsup.view_commands(m, g, first, view["view_proj"], hizzes[v], base, t, r, c)
            base += census["candidates"]
            per_view.append(commands), tested.append(n)
        return per_view, np.array([len(x) for x in per_view], np.uint32), np.array(tested, np.uint32)

    def second(self, hiz1s, hiz2s):
        per_view, pending = [], []
        for v, (m, g, first, view) in enumerate(self._views()):
            if hiz1s[v] is None:
                per_view.append(np.zeros(0, ksup.COMMAND_DTYPE)), pending.append(0)
                continue
            commands, stats = ssup.second_view_commands(m, g, first, view["view_proj"], hiz1s[v], hiz2s[v], self.tables[:3])
            per_view.append(commands), pending.append(stats["pending"])
        return per_view, np.array([len(x) for x in per_view], np.uint32), np.array(pending, np.uint32)

    def wide(self, lod_views, eyes, hizzes, mode, hiz2s=None):
        per_view, tested = [], []
        for v, (m, g, first, view) in enumerate(self._views()):
            if mode == lsup.SECOND_PHASE and hizzes[v] is None:
                per_view.append(np.zeros(0, ksup.COMMAND_DTYPE)), tested.append(0)
                continue
            commands, n, _, _, _ = lsup.view_commands(m, g, first, view["view_proj"], lod_views[v], eyes[v], hizzes[v], mode,
                                                      None if hiz2s is None else hiz2s[v], self.tables)
            per_view.append(commands), tested.append(n)
        return per_view, np.array([len(x) for x in per_view], np.uint32), np.array(tested, np.uint32)


def check(vis, expected, launches, phase=1, dtype=csup.INDEXED, region=0, held=None, own=True, **call):
    """One call — phase 1: cull_clusters(**call), phase 2: cull_clusters_second_phase — own: into caller-owned device memory over the
    background, cut after `held` positions when given; every byte on the device and of a host fetch, both kinds of counts and the
    launch count against `expected` = (commands per view, counts, tested or pending). Returns the expected bytes."""
    import torch
    per_view, counts, tested = expected
    stride = dtype.itemsize
    rows = (len(per_view) * region if region else int(counts.sum())) + 7  # (a few rows behind the last position must stay untouched)
    pattern = csup.background(rows, stride)
    exp = xsup.place(per_view, dtype, region, held, pattern)
    if phase == 1:
        vis.set_command_layout(0, dtype=dtype)
    before = second.emit_launches(vis)
    target = None
    if own:
        dev = torch.full((rows, stride), csup.BACKGROUND, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # (torch's stream; the library's stream is non-blocking)
        target = (dev.data_ptr(), rows * stride if held is None else held * stride + 5)
    else:
        assert held is None
    if phase == 1:
        vis.cull_clusters(0, False, region, device=target, **call)
    else:
        vis.cull_clusters_second_phase(0, region, target=target)
    assert second.emit_launches(vis) - before == launches
    host = pattern.copy()
    _, got_counts, got_tested = (vis.cluster_commands if phase == 1 else vis.cluster_second_commands)(0, out=host)  # waits for the call
    print("commands", got_counts.tolist(), "expected", counts.tolist(), "tested" if phase == 1 else "pending", got_tested.tolist(), "expected", tested.tolist())
    assert got_tested.tolist() == tested.tolist()
    assert got_counts.tolist() == counts.tolist()  # (the true counts, also when the target is too small or a region is cut)
    first_wrong(host, exp)
    if own:
        first_wrong(dev.cpu().numpy(), exp)
    return exp


def first_wrong(got, exp):
    """exact equality of the bytes; a mismatch names the first wrong row (in place of a diff of megabytes)"""
    if got.tobytes() == exp.tobytes():
        return
    rows = np.nonzero((np.asarray(got).reshape(exp.shape) != exp).any(axis=1))[0]
    raise AssertionError(f"{len(rows)} of {len(exp)} rows differ, the first at position {int(rows[0])}: "
                         f"{np.asarray(got).reshape(exp.shape)[rows[0]].tolist()} for {exp[rows[0]].tolist()}")


# ---- world A: the count side -------------------------------------------------------------------------------------------------------

_A = {}


def frame_a(vis, oracle):
    """world A stood up on `vis`, its frame, and the conditions of the census that depend on the order of the records — repeated on the
    FETCHED records (reference-side data only) before a pass is trusted"""
    world = xsup.world_a()
    views = stand_up(vis, world)
    frame = Frame(vis, world, views, world.tables)
    if "checked" not in _A:
        records = list(zip(frame.models, frame.g, [np.arange(n + 1, dtype=np.uint32) for n in frame.n]))
        wall = oracle.Hiz(xsup.a_image("wall"))
        c = xsup.Candidates(records, views, [wall if h else None for h in world.hiz], world.tables, world.occupancy)
        assert c.blocks > xsup.SCAN_TURN and c.blocks % 4 != 0
        for v in (0, 1, 3, 4):
            assert frame.n[v] > xsup.SCAN_BLOCK * xsup.TILE, (v, frame.n[v])
            assert np.count_nonzero(c.is_cluster & (c.view == v) & (c.draw >= xsup.SCAN_BLOCK * xsup.TILE)) > 0, v
        assert frame.n[2] == 0 and c.start[5] > c.start[4] > 0
        assert c.widest_tile() >= 32 and c.emptied_blocks() >= 100
        assert sum(1 for v in range(5) if c.start[v] % xsup.TILE) >= 2
        _A["checked"] = True
    return world, views, frame


def a_hizzes(oracle, world, name):
    hiz = oracle.Hiz(xsup.a_image(name))
    return [hiz if h else None for h in world.hiz]


def test_world_a_plain_packed(oracle):
    with GpuVisibility(device=0) as vis:
        world, _, frame = frame_a(vis, oracle)
        vis.hiz_build(xsup.a_image("wall"))
        check(vis, frame.plain(a_hizzes(oracle, world, "wall")), PLAIN_LAUNCHES)


def test_world_a_plain_regions_library_owned(oracle):
    with GpuVisibility(device=0) as vis:
        world, _, frame = frame_a(vis, oracle)
        vis.hiz_build(xsup.a_image("wall"))
        expected = frame.plain(a_hizzes(oracle, world, "wall"))
        counts = expected[1]
        region = (int(counts[0]) + int(counts[1])) // 2
        assert int(counts[1]) < region < int(counts[0])   # R below one view's count and above another's
        check(vis, expected, PLAIN_LAUNCHES, region=region, own=False)


def test_world_a_runs_packed(oracle):
    with GpuVisibility(device=0) as vis:
        world, _, frame = frame_a(vis, oracle)
        vis.hiz_build(xsup.a_image("wall"))
        check(vis, frame.runs(a_hizzes(oracle, world, "wall")), RUN_LAUNCHES, runs=True)


def test_world_a_second_phase(oracle):
    with GpuVisibility(device=0) as vis:
        world, _, frame = frame_a(vis, oracle)
        hiz1s, hiz2s = a_hizzes(oracle, world, "wall"), a_hizzes(oracle, world, "narrow")
        vis.hiz_build(xsup.a_image("wall"))
        check(vis, frame.plain(hiz1s), PLAIN_LAUNCHES, own=False)
        vis.hiz_build(xsup.a_image("narrow"))
        expected = frame.second(hiz1s, hiz2s)
        assert 0 < int(expected[1].sum()) < int(expected[2].sum())
        check(vis, expected, SECOND_LAUNCHES, phase=2)


# ---- world B: the tile side --------------------------------------------------------------------------------------------------------

def frame_b(vis, wide=False):
    world = xsup.world_b()
    tables = xsup.b_wide_tables() if wide else world.tables
    views = stand_up(vis, world, tables if wide else None)
    frame = Frame(vis, world, views, tables)
    tiles = xsup.tiles_of(sum(int(xsup.candidates_per_draw(g, tables[0], tables[1]).sum()) for g in frame.g))
    assert tiles > 2 * walk_grid(), f"{tiles} candidate tiles are no third pass of a grid of {walk_grid()} workgroups: the test covers nothing here"
    assert tiles > xsup.SCAN_TURN and tiles % 4 != 0
    return world, views, frame


def b_hizzes(oracle, world, name):
    hiz = oracle.Hiz(xsup.image(name))
    return [hiz if h else None for h in world.hiz]


B_REGION = 300000   # 2 R > 524 288 positions: the padding loop strides; R is below view 0's count: the region is cut


def test_world_b_plain_packed_regions_held(oracle):
    with GpuVisibility(device=0) as vis:
        world, _, frame = frame_b(vis)
        vis.hiz_build(xsup.image("wall"))
        expected = frame.plain(b_hizzes(oracle, world, "wall"))
        counts = expected[1]
        assert int(counts[1]) < B_REGION < int(counts[0]) and 2 * B_REGION > walk_grid() * xsup.TILE   # (the padding loop strides by the grid)
        check(vis, expected, PLAIN_LAUNCHES)
        check(vis, expected, PLAIN_LAUNCHES, region=B_REGION)
        check(vis, expected, PLAIN_LAUNCHES, held=int(counts[0]) // 3 + 77)   # well below the counts: true counts, 0xA5 beyond


def test_world_b_runs_packed_and_regions(oracle):
    with GpuVisibility(device=0) as vis:
        world, _, frame = frame_b(vis)
        vis.hiz_build(xsup.image("wall"))
        expected = frame.runs(b_hizzes(oracle, world, "wall"))
        check(vis, expected, RUN_LAUNCHES, runs=True)
        check(vis, expected, RUN_LAUNCHES, runs=True, region=B_REGION)


def test_world_b_second_phase_dense(oracle):
    """K1 under a full-screen near wall: every tested cluster of view 0 (but the NaN boxes, which nothing rejects) is pending"""
    with GpuVisibility(device=0) as vis:
        world, _, frame = frame_b(vis)
        hiz1s, hiz2s = b_hizzes(oracle, world, "near"), b_hizzes(oracle, world, "wall")
        vis.hiz_build(xsup.image("near"))
        check(vis, frame.plain(hiz1s), PLAIN_LAUNCHES, own=False)
        vis.hiz_build(xsup.image("wall"))
        expected = frame.second(hiz1s, hiz2s)
        pending = int(expected[2].sum())
        assert pending >= (1 << 20) + 1 and xsup.tiles_of(pending) > 2 * walk_grid() and 0 < int(expected[1].sum()) < pending
        check(vis, expected, SECOND_LAUNCHES, phase=2)
        check(vis, expected, SECOND_LAUNCHES, phase=2, region=B_REGION)


def test_world_b_second_phase_sparse(oracle):
    """K1 under two small near patches: one in a hundred of view 0's clusters is pending, a pending tile spans hundreds of candidate tiles"""
    with GpuVisibility(device=0) as vis:
        world, _, frame = frame_b(vis)
        hiz1s, hiz2s = b_hizzes(oracle, world, "dots"), b_hizzes(oracle, world, "wall")
        vis.hiz_build(xsup.image("dots"))
        k1 = frame.plain(hiz1s)
        check(vis, k1, PLAIN_LAUNCHES, own=False)
        vis.hiz_build(xsup.image("wall"))
        expected = frame.second(hiz1s, hiz2s)
        pending = int(expected[2].sum())
        assert 0.005 * int(k1[2][0]) <= pending <= 0.02 * int(k1[2][0]) and 0 < int(expected[1].sum()) < pending
        check(vis, expected, SECOND_LAUNCHES, phase=2)


def test_world_b_lods_cones_runs_and_second(oracle):
    """cones and LOD entries over B's clusters, a point eye and a scale above 0 in both views: the run form, then the second phase
    behind it under a rebuilt pyramid, against the LOD twin"""
    lod_views, eyes = np.array(xsup.b_lod_views(), lsup.CLUSTER_LOD_VIEW_DTYPE), xsup.B_EYES
    with GpuVisibility(device=0) as vis:
        world, _, frame = frame_b(vis, wide=True)
        hiz1s, hiz2s = b_hizzes(oracle, world, "wall"), b_hizzes(oracle, world, "narrow")
        vis.hiz_build(xsup.image("wall"))
        runs = frame.wide(lod_views, eyes, hiz1s, lsup.RUN_FORM)
        assert 0 < int(runs[1].sum()) < int(runs[2].sum())
        check(vis, runs, RUN_LAUNCHES, runs=True, eyes=eyes, lods=lod_views)
        vis.hiz_build(xsup.image("narrow"))
        expected = frame.wide(lod_views, eyes, hiz1s, lsup.SECOND_PHASE, hiz2s)
        assert xsup.tiles_of(int(expected[2].sum())) > walk_grid() and 0 < int(expected[1].sum()) < int(expected[2].sum())
        check(vis, expected, SECOND_LAUNCHES, phase=2)


def test_world_b_two_calls_identical(oracle):
    with GpuVisibility(device=0) as vis:
        world, _, frame = frame_b(vis)
        vis.hiz_build(xsup.image("wall"))
        vis.set_command_layout(0, dtype=csup.INDEXED)
        got = []
        for _ in range(2):
            vis.cull_clusters(0)
            got.append([x.tobytes() for x in vis.cluster_commands(0)])
        assert got[0] == got[1] and len(got[0][0]) > xsup.SCAN_TURN * xsup.TILE
