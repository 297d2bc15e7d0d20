"""gv_pool_cull_cluster_runs on the device: the cluster cull's decisions, one indirect command per run of adjacent surviving
clusters. Which cluster survives is decided only by the oracle's gvo_is_behind_frustum / gvo_hiz_occluded, called by cluster_twin.h
over the FETCHED records and the oracle's pyramid; linked, head, run and the run's command are restated in
tests/cluster_runs_twin.h, the placement in tests/clusters_support.py. Every comparison is exact: every command byte over a 0xA5
background, the bytes behind the last written position included, and every count word. The case table is clusters_support.CASES
over the contiguous tables of cluster_runs_support.geometry(); it and the designed scenes are held to their conditions on the oracle
and the twin alone by tests/test_cluster_runs_census.py."""
import numpy as np
import pytest

import cluster_runs_support as rsup
import clusters_support as ksup
import commands_support as csup
import instances_support as isup
import lod_support as lsup
from garden_amd.lib import GV_DIRTY_GEOMETRY, GV_DIRTY_MESH, GpuVisibility

pytestmark = pytest.mark.gpu

LAUNCHES = 6        # of one gv_pool_cull_cluster_runs, whatever the data holds (include/garden_vis.h)
PLAIN_LAUNCHES = 5  # of one gv_pool_cull_clusters


def bind(vis, sc, ids, tables=None, pool_id=0):
    table, _, ranges, clusters = rsup.geometry() if tables is None else (tables[0], None, tables[1], tables[2])
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()
    vis.bind_geometry(pool_id, ids, table)
    vis.bind_clusters(pool_id, ranges, clusters)
    vis.set_instance_layout(pool_id, dtype=isup.BARE)


def fetch_all(vis, pool_id, listed, occupancy):
    return [vis.fetch(v, write_back=False, occupancy=occupancy, order="raw", pool_id=pool_id) for v in listed]


def instance_starts(vis, pool_id):
    import ctypes as C
    views = vis.instances_info(pool_id)[0]
    starts = np.zeros(views + 1, np.uint32)
    vis._check(vis.lib.gv_pool_instances_fetch(vis.ctx, pool_id, None, 0, starts.ctypes.data_as(C.POINTER(C.c_uint32)), len(starts)))
    return starts


def emit_launches(vis):
    return vis.stats()["launches"]["emit"]


def slot_ids(ids):
    """g_k of a view's draws from the per-slot ids"""
    return lambda v, f: np.asarray(ids)[f["visible_idx"][:int(f["draw_count"])].astype(np.int64)].astype(np.uint32)


def check(vis, listed, occupancy, ids_of, views, hizzes, dtype=csup.INDEXED, frustum_only=False, region=0, held=None, own=True, draws=False,
          pool_id=0, tables=None):
    """Culls the clusters of the pool's last instance emission into runs — own: into caller-owned device memory over the background,
    cut after `held` positions when given — and compares every byte on the device and of a host fetch, and both kinds of counts, with
    the twin's. Arguments as test_gpu_clusters.check. Returns (expected bytes, counts, tested, the census, the commands per view)."""
    import torch
    fetched = fetch_all(vis, pool_id, listed, occupancy)
    starts = instance_starts(vis, pool_id)
    bases = vis.draw_bases(pool_id) if draws else None
    draw_ids = [ids_of(v, f) for v, f in enumerate(fetched)]
    stride = dtype.itemsize
    used = [None if frustum_only else h for h in hizzes]
    per_view, counts, tested, census = rsup.commands_of(fetched, starts, bases, draw_ids, views, used, tables)
    rows = (len(listed) * region if region else int(counts.sum())) + 7  # (a few rows behind the last position must stay untouched)
    pattern = csup.background(rows, stride)
    exp = ksup.place(per_view, dtype, region, held, pattern)
    vis.set_command_layout(pool_id, dtype=dtype)
    before = emit_launches(vis)
    if own:
        dev = torch.full((rows, stride), csup.BACKGROUND, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # (torch's stream; the library's stream is non-blocking)
        vis.cull_clusters(pool_id, frustum_only, region, device=(dev.data_ptr(), rows * stride if held is None else held * stride + 5), runs=True)
        assert vis.cluster_commands_device(pool_id)[0] == dev.data_ptr()
    else:
        assert held is None
        vis.cull_clusters(pool_id, frustum_only, region, runs=True)
    assert emit_launches(vis) - before == LAUNCHES
    host = pattern.copy()
    _, got_counts, got_tested = vis.cluster_commands(pool_id, out=host)  # waits for the call
    print("commands", got_counts.tolist(), "expected", counts.tolist(), "tested", got_tested.tolist(), "expected", tested.tolist(), census)
    assert got_counts.tolist() == counts.tolist()  # (the true counts, also when the target is too small or a region is cut)
    assert got_tested.tolist() == tested.tolist()
    assert host.tobytes() == exp.tobytes()
    if own:
        assert dev.cpu().numpy().tobytes() == exp.tobytes()
    return exp, counts, tested, census, per_view


def plain_commands(vis, pool_id, dtype=csup.INDEXED):
    """(the bytes, counts, tested) of a plain cluster cull of the pool's emission into the library's buffer"""
    vis.set_command_layout(pool_id, dtype=dtype)
    before = emit_launches(vis)
    vis.cull_clusters(pool_id)
    assert emit_launches(vis) - before == PLAIN_LAUNCHES
    commands, counts, tested = vis.cluster_commands(pool_id)
    return np.asarray(commands).copy(), counts.copy(), tested.copy()


# ---- 1. the case table ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ksup.CASES, ids=[c.name for c in ksup.CASES])
def test_case_table_against_the_twin(case, oracle):
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    views = ksup.case_views(case)
    listed = list(range(len(views)))
    depth = ksup.wall_depth()
    hiz = oracle.Hiz(depth)
    hizzes = [hiz if h else None for h in case.hiz]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        if any(case.hiz):
            vis.hiz_build(depth)
        vis.cull(0, views)
        vis.emit_instances(0, listed)
        # the per-draw commands and the instance data, as they stand before the cluster cull
        vis.set_command_layout(0, dtype=csup.INDEXED)
        vis.emit_draw_commands(0)
        per_draw = vis.draw_commands(0)[0].tobytes()
        instances = vis.instances(0)[0].tobytes()
        _, counts, _, census, _ = check(vis, listed, sc.count, slot_ids(ids), views, hizzes)  # caller-owned, packed
        check(vis, listed, sc.count, slot_ids(ids), views, hizzes, own=False)                 # library-owned
        if case.draws:
            assert census["runs"] + census["whole"] == int(counts.sum()) and 2 * census["runs"] <= census["survivors"]
        assert vis.draw_commands(0)[0].tobytes() == per_draw and vis.instances(0)[0].tobytes() == instances


# ---- 2. the rule's edges, in designed scenes --------------------------------------------------------------------------------------

def design_check(vis, sc, order, name, lead):
    """designed scene `name` behind `lead` whole draws: ids by delivery order, bound anew in front of the emission; every byte against the twin"""
    survive, rows, gfirst, want = rsup.design_patterns()[name]
    tables = rsup.design_tables(survive, rows, gfirst)
    ids = np.full(sc.count, rsup.VOID_ID, np.uint32)
    ids[order[:lead]] = rsup.WHOLE_ID
    ids[order[lead]] = rsup.CLUSTERED_ID
    vis.bind_geometry(0, ids, tables[0])
    vis.bind_clusters(0, tables[1], tables[2])
    vis.emit_instances(0, [0])
    _, counts, tested, census, per_view = check(vis, [0], sc.count, slot_ids(ids), [ksup.camera()], [None], tables=tables)
    assert int(tested[0]) == len(survive) and census["whole"] == lead and census["survivors"] == sum(survive)
    for key, value in want.items():
        assert census[key] == value, (key, census)
    assert int(counts[0]) == lead + census["runs"]
    return per_view[0]


@pytest.mark.parametrize("lead", rsup.LEADS)
def test_designed_scenes_at_every_lead(lead, oracle):
    """one clustered draw of an unrotated entity wholly inside the frustum, its first candidate at offset `lead` of a word and a tile"""
    sc = rsup.design_scene()
    patterns = rsup.design_patterns()
    with GpuVisibility(device=0) as vis:
        first = rsup.design_tables(*patterns["all-1"][:3])
        bind(vis, sc, np.full(sc.count, rsup.VOID_ID, np.uint32), tables=first)
        vis.cull(0, [ksup.camera()])
        f = fetch_all(vis, 0, [0], sc.count)[0]
        assert int(f["draw_count"]) == sc.count
        order = f["visible_idx"][:sc.count].astype(np.int64)
        for name in sorted(patterns):
            commands = design_check(vis, sc, order, name, lead)
            if name == "all-513":
                assert [int(c) for c in commands["draw"][lead:]] == [lead] * 3
            if name == "wrap":  # the head's uint32 add wraps, and the cluster that ends at 2^32 stands alone
                rows, gfirst = rsup.rows_of_geometry(rsup.WRAP_GEOMETRY)
                assert int(commands[lead]["first"]) == (gfirst + rows[0][0]) & 0xFFFFFFFF
                assert int(commands[lead + 1]["count"]) == rows[rsup.WRAP_AT][1]


# ---- 3. views and placement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["plain16", "gaps32", "wide64"])
def test_layouts_every_byte_of_the_stride(layout, oracle):
    dtype = {"plain16": csup.PLAIN, "gaps32": csup.GAPS, "wide64": csup.WIDE}[layout]
    sc, ids = ksup.world(64)
    view = ksup.camera()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.cull(0, [view])
        vis.emit_instances(0, [0])
        check(vis, [0], sc.count, slot_ids(ids), [view], [None], dtype=dtype)


@pytest.mark.parametrize("name", ["views-2", "views-8"])
def test_views_with_and_without_the_query_regions_and_a_cut_target(name, oracle):
    case = ksup.CASE[name]
    sc, ids = ksup.world(case.draws)
    views = ksup.case_views(case)
    listed = list(range(len(views)))
    depth = ksup.wall_depth()
    hiz = oracle.Hiz(depth)
    hizzes = [hiz if h else None for h in case.hiz]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(depth)
        vis.cull(0, views)
        vis.emit_instances(0, listed)
        _, counts, _, census, _ = check(vis, listed, sc.count, slot_ids(ids), views, hizzes)
        starts = np.concatenate([[0], np.cumsum(counts)])
        assert census["cross_word"] >= 1
        _, plain, _, _, _ = check(vis, listed, sc.count, slot_ids(ids), views, hizzes, frustum_only=True)  # the flag against the same world
        assert int(plain.sum()) != int(counts.sum())
        low, high = int(counts.min()), int(counts.max())
        assert low > 20
        check(vis, listed, sc.count, slot_ids(ids), views, hizzes, region=low - 9)         # R below every C_v: commands beyond R are not written
        check(vis, listed, sc.count, slot_ids(ids), views, hizzes, region=high + 30)       # R above every C_v: zero padding
        check(vis, listed, sc.count, slot_ids(ids), views, hizzes, region=high + 30, own=False)
        check(vis, listed, sc.count, slot_ids(ids), views, hizzes, held=int(starts[1]) + int(counts[1]) // 2)  # a cut inside view 1
        check(vis, listed, sc.count, slot_ids(ids), views, hizzes, region=high + 30, held=high + 30 + 11)


# ---- 4. where the ids, the instance ranges and the order come from ------------------------------------------------------------------

def test_ids_from_a_lod_selection(oracle, tmp_path):
    sc, ids = ksup.world(257, ids_mode="lod")
    view = ksup.camera()
    switch_at = lsup.quantile_thresholds(sc.transforms["position"], np.ones(sc.count, np.float32), ksup.LOD_LEVELS)
    lod = lsup.lod_table([(1, [])] * ksup.LOD_BASE + [(ksup.LOD_LEVELS, switch_at)])
    twin = lsup.build_twin(tmp_path)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.bind_lod(0, None, lod)
        vis.cull(0, [view])
        vis.emit_instances(0, [0])
        fetched = fetch_all(vis, 0, [0], sc.count)
        selected, level_counts = lsup.select_expected(twin, fetched, [1.0], ids, None, lod)
        assert np.count_nonzero(level_counts[0]) == ksup.LOD_LEVELS  # every level holds draws
        vis.select_lods(0, [1.0])
        _, _, tested, _, _ = check(vis, [0], sc.count, lambda v, f: selected[v], [view], [None])
        assert int(tested[0]) == int((level_counts[0][:3] * np.array([64, 8, 1])).sum())


def test_a_mark_made_between_the_emission_and_the_call_is_seen(oracle):
    sc, ids = ksup.world(255)
    ids = ids.copy()
    view = ksup.camera()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.cull(0, [view])
        vis.emit_instances(0, [0])
        exp, _, _, _, _ = check(vis, [0], sc.count, slot_ids(ids), [view], [None])
        ids[:] = (ids + 3) % (ksup.TABLE_COUNT + 1)  # every slot another geometry; some become void, some whole
        vis.mark_dirty(GV_DIRTY_GEOMETRY, 0, sc.count, pool_id=0)
        after, _, _, _, _ = check(vis, [0], sc.count, slot_ids(ids), [view], [None])
        assert after.tobytes() != exp.tobytes()


def test_after_a_draw_emission_with_counts_0_1_and_3(oracle):
    sc, ids = ksup.world(257)
    view = ksup.camera()
    ready = (np.arange(sc.count, dtype=np.uint32) % 3) * np.uint32(3) // np.uint32(2)  # 0, 1, 3 in turn
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        column = np.ones(sc.count, np.uint32)
        vis.bind_ready(0, column)
        vis.cull(0, [view])
        column[:] = ready  # changed and marked after the cull, so that every box stays a draw
        vis.mark_dirty(GV_DIRTY_MESH, 0, sc.count, pool_id=0)
        vis.emit_draw_instances(0, [0])
        exp, counts, _, _, _ = check(vis, [0], sc.count, slot_ids(ids), [view], [None], dtype=csup.GAPS, draws=True)
        got = exp[:int(counts[0])].reshape(-1).view(csup.GAPS)
        assert set(got["instance_count"].tolist()) == {1, 3}


def test_a_sorted_and_a_grouped_view_and_a_view_that_names_pyramid_3(oracle):
    case = ksup.CASE["views-2"]
    sc, ids = ksup.world(case.draws)
    views = [ksup.camera(0.0, use_hiz=4), ksup.camera(0.4, use_hiz=0, shadow_pass=1)]
    depth = ksup.wall_depth()
    hiz = oracle.Hiz(depth)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_select(3)
        vis.hiz_build(depth)
        vis.hiz_select(0)
        vis.cull(0, views)
        vis.sort(0, descending=False, pool_id=0)
        vis.group_draws(1, pool_id=0)
        vis.emit_instances(0, [0, 1])
        _, counts, _, _, _ = check(vis, [0, 1], sc.count, slot_ids(ids), views, [hiz, None])
        _, plain, _, _, _ = check(vis, [0, 1], sc.count, slot_ids(ids), views, [hiz, None], frustum_only=True)
        assert int(counts[0]) != int(plain[0]) and int(counts[1]) == int(plain[1])  # the wall of pyramid 3 was queried, for view 0 alone


# ---- 5. against the plain form ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["draws-257", "views-8", "two-tiles-plus-1"])
def test_the_runs_are_the_plain_commands_coalesced_by_the_rule(name, oracle):
    case = ksup.CASE[name]
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    views = ksup.case_views(case)
    listed = list(range(len(views)))
    depth = ksup.wall_depth()
    table, _, ranges, clusters = rsup.geometry()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        if any(case.hiz):
            vis.hiz_build(depth)
        vis.cull(0, views)
        vis.emit_instances(0, listed)
        fetched = fetch_all(vis, 0, listed, sc.count)
        plain, plain_counts, plain_tested = plain_commands(vis, 0, dtype=csup.WIDE)  # (a layout that carries the draw's number)
        vis.cull_clusters(0, runs=True)
        runs, run_counts, run_tested = vis.cluster_commands(0)
        runs = np.asarray(runs).copy()
        assert run_tested.tolist() == plain_tested.tolist()
        again, again_counts, _ = plain_commands(vis, 0, dtype=csup.WIDE)  # the plain form afterwards: its old bytes
        assert again.tobytes() == plain.tobytes() and again_counts.tolist() == plain_counts.tolist()
    plain, runs = plain.reshape(-1).view(csup.WIDE), runs.reshape(-1).view(csup.WIDE)
    fields = ("count", "instance_count", "first", "first_instance", "vertex_offset", "draw")
    at, run_at, merged = 0, 0, 0
    for v, f in enumerate(fetched):
        g = slot_ids(ids)(v, f)

        def clusters_of_draw(k):
            if g[k] >= len(ranges) or not int(ranges[g[k]]["count"]):
                return int(table[g[k]]["first"]), None
            a, n = int(ranges[g[k]]["first"]), int(ranges[g[k]]["count"])
            return int(table[g[k]]["first"]), clusters[a:a + n]

        mine = plain[at:at + int(plain_counts[v])]
        rows = np.zeros(len(mine), ksup.COMMAND_DTYPE)
        for field in fields:
            rows[field] = mine[field]
        want = rsup.coalesce(rows, clusters_of_draw)
        got = runs[run_at:run_at + int(run_counts[v])]
        assert len(got) == len(want)
        for field in fields:
            assert got[field].tolist() == want[field].tolist(), field
        merged += len(mine) - len(got)
        at += int(plain_counts[v])
        run_at += int(run_counts[v])
    assert merged > 0


# ---- 6. the second phase behind a run cull ------------------------------------------------------------------------------------------

def test_the_second_phase_behind_a_run_cull_is_the_one_behind_a_plain_cull(oracle):
    sc, ids = ksup.world(257)
    views = [ksup.camera(0.0, use_hiz=1), ksup.camera(0.4, use_hiz=0, shadow_pass=1)]
    old, new = ksup.wall_depth(x0=0.0), ksup.wall_depth(x0=0.7)
    got = {}
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(old)
        vis.cull(0, views)
        vis.emit_instances(0, [0, 1])
        vis.set_command_layout(0, dtype=csup.WIDE)
        for runs in (False, True, False):
            vis.hiz_build(old)
            vis.cull_clusters(0, runs=runs)
            first = [np.asarray(x).copy() for x in vis.cluster_commands(0)]
            vis.hiz_build(new)
            vis.cull_clusters_second_phase(0)
            second = [np.asarray(x).copy() for x in vis.cluster_second_commands(0)]
            assert [np.asarray(x).tobytes() for x in vis.cluster_commands(0)] == [x.tobytes() for x in first]  # the second phase writes none of it
            got.setdefault(runs, []).append(second)
    (plain, again), (behind_runs,) = got[False], got[True]
    assert int(plain[1][0]) > 0 and int(plain[2][0]) > 0  # clusters were pending, and some came out from behind the narrower wall
    for a, b, c in zip(plain, behind_runs, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()


# ---- 7. repeatability and the launch count ------------------------------------------------------------------------------------------

def test_two_calls_give_identical_bytes_and_the_launch_count_is_constant(oracle):
    got = {}
    for draws in (0, 257):
        sc, ids = ksup.world(draws)
        view = ksup.camera(use_hiz=1)
        with GpuVisibility(device=0) as vis:
            bind(vis, sc, ids)
            vis.hiz_build(ksup.wall_depth())
            vis.cull(0, [view])
            vis.emit_instances(0, [0])
            vis.set_command_layout(0, dtype=csup.GAPS)
            before = emit_launches(vis)
            vis.cull_clusters(0, runs=True)
            got[draws] = emit_launches(vis) - before
            one = [np.asarray(x).tobytes() for x in vis.cluster_commands(0)]
            vis.cull_clusters(0, runs=True)
            two = [np.asarray(x).tobytes() for x in vis.cluster_commands(0)]
            assert one == two and (draws == 0 or len(one[0]) > 0)
    assert got[0] == got[257] == LAUNCHES


# ---- 8. the shim --------------------------------------------------------------------------------------------------------------------

def test_cluster_runs_shim_five_ticks_against_the_twin():
    """tests/cpp/cluster_runs.cpp: main pass + three cascades, a moving camera, LODs on, GpuClusterCommands::setRuns on; every command
    equals a host path that fetches the records, calls the oracle and merges by the twin's rule"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "build", "cluster_runs")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "tests", "cpp"), "-f", "cluster_runs.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    result = json.loads(run.stdout.splitlines()[-1])
    print(result)
    assert result["ok"] and result["ticks"] == 5 and result["passes"] == 4
    assert result["whole"] > 0 and result["gaps"] > 0 and result["longest"] == 11
    assert result["tested"] > result["survivors"] >= 2 * result["runs"] > 0  # clusters were culled, and survivors merged
