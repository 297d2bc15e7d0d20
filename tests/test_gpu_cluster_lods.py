"""gv_pool_bind_cluster_lods / gv_pool_cull_cluster_lods on the device: the cluster cull over the cut through a bound cluster DAG.
Which cluster passes the frustum and the pyramid is decided only by the oracle's gvo_is_behind_frustum / gvo_hiz_occluded, called by
cluster_twin.h over the FETCHED records and the oracle's pyramid; the cut, the conjunction and the second phase's pending set under
it are restated in tests/cluster_lod_twin.h, the cone test in tests/cluster_cone_twin.h, the run rule in tests/cluster_runs_twin.h,
the placement in tests/clusters_support.py. Every comparison is exact: every command byte over a 0xA5 background, the bytes behind
the last written position included, and every count word. The case table, the DAG fixture and the designed entries, draws and views
are cluster_lods_support's; tests/test_cluster_lods_census.py holds them to their conditions on the oracle and the twin alone."""
import numpy as np
import pytest

import cluster_lods_support as dsup
import clusters_second_support as ssup
import clusters_support as ksup
import commands_support as csup
import instances_support as isup
import lod_support as lsup
from garden_amd.lib import GpuVisibility

pytestmark = pytest.mark.gpu

LAUNCHES = {False: 5, True: 6}  # of one gv_pool_cull_cluster_lods without / with GV_CLUSTERS_RUNS, whatever the data holds


def bind(vis, sc, ids, pool_id=0):
    table, ranges, clusters, cones, lods = dsup.geometry()
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()
    vis.bind_geometry(pool_id, ids, table)
    vis.bind_clusters(pool_id, ranges, clusters)
    vis.bind_cluster_cones(pool_id, cones)
    vis.bind_cluster_lods(pool_id, lods)
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


def check(vis, listed, occupancy, ids_of, views, lod_views, eyes, hizzes, runs=False, dtype=csup.INDEXED, frustum_only=False, region=0, held=None,
          own=True, pool_id=0):
    """Culls the clusters of the pool's last instance emission over the cut — own: into caller-owned device memory over the
    background, cut after `held` positions when given — and compares every byte on the device and of a host fetch, and both kinds of
    counts, with the twin's. Returns (expected bytes, counts, tested, the census, the verdicts per view)."""
    import torch
    fetched = fetch_all(vis, pool_id, listed, occupancy)
    starts = instance_starts(vis, pool_id)
    draw_ids = [ids_of(v, f) for v, f in enumerate(fetched)]
    stride = dtype.itemsize
    used = [None if frustum_only else h for h in hizzes]
    per_view, counts, tested, census, verdicts = dsup.commands_of(fetched, starts, None, draw_ids, views, lod_views, eyes, used,
                                                                  dsup.RUN_FORM if runs else dsup.PLAIN_FORM)
    rows = (len(listed) * region if region else int(counts.sum())) + 7  # (a few rows behind the last position must stay untouched)
    pattern = csup.background(rows, stride)
    exp = ksup.place(per_view, dtype, region, held, pattern)
    vis.set_command_layout(pool_id, dtype=dtype)
    before = emit_launches(vis)
    if own:
        dev = torch.full((rows, stride), csup.BACKGROUND, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # (torch's stream; the library's stream is non-blocking)
        vis.cull_clusters(pool_id, frustum_only, region, device=(dev.data_ptr(), rows * stride if held is None else held * stride + 5), runs=runs,
                          eyes=eyes, lods=lod_views)
        assert vis.cluster_commands_device(pool_id)[0] == dev.data_ptr()
    else:
        assert held is None
        vis.cull_clusters(pool_id, frustum_only, region, runs=runs, eyes=eyes, lods=lod_views)
    assert emit_launches(vis) - before == LAUNCHES[runs]
    host = pattern.copy()
    _, got_counts, got_tested = vis.cluster_commands(pool_id, out=host)  # waits for the call
    print("runs" if runs else "plain", "commands", got_counts.tolist(), "expected", counts.tolist(), "tested", got_tested.tolist(), "expected",
          tested.tolist(), census)
    assert got_counts.tolist() == counts.tolist()  # (the true counts, also when the target is too small or a region is cut)
    assert got_tested.tolist() == tested.tolist()  # (a LOD-rejected cluster counts as tested)
    assert host.tobytes() == exp.tobytes()
    if own:
        assert dev.cpu().numpy().tobytes() == exp.tobytes()
    return exp, counts, tested, census, verdicts


def fetched_bytes(vis, pool_id=0):
    return [np.asarray(x).copy().tobytes() for x in vis.cluster_commands(pool_id)]


# ---- 1. the case table ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", dsup.CASES, ids=[c.name for c in dsup.CASES])
def test_case_table_against_the_twin(case, oracle):
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    views = dsup.case_views(case)
    lod_views, eyes = dsup.lod_views_of(case), dsup.eyes_of(case)
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
        args = (vis, listed, sc.count, slot_ids(ids), views, lod_views)
        _, plain_counts, _, census, _ = check(*args, eyes, hizzes)   # caller-owned, packed
        check(*args, eyes, hizzes, own=False)                        # library-owned
        _, run_counts, _, _, _ = check(*args, eyes, hizzes, runs=True)
        check(*args, eyes, hizzes, runs=True, own=False)
        check(*args, None if eyes is not None else dsup.nsup.eyes_of(case._replace(eyes="P" * len(views))), hizzes)  # the other form: without / with eyes
        if any(case.hiz):
            check(*args, eyes, hizzes, frustum_only=True)
            check(*args, eyes, hizzes, runs=True, frustum_only=True)
        if census["tested"] >= dsup.SHARE_FROM:
            assert 0 < census["survivors"] < census["lod_kept"] < census["tested"] and int(run_counts.sum()) <= int(plain_counts.sum())
        assert vis.draw_commands(0)[0].tobytes() == per_draw and vis.instances(0)[0].tobytes() == instances


# ---- 2. scale 0 in every view: the bytes of the older forms --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["draws-257", "views-8-eyes"])
def test_scale_0_in_every_view_gives_the_bytes_of_the_older_forms(name, oracle):
    case = dsup.CASE[name]
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    views = dsup.case_views(case)
    listed = list(range(len(views)))
    eyes = dsup.eyes_of(case)
    off = np.array([dsup.lod_view(scale=0.0 if v % 2 else -0.0) for v in listed], dsup.CLUSTER_LOD_VIEW_DTYPE)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(ksup.wall_depth())
        vis.cull(0, views)
        vis.emit_instances(0, listed)
        vis.set_command_layout(0, dtype=csup.WIDE)
        for runs in (False, True):
            for e in (None, eyes):
                vis.cull_clusters(0, runs=runs, eyes=e)
                older = fetched_bytes(vis)
                vis.cull_clusters(0, runs=runs, eyes=e, lods=off)
                assert fetched_bytes(vis) == older and len(older[0]) > 0
                vis.cull_clusters(0, runs=runs, eyes=e, lods=dsup.lod_views_of(case))
                cut = fetched_bytes(vis)
                assert cut[0] != older[0] and len(cut[0]) < len(older[0]) and cut[2] == older[2]  # (fewer commands, as many tested)


# ---- 3. views and placement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("runs", [False, True], ids=["plain", "runs"])
@pytest.mark.parametrize("name", ["views-2", "views-8-eyes"])
def test_views_regions_and_a_cut_target(name, runs, oracle):
    case = dsup.CASE[name]
    sc, ids = ksup.world(case.draws)
    views = dsup.case_views(case)
    lod_views, eyes = dsup.lod_views_of(case), dsup.eyes_of(case)
    listed = list(range(len(views)))
    depth = ksup.wall_depth()
    hiz = oracle.Hiz(depth)
    hizzes = [hiz if h else None for h in case.hiz]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(depth)
        vis.cull(0, views)
        vis.emit_instances(0, listed)
        args = (vis, listed, sc.count, slot_ids(ids), views, lod_views, eyes, hizzes)
        _, counts, _, _, _ = check(*args, runs=runs, dtype=csup.GAPS)
        starts = np.concatenate([[0], np.cumsum(counts)])
        low, high = int(counts.min()), int(counts.max())
        assert low > 20
        check(*args, runs=runs, region=low - 9)     # R below every C_v
        check(*args, runs=runs, region=high + 30)   # R above every C_v: zero padding
        check(*args, runs=runs, region=high + 30, own=False)
        check(*args, runs=runs, held=int(starts[1]) + int(counts[1]) // 2)  # a cut inside view 1
        check(*args, runs=runs, region=high + 30, held=high + 30 + 11)


# ---- 4. the designed entries, draws and views ------------------------------------------------------------------------------------------

def test_designed_entries_draws_and_views(oracle):
    sc, ids, _, _ = dsup.design_scene()
    view = ksup.camera()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.cull(0, [view])
        vis.emit_instances(0, [0])
        for name, lod in dsup.design_views().items():
            lod_views = np.array([lod], dsup.CLUSTER_LOD_VIEW_DTYPE)
            for runs in (False, True):
                _, counts, tested, census, verdicts = check(vis, [0], sc.count, slot_ids(ids), [view], lod_views, None, [None], runs=runs, dtype=csup.WIDE)
                assert int(tested[0]) == census["tested"] == 4 * len(dsup.DESIGNED) + 60 * dsup.GEOMETRY_CLUSTERS[dsup.DAG_ID]
                assert census["base_kept"] == census["tested"]  # every cluster is inside the frustum: the commands are the cut
                if not runs:
                    assert int(counts[0]) == census["lod_kept"] > 0
            if name in ("camera", "parallel"):  # the side every designed entry was designed for (the census holds the twin to it)
                verdict, at, g = verdicts[0]
                fetched = fetch_all(vis, 0, [0], sc.count)[0]
                k = int(np.flatnonzero(fetched["visible_idx"][:int(fetched["draw_count"])] == dsup.DESIGN_IDENTITY)[0])
                kept = [bool(b & dsup.KEPT) for b in verdict[int(at[k]):int(at[k + 1])]]
                assert kept == [d[3 if name == "camera" else 4] for d in dsup.DESIGNED]


# ---- 5. ids from a LOD selection ---------------------------------------------------------------------------------------------------------

def test_ids_from_a_lod_selection(oracle, tmp_path):
    sc, ids = ksup.world(257, ids_mode="lod")
    view = ksup.camera()
    lod_views = np.array([dsup.lod_view(scale=dsup.CAMERA_SCALE * 0.1)], dsup.CLUSTER_LOD_VIEW_DTYPE)
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
        for runs in (False, True):
            _, _, tested, census, _ = check(vis, [0], sc.count, lambda v, f: selected[v], [view], lod_views, None, [None], runs=runs)
            per_id = np.array(dsup.GEOMETRY_CLUSTERS + (len(dsup.DESIGNED), 0))  # (the anchor keeps its own id: it has one level)
            assert set(range(ksup.LOD_BASE, ksup.LOD_BASE + ksup.LOD_LEVELS)) <= set(selected[0].tolist())
            assert int(tested[0]) == int(per_id[selected[0]].sum()) and 0 < census["lod_kept"] < census["tested"]


# ---- 6. the second phase -------------------------------------------------------------------------------------------------------------

def second_check(vis, listed, occupancy, ids, views, lod_views, eyes, hiz1s, hiz2s, lods):
    """the second phase behind the pool's cluster result against the twin: under the LOD conjunction, or an older form's own rule
    (the LOD twin with every view switched off, which the census holds equal to the plain form's twin)"""
    fetched = fetch_all(vis, 0, listed, occupancy)
    starts = instance_starts(vis, 0)
    draw_ids = [slot_ids(ids)(v, f) for v, f in enumerate(fetched)]
    off = np.array([dsup.lod_view(scale=0.0)] * len(listed), dsup.CLUSTER_LOD_VIEW_DTYPE)
    per_view, counts, pending, census, _ = dsup.commands_of(fetched, starts, None, draw_ids, views, lod_views if lods else off, eyes, hiz1s,
                                                            dsup.SECOND_PHASE, hiz2s)
    if not lods and eyes is None:  # the plain form's own twin
        table, ranges, clusters, _, _ = dsup.geometry()
        own = ssup.second_commands_of(fetched, starts, None, draw_ids, views, hiz1s, hiz2s, (table, ranges, clusters))
        assert own[1].tolist() == counts.tolist() and own[2].tolist() == pending.tolist()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(own[0], per_view))
    stride = csup.WIDE.itemsize
    rows = int(counts.sum()) + 7
    pattern = csup.background(rows, stride)
    exp = ksup.place(per_view, csup.WIDE, 0, None, pattern)
    before = emit_launches(vis)
    vis.cull_clusters_second_phase(0)
    assert emit_launches(vis) - before == 5
    host = pattern.copy()
    _, got_counts, got_pending = vis.cluster_second_commands(0, out=host)
    print("second phase", "lods" if lods else "older", got_counts.tolist(), counts.tolist(), "pending", got_pending.tolist(), pending.tolist(), census)
    assert got_counts.tolist() == counts.tolist() and got_pending.tolist() == pending.tolist()
    assert host.tobytes() == exp.tobytes()
    return counts, pending, host.tobytes()


def test_the_second_phase_behind_a_lod_result_and_behind_the_older_forms(oracle):
    sc, ids = ksup.world(257)
    views = [ksup.camera(0.0, use_hiz=1), ksup.camera(0.4, use_hiz=0, shadow_pass=1)]
    eyes = np.array([dsup.nsup.POINT_EYE, dsup.nsup.direction_eye(0.4)], np.float32)
    lod_views = np.array([dsup.lod_view(scale=dsup.CAMERA_SCALE * 0.1), dsup.lod_view(eye=(0, 0, 0, 0), scale=dsup.PARALLEL_SCALE * 0.1)],
                         dsup.CLUSTER_LOD_VIEW_DTYPE)
    old, new = ksup.wall_depth(x0=0.0), ksup.wall_depth(x0=0.7)
    hiz1, hiz2 = oracle.Hiz(old), oracle.Hiz(new)
    hiz1s, hiz2s = [hiz1, None], [hiz2, None]
    forms = {"plain": (False, None, None), "lods": (False, None, lod_views), "lod-runs": (True, None, lod_views), "lod-cones": (False, eyes, lod_views),
             "lod-cone-runs": (True, eyes, lod_views), "runs": (True, None, None), "cones": (False, eyes, None), "plain-again": (False, None, None)}
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(old)
        vis.cull(0, views)
        vis.emit_instances(0, [0, 1])
        vis.set_command_layout(0, dtype=csup.WIDE)
        seen = {}
        for form, (runs, e, lods) in forms.items():
            vis.hiz_build(old)
            vis.cull_clusters(0, runs=runs, eyes=e, lods=lods)
            first = fetched_bytes(vis)
            vis.hiz_build(new)
            seen[form] = second_check(vis, [0, 1], sc.count, ids, views, lod_views, e, hiz1s, hiz2s, lods is not None)
            assert fetched_bytes(vis) == first  # the second phase writes none of the first
        assert seen["plain"][2] == seen["runs"][2] == seen["plain-again"][2]   # behind the older forms: their own bytes
        assert seen["lods"][2] == seen["lod-runs"][2] != seen["plain"][2] and seen["lod-cones"][2] == seen["lod-cone-runs"][2] != seen["cones"][2]
        counts, pending, _ = seen["lods"]
        assert int(counts[0]) > 0 and int(counts[1]) == 0 and int(pending[1]) == 0
        # the LOD-rejected clusters of the queried view are pending: more than the plain form leaves, and fewer commands come of them
        assert int(pending[0]) > int(seen["plain"][1][0]) and int(counts[0]) < int(seen["plain"][0][0])


# ---- 7. repeatability and the launch count ------------------------------------------------------------------------------------------

def test_two_calls_give_identical_bytes_and_the_launch_count_is_constant(oracle):
    got = {}
    for draws in (0, 257):
        sc, ids = ksup.world(draws)
        view = ksup.camera(use_hiz=1)
        lod_views = np.array([dsup.lod_view(scale=dsup.CAMERA_SCALE * 0.1)], dsup.CLUSTER_LOD_VIEW_DTYPE)
        with GpuVisibility(device=0) as vis:
            bind(vis, sc, ids)
            vis.hiz_build(ksup.wall_depth())
            vis.cull(0, [view])
            vis.emit_instances(0, [0])
            vis.set_command_layout(0, dtype=csup.GAPS)
            for runs in (False, True):
                for eyes in (None, np.array([dsup.nsup.POINT_EYE], np.float32)):
                    before = emit_launches(vis)
                    vis.cull_clusters(0, runs=runs, eyes=eyes, lods=lod_views)
                    got[draws, runs, eyes is not None] = emit_launches(vis) - before
                    one = fetched_bytes(vis)
                    vis.cull_clusters(0, runs=runs, eyes=eyes, lods=lod_views)
                    two = fetched_bytes(vis)
                    assert one == two and (draws == 0 or len(one[0]) > 0)
    assert got == {(d, r, e): 6 if r else 5 for d in (0, 257) for r in (False, True) for e in (False, True)}
