"""gv_pool_bind_cluster_cones / gv_pool_cull_cluster_cones on the device: the cluster cull with normal-cone backface rejection in its
conjunction. Which cluster passes the frustum and the pyramid is decided only by the oracle's gvo_is_behind_frustum /
gvo_hiz_occluded, called by cluster_twin.h over the FETCHED records and the oracle's pyramid; the cone test, the conjunction and the
second phase's pending set under it are restated in tests/cluster_cone_twin.h, the run rule in tests/cluster_runs_twin.h, the
placement in tests/clusters_support.py. Every comparison is exact: every command byte over a 0xA5 background, the bytes behind the
last written position included, and every count word. The case table, the designed cones and the designed draws are
cluster_cones_support's; tests/test_cluster_cones_census.py holds them to their conditions on the oracle and the twin alone."""
import numpy as np
import pytest

import cluster_cones_support as nsup
import clusters_second_support as ssup
import clusters_support as ksup
import commands_support as csup
import instances_support as isup
import lod_support as lsup
from garden_amd.lib import GV_DIRTY_MESH, GpuVisibility

pytestmark = pytest.mark.gpu

LAUNCHES = {False: 5, True: 6}  # of one gv_pool_cull_cluster_cones without / with GV_CLUSTERS_RUNS, whatever the data holds


def bind(vis, sc, ids, tables=None, pool_id=0):
    table, ranges, clusters, cones = nsup.geometry() if tables is None else tables
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()
    vis.bind_geometry(pool_id, ids, table)
    vis.bind_clusters(pool_id, ranges, clusters)
    vis.bind_cluster_cones(pool_id, cones)
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


def check(vis, listed, occupancy, ids_of, views, eyes, hizzes, runs=False, dtype=csup.INDEXED, frustum_only=False, region=0, held=None, own=True,
          draws=False, pool_id=0, tables=None):
    """Culls the clusters of the pool's last instance emission with the cone test — own: into caller-owned device memory over the
    background, cut after `held` positions when given — and compares every byte on the device and of a host fetch, and both kinds of
    counts, with the twin's. Returns (expected bytes, counts, tested, the census, the commands per view)."""
    import torch
    fetched = fetch_all(vis, pool_id, listed, occupancy)
    starts = instance_starts(vis, pool_id)
    bases = vis.draw_bases(pool_id) if draws else None
    draw_ids = [ids_of(v, f) for v, f in enumerate(fetched)]
    stride = dtype.itemsize
    used = [None if frustum_only else h for h in hizzes]
    per_view, counts, tested, census, _ = nsup.commands_of(fetched, starts, bases, draw_ids, views, eyes, used,
                                                           nsup.RUN_FORM if runs else nsup.PLAIN_FORM, tables=tables)
    rows = (len(listed) * region if region else int(counts.sum())) + 7  # (a few rows behind the last position must stay untouched)
    pattern = csup.background(rows, stride)
    exp = ksup.place(per_view, dtype, region, held, pattern)
    vis.set_command_layout(pool_id, dtype=dtype)
    before = emit_launches(vis)
    if own:
        dev = torch.full((rows, stride), csup.BACKGROUND, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # (torch's stream; the library's stream is non-blocking)
        vis.cull_clusters(pool_id, frustum_only, region, device=(dev.data_ptr(), rows * stride if held is None else held * stride + 5), runs=runs,
                          eyes=eyes)
        assert vis.cluster_commands_device(pool_id)[0] == dev.data_ptr()
    else:
        assert held is None
        vis.cull_clusters(pool_id, frustum_only, region, runs=runs, eyes=eyes)
    assert emit_launches(vis) - before == LAUNCHES[runs]
    host = pattern.copy()
    _, got_counts, got_tested = vis.cluster_commands(pool_id, out=host)  # waits for the call
    print("runs" if runs else "plain", "commands", got_counts.tolist(), "expected", counts.tolist(), "tested", got_tested.tolist(), "expected",
          tested.tolist(), census)
    assert got_counts.tolist() == counts.tolist()  # (the true counts, also when the target is too small or a region is cut)
    assert got_tested.tolist() == tested.tolist()  # (a cone-rejected cluster counts as tested)
    assert host.tobytes() == exp.tobytes()
    if own:
        assert dev.cpu().numpy().tobytes() == exp.tobytes()
    return exp, counts, tested, census, per_view


def fetched_bytes(vis, pool_id=0):
    return [np.asarray(x).copy().tobytes() for x in vis.cluster_commands(pool_id)]


# ---- 1. the case table ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", nsup.CASES, ids=[c.name for c in nsup.CASES])
def test_case_table_against_the_twin(case, oracle):
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    views = nsup.case_views(case)
    eyes = nsup.eyes_of(case)
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
        _, plain_counts, _, census, _ = check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes)   # caller-owned, packed
        check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, own=False)                          # library-owned
        _, run_counts, _, _, _ = check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, runs=True)
        check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, runs=True, own=False)
        if any(case.hiz):
            check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, frustum_only=True)
            check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, runs=True, frustum_only=True)
        if census["tested"] >= nsup.SHARE_FROM:
            assert census["cone_only"] >= 1 and int(run_counts.sum()) < int(plain_counts.sum())
        assert vis.draw_commands(0)[0].tobytes() == per_draw and vis.instances(0)[0].tobytes() == instances


# ---- 2. all-zero eyes: the bytes of the calls without the cone test ----------------------------------------------------------------

@pytest.mark.parametrize("name", ["draws-257", "views-8"])
def test_all_zero_eyes_give_the_bytes_of_the_calls_without_cones(name, oracle):
    case = nsup.CASE[name]
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    views = nsup.case_views(case)
    listed = list(range(len(views)))
    zero = np.zeros((len(views), 4), np.float32)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(ksup.wall_depth())
        vis.cull(0, views)
        vis.emit_instances(0, listed)
        vis.set_command_layout(0, dtype=csup.WIDE)
        got = {}
        for runs in (False, True):
            vis.cull_clusters(0, runs=runs)
            got[runs, "without"] = fetched_bytes(vis)
            vis.cull_clusters(0, runs=runs, eyes=zero)
            got[runs, "zero"] = fetched_bytes(vis)
            vis.cull_clusters(0, runs=runs, eyes=nsup.eyes_of(case))
            got[runs, "eyes"] = fetched_bytes(vis)
        for runs in (False, True):
            assert got[runs, "zero"] == got[runs, "without"] and len(got[runs, "zero"][0]) > 0
            assert got[runs, "eyes"][0] != got[runs, "without"][0] and got[runs, "eyes"][2] == got[runs, "without"][2]  # (as many tested)


# ---- 3. views and placement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("runs", [False, True], ids=["plain", "runs"])
@pytest.mark.parametrize("name", ["views-2", "views-8"])
def test_views_regions_and_a_cut_target(name, runs, oracle):
    case = nsup.CASE[name]
    sc, ids = ksup.world(case.draws)
    views = nsup.case_views(case)
    eyes = nsup.eyes_of(case)
    listed = list(range(len(views)))
    depth = ksup.wall_depth()
    hiz = oracle.Hiz(depth)
    hizzes = [hiz if h else None for h in case.hiz]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(depth)
        vis.cull(0, views)
        vis.emit_instances(0, listed)
        _, counts, _, _, _ = check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, runs=runs, dtype=csup.GAPS)
        starts = np.concatenate([[0], np.cumsum(counts)])
        low, high = int(counts.min()), int(counts.max())
        assert low > 20
        check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, runs=runs, region=low - 9)     # R below every C_v
        check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, runs=runs, region=high + 30)   # R above every C_v: zero padding
        check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, runs=runs, region=high + 30, own=False)
        check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, runs=runs, held=int(starts[1]) + int(counts[1]) // 2)  # a cut inside view 1
        check(vis, listed, sc.count, slot_ids(ids), views, eyes, hizzes, runs=runs, region=high + 30, held=high + 30 + 11)


# ---- 4. the designed cones and the designed draws -----------------------------------------------------------------------------------

def test_designed_cones_and_designed_draws(oracle):
    sc, ids, _ = nsup.design_scene()
    view = ksup.camera()
    rejected = sum(d[4] for d in nsup.DESIGNED)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.cull(0, [view])
        vis.emit_instances(0, [0])
        for runs in (False, True):
            eyes = nsup.design_eyes()["camera"].reshape(1, 4)
            _, counts, tested, census, per_view = check(vis, [0], sc.count, slot_ids(ids), [view], eyes, [None], runs=runs, dtype=csup.WIDE)
            assert int(tested[0]) == 3 * len(nsup.DESIGNED) and census["frustum_kept"] == census["tested"]
            assert census["cone_rejected"] == rejected  # the identity draw alone; the mirrored and the flat draw keep every cluster
            if not runs:
                assert int(counts[0]) == 3 * len(nsup.DESIGNED) - rejected
                per_draw = np.bincount(per_view[0]["draw"], minlength=sc.count)
                assert sorted(per_draw[per_draw > 0].tolist()) == [len(nsup.DESIGNED) - rejected, len(nsup.DESIGNED), len(nsup.DESIGNED)]
            at_apex = nsup.design_eyes()["at-apex"].reshape(1, 4)
            _, _, _, census, _ = check(vis, [0], sc.count, slot_ids(ids), [view], at_apex, [None], runs=runs, dtype=csup.WIDE)
            assert census["tested"] == 3 * len(nsup.DESIGNED)


# ---- 5. where the ids and the instance ranges come from ------------------------------------------------------------------------------

def test_ids_from_a_lod_selection(oracle, tmp_path):
    sc, ids = ksup.world(257, ids_mode="lod")
    view = ksup.camera()
    eyes = np.array([nsup.POINT_EYE], np.float32)
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
            _, _, tested, census, _ = check(vis, [0], sc.count, lambda v, f: selected[v], [view], eyes, [None], runs=runs)
            assert int(tested[0]) == int((level_counts[0][:3] * np.array([64, 8, 1])).sum()) and census["cone_rejected"] > 0


def test_after_a_draw_emission_with_counts_0_1_and_3(oracle):
    sc, ids = ksup.world(257)
    view = ksup.camera()
    eyes = np.array([nsup.direction_eye(0.0)], np.float32)
    ready = (np.arange(sc.count, dtype=np.uint32) % 3) * np.uint32(3) // np.uint32(2)  # 0, 1, 3 in turn
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        column = np.ones(sc.count, np.uint32)
        vis.bind_ready(0, column)
        vis.cull(0, [view])
        column[:] = ready  # changed and marked after the cull, so that every box stays a draw
        vis.mark_dirty(GV_DIRTY_MESH, 0, sc.count, pool_id=0)
        vis.emit_draw_instances(0, [0])
        for runs in (False, True):
            exp, counts, _, _, _ = check(vis, [0], sc.count, slot_ids(ids), [view], eyes, [None], runs=runs, dtype=csup.GAPS, draws=True)
            got = exp[:int(counts[0])].reshape(-1).view(csup.GAPS)
            assert set(got["instance_count"].tolist()) == {1, 3}


# ---- 6. the second phase -------------------------------------------------------------------------------------------------------------

def second_check(vis, listed, occupancy, ids, views, eyes, hiz1s, hiz2s, cones):
    """the second phase behind the pool's cluster result against the twin: with the cone conjunction (cones) or the rule as it was"""
    fetched = fetch_all(vis, 0, listed, occupancy)
    starts = instance_starts(vis, 0)
    draw_ids = [slot_ids(ids)(v, f) for v, f in enumerate(fetched)]
    if cones:
        per_view, counts, pending, census, _ = nsup.commands_of(fetched, starts, None, draw_ids, views, eyes, hiz1s, nsup.SECOND_PHASE, hiz2s)
    else:
        table, ranges, clusters, _ = nsup.geometry()
        per_view, counts, pending, census = ssup.second_commands_of(fetched, starts, None, draw_ids, views, hiz1s, hiz2s, (table, ranges, clusters))
    stride = csup.WIDE.itemsize
    rows = int(counts.sum()) + 7
    pattern = csup.background(rows, stride)
    exp = ksup.place(per_view, csup.WIDE, 0, None, pattern)
    before = emit_launches(vis)
    vis.cull_clusters_second_phase(0)
    assert emit_launches(vis) - before == 5
    host = pattern.copy()
    _, got_counts, got_pending = vis.cluster_second_commands(0, out=host)
    print("second phase", "cones" if cones else "plain", got_counts.tolist(), counts.tolist(), "pending", got_pending.tolist(), pending.tolist(), census)
    assert got_counts.tolist() == counts.tolist() and got_pending.tolist() == pending.tolist()
    assert host.tobytes() == exp.tobytes()
    return counts, pending, census, host.tobytes()


def test_the_second_phase_behind_a_cone_result_and_behind_a_plain_one(oracle):
    sc, ids = ksup.world(257)
    views = [ksup.camera(0.0, use_hiz=1), ksup.camera(0.4, use_hiz=0, shadow_pass=1)]
    eyes = np.array([nsup.POINT_EYE, nsup.direction_eye(0.4)], np.float32)
    old, new = ksup.wall_depth(x0=0.0), ksup.wall_depth(x0=0.7)
    hiz1, hiz2 = oracle.Hiz(old), oracle.Hiz(new)
    hiz1s, hiz2s = [hiz1, None], [hiz2, None]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(old)
        vis.cull(0, views)
        vis.emit_instances(0, [0, 1])
        vis.set_command_layout(0, dtype=csup.WIDE)
        seen = {}
        for form in ("plain", "cones", "cone-runs", "runs", "plain-again"):
            vis.hiz_build(old)
            vis.cull_clusters(0, runs=form in ("cone-runs", "runs"), eyes=eyes if form in ("cones", "cone-runs") else None)
            first = fetched_bytes(vis)
            vis.hiz_build(new)
            cones = form in ("cones", "cone-runs")
            counts, pending, census, second = second_check(vis, [0, 1], sc.count, ids, views, eyes, hiz1s, hiz2s, cones)
            assert fetched_bytes(vis) == first  # the second phase writes none of the first
            seen[form] = (counts, pending, census, second)
        assert seen["plain"][3] == seen["runs"][3] == seen["plain-again"][3]   # behind a plain or a run result: today's bytes
        assert seen["cones"][3] == seen["cone-runs"][3] != seen["plain"][3]
        counts, pending, census, _ = seen["cones"]
        assert int(counts[0]) > 0 and int(counts[1]) == 0 and int(pending[1]) == 0
        # the cone-rejected clusters of the queried view are pending: tested - survivors of the conjunction, more than the plain form leaves
        assert int(pending[0]) > int(seen["plain"][1][0]) and int(counts[0]) < int(seen["plain"][0][0])


# ---- 7. repeatability and the launch count ------------------------------------------------------------------------------------------

def test_two_calls_give_identical_bytes_and_the_launch_count_is_constant(oracle):
    got = {}
    for draws in (0, 257):
        sc, ids = ksup.world(draws)
        view = ksup.camera(use_hiz=1)
        eyes = np.array([nsup.POINT_EYE], np.float32)
        with GpuVisibility(device=0) as vis:
            bind(vis, sc, ids)
            vis.hiz_build(ksup.wall_depth())
            vis.cull(0, [view])
            vis.emit_instances(0, [0])
            vis.set_command_layout(0, dtype=csup.GAPS)
            for runs in (False, True):
                before = emit_launches(vis)
                vis.cull_clusters(0, runs=runs, eyes=eyes)
                got[draws, runs] = emit_launches(vis) - before
                one = fetched_bytes(vis)
                vis.cull_clusters(0, runs=runs, eyes=eyes)
                two = fetched_bytes(vis)
                assert one == two and (draws == 0 or len(one[0]) > 0)
    assert got == {(0, False): 5, (0, True): 6, (257, False): 5, (257, True): 6}


# ---- 8. the shim --------------------------------------------------------------------------------------------------------------------

def test_cluster_cones_shim_five_ticks_against_the_twin():
    """tests/cpp/cluster_cones.cpp: main pass + one cascade, a moving camera, GpuClusterCommands::setCones on; every command equals a
    host path that fetches the records, calls the oracle and applies the twin's cone rule"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "build", "cluster_cones")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "tests", "cpp"), "-f", "cluster_cones.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    result = json.loads(run.stdout.splitlines()[-1])
    print(result)
    assert result["ok"] and result["ticks"] == 5 and result["passes"] == 2
    assert result["tested"] > result["base_kept"] > result["survivors"] > 0  # clusters were culled, and the cone rejected more
    assert 10 * result["cone_rejected"] >= result["tested"] and result["point_rejected"] > 0 and result["direction_rejected"] > 0
