"""gv_pool_cull_clusters_second_phase on the device: the clusters the pool's cluster cull K1 tested and did not keep, in the views for
which it queried a pyramid, tested again against the pyramid as it stands now. Expected values come only from the oracle's
gvo_is_behind_frustum / gvo_hiz_occluded, called by the C twins (tests/cluster_second_twin.h over tests/cluster_twin.h) over the
FETCHED records and the pyramids the oracle builds from the same depth images; the placement is clusters_support.place. Every
comparison is exact: every command byte over a 0xA5 background, every count word, and K1's commands and counts, the per-draw commands
and the instance data byte for byte before and after. The case table is clusters_second_support.CASES, held to its conditions on the
oracle alone by tests/test_clusters_second_census.py."""
import numpy as np
import pytest

import clusters_second_support as ssup
import clusters_support as ksup
import commands_support as csup
import instances_support as isup
import lod_support as lsup
from garden_amd.lib import GV_DIRTY_GEOMETRY, GV_DIRTY_MESH, GpuVisibility

pytestmark = pytest.mark.gpu

LAUNCHES = 5  # of one gv_pool_cull_clusters_second_phase, whatever the data holds (include/garden_vis.h)


def bind(vis, sc, ids, tables=None, pool_id=0):
    table, _, ranges, clusters = ksup.geometry()
    if tables is not None:
        table, ranges, clusters = tables
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


class Frame:
    """What the twins need of the emission K1 was made behind: fetched once, before K1, since the second phase takes everything as
    K1 used it."""

    def __init__(self, vis, listed, occupancy, ids_of, views, draws=False, tables=None, pool_id=0):
        self.vis, self.pool_id, self.views, self.tables = vis, pool_id, views, tables
        self.fetched = fetch_all(vis, pool_id, listed, occupancy)
        self.starts = instance_starts(vis, pool_id)
        self.bases = vis.draw_bases(pool_id) if draws else None
        self.draw_ids = [ids_of(v, f) for v, f in enumerate(self.fetched)]

    def first_phase(self, hiz1s):
        """K1's commands per view by the twin (hiz1s[v] None: frustum only)"""
        extra = {} if self.tables is None else dict(table=self.tables[0], ranges=self.tables[1], clusters=self.tables[2])
        out = []
        for v, (f, first) in enumerate(zip(self.fetched, ksup.firsts(self.fetched, self.starts, self.bases))):
            n = int(f["draw_count"])
            out.append(ksup.view_commands(np.asarray(f["baked_model"]).reshape(-1, 12)[:n], self.draw_ids[v], first, self.views[v]["view_proj"],
                                          hiz1s[v], **extra)[0])
        return out

    def second_phase(self, hiz1s, hiz2s):
        return ssup.second_commands_of(self.fetched, self.starts, self.bases, self.draw_ids, self.views, hiz1s, hiz2s, self.tables)


def first_phase(frame, hiz1s, dtype=csup.INDEXED, frustum_only=False):
    """K1 into the library's buffer, held to the twin; returns (its bytes, counts, tested) as fetched"""
    vis, pool_id = frame.vis, frame.pool_id
    vis.set_command_layout(pool_id, dtype=dtype)
    vis.cull_clusters(pool_id, frustum_only)
    got, counts, tested = vis.cluster_commands(pool_id)
    exp = frame.first_phase([None if frustum_only else h for h in hiz1s])
    assert counts.tolist() == [len(c) for c in exp]
    return got.tobytes(), counts.tolist(), tested.tolist()


def check(frame, hiz1s, hiz2s, dtype=csup.INDEXED, region=0, held=None, own=True):
    """The second phase of the pool's cluster cull — own: into caller-owned device memory over the background, cut after `held`
    positions when given — compared byte for byte, on the device and through the fetch, and count for count with the twin's; K1's
    result is fetched before and after and must not change. hiz1s[v] None: K1 did not query for view v. Returns (expected bytes,
    counts, pending, the twin's stats)."""
    import torch
    vis, pool_id = frame.vis, frame.pool_id
    stride = dtype.itemsize
    per_view, counts, pending, stats = frame.second_phase(hiz1s, hiz2s)
    rows = (len(per_view) * region if region else int(counts.sum())) + 7  # (a few rows behind the last position must stay untouched)
    pattern = csup.background(rows, stride)
    exp = ksup.place(per_view, dtype, region, held, pattern)
    k1 = [x.tobytes() for x in vis.cluster_commands(pool_id)]
    before = emit_launches(vis)
    if own:
        dev = torch.full((rows, stride), csup.BACKGROUND, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # (torch's stream; the library's stream is non-blocking)
        vis.cull_clusters_second_phase(pool_id, region, target=(dev.data_ptr(), rows * stride if held is None else held * stride + 5))
        assert vis.cluster_second_commands_device(pool_id)[0] == dev.data_ptr()
    else:
        assert held is None
        vis.cull_clusters_second_phase(pool_id, region)
    assert emit_launches(vis) - before == LAUNCHES
    host = pattern.copy()
    _, got_counts, got_pending = vis.cluster_second_commands(pool_id, out=host)  # waits for the call
    print("commands", got_counts.tolist(), "expected", counts.tolist(), "pending", got_pending.tolist(), "expected", pending.tolist())
    assert got_counts.tolist() == counts.tolist()  # (the true counts, also when the target is too small or a region is cut)
    assert got_pending.tolist() == pending.tolist()
    assert host.tobytes() == exp.tobytes()
    if own:
        assert dev.cpu().numpy().tobytes() == exp.tobytes()
    assert [x.tobytes() for x in vis.cluster_commands(pool_id)] == k1  # K1's commands, counts and tested counts
    return exp, counts, pending, stats


def hizzes(oracle, name, query, rg16f=False):
    hiz = oracle.Hiz(ssup.image(name), rg16f=rg16f)
    return [hiz if q else None for q in query]


def rows_of(commands):
    return {bytes(c.tobytes()) for c in commands}


# ---- 1. the case table -----------------------------------------------------------------------------------------------------------

_RESULTS = {}


def run_case(case, oracle):
    """One case end to end (once per session): cull under image 0, emission, per-draw commands, K1 under image 1, the second phase
    under image 2 into a caller-owned and a library-owned target and a second time. Returns what the cover property needs."""
    if case.name in _RESULTS:
        return _RESULTS[case.name]
    sc, ids, tables = ssup.case_world(case)
    views = ssup.case_views(case)
    listed = list(range(len(views)))
    hiz1s, hiz2s = hizzes(oracle, case.images[1], case.hiz), hizzes(oracle, case.images[2], case.hiz)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids, tables)
        vis.hiz_build(ssup.image(case.images[0]))
        vis.cull(0, views)
        vis.emit_instances(0, listed)
        vis.set_command_layout(0, dtype=csup.INDEXED)
        vis.emit_draw_commands(0)
        per_draw = vis.draw_commands(0)[0].tobytes()
        instances = vis.instances(0)[0].tobytes()
        frame = Frame(vis, listed, sc.count, slot_ids(ids), views, tables=tables)
        vis.hiz_build(ssup.image(case.images[1]))
        first_phase(frame, hiz1s)
        # against the pyramid K1 itself queried: zero commands in every view
        _, counts, _, _ = check(frame, hiz1s, hiz1s)
        assert not counts.any()
        vis.hiz_build(ssup.image(case.images[2]))
        exp, counts, pending, stats = check(frame, hiz1s, hiz2s)                 # caller-owned, packed
        again, _, _, _ = check(frame, hiz1s, hiz2s, own=False)                    # library-owned; and a second call: identical bytes
        assert again[:int(counts.sum())].tobytes() == exp[:int(counts.sum())].tobytes()
        assert vis.draw_commands(0)[0].tobytes() == per_draw and vis.instances(0)[0].tobytes() == instances
        if case.pending is not None:
            assert int(pending.sum()) == case.pending
        if case.kept is not None:
            assert int(counts.sum()) == case.kept
        # for the cover property: what the device wrote in both phases, and what the twin keeps under hiz2 alone
        k1_rows = vis.cluster_commands(0, dtype=csup.INDEXED)
        second_rows = vis.cluster_second_commands(0, dtype=csup.INDEXED)
        alone = frame.first_phase(hiz2s)
    _RESULTS[case.name] = dict(k1=k1_rows, second=second_rows, alone=alone, fetched=frame.fetched, ids=ids, stats=stats)
    return _RESULTS[case.name]


@pytest.mark.parametrize("case", ssup.CASES, ids=[c.name for c in ssup.CASES])
def test_case_table_against_the_oracle(case, oracle):
    run_case(case, oracle)


@pytest.mark.parametrize("case", ssup.CASES, ids=[c.name for c in ssup.CASES])
def test_cover_what_the_new_pyramid_alone_keeps_is_drawn_in_one_of_the_two_phases(case, oracle):
    """the set of (view, draw, cluster) the twin keeps under hiz2 alone is a subset of the phase-1 commands ∪ the phase-2 commands
    the DEVICE wrote (a command row names its draw and its cluster's index range)"""
    r = run_case(case, oracle)
    (k1, k1_counts, _), (second, second_counts, _) = r["k1"], r["second"]
    at1 = at2 = 0
    for v, alone in enumerate(r["alone"]):
        drawn = rows_of(k1[at1:at1 + int(k1_counts[v])]) | rows_of(second[at2:at2 + int(second_counts[v])])
        at1, at2 = at1 + int(k1_counts[v]), at2 + int(second_counts[v])
        laid = np.zeros(len(alone), csup.INDEXED)  # the twin's commands in the layout the device wrote (first_instance names the draw)
        for field in csup.INDEXED.names:
            laid[field] = alone[field]
        want = rows_of(laid)
        assert want <= drawn, (case.name, v, len(want - drawn))


def test_the_bad_boxes_are_among_the_pending_clusters(oracle):
    """the NaN and the inverted box of geometry 5 belong to draws of the largest case (whose bytes the case table compares); K1 keeps
    neither, so both are pending in a queried view"""
    r = run_case(ssup.CASE["draws-257"], oracle)
    f = r["fetched"][0]
    assert np.count_nonzero(r["ids"][f["visible_idx"][:int(f["draw_count"])]] == ksup.BAD_GEOMETRY) >= 1


def test_the_launch_count_is_the_same_for_the_empty_and_the_largest_case(oracle):
    """(check() holds every call to LAUNCHES; here: both cases ran)"""
    run_case(ssup.CASE["pending-0"], oracle)
    run_case(ssup.CASE["draws-257"], oracle)


# ---- 2. placement ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["views-2", "views-8"])
def test_regions_below_and_above_the_counts_and_a_cut_target(name, oracle):
    case = ssup.CASE[name]
    sc, ids, _ = ssup.case_world(case)
    views = ssup.case_views(case)
    listed = list(range(len(views)))
    hiz1s, hiz2s = hizzes(oracle, case.images[1], case.hiz), hizzes(oracle, case.images[2], case.hiz)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(ssup.image(case.images[0]))
        vis.cull(0, views)
        vis.emit_instances(0, listed)
        frame = Frame(vis, listed, sc.count, slot_ids(ids), views)
        vis.hiz_build(ssup.image(case.images[1]))
        first_phase(frame, hiz1s, dtype=csup.GAPS)
        vis.hiz_build(ssup.image(case.images[2]))
        _, counts, _, _ = check(frame, hiz1s, hiz2s, dtype=csup.GAPS)
        queried = counts[np.array(case.hiz)]
        low, high = int(queried.min()), int(queried.max())
        assert low > 200 and not counts[~np.array(case.hiz)].any()
        check(frame, hiz1s, hiz2s, dtype=csup.GAPS, region=low - 129)        # R below every queried C_v: commands beyond R are not written
        check(frame, hiz1s, hiz2s, dtype=csup.GAPS, region=high + 300)       # R above every C_v: zero padding, whole regions for the others
        check(frame, hiz1s, hiz2s, dtype=csup.GAPS, region=high + 300, own=False)
        cut = int(counts[:len(counts) - 1].sum()) + 77 if case.hiz[-1] else int(counts[0]) - 77
        check(frame, hiz1s, hiz2s, dtype=csup.GAPS, held=cut)                # a cut inside a view: true counts, 0xA5 beyond
        check(frame, hiz1s, hiz2s, dtype=csup.GAPS, region=high + 300, held=high + 300 + 11)


# ---- 3. what K1 was made with ----------------------------------------------------------------------------------------------------

def stand_up(vis, sc, ids, views, image0, listed=None, draws=False):
    bind(vis, sc, ids)
    vis.hiz_build(ssup.image(image0))
    vis.cull(0, views)
    (vis.emit_draw_instances if draws else vis.emit_instances)(0, list(range(len(views))) if listed is None else listed)


def test_after_a_frustum_only_cluster_cull_nothing_is_pending(oracle):
    sc, ids = ksup.world(64)
    view = ksup.camera(use_hiz=1)
    with GpuVisibility(device=0) as vis:
        stand_up(vis, sc, ids, [view], "far")
        frame = Frame(vis, [0], sc.count, slot_ids(ids), [view])
        vis.hiz_build(ssup.image("close"))
        first_phase(frame, [None], frustum_only=True)
        vis.hiz_build(ssup.image("wall"))
        _, counts, pending, _ = check(frame, [None], [None])
        assert counts.tolist() == [0] and pending.tolist() == [0]


@pytest.mark.parametrize("rg16f", [False, True], ids=["fp32", "rg16f"])
def test_a_view_that_names_another_pyramid_slot(rg16f, oracle):
    """pyramid slot 3 holds the walls, slot 0 stays empty: the view names 1 + 3; with GV_CONFIG_HIZ_RG16F the levels are half pairs"""
    sc, ids = ksup.world(257)
    view = ksup.camera(use_hiz=4)
    hiz1s, hiz2s = hizzes(oracle, "wide", [True], rg16f), hizzes(oracle, "narrow", [True], rg16f)
    with GpuVisibility(device=0, hiz_rg16f=rg16f) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(ssup.image("far"))
        vis.hiz_select(3)
        vis.hiz_build(ssup.image("wall"))
        vis.hiz_select(0)
        vis.cull(0, [view])
        vis.emit_instances(0, [0])
        frame = Frame(vis, [0], sc.count, slot_ids(ids), [view])
        vis.hiz_select(3)
        vis.hiz_build(ssup.image("wide"))
        vis.hiz_select(0)
        first_phase(frame, hiz1s)
        vis.hiz_select(3)
        vis.hiz_build(ssup.image("narrow"))
        vis.hiz_select(0)  # (the selected pyramid is slot 0 when the call is issued: the view's own slot is read)
        _, counts, pending, _ = check(frame, hiz1s, hiz2s)
        assert 0 < int(counts[0]) < int(pending[0])


def test_ids_from_a_lod_selection_that_is_dropped_before_the_second_phase(oracle, tmp_path):
    """g_k is the id K1 kept: the selection K1 read is dropped, and the second phase still writes the selected levels' clusters"""
    sc, ids = ksup.world(257, ids_mode="lod")
    view = ksup.camera(use_hiz=1)
    switch_at = lsup.quantile_thresholds(sc.transforms["position"], np.ones(sc.count, np.float32), ksup.LOD_LEVELS)
    lod = lsup.lod_table([(1, [])] * ksup.LOD_BASE + [(ksup.LOD_LEVELS, switch_at)])
    twin = lsup.build_twin(tmp_path)
    hiz1s, hiz2s = hizzes(oracle, "close", [True]), hizzes(oracle, "wall", [True])
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.bind_lod(0, None, lod)
        vis.hiz_build(ssup.image("far"))
        vis.cull(0, [view])
        vis.emit_instances(0, [0])
        fetched = fetch_all(vis, 0, [0], sc.count)
        selected, level_counts = lsup.select_expected(twin, fetched, [1.0], ids, None, lod)
        assert np.count_nonzero(level_counts[0]) == ksup.LOD_LEVELS  # every level holds draws
        vis.select_lods(0, [1.0])
        frame = Frame(vis, [0], sc.count, lambda v, f: selected[v], [view])
        vis.hiz_build(ssup.image("close"))
        first_phase(frame, hiz1s)
        vis.select_lods(0, None)  # dropped: a command emission would go back to the id mirror (every id LOD_BASE)
        vis.hiz_build(ssup.image("wall"))
        _, counts, pending, _ = check(frame, hiz1s, hiz2s)
        assert 0 < int(counts[0]) < int(pending[0])
        base_only = Frame(vis, [0], sc.count, slot_ids(ids), [view]).second_phase(hiz1s, hiz2s)
        assert base_only[1].tolist() != counts.tolist()  # (the unselected ids would have given other commands)


def test_an_id_mark_between_the_cluster_cull_and_the_second_phase_has_no_effect(oracle):
    sc, ids = ksup.world(255)
    ids = ids.copy()
    view = ksup.camera(use_hiz=1)
    hiz1s, hiz2s = hizzes(oracle, "close", [True]), hizzes(oracle, "wall", [True])
    with GpuVisibility(device=0) as vis:
        stand_up(vis, sc, ids, [view], "far")
        frame = Frame(vis, [0], sc.count, slot_ids(ids.copy()), [view])
        vis.hiz_build(ssup.image("close"))
        first_phase(frame, hiz1s)
        vis.hiz_build(ssup.image("wall"))
        exp, counts, _, _ = check(frame, hiz1s, hiz2s)
        ids[:] = (ids + 3) % (ksup.TABLE_COUNT + 1)  # every slot another geometry
        vis.mark_dirty(GV_DIRTY_GEOMETRY, 0, sc.count, pool_id=0)
        after, _, _, _ = check(frame, hiz1s, hiz2s)
        assert after.tobytes() == exp.tobytes() and int(counts[0]) > 0


def test_after_a_draw_emission_with_counts_0_1_and_3(oracle):
    sc, ids = ksup.world(257)
    view = ksup.camera(use_hiz=1)
    ready = (np.arange(sc.count, dtype=np.uint32) % 3) * np.uint32(3) // np.uint32(2)  # 0, 1, 3 in turn
    hiz1s, hiz2s = hizzes(oracle, "close", [True]), hizzes(oracle, "wall", [True])
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        column = np.ones(sc.count, np.uint32)
        vis.bind_ready(0, column)
        vis.hiz_build(ssup.image("far"))
        vis.cull(0, [view])
        column[:] = ready  # changed and marked after the cull, so that every box stays a draw
        vis.mark_dirty(GV_DIRTY_MESH, 0, sc.count, pool_id=0)
        vis.emit_draw_instances(0, [0])
        frame = Frame(vis, [0], sc.count, slot_ids(ids), [view], draws=True)
        vis.hiz_build(ssup.image("close"))
        first_phase(frame, hiz1s, dtype=csup.GAPS)
        vis.hiz_build(ssup.image("wall"))
        exp, counts, _, _ = check(frame, hiz1s, hiz2s, dtype=csup.GAPS)
        n = int(frame.fetched[0]["draw_count"])
        got = exp[:int(counts[0])].reshape(-1).view(csup.GAPS)
        per_draw = ready[frame.fetched[0]["visible_idx"][:n]]
        assert len(got) > 0 and set(got["instance_count"].tolist()) <= {1, 3} and got["instance_count"].tolist() == per_draw[got["draw"]].tolist()
        assert not np.isin(got["draw"], np.nonzero(per_draw == 0)[0]).any()  # a draw without an instance is void: never pending


def test_a_sorted_and_a_grouped_view(oracle):
    """view 0 after gv_pool_sort, view 1 after gv_pool_group_draws: draw k is record k of the order delivered"""
    sc, ids = ksup.world(64)
    views = [ksup.camera(0.0, use_hiz=1), ksup.camera(0.4, use_hiz=1, shadow_pass=1)]
    hiz1s, hiz2s = hizzes(oracle, "close", [True, True]), hizzes(oracle, "wall", [True, True])
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, ids)
        vis.hiz_build(ssup.image("far"))
        vis.cull(0, views)
        unsorted = fetch_all(vis, 0, [0, 1], sc.count)
        vis.sort(0, descending=False, pool_id=0)
        vis.group_draws(1, pool_id=0)
        vis.emit_instances(0, [0, 1])
        frame = Frame(vis, [0, 1], sc.count, slot_ids(ids), views)
        for before, after in zip(unsorted, frame.fetched):
            n = int(after["draw_count"])
            assert n > 2 and before["visible_idx"][:n].tolist() != after["visible_idx"][:n].tolist()
        vis.hiz_build(ssup.image("close"))
        first_phase(frame, hiz1s)
        vis.hiz_build(ssup.image("wall"))
        _, counts, _, _ = check(frame, hiz1s, hiz2s)
        assert counts.all()


# ---- 4. the shim -----------------------------------------------------------------------------------------------------------------

def test_cluster_second_shim_five_ticks_against_the_oracle():
    """tests/cpp/cluster_second.cpp: five ticks with a moving camera, each phase 1, a rebuilt pyramid, the cluster second phase, then
    the draw-level second phase with its own emission and cluster cull; every buffer equals a host path over the oracle"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "build", "cluster_second")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "tests", "cpp"), "-f", "cluster_second.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    result = json.loads(run.stdout.splitlines()[-1])
    print(result)
    assert result["ok"] and result["ticks"] == 5
    assert result["pending"] > result["second"] > 0 and result["first"] > 0 and result["late_draws"] > 0 and result["late_commands"] > 0
