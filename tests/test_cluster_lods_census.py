"""The case table, the DAG fixture and the designed entries, draws and views of tests/test_gpu_cluster_lods.py on the ORACLE AND THE
TWIN ALONE (no GPU, no product code): every case must put the LOD cut of gv_pool_cull_cluster_lods to work, so that a kernel which
ignores an entry, a view or the order of the conjunction cannot pass it. The records are the oracle's own cull of the case's world;
which cluster passes the frustum and the pyramid is decided by the twin's calls of gvo_is_behind_frustum / gvo_hiz_occluded
(cluster_twin.h); the cone test by tests/cluster_cone_twin.h; the cut by tests/cluster_lod_twin.h. These are conditions that keep the
GPU test from being vacuous, not measurements:
  - every case that tests at least SHARE_FROM clusters: the LOD-kept share lies between 1/20 and 1/2 of the tested clusters, and at
    least three DAG levels each hold >= 5 % of the kept clusters;
  - in every tested draw of a DAG geometry, of every case and of the designed scene, every leaf is covered by exactly one LOD-kept
    cluster;
  - somewhere in the table there is a cluster LOD keeps and the frustum rejects, one LOD keeps and the pyramid rejects, one LOD keeps
    and the cone rejects, a draw whose cut is only leaves, a draw whose cut is only the root, and a cluster on which the point eye and
    the parallel eye disagree;
  - behind a LOD result the second phase's pending set is strictly larger than behind the plain form on the same state;
  - every designed entry and every designed draw lands on the side it was designed for.
As built (the figures this file prints): see AS_BUILT below."""
import functools

import numpy as np
import pytest

import cluster_lods_support as dsup
import clusters_second_support as ssup
import clusters_support as ksup

# name -> (tested, LOD-kept, levels that hold >= 5 % of the kept clusters) as the fixture stands; the test holds the table to them, so
# that a change of the fixture shows
AS_BUILT = {
    'draws-0': (0, 0, []),
    'draws-1-of-1': (1, 1, [0]),
    'draws-1-of-3': (3, 1, [1]),
    'draws-1-of-63': (63, 21, [0, 1]),
    'draws-1-of-64': (64, 3, [4]),
    'draws-1-of-65': (65, 10, [2]),
    'draws-1-of-127': (127, 38, [0, 1, 2]),
    'draws-2': (192, 42, [0, 1, 2]),
    'draws-256': (23633, 3426, [0, 1, 2, 3]),
    'draws-257': (19339, 2858, [0, 1, 2, 3]),
    'tile-minus-1': (255, 67, [0, 1, 2]),
    'tile': (256, 54, [0, 1, 2, 3]),
    'tile-plus-1': (257, 65, [0, 1, 2]),
    'two-tiles-plus-1': (513, 99, [0, 1, 2]),
    'views-2': (11186, 1087, [0, 1, 2, 3, 4]),
    'views-8': (26467, 8367, [0, 1, 2, 3, 4]),
    'views-8-eyes': (26467, 8699, [0, 1, 2, 3]),
}


@functools.lru_cache(maxsize=None)
def case_census(oracle, case):
    """(the census summed over the views, the verdicts per view, draws of view 0)"""
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    hiz = oracle.Hiz(ksup.wall_depth())
    lod_views, eyes = dsup.lod_views_of(case), dsup.eyes_of(case)
    total = dict.fromkeys(dsup.CENSUS_FIELDS, 0)
    verdicts, draws = [], 0
    for v, (view, query) in enumerate(zip(dsup.case_views(case), case.hiz)):
        got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view, hiz=hiz if query else None)
        n = int(got["draw_count"])
        g = ids[got["visible_idx"][:n]].astype(np.uint32)
        _, _, one, verdict, at = dsup.view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], lod_views[v],
                                                    None if eyes is None else eyes[v], hiz if query else None)
        for name in dsup.CENSUS_FIELDS:
            total[name] += one[name]
        verdicts.append((verdict, at, g))
        if v == 0:
            draws = n
    return total, verdicts, draws


def level_shares(levels):
    kept = sum(levels.values())
    return {level: count / kept for level, count in sorted(levels.items())} if kept else {}


@pytest.mark.parametrize("case", dsup.CASES, ids=[c.name for c in dsup.CASES])
def test_every_case_puts_the_cut_to_work(case, oracle):
    census, verdicts, draws = case_census(oracle, case)
    levels, _, only_leaves, only_root = dsup.cut_statistics(verdicts)
    uncovered = dsup.cut_statistics([one for one, kind in zip(verdicts, case.lods) if kind != "Z"])[1]  # (scale 0 keeps every cluster)
    shares = level_shares(levels)
    print(case.name, "draws", draws, census, "kept per level", levels, "only leaves", only_leaves, "only the root", only_root)
    assert draws == case.draws if not case.hiz[0] else 0 < draws <= case.draws  # (the wall hides whole entities from a view that queries)
    big = sorted(level for level, share in shares.items() if level >= 0 and share >= 0.05)
    assert AS_BUILT[case.name] == (census["tested"], census["lod_kept"], big)
    assert uncovered == 0  # the cover property: every leaf of every tested DAG draw under exactly one kept cluster
    if case.draws == 0:
        assert census["tested"] == 0
        return
    assert census["tested"] > 0 and census["lod_kept"] > 0
    if census["tested"] < dsup.SHARE_FROM:
        return
    assert 20 * census["lod_kept"] >= census["tested"] and 2 * census["lod_kept"] <= census["tested"], census
    assert sum(1 for level, share in shares.items() if level >= 0 and share >= 0.05) >= 3, shares
    assert census["survivors"] < census["lod_kept"]  # the unchanged test has work left on the cut


def test_the_table_holds_one_of_each(oracle):
    total = dict.fromkeys(dsup.CENSUS_FIELDS, 0)
    only_leaves = only_root = 0
    for case in dsup.CASES:
        census, verdicts, _ = case_census(oracle, case)
        for name in dsup.CENSUS_FIELDS:
            total[name] += census[name]
        _, _, leaves, root = dsup.cut_statistics(verdicts)
        only_leaves += leaves
        only_root += root
    print(total, "draws whose cut is only leaves", only_leaves, "only the root", only_root)
    assert total["lod_frustum"] >= 1 and total["lod_hiz"] >= 1 and total["lod_cone"] >= 1 and total["eyes_disagree"] >= 1
    assert only_leaves >= 1 and only_root >= 1


def design_verdicts(oracle, view_name):
    sc, ids, _, _ = dsup.design_scene()
    view = ksup.camera()
    got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view)
    n = int(got["draw_count"])
    slots = got["visible_idx"][:n].astype(np.int64)
    g = ids[slots].astype(np.uint32)
    _, _, census, verdict, at = dsup.view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], dsup.design_views()[view_name], None, None)
    return slots, g, verdict, at, census


def kept_of(slots, verdict, at, slot):
    k = int(np.flatnonzero(slots == slot)[0])
    return [bool(b & dsup.KEPT) for b in verdict[int(at[k]):int(at[k + 1])]]


def test_designed_entries_draws_and_views_land_where_designed(oracle):
    sc, _, _, _ = dsup.design_scene()
    slots, g, verdict, at, census = design_verdicts(oracle, "camera")
    assert len(slots) == sc.count  # every designed draw is delivered: the far ones and the zero-scale ones too
    point = kept_of(slots, verdict, at, dsup.DESIGN_IDENTITY)
    assert point == [d[3] for d in dsup.DESIGNED], list(zip(dsup.DESIGNED_NAMES, point))
    assert kept_of(slots, verdict, at, dsup.DESIGN_MIRRORED) == point  # scale -1 on one axis: s2 = 1, the same decisions
    assert not any(kept_of(slots, verdict, at, dsup.DESIGN_ZERO))       # s2 = 0: nothing exceeds, the roots included
    assert not any(kept_of(slots, verdict, at, dsup.DESIGN_FAR))        # D overflows: nothing exceeds
    assert not any(kept_of(slots, verdict, at, dsup.DESIGN_DAG_ZERO)) and not any(kept_of(slots, verdict, at, dsup.DESIGN_DAG_FAR))
    assert dsup.cut_statistics([(verdict, at, np.where(np.isin(slots, [dsup.DESIGN_DAG_ZERO, dsup.DESIGN_DAG_FAR]), dsup.DESIGNED_ID, g))])[1] == 0
    slots, g, verdict, at, _ = design_verdicts(oracle, "parallel")
    parallel = kept_of(slots, verdict, at, dsup.DESIGN_IDENTITY)
    assert parallel == [d[4] for d in dsup.DESIGNED], list(zip(dsup.DESIGNED_NAMES, parallel))
    assert parallel != point
    dag = dsup.GEOMETRY_CLUSTERS[dsup.DAG_ID]
    for name, want in (("scale-1e30", [j < 64 for j in range(dag)]), ("scale-tiny", [j == dag - 1 for j in range(dag)]), ("off", [True] * dag)):
        slots, g, verdict, at, _ = design_verdicts(oracle, name)
        assert kept_of(slots, verdict, at, 7) == want, name  # all leaves; the root alone; the test switched off
    for name in ("near-0", "at-a-centre", "inside-the-root"):
        slots, g, verdict, at, census = design_verdicts(oracle, name)
        ordinary = np.where(np.isin(slots, [dsup.DESIGN_DAG_ZERO, dsup.DESIGN_DAG_FAR]), dsup.DESIGNED_ID, g)
        levels, uncovered, _, _ = dsup.cut_statistics([(verdict, at, ordinary)])
        print(name, census, levels)
        assert uncovered == 0 and census["lod_kept"] > 0
    # an eye inside the root sphere of draw 7 refines it further than its neighbours at the same scale
    slots, g, verdict, at, _ = design_verdicts(oracle, "inside-the-root")
    inside = kept_of(slots, verdict, at, 7)
    assert sum(inside) > 1


def test_the_second_phase_has_more_pending_behind_a_lod_result(oracle):
    case = dsup.CASE["draws-257"]
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    view = dsup.case_views(case)[0]
    old, new = oracle.Hiz(ksup.wall_depth(x0=0.0)), oracle.Hiz(ksup.wall_depth(x0=0.7))
    got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view, hiz=old)
    n = int(got["draw_count"])
    g = ids[got["visible_idx"][:n]].astype(np.uint32)
    table, ranges, clusters, _, _ = dsup.geometry()
    lod = dsup.lod_views_of(case)[0]
    off = dsup.lod_view(scale=0.0)
    _, pending_lod, _, _, _ = dsup.view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], lod, None, old, dsup.SECOND_PHASE, new)
    _, pending_off, _, _, _ = dsup.view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], off, None, old, dsup.SECOND_PHASE, new)
    pending_plain = ssup.second_view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], old, new, (table, ranges, clusters))[1]["pending"]
    print("pending behind a LOD result", pending_lod, "behind the plain form", pending_plain)
    assert pending_off == pending_plain and pending_lod > pending_plain > 0
