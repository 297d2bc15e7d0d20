"""The case table and the designed scenes of tests/test_gpu_cluster_runs.py on the ORACLE AND THE TWIN ALONE (no GPU, no product
code): every case must put the kernels of gv_pool_cull_cluster_runs to work, so that a kernel which ignores a link, a span or a
word edge cannot pass it. The records are the oracle's own cull of the case's world; which cluster survives is decided by the twin's
calls of gvo_is_behind_frustum / gvo_hiz_occluded (cluster_twin.h); links, heads and runs by tests/cluster_runs_twin.h.
  - every non-empty case: survivors between 1/5 and 4/5 of the tested clusters (the boxes are clusters_support's), 1 <= runs and
    2 * runs <= survivors;
  - over the table as a whole: every break reason (a non-survivor, a gap, the span) occurs, a run of GV_CLUSTER_RUN_SPAN clusters
    occurs, a run crosses a 64-candidate word edge and one a 256-candidate tile edge;
  - every designed scene shows exactly the pattern it was designed for, at every lead."""
import numpy as np
import pytest

import cluster_runs_support as rsup
import clusters_support as ksup


@pytest.fixture(scope="module")
def table_census(oracle):
    """case name -> (the census summed over the case's views, tested, the first view's records)"""
    out = {}
    hiz = oracle.Hiz(ksup.wall_depth())
    for case in ksup.CASES:
        sc, ids = ksup.world(case.draws, anchor=case.anchor)
        total, tested, base, first_view = {}, 0, 0, None
        for view, query in zip(ksup.case_views(case), case.hiz):
            got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view, hiz=hiz if query else None)
            first_view = got if first_view is None else first_view
            n = int(got["draw_count"])
            g = ids[got["visible_idx"][:n]]
            _, t, one = rsup.view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], hiz if query else None, base)
            base += one["candidates"]
            tested += t
            rsup.add_census(total, one)
        out[case.name] = (total, tested, first_view)
    return out


@pytest.mark.parametrize("case", ksup.CASES, ids=[c.name for c in ksup.CASES])
def test_every_case_puts_the_runs_to_work(case, table_census):
    total, tested, first_view = table_census[case.name]
    print(case.name, "tested", tested, total)
    if case.draws == 0:
        assert int(first_view["draw_count"]) == 0 and tested == 0 and total.get("runs", 0) == 0
        return
    assert tested > 0
    assert tested <= 5 * total["survivors"] and 5 * total["survivors"] <= 4 * tested, total
    assert 1 <= total["runs"] and 2 * total["runs"] <= total["survivors"], total


def test_the_table_as_a_whole_shows_every_break_and_every_edge(table_census):
    total = {}
    for name, (one, _, _) in table_census.items():
        rsup.add_census(total, one)
    print(total)
    assert total["break_nonsurvivor"] >= 1 and total["break_gap"] >= 1 and total["break_span"] >= 1
    assert total["longest"] == rsup.SPAN
    assert total["cross_word"] >= 1 and total["cross_tile"] >= 1
    assert total["whole"] >= 1


def test_the_tables_hold_the_designed_breaks():
    table, _, ranges, clusters = rsup.geometry()
    _, _, _, plain = ksup.geometry()
    assert np.array_equal(clusters["box_min"], plain["box_min"], equal_nan=True) and np.array_equal(clusters["box_max"], plain["box_max"], equal_nan=True)
    follows = {}
    for g, r in enumerate(ranges):
        a, n = int(r["first"]), int(r["count"])
        cl = clusters[a:a + n]
        follows[g] = [int(cl[j - 1]["first"]) + int(cl[j - 1]["count"]) == int(cl[j]["first"]) for j in range(1, n)]
    for g in rsup.GAP_GEOMETRIES:
        assert [j + 1 for j, f in enumerate(follows[g]) if not f] == list(range(rsup.GAP_EVERY, len(follows[g]) + 1, rsup.GAP_EVERY))
    a = int(ranges[rsup.OVERLAP_GEOMETRY]["first"])
    assert int(clusters[a + rsup.OVERLAP_AT]["first"]) < int(clusters[a + rsup.OVERLAP_AT - 1]["first"]) + int(clusters[a + rsup.OVERLAP_AT - 1]["count"])
    a = int(ranges[rsup.ZERO_GEOMETRY]["first"])
    assert all(int(clusters[a + j]["count"]) == 0 for j in rsup.ZERO_AT) and all(follows[rsup.ZERO_GEOMETRY])
    a = int(ranges[rsup.WRAP_GEOMETRY]["first"])
    assert int(clusters[a + rsup.WRAP_AT]["first"]) + int(clusters[a + rsup.WRAP_AT]["count"]) == 1 << 32
    assert int(table[rsup.WRAP_GEOMETRY]["first"]) + int(clusters[a]["first"]) > 0xFFFFFFFF  # the head's uint32 add wraps
    untouched = [g for g in range(len(ranges)) if g not in rsup.GAP_GEOMETRIES + (rsup.OVERLAP_GEOMETRY, rsup.WRAP_GEOMETRY)]
    assert all(all(follows[g]) for g in untouched)


def design_census(oracle, name, lead):
    """the twin's commands and census of designed scene `name` behind `lead` whole draws, over the oracle's own records"""
    survive, rows, gfirst, _ = rsup.design_patterns()[name]
    sc = rsup.design_scene()
    view = ksup.camera()
    got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view)
    n = int(got["draw_count"])
    assert n == rsup.DESIGN_ENTITIES  # every entity is wholly inside the frustum
    g = np.full(n, rsup.VOID_ID, np.uint32)
    g[:lead] = rsup.WHOLE_ID
    g[lead] = rsup.CLUSTERED_ID
    table, ranges, clusters = rsup.design_tables(survive, rows, gfirst)
    commands, tested, census = rsup.view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], None, 0, table, ranges, clusters)
    return commands, tested, census, survive


@pytest.mark.parametrize("lead", rsup.LEADS)
@pytest.mark.parametrize("name", sorted(rsup.design_patterns()))
def test_a_designed_scene_shows_its_pattern(name, lead, oracle):
    commands, tested, census, survive = design_census(oracle, name, lead)
    want = rsup.design_patterns()[name][3]
    print(name, lead, census)
    assert tested == len(survive) and census["whole"] == lead and census["candidates"] == lead + len(survive)
    assert census["survivors"] == sum(survive)  # a box inside the entity survives, one behind the camera does not
    for key, value in want.items():
        assert census[key] == value, (key, census)
    assert len(commands) == lead + census["runs"]
    assert commands["draw"].tolist() == list(range(lead)) + [lead] * census["runs"]
