"""The case table of tests/test_gpu_clusters.py on the ORACLE ALONE (no GPU, no product code): every case must put the kernels of
gv_pool_cull_clusters to work, so that a kernel which ignores a test, a threshold or an order cannot pass it. Per case, over the
views of its emission (the records are the oracle's own cull of the case's world, the clusters are decided by the twin's calls of
gvo_is_behind_frustum / gvo_hiz_occluded):
  - the surviving clusters are between one fifth and four fifths of the tested ones;
  - at least one draw keeps some but not all of its clusters;
  - over the views that query the wall, the Hi-Z query removes at least one cluster the frustum test keeps, and keeps at least one;
  - visible_idx of the first view is not the identity when the case has more than one draw.
"draws-0" has no draw and hence nothing to count: it is held to having none. The world's constants (clusters_support.py: the cube,
the box sizes, the anchor's place, the wall) were fixed by running this census."""
import numpy as np
import pytest

import clusters_support as ksup


def census(case, oracle):
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    hiz = oracle.Hiz(ksup.wall_depth())
    total = dict(tested=0, kept=0, plain=0, partial=0, hiz_tested=0, hiz_kept=0, hiz_plain=0, commands=0)
    first_view = None
    for view, query in zip(ksup.case_views(case), case.hiz):
        got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view, hiz=hiz if query else None)
        first_view = got if first_view is None else first_view
        n = int(got["draw_count"])
        g = ids[got["visible_idx"][:n]]
        commands, tested, plain, partial = ksup.view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], hiz if query else None)
        ranged = np.array([x < ksup.RANGED and ksup.GEOMETRY_CLUSTERS[x] > 0 for x in g], bool)
        whole = int(np.count_nonzero((g < ksup.TABLE_COUNT) & ~ranged))
        kept = len(commands) - whole
        total["tested"] += tested
        total["kept"] += kept
        total["plain"] += plain
        total["partial"] += partial
        total["commands"] += len(commands)
        if query:
            total["hiz_tested"] += tested
            total["hiz_kept"] += kept
            total["hiz_plain"] += plain
    return total, first_view


@pytest.mark.parametrize("case", ksup.CASES, ids=[c.name for c in ksup.CASES])
def test_every_case_puts_the_cluster_tests_to_work(case, oracle):
    total, first_view = census(case, oracle)
    print(case.name, total)
    if case.draws == 0:
        assert int(first_view["draw_count"]) == 0 and total["tested"] == 0 and total["commands"] == 0
        return
    assert total["tested"] > 0
    assert total["tested"] <= 5 * total["kept"] and 5 * total["kept"] <= 4 * total["tested"], total
    assert total["partial"] >= 1, total
    if any(case.hiz):
        assert total["hiz_plain"] > total["hiz_kept"] >= 1, total
    if case.draws > 1 and not case.hiz[0]:
        assert int(first_view["draw_count"]) == case.draws
    if case.draws > 1:
        n = int(first_view["draw_count"])
        assert first_view["visible_idx"][:n].tolist() != list(range(n))


def test_the_case_table_covers_the_edges_it_names():
    """candidate totals at a tile's edge, a range beyond a tile by 1 and by a whole tile + 1, and every cluster count of the issue"""
    counts = ksup.GEOMETRY_CLUSTERS
    assert {0, 1, 2, 63, 64, 65} <= set(counts) and ksup.TILE + 1 in counts and 2 * ksup.TILE + 1 in counts
    assert [counts[ksup.CASE[name].anchor] for name in ("tile-minus-1", "tile", "tile-plus-1")] == [ksup.TILE - 1, ksup.TILE, ksup.TILE + 1]
    assert sorted({c.draws for c in ksup.CASES}) == [0, 1, 2, 64, 255, 256, 257]
    assert {len(c.yaws) for c in ksup.CASES} == {1, 2, 8}
    _, _, ranges, clusters = ksup.geometry()
    bad = clusters[int(ranges[ksup.BAD_GEOMETRY]["first"]):][:ksup.GEOMETRY_CLUSTERS[ksup.BAD_GEOMETRY]]
    assert np.isnan(bad[ksup.NAN_CLUSTER]["box_min"][0]) and (bad[ksup.INVERTED_CLUSTER]["box_min"] > bad[ksup.INVERTED_CLUSTER]["box_max"]).all()
