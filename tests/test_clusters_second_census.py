"""The case table of tests/test_gpu_clusters_second.py on the ORACLE ALONE (no GPU, no product code): every case must put the
kernels of gv_pool_cull_clusters_second_phase to work. Per case (clusters_second_support.case_census: the records are the oracle's
own cull, the clusters are decided by the twins' calls of gvo_is_behind_frustum / gvo_hiz_occluded):
  - the pending total and the second-phase survivor total are the values the case names;
  - unless the case is named as a 0 / all edge, the second phase keeps at least one pending cluster and rejects at least one pending
    cluster that passes the frustum test.
Over the table: a pending cluster that is a frustum reject, a draw with commands in both phases, a multi-view case in which a pending
tile crosses from one view into the next and a non-queried view lies between two queried ones. The images and the worlds of
clusters_second_support.py were fixed by running this census."""
import pytest

import clusters_second_support as ssup


@pytest.mark.parametrize("case", ssup.CASES, ids=[c.name for c in ssup.CASES])
def test_every_case_meets_its_conditions_on_the_oracle(case, oracle):
    total, kept, first_phase, per_view = ssup.case_census(case, oracle)
    print(case.name, total, "kept", kept, "phase 1", first_phase, "pending per queried view", per_view)
    if case.pending is not None:
        assert total["pending"] == case.pending
    if case.kept is not None:
        assert kept == case.kept
    assert kept <= total["pending"]
    if not case.edge:
        assert kept >= 1 and total["rejected_in_view"] >= 1, (total, kept)


def table_census(oracle):
    return {case.name: ssup.case_census(case, oracle) for case in ssup.CASES}


def test_the_table_holds_a_frustum_reject_and_a_draw_with_commands_in_both_phases(oracle):
    every = table_census(oracle)
    assert any(total["frustum_rejects"] >= 1 for total, _, _, _ in every.values())
    assert any(total["both_phases"] >= 1 for total, _, _, _ in every.values())
    # ... both in one case that also keeps and rejects: the two phases are at work on the same draws
    assert any(total["frustum_rejects"] >= 1 and total["both_phases"] >= 1 and kept >= 1 and total["rejected_in_view"] >= 1
               for total, kept, _, _ in every.values())


def test_a_pending_tile_crosses_views_and_a_view_that_is_not_queried_lies_between_two_that_are(oracle):
    found = False
    for case in ssup.CASES:
        if len(case.yaws) < 2:
            continue
        _, _, _, per_view = ssup.case_census(case, oracle)
        between = any(a + 1 < b and not any(case.hiz[a + 1:b]) and pa and pb for (a, pa), (b, pb) in zip(per_view, per_view[1:]))
        start, crossing = 0, False
        for _, pending in per_view[:-1]:
            start += pending
            rest = sum(p for _, p in per_view) - start
            crossing = crossing or (pending and rest and start % ssup.TILE != 0)  # the next view's first pending shares this one's last tile
        print(case.name, per_view, "between", between, "crossing", crossing)
        found = found or (between and crossing)
    assert found


def test_the_case_table_covers_the_edges_it_names():
    named = {c.pending for c in ssup.CASES}
    assert {0, 1, ssup.TILE - 1, ssup.TILE, ssup.TILE + 1, 2 * ssup.TILE + 1} <= named
    assert any(c.kept == 0 and c.pending != 0 for c in ssup.CASES) and any(c.kept is not None and c.kept == c.pending and c.kept for c in ssup.CASES)
    assert {1, 2, 255, 256, 257} <= {c.draws for c in ssup.CASES if c.world == "mix"}
    assert {len(c.yaws) for c in ssup.CASES} == {1, 2, 8}
    sparse = ssup.CASE["sparse"]
    assert sparse.pending == sparse.draws == 257  # one pending cluster per draw of 64: 257 pending over 65 candidate tiles
