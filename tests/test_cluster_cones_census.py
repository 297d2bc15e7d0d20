"""The case table, the designed cones and the designed draws of tests/test_gpu_cluster_cones.py on the ORACLE AND THE TWIN ALONE (no
GPU, no product code): every case must put the cone test of gv_pool_cull_cluster_cones to work, so that a kernel which ignores a
cone, an eye or the order of the conjunction cannot pass it. The records are the oracle's own cull of the case's world; which cluster
passes the frustum and the pyramid is decided by the twin's calls of gvo_is_behind_frustum / gvo_hiz_occluded (cluster_twin.h); the
cone test by tests/cluster_cone_twin.h.
  - every case that tests at least SHARE_FROM clusters: the cone rejects between 1/10 and 1/2 of the tested clusters of the views
    whose eye is not all zero, at least one draw is partly cone-rejected, at least one cluster is cone-rejected that the frustum (and
    the pyramid) keep, and a direction eye and a point eye disagree on at least one cluster; an all-zero eye rejects nothing;
  - every such case with a queried view: at least one cluster is rejected by the pyramid that the cone keeps;
  - the smaller cases (0 draws; one draw of one cluster) test what the world gives them;
  - every designed cone and every designed draw lands on the side it was designed for."""
import numpy as np
import pytest

import cluster_cones_support as nsup
import clusters_support as ksup


def case_census(oracle, case):
    """(the census summed over the views with an eye, the one of the all-zero eyes, verdicts of view 0 under the point and the
    direction eye, draws of view 0)"""
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    hiz = oracle.Hiz(ksup.wall_depth())
    eyes = nsup.eyes_of(case)
    seeing, blind = dict.fromkeys(nsup.CENSUS_FIELDS, 0), dict.fromkeys(nsup.CENSUS_FIELDS, 0)
    both, draws = None, 0
    for v, (view, query, kind) in enumerate(zip(nsup.case_views(case), case.hiz, case.eyes)):
        got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view, hiz=hiz if query else None)
        n = int(got["draw_count"])
        g = ids[got["visible_idx"][:n]]
        _, _, one, _ = nsup.view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], eyes[v], hiz if query else None)
        for name in nsup.CENSUS_FIELDS:
            (blind if kind == "Z" else seeing)[name] += one[name]
        if v == 0:
            draws = n
            both = [nsup.view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], np.array(eye, np.float32), None)[3]
                    for eye in (nsup.POINT_EYE, nsup.direction_eye(case.yaws[0]))]
    return seeing, blind, both, draws


@pytest.mark.parametrize("case", nsup.CASES, ids=[c.name for c in nsup.CASES])
def test_every_case_puts_the_cone_to_work(case, oracle):
    seeing, blind, both, draws = case_census(oracle, case)
    print(case.name, "draws", draws, "with an eye", seeing, "all-zero eyes", blind)
    assert draws == case.draws if not case.hiz[0] else 0 < draws <= case.draws  # (the wall hides whole entities from a view that queries)
    assert blind["cone_rejected"] == 0 and ("Z" not in case.eyes or blind["tested"] > 0)
    if case.draws == 0:
        assert seeing["tested"] == 0
        return
    assert seeing["tested"] > 0
    if seeing["tested"] < nsup.SHARE_FROM:
        return
    assert 10 * seeing["cone_rejected"] >= seeing["tested"] and 2 * seeing["cone_rejected"] <= seeing["tested"], seeing
    assert seeing["partial"] >= 1 and seeing["cone_only"] >= 1, seeing
    if any(case.hiz):
        assert seeing["hiz_only"] >= 1, seeing
    point, direction = both
    assert np.count_nonzero((point ^ direction) & nsup.CONE) >= 1


def test_the_measured_shares_of_the_plain_worlds(oracle):
    """the share of cone-rejected clusters under the camera's point eye over clusters_support's own tables: what the rule was
    measured with before it was built (7 263 of 22 354 in world(257), 35 of 129 in world(2))"""
    table, _, ranges, clusters = ksup.geometry()
    tables = (table, ranges, clusters, nsup.outward_cones(clusters))
    view = ksup.camera()
    for draws, rejected, tested in ((257, 7263, 22354), (2, 35, 129)):
        sc, ids = ksup.world(draws)
        got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view)
        n = int(got["draw_count"])
        _, t, census, _ = nsup.view_commands(got["baked_model"], ids[got["visible_idx"][:n]], np.arange(n + 1), view["view_proj"],
                                             np.array(nsup.POINT_EYE, np.float32), None, tables=tables)
        print(draws, census)
        assert (census["cone_rejected"], t) == (rejected, tested)


def design_verdicts(oracle, eye):
    """slot -> the verdict bytes of the designed cones of that draw, over the oracle's own records of the designed scene"""
    sc, ids, _ = nsup.design_scene()
    view = ksup.camera()
    got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view)
    n = int(got["draw_count"])
    assert n == sc.count  # every entity is delivered, the mirrored and the flat one too
    slots = got["visible_idx"][:n].astype(np.int64)
    commands, tested, census, verdict = nsup.view_commands(got["baked_model"], ids[slots], np.arange(n + 1), view["view_proj"], eye, None)
    assert tested == 3 * len(nsup.DESIGNED)
    clustered = [int(s) for s in slots if ids[s] == nsup.DESIGNED_ID]  # in draw order
    return {slot: verdict[i * len(nsup.DESIGNED):(i + 1) * len(nsup.DESIGNED)] for i, slot in enumerate(clustered)}, commands, got


def test_every_designed_cone_lands_on_its_side(oracle):
    verdicts, _, _ = design_verdicts(oracle, nsup.design_eyes()["camera"])
    mine = verdicts[nsup.DESIGN_IDENTITY]
    assert all(int(b) & nsup.FRUSTUM for b in mine)  # every box is inside the frustum: only the cone decides
    for (name, _, _, _, rejected), bits in zip(nsup.DESIGNED, mine):
        assert bool(int(bits) & nsup.CONE) == rejected, name
    assert sum(d[4] for d in nsup.DESIGNED) == 3


def test_every_designed_draw_lands_on_its_side(oracle):
    verdicts, commands, got = design_verdicts(oracle, nsup.design_eyes()["camera"])
    n = int(got["draw_count"])
    models = np.asarray(got["baked_model"]).reshape(-1, 12)[:n]
    slot_of = got["visible_idx"][:n].astype(np.int64).tolist()
    det = {slot: float(np.linalg.det(models[slot_of.index(slot)][:9].reshape(3, 3).astype(np.float64)))
           for slot in (nsup.DESIGN_IDENTITY, nsup.DESIGN_MIRRORED, nsup.DESIGN_FLAT)}
    assert det[nsup.DESIGN_IDENTITY] == 1.0 and det[nsup.DESIGN_MIRRORED] < 0.0 and det[nsup.DESIGN_FLAT] == 0.0
    # a mirrored and a singular model are never cone-rejected; the frustum keeps the clusters of all three draws
    for slot in (nsup.DESIGN_MIRRORED, nsup.DESIGN_FLAT):
        assert not any(int(b) & nsup.CONE for b in verdicts[slot]) and all(int(b) & nsup.FRUSTUM for b in verdicts[slot])
    # the identity draw's translation puts the apex of the apex-0 cones exactly at the second eye: w = 0 keeps what the camera's eye rejects
    at_apex, _, _ = design_verdicts(oracle, nsup.design_eyes()["at-apex"])
    for name in ("cutoff-0", "cutoff-0.5", "cutoff-minus-0.5"):
        j = nsup.DESIGNED_NAMES.index(name)
        assert int(verdicts[nsup.DESIGN_IDENTITY][j]) & nsup.CONE and not int(at_apex[nsup.DESIGN_IDENTITY][j]) & nsup.CONE, name
    assert len(commands) == 3 * len(nsup.DESIGNED) - 3  # only the identity draw loses its three rejected clusters


def test_the_tables_are_parallel_and_the_designed_geometry_is_the_last_range():
    table, ranges, clusters, cones = nsup.geometry()
    assert len(cones) == len(clusters) and cones.dtype.itemsize == 32
    assert int(ranges[nsup.DESIGNED_ID]["first"]) + int(ranges[nsup.DESIGNED_ID]["count"]) == len(clusters)
    axis = cones["axis"][:int(ranges[nsup.DESIGNED_ID]["first"])]
    length = np.linalg.norm(axis, axis=1)
    assert np.all((np.abs(length - 1.0) < 1e-6) | (length == 0.0)) and np.count_nonzero(length == 0.0) >= 1  # (the NaN box's cone)
