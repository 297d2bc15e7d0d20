"""GPU parity of the cull over every launch form its dispatch can pick: the cases of tests/cull_paths_support.py (CASES), which
tests/test_cull_plan_census.py proves on the CPU to take every reachable (cull form, HIZ, MAP, emit form) between them.

A case binds its scene to one of the session's contexts, brings the pool to a known state (two quiet culls, then every transform
marked dirty) and walks its program. At every cull: the launch counts of GvStats and bounds_blocks_total must be the ones
cull_plan expects (that keeps the Python restatement honest), and every view's outputs must equal the oracle's bit for bit —
draw count, visible_idx, bakedModel and distanceSq as uint32, the isVisible bytes of a main pass (the poison value left alone
by shadow passes), count and bytes alone for count-only views. A sweep riding on a cull must leave the oracle's world matrices.
The programs cull the same pool many times with other views, so whatever alternates from cull to cull (chunk totals, the listed
cull's counters, the one-launch form's tickets and epochs, the emit's quarter-chunk flags) is carried through."""
import functools

import numpy as np
import pytest

import cull_paths_support as cp
from garden_amd import scene

pytestmark = pytest.mark.gpu

GV_DIRTY_TRANSFORM = 0
GV_SWEEP_VALU = 0
COUNTED = ("cull", "scan", "emit", "sweep")


@functools.lru_cache(maxsize=4)
def depth_image(size):
    d = scene.synthetic_depth(*size)
    d.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def pyramids(oracle):
    """{size: the oracle's pyramid of depth_image(size)}, built once"""
    cache = {}

    def get(size):
        if size not in cache:
            cache[size] = oracle.Hiz(depth_image(size))
        return cache[size]
    return get


def private_copy(sc):
    """the cached scene is shared with other cases and with the census: a case edits its own copy"""
    return scene.Scene(sc.meshes.copy(), sc.transforms.copy(), sc.entity_to_transform)


def compare_view(vis, oracle, meshes, transforms, e2t, view, index, hz, what, pool_id=None):
    """one view's results against the oracle's; returns the oracle's result"""
    main_pass = view["shadow_pass"] < 0
    meshes["isVisible"] = 7  # poison: a main pass overwrites every slot, a shadow pass none
    got = vis.fetch(index, write_back=True, occupancy=meshes.shape[0], pool_id=pool_id)
    got_vis = meshes["isVisible"].copy()
    expected = meshes.copy()
    expected["isVisible"] = 7
    exp = oracle.prepare_meshes(expected, transforms, e2t, view, hiz=hz if view["use_hiz"] else None, threads=4)
    exp_vis = expected["isVisible"]
    assert got["draw_count"] == exp["draw_count"], what
    if main_pass:
        assert np.array_equal(got_vis, exp_vis), what
        assert got["is_visible"] is not None and np.array_equal(got["is_visible"], exp_vis), what
    else:
        assert np.all(got_vis == 7) and np.all(exp_vis == 7), what
    if view["emit_records"]:
        o = np.argsort(exp["visible_idx"], kind="stable")  # (the oracle's workers deliver in ranges: by slot, as fetch() orders)
        assert np.array_equal(got["visible_idx"], exp["visible_idx"][o]), what
        assert np.array_equal(got["baked_model"].view(np.uint32), exp["baked_model"][o].view(np.uint32)), what
        assert np.array_equal(got["distance_sq"].view(np.uint32), exp["distance_sq"][o].view(np.uint32)), what
    return exp


def assert_launches(stats, plan, what):
    got = {k: stats["launches"][k] for k in COUNTED}
    assert got == plan.launches, f"{what}: launches {got}, cull_plan expects {plan.launches} (upkeep {plan.upkeep}, cull {plan.cull_forms}, emit {plan.emit_forms})"
    assert (stats["bounds_blocks_total"] != 0) == plan.bounds_blocks, what


def move_a_few(oracle, sc, c, view, hz, rng):
    """EDIT_SLOTS scattered transforms of entities the next view does not see take the place of ones it sees; returns their slots"""
    e2t = np.asarray(sc.entity_to_transform)
    seen = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, e2t, dict(view, use_hiz=0), threads=4)["visible_idx"]
    ent = sc.meshes["entity"]
    live = np.nonzero((ent != 0) & (sc.meshes["isEnabled"] != 0))[0]
    slot_of = lambda mesh_slots: e2t[ent[mesh_slots]]
    hidden = np.setdiff1d(slot_of(np.setdiff1d(live, seen)), [int(scene.GV_NONE)])
    shown = np.setdiff1d(slot_of(seen), [int(scene.GV_NONE)])
    moved = np.sort(rng.choice(hidden, cp.EDIT_SLOTS, replace=False))
    sc.transforms["position"][moved, :3] = sc.transforms["position"][rng.choice(shown, cp.EDIT_SLOTS), :3]
    sc.transforms["selfActive"][moved] = 1
    return moved


@pytest.mark.parametrize("c", cp.CASES, ids=lambda c: c.name)
def test_cull_paths(request, oracle, pyramids, c):
    vis = request.getfixturevalue(c.fixture)
    sc = private_copy(cp.build_scene(c.kind, c.n, c.transforms))
    e2t = sc.entity_to_transform
    if cp.FIXTURE_FLAGS[c.fixture].slot_order:
        assert cp.mirror_mapping(sc) == c.MAP
    else:
        assert c.MAP == "exact" and c.n == c.transforms  # (pools that pair slot for slot: exact under any mirror order)
    side = cp.scene_side(c.transforms)
    rng = np.random.Generator(np.random.PCG64(c.n))
    size = c.hiz
    vis.hiz_build(depth_image(size))
    vis.bind_transforms(sc.transforms, e2t)
    vis.bind_pool(0, sc.meshes)
    vis.hierarchy_rebuild()
    assert vis.stats()["max_depth"] == c.depth
    # a known state: a quiet cull behind the first one, then every transform re-mirrored (nothing derived is current, nothing
    # is on record, the cull before was quiet)
    settle = cp.make_views("C", 99, side)
    vis.cull(0, settle)
    vis.cull(0, settle)
    vis.mark_dirty(GV_DIRTY_TRANSFORM, 0, c.transforms)

    program = cp.PROGRAMS[c.program]
    plans = {i: plan for i, _step, plan in cp.run_program(c)}
    for i, step in enumerate(program):
        what = f"{c.name} step {i} {step.kind} {step.views}"
        if step.kind == "dense":
            vis.mark_dirty(GV_DIRTY_TRANSFORM, 0, c.transforms)
        elif step.kind == "few":
            nxt = next(s for s in program[i:] if s.kind == "cull")
            view = cp.make_views(nxt.views, program.index(nxt, i), side)[0]
            moved = move_a_few(oracle, sc, c, view, None, rng)
            for s in moved:
                vis.mark_dirty(GV_DIRTY_TRANSFORM, int(s), 1)
        elif step.kind == "sweep":
            vis.sweep(GV_SWEEP_VALU)
        elif step.kind == "hiz":
            size = step.views
            vis.hiz_build(depth_image(size))
        else:
            views = cp.make_views(step.views, i, side)
            plan = plans[i]
            if step.sweep:
                vis.sweep(step.sweep)
            vis.stats_reset()
            vis.cull(0, views)
            assert_launches(vis.stats(), plan, what)
            for index, view in enumerate(views):
                exp = compare_view(vis, oracle, sc.meshes, sc.transforms, e2t, view, index, pyramids(size), f"{what} view {index}")
                if index == 0 and i > 0 and program[i - 1].kind == "few" and c.depth == 0 and c.MAP == "exact" and not view["use_hiz"]:
                    assert np.intersect1d(moved, exp["visible_idx"]).size > 0, f"{what}: none of the moved slots came into view"
            if step.sweep:
                world = vis.get_world(0, c.transforms)
                assert np.array_equal(world.view(np.uint32), oracle.world_matrices(sc.transforms, e2t, threads=4).view(np.uint32)), what


@pytest.mark.parametrize("t", cp.TABLE_CASES, ids=lambda t: t.name)
def test_table_paths(request, oracle, pyramids, t):
    """Recorded pools of different sizes and mappings in one gv_cull_batch_begin / _end: one cull launch and one emit launch for
    all of them, twice (the second batch with other views, Hi-Z swapped between the pools)."""
    vis = request.getfixturevalue(t.fixture)
    sc, pools = cp.table_pools(t)
    transforms, e2t = sc.transforms.copy(), sc.entity_to_transform
    side = cp.scene_side(t.n)
    vis.hiz_build(depth_image(t.hiz))
    vis.bind_transforms(transforms, e2t)
    for pool_id, mapping, n, _a, _b in t.pools:
        assert cp.mirror_mapping(scene.Scene(pools[pool_id], transforms, e2t)) == mapping and pools[pool_id].shape[0] == n
        vis.bind_pool(pool_id, pools[pool_id])
    vis.hierarchy_rebuild()
    for batch in (0, 1):
        plan = cp.table_plan(cp.table_jobs(t, batch))
        vis.sync()
        vis.stats_reset()
        vis.cull_batch_begin()
        views = {}
        for pool_id, _mapping, _n, first, second in t.pools:
            views[pool_id] = cp.make_views(first if batch == 0 else second, 7 + 5 * batch + pool_id, side)
            vis.cull(pool_id, views[pool_id])
        assert sum(vis.stats()["launches"][k] for k in COUNTED) == 0  # recorded, not launched
        vis.cull_batch_end()
        assert_launches(vis.stats(), plan, f"{t.name} batch {batch}")
        for pool_id, _mapping, _n, _a, _b in t.pools:
            for index, view in enumerate(views[pool_id]):
                compare_view(vis, oracle, pools[pool_id], transforms, e2t, view, index, pyramids(t.hiz),
                             f"{t.name} batch {batch} pool {pool_id} view {index}", pool_id=pool_id)
