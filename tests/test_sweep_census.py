"""Census of the worlds of tests/sweep_support.py, on the CPU with the oracle alone: the conditions that keep
tests/test_gpu_sweep_forms.py from being vacuous (the planted extremes really reach the world matrices as subnormals, -0, +-inf,
NaN and rank-0 blocks; the deep chains really walk through the subnormal range and up to overflow) and from hiding a failure
behind the NaN clause of same_floats (a NaN row compares as a class only: a world that is mostly NaN would compare nothing).
Every view the GPU tests cull with must show something, entries that carry or inherit an extreme among it."""
import numpy as np
import pytest

import sweep_support as ss

NAN_ROWS_MAX = 0.25      # per edge world: at most this share of rows holds a NaN
FINITE_ROWS_MIN = 0.60   # per edge world: at least this share of rows is entirely finite
POOLED_FLOOR = 20        # over all edge worlds: rows of each class
PLANTED_VISIBLE_MIN = 5  # per (world, view): visible entries from planted slots or slots with a planted ancestor


def world_of(oracle, sc):
    return oracle.world_matrices(sc.transforms, sc.entity_to_transform)


def visible_slots(oracle, sc, view):
    """transform slots of the entries the oracle draws under `view`"""
    exp = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view)
    return np.asarray(sc.entity_to_transform)[sc.meshes["entity"][exp["visible_idx"]]]


def test_same_floats_is_bitwise_except_between_nans():
    nan_x86, nan_gpu = np.uint32(0xFFC00000), np.uint32(0x7FC00000)
    bits = lambda *b: np.array(b, np.uint32).view(np.float32)
    assert ss.same_floats(bits(nan_x86, 0x80000000, 1, 0x7F800000), bits(nan_gpu, 0x80000000, 1, 0x7F800000)).size == 0
    assert list(ss.same_floats(bits(0x80000000, 0), bits(0, 0x80000000))) == [0, 1]          # the sign of a zero
    assert list(ss.same_floats(bits(0, 1), bits(1, 0))) == [0, 1]                            # a flushed subnormal
    assert list(ss.same_floats(bits(nan_gpu, 0x7F800000), bits(0x7F800000, nan_x86))) == [0, 1]  # NaN against inf
    assert list(ss.same_floats(bits(0x7F800000), bits(0xFF800000))) == [0]
    assert list(ss.same_floats(bits(0x3F800000), bits(0x3F800001))) == [0]


@pytest.mark.parametrize("n,seed", ss.EDGE_WORLDS)
def test_edge_world_is_mostly_finite(oracle, n, seed):
    sc = ss.edge_world(n, seed)
    assert sc.transforms.shape[0] == n and sc.count == n and np.array_equal(sc.meshes["entity"], sc.transforms["entity"])
    c = ss.row_census(world_of(oracle, sc))
    print(f"edge_world({n}, {seed}): " + ", ".join(f"{k} {int(v.sum())}" for k, v in c.items()))
    assert c["nan"].mean() <= NAN_ROWS_MAX
    assert c["finite"].mean() >= FINITE_ROWS_MIN


def test_edge_worlds_hold_every_class(oracle):
    total = dict(subnormal=0, minus_zero=0, inf=0, nan=0, zero3x3=0)
    for n, seed in ss.EDGE_WORLDS:
        sc = ss.edge_world(n, seed)
        c = ss.row_census(world_of(oracle, sc))
        live = sc.transforms["entity"] != 0  # (a free slot's row is all zero: not a product that reached zero)
        for k in total:
            total[k] += int((c[k] & live).sum())
    print(f"pooled over the edge worlds: {total}")
    for k, rows in total.items():
        assert rows >= POOLED_FLOOR, (k, rows)


def test_edge_world_shares():
    sc = ss.edge_world(4099, 0)
    tr = sc.transforms
    assert 0.80 < (tr["parent"] != 0).mean() < 0.90
    assert 0.07 < (tr["modelWithAncestors"] == 0).mean() < 0.13
    assert 0.20 < sc.planted.mean() < 0.31  # 8 classes of 3 %, 4 of 0.4 %
    e2t = np.asarray(sc.entity_to_transform)
    chained = np.flatnonzero((tr["parent"] != 0))
    up = e2t[tr["parent"][chained]]
    ok = up != 0xFFFFFFFF
    assert np.all((chained[ok] - up[ok] >= 1) & (chained[ok] - up[ok] <= 8))
    assert ss.edge_world(4099, 0).transforms.tobytes() == tr.tobytes()  # deterministic from its arguments


def test_deep_worlds_walk_through_the_subnormal_range_and_up_to_overflow(oracle):
    census = {s: ss.row_census(world_of(oracle, ss.deep_world(ss.DEEP_LENGTH, s))) for s in ss.DEEP_SCALES}
    for s, c in census.items():
        print(f"deep_world({ss.DEEP_LENGTH}, {s}): " + ", ".join(f"{k} {int(v.sum())}" for k, v in c.items()))
    down, up, level = census[0.6], census[1.6], census[1.0]
    assert down["subnormal"].sum() >= 30 and down["nan"].sum() == 0 and down["zero3x3"].sum() >= 50
    assert up["inf"].sum() >= 1 and up["nan"].sum() >= 50
    assert level["finite"].all()
    tr = ss.deep_world(ss.DEEP_LENGTH, 0.6).transforms
    assert tr["parent"][0] == 0 and np.array_equal(tr["parent"][1:], tr["entity"][:-1])


@pytest.mark.parametrize("nt,nm", [(n, n) for n in ss.TILE_COUNTS] + ss.TILE_MESH_ENDS + [ss.TILE_UNPAIRED])
def test_tile_world_puts_chains_where_it_says(oracle, nt, nm):
    import cull_paths_support as cp
    sc = ss.tile_world(nt, nm, 0)
    tr, e2t = sc.transforms, np.asarray(sc.entity_to_transform)
    assert tr.shape[0] == nt and sc.count == nm
    assert (cp.mirror_mapping(sc) == "exact") == (nm <= nt)
    chained = (tr["parent"] != 0) & (tr["entity"] != 0)
    assert not chained[:64].any()                                            # wave 0: roots
    assert list(np.flatnonzero(chained[64:128])) == ([63] if nt > 127 else [])  # wave 1: lane 63 alone
    assert list(np.flatnonzero(chained[128:192])) == ([0] if nt > 128 else [])  # wave 2: lane 0 alone
    # walked depth of every slot: the nominal one, except below the planted exceptions
    depth = np.zeros(nt, np.int64)
    for s in range(nt):
        p, d = int(tr["parent"][s]), 0
        while p and p < e2t.shape[0] and e2t[p] != 0xFFFFFFFF:
            d += 1
            assert d <= 7
            p = int(tr["parent"][e2t[p]])
        depth[s] = d
    if nt >= 769:
        assert set(depth[192:]) == set(range(8))
        up = e2t[np.minimum(tr["parent"], e2t.shape[0] - 1)]
        resolved = (tr["parent"] != 0) & (tr["parent"] < e2t.shape[0]) & (up != 0xFFFFFFFF)
        slots = np.flatnonzero(resolved)
        assert np.any(up[slots] // 256 > slots // 256)  # a parent at a higher slot, in another workgroup
        assert np.any(tr["parent"] >= e2t.shape[0])      # the dangling id
        assert np.any((tr["parent"] != 0) & (tr["parent"] < e2t.shape[0]) & (up == 0xFFFFFFFF))  # the id of a freed slot
    assert np.isfinite(world_of(oracle, sc)).all()
    assert visible_slots(oracle, sc, ss.tile_view()).size > 0


@pytest.mark.parametrize("n,seed", ss.EDGE_WORLDS)
def test_edge_world_views_show_planted_entries(oracle, n, seed):
    sc = ss.edge_world(n, seed)
    closure = ss.planted_closure(sc)
    for name, view in ss.edge_views() + [(f"batch view {k}", v) for k, v in enumerate(ss.edge_batch())]:
        slots = visible_slots(oracle, sc, view)
        print(f"edge_world({n}, {seed}) {name}: {slots.size} visible, {int(closure[slots].sum())} of them planted or below a planted slot")
        assert slots.size > 0 and closure[slots].sum() >= PLANTED_VISIBLE_MIN, name
        assert slots.size < n  # (and not everything: the cull decides something)


@pytest.mark.parametrize("scale", ss.DEEP_SCALES)
def test_deep_world_view_shows_the_far_end_of_the_chain(oracle, scale):
    """(a chain of scale 1 has no slot outside the normal range: there the view must only show something)"""
    sc = ss.deep_world(ss.DEEP_LENGTH, scale)
    slots = visible_slots(oracle, sc, ss.deep_view(scale))
    planted = ss.deep_planted(sc, scale)
    print(f"deep_world({ss.DEEP_LENGTH}, {scale}): {slots.size} visible, {int(planted[slots].sum())} of them outside the normal range")
    assert slots.size > 0
    if planted.any():
        assert planted[slots].sum() >= PLANTED_VISIBLE_MIN


def test_sphere_world_views_show_planted_entries(oracle):
    import cull_paths_support as cp
    sc = ss.sphere_world()
    assert sc.count == ss.SPHERE_N > cp.HOT_MIN and not sc.transforms["parent"].any() and cp.mirror_mapping(sc) == "exact"
    assert 0.015 < sc.planted.mean() < 0.05
    w = world_of(oracle, sc)
    radius_inputs = ss.row_census(w)
    assert radius_inputs["subnormal"].sum() >= 20 and radius_inputs["nan"].sum() >= 5 and radius_inputs["inf"].sum() >= 5
    for name, view in ss.sphere_views():
        slots = visible_slots(oracle, sc, view)
        print(f"sphere_world {name}: {slots.size} visible, {int(sc.planted[slots].sum())} of them planted")
        assert 0 < slots.size < ss.SPHERE_N and sc.planted[slots].sum() >= PLANTED_VISIBLE_MIN, name
