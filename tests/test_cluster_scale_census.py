"""The two worlds of tests/test_gpu_cluster_scale.py on the ORACLE AND THE TWINS ALONE (no GPU, no product code): each must take the
index machinery of the cluster cull past its first iteration, so that a wrong carry, a stale partial sum, a missing barrier or a search
that only works over two entries cannot pass the GPU tests. The records are the oracle's own cull of the world, the clusters are
decided by the twins' calls of gvo_is_behind_frustum / gvo_hiz_occluded; the thresholds are cluster_scale_support's restatement of
gv_cluster_kernels.hpp with the MI355X's 256 compute units. The worlds' constants were fixed by running this census; it prints the
totals its conditions are about. It also holds the numpy placement of cluster_scale_support to clusters_support.place."""
import functools

import numpy as np
import pytest

import cluster_scale_support as xsup
import clusters_support as ksup
import commands_support as csup

WALK = xsup.GRID_PER_CU * xsup.CUS   # workgroups of a walk's grid


# ---- the numpy placement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [csup.INDEXED, csup.GAPS], ids=["indexed20", "gaps32"])
def test_the_numpy_placement_gives_the_bytes_of_clusters_support_place(dtype, oracle):
    case = ksup.CASE["views-8"]
    sc, ids = ksup.world(case.draws, anchor=case.anchor)
    hiz = oracle.Hiz(ksup.wall_depth())
    per_view = []
    for view, query in zip(ksup.case_views(case), case.hiz):
        got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view, hiz=hiz if query else None)
        n = int(got["draw_count"])
        per_view.append(ksup.view_commands(got["baked_model"], ids[got["visible_idx"][:n]], np.arange(n + 1), view["view_proj"],
                                           hiz if query else None)[0])
    counts = [len(c) for c in per_view]
    assert min(counts) > 11 and len(per_view) == 8
    for region, held in ((0, None), (5, None), (0, 11), (5, 11), (max(counts) + 3, None), (0, counts[0] + 2)):
        rows = (len(per_view) * region if region else sum(counts)) + 7
        pattern = csup.background(rows, dtype.itemsize)
        assert xsup.place(per_view, dtype, region, held, pattern).tobytes() == ksup.place(per_view, dtype, region, held, pattern).tobytes(), (region, held)


def test_the_numpy_firsts_are_clusters_support_firsts():
    fetched = [dict(draw_count=3), dict(draw_count=0), dict(draw_count=2)]
    starts = np.array([4, 7, 7, 9], np.uint32)
    bases = (np.array([10, 12, 15, 20, 21], np.uint32), np.array([0, 3, 3, 5], np.uint32))
    for b, ends in ((None, starts), (bases, np.array([0, 17, 17, 30], np.uint32))):
        assert [x.tolist() for x in xsup.firsts(fetched, ends, b)] == ksup.firsts(fetched, ends, b)


# ---- world A: the count side -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def candidates_a(oracle):
    w = xsup.world_a()
    hiz = oracle.Hiz(xsup.a_image("wall"))
    return xsup.Candidates(xsup.records_of(w, oracle), xsup.views_of(w), [hiz if h else None for h in w.hiz], w.tables, w.occupancy)


def test_world_a_takes_the_count_side_past_one_scan_turn(oracle):
    w, c = xsup.world_a(), candidates_a(oracle)
    queried = [v for v, h in enumerate(w.hiz) if h]
    looking = [v for v in range(len(w.yaws)) if v != 2]
    tested = [int(np.count_nonzero(c.is_cluster & (c.view == v))) for v in range(5)]
    kept = [int(np.count_nonzero(c.is_cluster & c.survives & (c.view == v))) for v in range(5)]
    plain = [int(np.count_nonzero(c.is_cluster & c.frustum & (c.view == v))) for v in range(5)]
    tail = [int(np.count_nonzero(c.is_cluster & (c.view == v) & (c.draw >= xsup.SCAN_BLOCK * xsup.TILE))) for v in range(5)]
    print("world A: blocks", c.blocks, "T", c.total, "tiles", c.tiles, "draws", c.draws, "starts", c.start, "tested", tested, "survivors", kept,
          "frustum alone", plain, "tested behind draw 262144", tail, "widest tile span", c.widest_tile(), "emptied count workgroups", c.emptied_blocks())
    assert w.occupancy == xsup.A_SLOTS and c.blocks == 5 * 1026
    assert c.blocks > xsup.SCAN_TURN and c.blocks % 4 != 0          # a second turn of scan_table, through its scalar tail
    assert len(w.tables[1]) and int(w.tables[1]["count"].max()) == xsup.A_MAX_RANGE and len(w.tables[0]) == xsup.A_TABLE_COUNT
    for v in looking:                                               # the per-view sum of block_tested strides, and its second stride holds something
        assert xsup.SCAN_BLOCK * xsup.TILE < c.draws[v] < w.occupancy, (v, c.draws[v])
        assert tail[v] > 0, v
    assert c.draws[2] == 0 and c.start[2] == c.start[3]             # a view without candidates between views with candidates
    assert c.start[5] > c.start[4] > 0                              # the carry into the second turn is not zero, and view 4 needs it
    assert c.start[4] == c.start[3] + int(np.count_nonzero(c.view == 3))
    assert c.widest_tile() >= 32                                    # locate searches over 32 and more count workgroups
    assert c.emptied_blocks() >= 100                                # the tile_block fill skips workgroups without candidates
    assert sum(1 for v in range(5) if c.start[v] % xsup.TILE) >= 2  # views that start mid-tile
    assert 5 * sum(kept) >= sum(tested) and 5 * sum(kept) <= 4 * sum(tested)
    for v in queried:
        assert plain[v] > kept[v] >= 1, v                           # the query removes a cluster and keeps one


def test_world_a_behind_a_rebuilt_pyramid_has_a_second_phase(oracle):
    w, c = xsup.world_a(), candidates_a(oracle)
    queried = np.array(w.hiz)
    pending, span = c.widest_pending_tile(queried)
    narrow = oracle.Hiz(xsup.a_image("narrow"))
    again = xsup.Candidates(xsup.records_of(w, oracle), xsup.views_of(w), [narrow if h else None for h in w.hiz], w.tables, w.occupancy)
    kept = int(np.count_nonzero(c.pending(queried) & again.survives))
    print("world A: pending", pending, "widest pending tile (candidate tiles)", span, "second-phase survivors", kept)
    assert pending > xsup.TILE and 0 < kept < pending


# ---- world B: the tile side --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def candidates_b(oracle, image="wall", wide=False):
    w = xsup.world_b()
    hiz = oracle.Hiz(xsup.image(image))
    extra = dict(lod_views=xsup.b_lod_views(), eyes=xsup.B_EYES) if wide else {}
    return xsup.Candidates(xsup.records_of(w, oracle), xsup.views_of(w), [hiz if h else None for h in w.hiz],
                           xsup.b_wide_tables() if wide else w.tables, w.occupancy, **extra)


def test_world_b_tables_hold_the_edges_they_name():
    _, ranges, clusters = xsup.world_b().tables
    assert tuple(int(x) for x in ranges["count"]) == (4096, 4097, 1000) and int(ranges["count"].max()) == xsup.B_MAX_RANGE
    for g, r in enumerate(ranges):
        cl = clusters[int(r["first"]):int(r["first"]) + int(r["count"])]
        follows = cl["first"][:-1].astype(np.int64) + cl["count"][:-1] == cl["first"][1:]
        broken = np.nonzero(~follows)[0] + 1                        # the clusters that do not follow their predecessor
        assert set(range(37, len(cl), 37)) <= set(broken.tolist()) and set(xsup.B_BREAKS[g]) <= set(broken.tolist())
        assert len(broken) == len(set(range(37, len(cl), 37)) | set(xsup.B_BREAKS[g]))   # consecutive everywhere else
        assert all(min(b % xsup.SPAN, xsup.SPAN - b % xsup.SPAN) == 1 for b in xsup.B_BREAKS[g])
    table = xsup.world_b().tables[0]
    wrap = clusters[int(ranges[xsup.B_WRAP_GEOMETRY]["first"])]
    assert int(table[xsup.B_WRAP_GEOMETRY]["first"]) + int(wrap["first"]) > 0xFFFFFFFF   # the command's first wraps 32 bits
    bad = clusters[int(ranges[xsup.B_BAD_GEOMETRY]["first"]):]
    assert np.isnan(bad[xsup.B_NAN_CLUSTER]["box_min"][0]) and (bad[xsup.B_INVERTED_CLUSTER]["box_min"] > bad[xsup.B_INVERTED_CLUSTER]["box_max"]).all()


def test_world_b_takes_the_tile_side_past_one_scan_turn_and_two_grid_passes(oracle):
    w, c = xsup.world_b(), candidates_b(oracle)
    tested, kept = int(np.count_nonzero(c.is_cluster)), int(np.count_nonzero(c.is_cluster & c.survives))
    edge = xsup.SCAN_TURN * xsup.TILE
    per_draw_kept = np.bincount(c.draw[(c.view == 0) & c.is_cluster & c.survives], minlength=c.draws[0])
    per_draw = np.bincount(c.draw[(c.view == 0) & c.is_cluster], minlength=c.draws[0])
    partial = int(np.count_nonzero((per_draw_kept > 0) & (per_draw_kept < per_draw)))
    print("world B: blocks", c.blocks, "T", c.total, "tiles", c.tiles, "draws", c.draws, "starts", c.start, "tested", c.tested, "survivors", kept,
          "of them behind tile 4096", int(c.survives[edge:].sum()), "partially kept draws of view 0", partial)
    assert w.occupancy == xsup.B_SLOTS == 300 and c.total >= 1100000
    assert c.tiles > xsup.SCAN_TURN and c.tiles > 2 * WALK and c.tiles % 4 != 0
    assert c.tested[0] >= (1 << 20) + 1 and sum(c.tested) >= (1 << 20) + 1
    assert 5 * kept >= tested and 5 * kept <= 4 * tested and partial >= 1
    assert int(c.survives[edge:].sum()) > 0 and int(c.survives[:edge].sum()) > 0
    assert c.start[1] % xsup.TILE != 0 and c.start[1] // xsup.TILE >= WALK      # view 1 starts mid-tile, in the third pass of the walks
    assert {0, 1, 2, 3, xsup.B_VOID} <= set(w.ids.tolist())
    assert np.count_nonzero(c.g[0] == xsup.B_BAD_GEOMETRY) >= 1                # (the NaN and the inverted box are among the tested clusters)


def test_world_b_run_form_heads_meet_the_same_thresholds(oracle):
    c = candidates_b(oracle)
    head, ends = c.heads()
    at = np.nonzero(head)[0]
    assert len(at) == len(ends) and np.all(ends >= at)
    crossing = (at // xsup.TILE != ends // xsup.TILE) & (at // xsup.TILE >= WALK)
    edge = xsup.SCAN_TURN * xsup.TILE
    print("world B: run heads", len(at), "of them behind tile 4096", int(head[edge:].sum()), "runs across a tile edge behind tile 2048",
          int(crossing.sum()), "longest run", int((ends - at + 1).max()), "last run", int(at[-1]), "to", int(ends[-1]), "T", c.total)
    assert int(head[edge:].sum()) > 0 and int(head[:edge].sum()) > 0          # the head scan's carry matters
    assert int(crossing.sum()) >= 1
    assert int(ends[-1]) + 1 == c.total and int(at[-1]) < int(ends[-1])       # a run of several clusters ends exactly at T
    assert int((ends - at + 1).max()) <= xsup.SPAN and 2 * len(at) <= int(c.survives.sum())


def test_world_b_dense_and_sparse_second_phases(oracle):
    queried = np.array(xsup.world_b().hiz)
    dense, sparse, wall = candidates_b(oracle, "near"), candidates_b(oracle, "dots"), candidates_b(oracle, "wall")
    p_dense, span_dense = dense.widest_pending_tile(queried)
    p_sparse, span_sparse = sparse.widest_pending_tile(queried)
    kept_dense = int(np.count_nonzero(dense.pending(queried) & wall.survives))
    kept_sparse = int(np.count_nonzero(sparse.pending(queried) & wall.survives))
    print("world B: pending dense", p_dense, "pending tiles", xsup.tiles_of(p_dense), "sparse", p_sparse, "of", dense.tested[0],
          "widest pending tile (candidate tiles) dense", span_dense, "sparse", span_sparse, "second-phase survivors dense", kept_dense, "sparse", kept_sparse)
    assert p_dense >= (1 << 20) + 1 and xsup.tiles_of(p_dense) > xsup.SCAN_TURN and xsup.tiles_of(p_dense) > 2 * WALK
    assert 0 < kept_dense < p_dense
    assert 0.005 * sparse.tested[0] <= p_sparse <= 0.02 * sparse.tested[0] and p_sparse > xsup.TILE
    assert span_sparse >= 50                                                   # find_pending searches over 50 and more candidate tiles
    assert 0 < kept_sparse < p_sparse


def test_world_b_lod_cut_and_cones_remove_their_share(oracle):
    c = candidates_b(oracle, "wall", True)
    tested = sum(c.tested)
    print("world B: LOD-kept", c.lod_kept, "of", tested, "cone-rejected", c.cone_rejected, "of", c.cone_seen, "survivors", int(c.survives[c.is_cluster].sum()))
    assert 20 * (tested - c.lod_kept) >= tested and c.lod_kept > 0             # the cut removes 5 % and more of the tested
    assert 20 * c.cone_rejected >= c.cone_seen and c.cone_rejected < c.cone_seen   # the cones 5 % and more of what the tests in front keep
    assert c.tiles > xsup.SCAN_TURN and int(c.survives[xsup.SCAN_TURN * xsup.TILE:].sum()) > 0
