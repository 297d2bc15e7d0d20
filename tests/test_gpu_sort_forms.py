"""Every form the sort dispatch takes beyond the one-launch batch of small pools (gv_sort.hip launch_sort_lists, planned by
gv_sort_kernels.hpp sort_plan), against the oracle's sortMeshes: frames of several mid-sized pools sorted by ONE set of launches
(batch widths 8 and 32, rank-only lists beside radix lists, a list that stays empty), and single pools whose record count sits
exactly on a handover — rank or radix sort (12 288 records), the rank-only launch's key table (16 384), short or long tiles
(524 288). Every list is compared as tests/test_gpu_cull.py::test_gpu_sort_matches_sort_meshes does it: ties canonicalised by
slot, then bit-equal visible_idx, baked_model and distance_sq."""
import functools

import numpy as np
import pytest

from garden_amd import scene

POOL_SLOTS = [16_385, 20_000, 19_999, 18_433, 17_011, 16_500, 17_777, 18_999, 19_321]  # all beyond the one-launch batch (16 384)


def box_view(lo, hi):
    """An orthographic view whose frustum is the axis-aligned box [lo, hi] (camera at the origin, no offset)."""
    m = np.zeros((4, 4), dtype=np.float32)  # m[c][r]
    for a in range(3):
        m[a][a] = (2.0 if a < 2 else 1.0) / (hi[a] - lo[a])
        m[3][a] = -(hi[a] + lo[a]) / (hi[a] - lo[a]) if a < 2 else -lo[a] / (hi[a] - lo[a])
    m[3][3] = 1.0
    return scene.make_view(m.reshape(16))


def scene_side(n):
    return 100.0 * n ** (1.0 / 3.0)  # (scene.flat_scene: positions within +- side / 2)


def kind_view(kind, side):
    """few: a slab of a fifth of the cube (a few thousand records of a 16-20 k pool); most: the whole cube (everything but the
    scene's defects); none: a box beside the cube."""
    if kind == "few":
        return box_view((-side, -side, -side), (-0.3 * side, side, side))
    if kind == "most":
        return box_view((-side, -side, -side), (side, side, side))
    return box_view((3 * side, -side, -side), (4 * side, side, side))


def assert_sorted_as_the_oracle(oracle, got, meshes, sc, view, descending):
    exp = oracle.prepare_meshes(meshes.copy(), sc.transforms, sc.entity_to_transform, view, sort="descending" if descending else "ascending")
    assert got["draw_count"] == exp["draw_count"]
    if exp["draw_count"] == 0:
        assert got["visible_idx"].shape == (0,)
        return 0
    d = got["distance_sq"]
    assert np.all(d[:-1] >= d[1:]) if descending else np.all(d[:-1] <= d[1:])
    o = np.lexsort((got["visible_idx"], -d if descending else d))  # ties: canonical by slot
    assert np.array_equal(got["visible_idx"][o], exp["visible_idx"])
    assert np.array_equal(got["baked_model"][o].view(np.uint32), exp["baked_model"].view(np.uint32))
    assert np.array_equal(got["distance_sq"][o].view(np.uint32), exp["distance_sq"].view(np.uint32))
    return int(exp["draw_count"])


KINDS = ("few", "most", "none")
# Frame 1 repeats frame 0: its short and empty lists are now expected short (rank-only). Frame 2 moves every kind on, frame 3
# repeats frame 2. A list with index 2 (mod 3) so goes: nothing (its first sort) - nothing (rank-only) - nearly all (rank-only,
# ranked from memory) - nearly all (the radix passes, on counters it last used in frame 0 and sat beside ever since).
FRAME_SHIFTS = (0, 0, 2, 2)


def frame_lists(k):
    """the (pool, view) lists of a frame of k pools: one view per pool, and with fewer than three pools a second view of the last
    pool, so that every frame holds a short, a long and an empty list"""
    return [(p, 0) for p in range(k)] + ([(k - 1, 1)] if k < 3 else [])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 8, 9])  # one batch of up to 8 lists, a full one, the first of the 32-wide form
def test_frames_of_mid_sized_pools_sort_by_one_set_of_launches(oracle, k):
    """k pools of 16 385 - 20 000 slots, every one sorted, flushed by the first fetch of the frame as ONE batch (k = 2: three
    lists, the second pool under two views). List i of frame f sees KINDS[(i + shift) % 3]: a few thousand records, nearly all,
    nothing - all three in every frame - ascending and descending alternating by list and by frame. Frame 0 is every list's first
    sort (the device's count picks rank sort or radix passes). In frame 1 the short and the empty lists take the rank-only form
    beside lists the radix passes sort. Frame 2 hands a rank-only list nearly all records (the from-memory form) and a radix list
    a short one. In frame 3 that formerly rank-only list is expected long and takes the radix passes again: its counter set must
    still be zero and its parity right after two batches it sat out behind sort_rank_body<FIRST>'s zeroing."""
    from garden_amd.lib import GpuVisibility
    sc = scene.flat_scene(20_000, seed=41)
    side = scene_side(20_000)
    pools = [sc.meshes[:n].copy() for n in POOL_SLOTS[:k]]
    lists = frame_lists(k)
    with GpuVisibility(device=0, profile_events=True) as vis:
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        for p, meshes in enumerate(pools):
            vis.bind_pool(p, meshes)
        vis.hierarchy_rebuild()
        for f, shift in enumerate(FRAME_SHIFTS):
            kinds = [KINDS[(i + shift) % 3] for i in range(len(lists))]
            views = [kind_view(kind, side) for kind in kinds]
            assert set(kinds) == set(KINDS)
            vis.stats_reset()
            for p in range(k):
                vis.cull(p, [views[i] for i, (q, _) in enumerate(lists) if q == p])
                for i, (q, v) in enumerate(lists):
                    if q == p:
                        vis.sort(v, descending=(i + f) % 2 == 1, pool_id=p)
            got = [vis.fetch(v, write_back=False, occupancy=POOL_SLOTS[p], pool_id=p, order="raw") for p, v in lists]
            assert vis.stats()["launches"]["sort"] == 1  # all the lists by one flush
            for i, (p, v) in enumerate(lists):
                count = assert_sorted_as_the_oracle(oracle, got[i], pools[p], sc, views[i], (i + f) % 2 == 1)
                print(f"frame {f} pool {p} view {v} ({POOL_SLOTS[p]} slots) {kinds[i]}: {count} records")
                if kinds[i] == "few":
                    assert 1000 < count <= 10_240  # (at most kRankOnlyHintRecords: rank-only in the next frame)
                elif kinds[i] == "most":
                    assert 12_288 < count < POOL_SLOTS[p]  # (beyond kRankSortMaxRecords: the radix passes, or rank-only from memory)
                else:
                    assert count == 0


# ---- exact handovers on one pool ----

# name: (slots, records m, a frame with a short list in front)
HANDOVERS = {
    "rank_sort_takes_it": (16_385, 12_288, False),   # kSortBoth on the pool's first sort: the device's count picks the rank sort ...
    "radix_takes_it": (16_385, 12_289, False),       # ... or the radix passes
    "rank_only_table_full": (20_000, 16_384, True),  # rank-only: the last count the LDS key table holds ...
    "rank_only_from_memory": (20_000, 16_385, True),  # ... and the first that is ranked from memory
    "last_short_tiles": (524_300, 524_288, False),   # 1024-key tiles up to kSortShortRecords ...
    "first_long_tiles": (524_300, 524_289, False),   # ... 4096-key tiles beyond
}


@functools.lru_cache(maxsize=2)
def handover_scene(n, m):
    """n entities without defects, exactly m of them (random slots) inside the cube the views look at, the rest 10^7 away"""
    sc = scene.flat_scene(n, seed=77 + n, defects=False)
    rng = np.random.Generator(np.random.PCG64(m))
    outside = rng.permutation(n)[m:]
    sc.transforms["position"][outside, 0] += np.float32(1e7)
    return sc


def handover_views(n):
    side = scene_side(n)
    return kind_view("few", side), kind_view("most", side)


@pytest.mark.parametrize("name", list(HANDOVERS))
def test_handover_scenes_hold_exactly_the_intended_count(oracle, name):
    """with the oracle alone: the view box holds exactly m entities, the short list in front at most kRankOnlyHintRecords"""
    n, m, short_first = HANDOVERS[name]
    sc = handover_scene(n, m)
    short, whole = handover_views(n)
    assert oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, whole)["draw_count"] == m
    if short_first:
        assert 0 < oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, short)["draw_count"] <= 10_240


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HANDOVERS))
def test_sort_at_an_exact_handover(oracle, name):
    n, m, short_first = HANDOVERS[name]
    from garden_amd.lib import GpuVisibility
    sc = handover_scene(n, m)
    short, whole = handover_views(n)
    with GpuVisibility(device=0) as vis:  # (a context of its own: the view's first sort, no count from an earlier test)
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        vis.bind_pool(0, sc.meshes)
        vis.hierarchy_rebuild()
        for f, view in enumerate(([short] if short_first else []) + [whole]):
            vis.cull(0, [view])
            vis.sort(0, descending=f % 2 == 1)
            got = vis.fetch(0, write_back=False, occupancy=n, order="raw")
            count = assert_sorted_as_the_oracle(oracle, got, sc.meshes, sc, view, f % 2 == 1)
        assert count == m
