"""gv_pool_emit_draw_commands on the device: one indirect command per draw (or per run of draws of one geometry) of the pool's last
instance emission, in the caller's command struct. Every comparison is byte for byte against the numpy restatement of the rule
(tests/commands_support.py) over a 0xA5 background, the bytes behind the last written position included.

The world is a flat pool of N small boxes at random positions, all inside the enclosing main view, so draw_count == N; every case
asserts that, and that visible_idx is not the identity (the mirror's Morton order is in play) — except N == 1, whose only order IS
the identity."""
import json
import os
import subprocess

import numpy as np
import pytest

import commands_support as csup
import instances_support as isup
from garden_amd import scene
from garden_amd.lib import (GV_COMMANDS_MERGE_RUNS, GV_DIRTY_GEOMETRY, GV_DIRTY_MESH, GV_E_ARG, GV_E_STATE, GV_MAX_DRAW_INSTANCES,
                            GV_MAX_GEOMETRIES, GpuVisibility, GvError, GvGeometry)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, CHUNK = 256, 4096  # kCommandBlock, kDrawChunk


def enclosing_main(half=1.0e7):
    """the main pass as an orthographic view that holds the whole scene: every box becomes a draw"""
    return scene.make_view(scene.ortho_rev_z(2 * half, 2 * half, -half, half), shadow_pass=-1)


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()


def fetch_all(vis, pool_id, listed, occupancy):
    return [vis.fetch(v, write_back=False, occupancy=occupancy, order="raw", pool_id=pool_id) for v in listed]


def whole_world(fetched, n):
    """the case is the size it claims to be, and in the mirror's order"""
    assert int(fetched["draw_count"]) == n
    if n > 1:
        assert fetched["visible_idx"][:n].tolist() != list(range(n))


def instance_starts(vis, pool_id):
    import ctypes as C
    views = vis.instances_info(pool_id)[0]
    starts = np.zeros(views + 1, np.uint32)
    vis._check(vis.lib.gv_pool_instances_fetch(vis.ctx, pool_id, None, 0, starts.ctypes.data_as(C.POINTER(C.c_uint32)), len(starts)))
    return starts


def random_table(count, seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    return csup.geometry_table([(int(rng.integers(1, 1 << 20)), int(rng.integers(0, 1 << 30)), int(rng.integers(-(1 << 20), 1 << 20)))
                                for _ in range(count)])


def launches(vis):
    return sum(vis.stats()["launches"].values())


def check(vis, listed, occupancy, ids, table, dtype, merge=False, region=0, held=None, own=True, draws=False, pool_id=0):
    """Emits the commands of the pool's last instance emission (which listed `listed`; draws: it was a draw emission) — own: into
    caller-owned device memory over the background, cut after `held` positions when given — and compares every byte on the device
    and of a host fetch, and the counts, with the restatement. Returns (expected bytes, counts, the fetched results)."""
    import torch
    fetched = fetch_all(vis, pool_id, listed, occupancy)
    starts = instance_starts(vis, pool_id)
    bases = vis.draw_bases(pool_id) if draws else None
    stride = dtype.itemsize
    rows = (len(listed) * region if region else sum(int(f["draw_count"]) for f in fetched)) + 7
    pattern = csup.background(rows, stride)
    exp, counts = csup.expected(fetched, starts, bases, ids, table, dtype, merge, region, held, pattern)
    vis.set_command_layout(pool_id, dtype=dtype)
    if own:
        dev = torch.full((rows, stride), csup.BACKGROUND, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # (torch's stream; the library's stream is non-blocking)
        vis.emit_draw_commands(pool_id, merge, region, device=(dev.data_ptr(), rows * stride if held is None else held * stride + 5))
        assert vis.draw_commands_device(pool_id)[0] == dev.data_ptr()
    else:
        assert held is None
        vis.emit_draw_commands(pool_id, merge, region)
    host = pattern.copy()
    _, got_counts = vis.draw_commands(pool_id, out=host)  # waits for the emission
    assert got_counts.tolist() == counts.tolist()  # (the true counts, also when the target is too small or a region is cut)
    assert host.tobytes() == exp.tobytes()
    if own:
        assert dev.cpu().numpy().tobytes() == exp.tobytes()
    return exp, counts, fetched


def runs_of(exp, dtype, count, n):
    """(head draws, run lengths) of the first `count` expected commands of a view of n draws (a layout with the draw field)"""
    heads = exp[:count].reshape(-1).view(dtype)["draw"].astype(np.int64)
    return heads, np.diff(np.concatenate([heads, [n]]))


def code(fn, *args, **kw):
    with pytest.raises(GvError) as e:
        fn(*args, **kw)
    return e.value.code


# ---- 1. per-draw mode at workgroup and chunk edges -----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_per_draw_commands_at_workgroup_and_chunk_edges(n):
    """the 20-byte indexed layout; after emit_instances (first_k = k), then after emit_draw_instances with ready counts drawn from
    0 .. 5 plus one 65 535, changed and marked after the cull so that every box stays a draw"""
    sc = scene.flat_scene(n, defects=False)
    rng = np.random.Generator(np.random.PCG64(n))
    ids = rng.integers(0, 7, n, dtype=np.uint32)
    table = random_table(7)
    ready = np.ones(n, np.uint32)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.bind_geometry(0, ids, table)
        vis.cull(0, [enclosing_main()])
        whole_world(fetch_all(vis, 0, [0], n)[0], n)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        check(vis, [0], n, ids, table, csup.INDEXED)
        check(vis, [0], n, ids, table, csup.INDEXED, own=False)
        ready[:] = rng.integers(0, 6, n, dtype=np.uint32)
        ready[n // 2] = GV_MAX_DRAW_INSTANCES
        vis.mark_dirty(GV_DIRTY_MESH, 0, n, pool_id=0)
        vis.emit_draw_instances(0, [0])
        exp, counts, fetched = check(vis, [0], n, ids, table, csup.INDEXED, draws=True)
        whole_world(fetched[0], n)
        got = exp[:n].reshape(-1).view(csup.INDEXED)
        assert counts.tolist() == [n] and got["instance_count"].tolist() == ready[fetched[0]["visible_idx"]].tolist()


# ---- 2. layouts -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("layout", ["plain16", "gaps32", "wide64"])
def test_layouts_every_byte_of_the_stride(layout, merge):
    """16 bytes without vertex_offset; 32 bytes with `draw` and gaps, which must read 0; stride 64"""
    n = 777
    dtype = {"plain16": csup.PLAIN, "gaps32": csup.GAPS, "wide64": csup.WIDE}[layout]
    sc = scene.flat_scene(n, defects=False)
    ids = (np.arange(n, dtype=np.uint32) // 3) % 5
    table = random_table(5)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, ids, table)
        vis.cull(0, [enclosing_main()])
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        exp, counts, fetched = check(vis, [0], n, ids, table, dtype, merge)
        whole_world(fetched[0], n)
        if layout == "gaps32":
            raw = exp[:int(counts[0])]
            assert not raw[:, 0:4].any() and not raw[:, 24:28].any() and raw[:, 4:8].any()


# ---- 3. run mode ----------------------------------------------------------------------------------------------------------------

def run_sequence(case, n):
    """(ids in DRAW order, the edges a run of length >= 2 must cross, whether a run of length 1 must exist)"""
    k = np.arange(n)
    if case == "all_equal":  # one command: a run across both chunk edges (and no run of length 1: there is only the one)
        return np.full(n, 5), [BLOCK, CHUNK, 2 * CHUNK], False
    if case == "no_neighbours_equal":
        return k % 3, [], True
    if case == "boundaries_at_the_edges":  # runs end exactly at 255|256, 256|257, 4095|4096, 4096|4097
        seq = np.full(n, 2)
        seq[BLOCK], seq[CHUNK] = 4, 1
        return seq, [2 * BLOCK, 2 * CHUNK], True
    if case == "one_long_run":  # draws 200 .. 4499, single draws around it
        seq = (k % 2) * 2
        seq[200:4500] = 1
        return seq, [BLOCK, CHUNK], True
    assert case == "random_runs"
    rng = np.random.Generator(np.random.PCG64(77))
    lengths = rng.geometric(0.3, n)
    seq = np.repeat(np.arange(len(lengths)) % 6, lengths)[:n]
    seq[BLOCK - 6:BLOCK + 6], seq[CHUNK - 6:CHUNK + 6] = 6, 7  # (ids of their own: these runs cross the edges whatever the draw gave)
    return seq, [BLOCK, CHUNK], True


@pytest.mark.parametrize("case", ["all_equal", "no_neighbours_equal", "boundaries_at_the_edges", "one_long_run", "random_runs"])
def test_run_mode_across_workgroup_and_chunk_edges(case):
    n = 8193
    sc = scene.flat_scene(n, defects=False)
    seq, crossed, single = run_sequence(case, n)
    table = random_table(8)
    ready = np.ones(n, np.uint32)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, [enclosing_main()])
        order = fetch_all(vis, 0, [0], n)[0]
        whole_world(order, n)
        ids = np.zeros(n, np.uint32)
        ids[order["visible_idx"]] = seq  # draw k has id seq[k]
        vis.bind_geometry(0, ids, table)
        vis.set_instance_layout(0, dtype=isup.BARE)
        draws = case == "random_runs"
        if draws:  # zero-count draws inside runs
            ready[:] = np.random.Generator(np.random.PCG64(3)).integers(0, 4, n, dtype=np.uint32)
            vis.mark_dirty(GV_DIRTY_MESH, 0, n, pool_id=0)
            vis.emit_draw_instances(0, [0])
        else:
            vis.emit_instances(0, [0])
        exp, counts, _ = check(vis, [0], n, ids, table, csup.GAPS, merge=True, draws=draws)
        heads, lengths = runs_of(exp, csup.GAPS, int(counts[0]), n)
        for edge in crossed:  # a run of length >= 2 lies across the edge
            inside = np.nonzero((heads < edge) & (heads + lengths > edge))[0]
            assert len(inside) == 1 and lengths[inside[0]] >= 2, edge
        assert (lengths == 1).any() == single
        if case == "all_equal":
            assert counts.tolist() == [1]
        if case == "no_neighbours_equal":
            assert counts.tolist() == [n]
        if case == "boundaries_at_the_edges":
            assert heads.tolist() == [0, BLOCK, BLOCK + 1, CHUNK, CHUNK + 1]
        if case == "one_long_run":
            assert 200 in heads.tolist() and lengths[heads.tolist().index(200)] == 4300
        if draws:
            got = exp[:int(counts[0])].reshape(-1).view(csup.GAPS)
            zero_inside = (ready[order["visible_idx"]] == 0) & ~np.isin(np.arange(n), heads)
            assert zero_inside.any() and int(got["instance_count"].sum()) == int(ready.sum())
        check(vis, [0], n, ids, table, csup.INDEXED, merge=True, own=False, draws=draws)


# ---- 4. views -------------------------------------------------------------------------------------------------------------------

def three_views(side):
    """the enclosing main pass, a cascade over the middle of the world, a cascade that looks at nothing"""
    part = scene.make_view(scene.ortho_rev_z(0.7 * side, 0.7 * side, -side, side), shadow_pass=0)
    nothing = scene.make_view(scene.ortho_rev_z(10.0, 10.0, -5.0, 5.0), camera_position=(50.0 * side, 0.0, 0.0), shadow_pass=1)
    return [enclosing_main(), part, nothing]


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("placement", ["packed", "regions_padded", "regions_cut", "own_target_cut_inside_a_region"])
def test_views_are_placed_and_never_merged(placement, merge):
    n = 3000
    sc = scene.flat_scene(n, defects=False)
    side = 100.0 * n ** (1.0 / 3.0)
    listed = [0, 2, 1]  # the empty view between the two others
    table = random_table(6)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, three_views(side))
        fetched = fetch_all(vis, 0, listed, n)
        whole_world(fetched[0], n)
        seen = int(fetched[2]["draw_count"])
        assert int(fetched[1]["draw_count"]) == 0 and 100 < seen < n - 100
        ids = (np.arange(n, dtype=np.uint32) // 2) % 5
        last, first = int(fetched[0]["visible_idx"][n - 1]), int(fetched[2]["visible_idx"][0])
        ids[last] = ids[first] = 5  # view 0's last id equals the next view's first: two commands all the same
        vis.bind_geometry(0, ids, table)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, listed)
        region, held = {"packed": (0, None), "regions_padded": (n + 10, None), "regions_cut": (100, None),
                        "own_target_cut_inside_a_region": (300, 350)}[placement]
        exp, counts, _ = check(vis, listed, n, ids, table, csup.GAPS, merge, region, held)
        if not merge:
            assert counts.tolist() == [n, 0, seen]
        else:
            assert counts[1] == 0 and 1 < counts[0] < n and 1 < counts[2] < seen
        got = exp.reshape(-1).view(csup.GAPS)
        if placement == "packed":  # the two views' neighbouring commands carry the same geometry and stay two
            a, b = got[int(counts[0]) - 1], got[int(counts[0])]
            assert a["count"] == b["count"] == table["count"][5] and b["draw"] == 0 and b["first_instance"] == n
        if placement == "regions_padded":
            assert not exp[int(counts[0]):region].any() and not exp[region:2 * region].any() and got["first_instance"][2 * region] == n
        if placement == "regions_cut":
            assert (got["count"][:3 * region:region] != 0).tolist() == [True, False, True]
        check(vis, listed, n, ids, table, csup.INDEXED, merge, region, own=False)


# ---- 5. a sorted view -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("merge", [False, True])
def test_commands_follow_the_sorted_order(merge):
    n = 5000
    sc = scene.flat_scene(n, defects=False)
    ids = np.arange(n, dtype=np.uint32) % 3
    ids[::7] = 1
    table = random_table(3)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, ids, table)
        vis.cull(0, [enclosing_main()])
        unsorted = fetch_all(vis, 0, [0], n)[0]["visible_idx"].copy()
        vis.sort(0, pool_id=0)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        _, _, fetched = check(vis, [0], n, ids, table, csup.GAPS, merge)
        whole_world(fetched[0], n)
        assert (np.diff(fetched[0]["distance_sq"]) >= 0).all() and fetched[0]["visible_idx"].tolist() != unsorted.tolist()


# ---- 6. currency ----------------------------------------------------------------------------------------------------------------

def test_ids_changed_after_the_cull_are_seen_and_uploads_are_what_the_rule_says():
    n = 6000
    sc = scene.flat_scene(n, defects=False)
    rng = np.random.Generator(np.random.PCG64(9))
    ids = rng.integers(0, 4, n, dtype=np.uint32)
    table = random_table(4)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, ids, table)
        vis.cull(0, [enclosing_main()])
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        uploaded = lambda: vis.stats()["upload_bytes"]
        before = uploaded()
        _, _, fetched = check(vis, [0], n, ids, table, csup.INDEXED)
        whole_world(fetched[0], n)
        assert uploaded() - before == n * 4  # the first command emission uploads the column
        for kind in (GV_DIRTY_GEOMETRY, GV_DIRTY_MESH):
            # three single slots: one packet [ids | slots]
            before = uploaded()
            for slot in (5, 900, 4000):
                ids[slot] = (ids[slot] + 1) % 4
                vis.mark_dirty(kind, slot, 1, pool_id=0)
            check(vis, [0], n, ids, table, csup.INDEXED, merge=True)
            assert uploaded() - before == 3 * 8
            # 2 048 contiguous slots: one copy into their place
            before = uploaded()
            ids[1000:3048] = (ids[1000:3048] + 2) % 4
            vis.mark_dirty(kind, 1000, 2048, pool_id=0)
            check(vis, [0], n, ids, table, csup.INDEXED)
            assert uploaded() - before == 2048 * 4
            before = uploaded()
            check(vis, [0], n, ids, table, csup.INDEXED)  # nothing marked: nothing travels
            assert uploaded() == before
        # a table-only rebind: the new table is seen (and the mirror is uploaded anew)
        other = random_table(4, seed=12)
        before = uploaded()
        vis.bind_geometry(0, ids, other)
        assert uploaded() - before == 4 * 12
        check(vis, [0], n, ids, other, csup.INDEXED)
        assert uploaded() - before == 4 * 12 + n * 4
        # gv_sync consumes the marks too (the mesh marks above are consumed by it as well: a sync in front settles them)
        vis.sync()
        ids[[7, 8]] = (ids[[7, 8]] + 1) % 4
        vis.mark_dirty(GV_DIRTY_GEOMETRY, 7, 2, pool_id=0)
        before = uploaded()
        vis.sync()
        assert uploaded() - before == 2 * 8
        before = uploaded()
        check(vis, [0], n, ids, other, csup.INDEXED, merge=True)
        assert uploaded() == before


# ---- 7. ids outside the table ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("merge", [False, True])
def test_ids_outside_the_table_give_void_commands(merge):
    n = 1500
    sc = scene.flat_scene(n, defects=False)
    table = random_table(4)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [enclosing_main()])
        order = fetch_all(vis, 0, [0], n)[0]
        whole_world(order, n)
        seq = np.arange(n, dtype=np.uint32) % 4
        seq[10:13] = 4             # the first id outside, three neighbours
        seq[300:302] = 0xFFFFFFFF  # two neighbours with the same bad id ...
        seq[302] = 0xFFFFFFFE      # ... and another bad one beside them
        seq[1000] = 70000
        ids = np.zeros(n, np.uint32)
        ids[order["visible_idx"]] = seq
        vis.bind_geometry(0, ids, table)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        exp, counts, _ = check(vis, [0], n, ids, table, csup.GAPS, merge)
        got = exp[:int(counts[0])].reshape(-1).view(csup.GAPS)
        void = got[np.isin(got["draw"], [10, 300, 302, 1000])]
        assert len(void) == 4 and not void["count"].any() and not void["instance_count"].any() and not void["first"].any()
        assert void["first_instance"].tolist() == [10, 300, 302, 1000]
        assert (11 in got["draw"].tolist()) == (not merge) and (301 in got["draw"].tolist()) == (not merge)


# ---- 8. id widths, and no id column ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("column", ["u8", "u16_strided", "u32", "none"])
def test_id_widths_and_no_id_column(column):
    n = 700
    sc = scene.flat_scene(n, defects=False)
    rng = np.random.Generator(np.random.PCG64(21))
    table = random_table(1 if column == "none" else 300)
    if column == "none":
        ids = None
    elif column == "u8":
        ids = rng.integers(0, 256, n, dtype=np.uint8)
    elif column == "u16_strided":  # a field of a component array
        component = np.zeros(n, np.dtype([("other", np.uint32), ("geometry", np.uint16), ("more", np.uint16)]))
        component["other"], component["more"] = 0xDEADBEEF, 0xFFFF
        component["geometry"] = rng.integers(0, 400, n, dtype=np.uint16)
        ids = component["geometry"]
    else:
        ids = rng.integers(0, 400, n, dtype=np.uint32)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, ids, table)
        vis.cull(0, [enclosing_main()])
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        before = vis.stats()["upload_bytes"]
        for merge in (False, True):
            exp, counts, fetched = check(vis, [0], n, ids, table, csup.INDEXED, merge)
            whole_world(fetched[0], n)
        if column == "none":
            assert counts.tolist() == [1] and vis.stats()["upload_bytes"] == before  # one run of table[0]; no mirror is kept
        else:
            assert vis.stats()["upload_bytes"] - before == n * 8  # (fewer than 2 048 slots: they travel as one packet [ids | slots])


# ---- 9. a pool with an index map -------------------------------------------------------------------------------------------------

def test_ids_are_read_by_pool_slot_under_an_index_map():
    n = 900
    sc = scene.flat_scene(n, defects=False)
    ids = np.arange(n, dtype=np.uint32) % 11
    table = random_table(11)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.set_index_map(0, (np.arange(n, dtype=np.uint32)[::-1] + 5000).copy())
        vis.bind_geometry(0, ids, table)
        vis.cull(0, [enclosing_main()])
        vis.set_instance_layout(0, dtype=isup.FULL)  # (with the slot field: the instances carry the MAPPED slot)
        vis.emit_instances(0, [0])
        for merge in (False, True):
            _, _, fetched = check(vis, [0], n, ids, table, csup.INDEXED, merge)
            whole_world(fetched[0], n)


# ---- 10. nothing else moves -------------------------------------------------------------------------------------------------------

def test_results_and_instances_stay_and_launches_are_counted():
    n = 5000
    sc = scene.flat_scene(n, defects=False)
    ids = np.arange(n, dtype=np.uint32) % 3
    table = random_table(3)
    views = [enclosing_main(), scene.cascade_view(index=0, size=400.0)]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, ids, table)
        vis.cull(0, views)
        vis.set_instance_layout(0, dtype=isup.FULL)
        vis.emit_instances(0, [0, 1])
        vis.set_command_layout(0, dtype=csup.INDEXED)
        results, (instances, starts) = fetch_all(vis, 0, [0, 1], n), vis.instances(0)
        whole_world(results[0], n)
        vis.emit_draw_commands(0)  # (the first one uploads the ids: a scatter or copies, not counted as launches)
        vis.wait()
        for merge, grown in ((False, 1), (True, 3)):
            before = launches(vis)
            vis.emit_draw_commands(0, merge_runs=merge)
            assert launches(vis) - before == grown
            vis.draw_commands(0)
            for a, b in zip(results, fetch_all(vis, 0, [0, 1], n)):
                isup.same_results(a, b)
            again, again_starts = vis.instances(0)
            assert again.tobytes() == instances.tobytes() and again_starts.tolist() == starts.tolist()


# ---- 11. errors -------------------------------------------------------------------------------------------------------------------

def test_error_codes_each_followed_by_a_correct_emission():
    import torch
    n = 1200
    sc = scene.flat_scene(n, defects=False)
    ids = np.arange(n, dtype=np.uint32) % 3
    table = random_table(3)
    views = [enclosing_main(), scene.cascade_view(index=0, size=400.0)]
    indexed = {name: csup.INDEXED.fields[name][1] for name in csup.INDEXED.names}
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, views)
        vis.set_instance_layout(0, dtype=isup.BARE)

        def good():
            vis.bind_geometry(0, ids, table)
            vis.emit_instances(0, [0, 1])
            check(vis, [0, 1], n, ids, table, csup.INDEXED, merge=True)

        # gv_pool_bind_geometry
        bad_width = np.zeros((n, 3), np.uint8)
        lib, ctx = vis.lib, vis.ctx
        rows = (GvGeometry * 3)()
        for args in ((99, ids.ctypes.data, 4, 4, n, rows, 3),        # a pool out of range
                     (0, bad_width.ctypes.data, 3, 3, n, rows, 3),   # a width other than 1, 2 or 4
                     (0, ids.ctypes.data, 2, 4, n, rows, 3),         # stride < width
                     (0, ids.ctypes.data, 4, 4, n, None, 3),         # a NULL table with table_count > 0
                     (0, ids.ctypes.data, 4, 4, n, rows, 0),         # table_count 0 with ids
                     (0, ids.ctypes.data, 4, 4, n, rows, GV_MAX_GEOMETRIES + 1)):
            assert lib.gv_pool_bind_geometry(ctx, *args) == GV_E_ARG, args
        good()
        # gv_pool_set_command_layout
        for change in (dict(stride=12), dict(stride=68), dict(stride=22), dict(count=2), dict(first=20), dict(first_instance=4),
                       dict(draw=8), dict(vertex_offset=0)):
            assert code(vis.set_command_layout, 0, offsets=dict(dict(indexed, stride=20), **change)) == GV_E_ARG, change
        assert code(vis.set_command_layout, 99, dtype=csup.INDEXED) == GV_E_ARG
        good()
        # gv_pool_emit_draw_commands: GV_E_ARG
        dev = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
        assert code(vis.emit_draw_commands, 99) == GV_E_ARG                                   # a pool out of range
        assert code(vis.emit_draw_commands, 0, flags=2) == GV_E_ARG                           # unknown flag bits
        assert code(vis.emit_draw_commands, 0, flags=GV_COMMANDS_MERGE_RUNS | 0x80000000) == GV_E_ARG
        assert code(vis.emit_draw_commands, 0, device=(dev.data_ptr() + 4, 1024)) == GV_E_ARG  # a misaligned dst_device
        assert code(vis.emit_draw_commands, 0, region=0x80000000) == GV_E_ARG                 # m * R beyond 32 bits (m = 2)
        good()
        # ... GV_E_STATE
        vis.set_command_layout(0)
        assert code(vis.emit_draw_commands, 0) == GV_E_STATE                                  # no command layout
        vis.set_command_layout(0, dtype=csup.INDEXED)
        vis.bind_geometry(0, None, None)
        assert code(vis.emit_draw_commands, 0) == GV_E_STATE                                  # no geometry bound
        vis.bind_geometry(0, ids[:n - 1], table)
        assert code(vis.emit_draw_commands, 0) == GV_E_STATE                                  # an id column below a view's occupancy
        vis.bind_geometry(0, ids, table)
        vis.cull(0, views)
        assert code(vis.emit_draw_commands, 0) == GV_E_STATE                                  # no emission since the last gv_cull
        assert code(vis.draw_commands_device, 0) == GV_E_STATE
        good()
        # the fetch: too small an array writes nothing
        import ctypes as C
        small, counts = np.full(40, csup.BACKGROUND, np.uint8), np.full(2, 0xA5A5A5A5, np.uint32)
        cp = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        assert lib.gv_pool_draw_commands_fetch(ctx, 0, small.ctypes.data, small.nbytes, cp, 2) == GV_E_ARG
        assert lib.gv_pool_draw_commands_fetch(ctx, 0, None, 0, cp, 1) == GV_E_ARG
        assert (small == csup.BACKGROUND).all() and (counts == 0xA5A5A5A5).all()
        # an instance emission ends the commands made from the one before
        vis.emit_instances(0, [0])
        assert code(vis.draw_commands_device, 0) == GV_E_STATE
        good()


# ---- 12. the drop-in's shim -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def draw_commands_driver(tmp_path_factory):
    """tests/cpp/draw_commands.cpp, built with the flags of the headless_tick rule of tests/cpp/Makefile"""
    cpp, lib = os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "garden_amd", "lib")
    exe = str(tmp_path_factory.mktemp("draw_commands") / "draw_commands")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-invalid-offsetof", "-fno-strict-aliasing", "-march=haswell",
                    "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(cpp, "draw_commands.cpp"),
                    "-o", exe, "-L" + lib, "-lgarden_vis", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64",
                    "-lm", "-lpthread"], check=True)
    return exe


def test_draw_commands_shim_matches_the_host_loop(draw_commands_driver):
    """GpuInstanceWriter + GpuDrawCommands of the drop-in against a host loop over the records in draw order (mesh.cpp:589-601)
    that writes the same structs: 30 000 entities in three mesh systems (one geometry without a column, 16 geometries, sorted),
    main pass + three cascades, 20 ticks with movers and geometry switches — every command array byte for byte, in both modes."""
    p = subprocess.run([draw_commands_driver, "--entities", "30000", "--ticks", "20"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["systems"] == 3 and out["passes"] == 4 and out["ticks"] == 20 and out["commands"] > 100_000, out
