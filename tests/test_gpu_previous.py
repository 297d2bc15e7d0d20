"""gv_pool_keep_models / gv_pool_forget_models / gv_pool_emit_previous on the device: last frame's viewProj * model per draw. Expected
bytes come from the C twin (tests/previous_twin.h) fed the FETCHED records of both frames, and are compared word for word (a NaN as a
class); the twin's history goes through the same keep / forget calls as the library's. tests/test_previous_abi.py asserts on the CPU
tier that every two-frame case holds kept-and-unmoved, kept-and-moved and fresh draws."""
import os
import subprocess

import numpy as np
import pytest

import group_support as gsup
import instances_support as isup
import previous_support as ps
import second_phase_support as sp
from garden_amd import scene
from garden_amd.lib import GV_DIRTY_MESH, GV_DIRTY_TRANSFORM, GV_E_ARG, GV_E_STATE, GpuVisibility, GvError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGGED = ps.layout_dtype(80, 0, 64)    # has_history behind prev_mvp
WIDE = ps.layout_dtype(128, 64, 16)     # prev_mvp in the second half of a {mvp, prevMvp} struct, the flag in the first
BARE = ps.layout_dtype()                # stride 64: the whole-line path


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return ps.build_twin(str(tmp_path_factory.mktemp("previous_twin")))


def context(c):
    return GpuVisibility(device=0, keep_slot_order=c.keep_slot_order, hiz_rg16f=c.rg16f)


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)


def launches(vis):
    return dict(vis.stats()["launches"])


def added(vis, call, *args, **kw):
    before = launches(vis)
    call(*args, **kw)
    after = launches(vis)
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def raw(vis, view_index, n):
    return vis.fetch(view_index, write_back=False, occupancy=n, order="raw", pool_id=0)


def emit(vis, dtype, view_index=0, **kw):
    names = dtype.names
    vis.emit_previous(0, view_index, stride=dtype.itemsize, prev_mvp=dtype.fields["prevMvp"][1],
                      has_history=dtype.fields["hasHistory"][1] if "hasHistory" in names else None, **kw)


def check(vis, dtype, h, view, fetched, epoch=None, what="", **kw):
    """the pool's last emission against the twin's answer over the fetched records; returns has_history as expected"""
    exp_mvp, exp_has, kept = h.expect(view, fetched, **kw)
    items, counts = vis.previous(0, stride=dtype.itemsize)
    n = int(fetched["draw_count"])
    assert counts.tolist() == [n, kept, n, h.epoch if epoch is None else epoch], (what, counts.tolist(), n, kept)
    assert items.shape == (n, dtype.itemsize)
    ps.same_items(items, dtype, exp_mvp, exp_has, what)
    return exp_has


def code(fn, *args, **kw):
    with pytest.raises(GvError) as e:
        fn(*args, **kw)
    return e.value.code


# ---- 1. the case table: two frames -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sp.CASES, ids=lambda c: c.name)
def test_two_frames_of_the_case_table(twin, case):
    c = case
    depth, _ = sp.depth_images(c)
    sc = sp.world(c)
    v1, v2 = ps.first_view(), ps.second_view()
    h = ps.History(twin)
    with context(c) as vis:
        bind(vis, sc)
        vis.hiz_build(depth)
        vis.cull(0, [v1])
        f1 = raw(vis, 0, c.n)
        assert added(vis, emit, vis, FLAGGED) == {"emit": 1}  # (the memset is no launch)
        assert not check(vis, FLAGGED, h, v1, f1, what="frame 1: an empty history").any()
        assert added(vis, vis.keep_models, 0, 0) == {"emit": 1}
        h.keep(v1, f1, c.n)
        for first, count in ps.move(sc):
            vis.mark_dirty(GV_DIRTY_TRANSFORM, first, count)
        vis.cull(0, [v2])
        f2 = raw(vis, 0, c.n)
        assert added(vis, emit, vis, FLAGGED) == {"emit": 1}
        has = check(vis, FLAGGED, h, v2, f2, what="frame 2")
        floor = ps.class_floor(c)
        assert has.sum() >= 2 * floor and (has == 0).sum() >= floor  # (kept holds the unmoved and the moved class)
        assert added(vis, vis.keep_models, 0, 0) == {"emit": 1}
        h.keep(v2, f2, c.n)
        # the same frame again: everything it draws is kept now, against its own matrix
        emit(vis, BARE)
        assert check(vis, BARE, h, v2, f2, what="frame 2 again").all()


# ---- 2. a third frame: stale stamps ----------------------------------------------------------------------------------------------

def test_a_slot_not_seen_last_frame_is_fresh_whatever_older_frames_kept(twin):
    c = sp.CASE_BY_NAME["flat-40000"]
    sc = sp.world(c)
    v1, v2 = scene.main_camera_view(), scene.main_camera_view(seed=scene.SEED + 1)
    h = ps.History(twin)
    with context(c) as vis:
        bind(vis, sc)
        seen = []
        for v in (v1, v2, v1):
            vis.cull(0, [v])
            f = raw(vis, 0, c.n)
            emit(vis, FLAGGED)
            has = check(vis, FLAGGED, h, v, f)
            vis.keep_models(0, 0)
            h.keep(v, f, c.n)
            seen.append((f["visible_idx"][:f["draw_count"]], has))
        (s1, _), (s2, _), (s3, has3) = seen
        only_first = np.isin(s3, s1) & ~np.isin(s3, s2)
        assert only_first.sum() >= 64 and not has3[only_first].any()  # their rows hold epoch 1, the history is at 2
        both = np.isin(s3, s2)
        assert both.sum() >= 64 and has3[both].all()


# ---- 3. the kernels' edges -----------------------------------------------------------------------------------------------------------

def line_world():
    """EDGE_SLOTS entities on a line along x, 10 apart (no box reaches 5 from its pivot), no defects"""
    sc = scene.flat_scene(ps.EDGE_SLOTS, seed=ps.SEED + ps.EDGE_SLOTS, defects=False)
    sc.transforms["position"][:, :3] = 0
    sc.transforms["position"][:, 0] = 10.0 * np.arange(ps.EDGE_SLOTS, dtype=np.float32)
    return sc


def picking(count, step=0.0):
    """an orthographic view that holds exactly entities [0, count) of the line world (count 0: a box beside the line)"""
    width = 10.0 * max(count, 1)
    centre = (0.5 * width - 5.0 + step) if count else -1000.0
    return scene.make_view(scene.ortho_rev_z(width, 50.0, -1000.0, 1000.0), camera_position=(centre, 0.0, 0.0))


@pytest.mark.parametrize("n", ps.EDGE_DRAWS)
def test_edges_of_lane_wave_and_workgroup(twin, n):
    import torch
    sc = line_world()
    half = (n + 1) // 2
    v1, v2 = picking(half), picking(n)
    h = ps.History(twin)
    rng = np.random.Generator(np.random.PCG64(n))
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [v1])
        f1 = raw(vis, 0, sc.count)
        assert f1["draw_count"] == half
        vis.keep_models(0, 0)
        h.keep(v1, f1, sc.count)
        vis.cull(0, [v2])
        f2 = raw(vis, 0, sc.count)
        assert f2["draw_count"] == n
        for dtype in (BARE, FLAGGED, WIDE):
            emit(vis, dtype)
            has = check(vis, dtype, h, v2, f2, what=(n, dtype.itemsize))
            assert has.sum() == half
        vis.emit_previous(0, 0, layout=False)  # a NULL layout is {64, 0, none}
        check(vis, BARE, h, v2, f2, what=(n, "NULL layout"))
        # a caller-owned target cut at 0, 1 and n - 1 items: bytes beyond the cut and between the fields stay
        exp_mvp, exp_has, kept = h.expect(v2, f2)
        mask = isup.field_mask(WIDE)
        for cut in sorted({0, min(1, n), max(n - 1, 0)}):
            pattern = rng.integers(1, 255, (n + 3, WIDE.itemsize), dtype=np.uint8)
            dev = torch.as_tensor(pattern, device="cuda:0")
            torch.cuda.synchronize()  # (the copy runs on torch's stream, the library's stream is non-blocking)
            emit(vis, WIDE, device=(dev.data_ptr(), cut * WIDE.itemsize + WIDE.itemsize - 1))
            assert vis.previous_device(0)[0] == dev.data_ptr()
            host = pattern.copy()
            items, counts = vis.previous(0, out=host, stride=WIDE.itemsize)
            assert counts.tolist() == [n, kept, cut, 1]
            on_device = dev.cpu().numpy()
            for got in (on_device, host):
                assert got[cut:].tobytes() == pattern[cut:].tobytes()
                assert (got[:cut][:, ~mask] == pattern[:cut][:, ~mask]).all()
                ps.same_items(got[:cut], WIDE, exp_mvp, exp_has, (n, cut))


def test_coverage_grows_between_keeps_and_old_rows_survive(twin):
    """the pool is bound with 1000 slots, then with 2048: a slot at H.slots - 1 is kept, one at H.slots is fresh; GV_KEEP_ADD of a
    view that holds only the new slots grows the coverage, and the rows of the old ones are still there a frame later"""
    sc = line_world()
    small = 1000
    v = picking(ps.EDGE_SLOTS)
    h = ps.History(twin)
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        vis.bind_pool(0, sc.meshes[:small])
        vis.cull(0, [v])
        f1 = raw(vis, 0, small)
        assert f1["draw_count"] == small
        vis.keep_models(0, 0)
        h.keep(v, f1, small)
        for first, count in ps.move(sc):
            vis.mark_dirty(GV_DIRTY_TRANSFORM, first, count)
        sc.meshes["isEnabled"][:small - 1] = 0
        vis.bind_pool(0, sc.meshes)  # (a larger occupancy appends to the mirror: the edit of the old slots is reported like any other)
        vis.mark_dirty(GV_DIRTY_MESH, 0, small, pool_id=0)
        vis.cull(0, [v])
        f2 = raw(vis, 0, sc.count)
        assert sorted(f2["visible_idx"].tolist()) == list(range(small - 1, sc.count))
        emit(vis, FLAGGED)
        has = check(vis, FLAGGED, h, v, f2, what="grown pool")
        assert has[f2["visible_idx"] == small - 1].tolist() == [1] and not has[f2["visible_idx"] >= small].any()
        vis.keep_models(0, 0, add=True)
        h.keep(v, f2, sc.count, add=True)
        assert (h.epoch, h.slots) == (1, sc.count)
        sc.meshes["isEnabled"][:] = 1
        vis.mark_dirty(GV_DIRTY_MESH, 0, small, pool_id=0)
        vis.cull(0, [v])
        f3 = raw(vis, 0, sc.count)
        assert f3["draw_count"] == sc.count
        emit(vis, FLAGGED)
        assert check(vis, FLAGGED, h, v, f3, what="a frame later").all()
        # ... and the moved ones among the old slots show frame 1's model, not this frame's
        items, _ = vis.previous(0, stride=FLAGGED.itemsize)
        now, _, _ = ps.History(twin).expect(v, f3)  # (an empty history is a cut: the view's own matrix times this frame's models)
        moved = ps.moved_transforms(sc.count)[f3["visible_idx"]] & (f3["visible_idx"] < small - 1)
        differs = (items.reshape(-1).view(FLAGGED)["prevMvp"].view(np.uint32) != now.view(np.uint32)).any(axis=1)
        assert moved.sum() >= 64 and differs[moved].all() and not differs[~ps.moved_transforms(sc.count)[f3["visible_idx"]]].any()


def test_beside_mvp_in_the_pools_own_instance_buffer(twin):
    c = sp.CASE_BY_NAME["flat-4097"]
    sc = sp.world(c)
    v1, v2 = scene.main_camera_view(), ps.second_view()
    v2["use_hiz"] = 0
    both = np.dtype(dict(names=["mvp", "prevMvp"], formats=[(np.float32, 16)] * 2, offsets=[0, 64], itemsize=128))
    h = ps.History(twin)
    with context(c) as vis:
        bind(vis, sc)
        vis.set_instance_layout(0, stride=128, mvp=0)
        vis.cull(0, [v1])
        vis.keep_models(0, 0)
        h.keep(v1, raw(vis, 0, c.n), c.n)
        vis.cull(0, [v2])
        f2 = raw(vis, 0, c.n)
        vis.emit_instances(0, [0])
        target, _ = vis.instances_device(0)
        _, stride, capacity = vis.instances_info(0)
        vis.emit_previous(0, 0, stride=128, prev_mvp=64, device=(target, capacity * stride))
        got, starts = vis.instances(0, dtype=isup.layout_dtype(128, 0))
        n = int(f2["draw_count"])
        assert starts.tolist() == [0, n] and n > 64
        exp_mvp, _, kept = h.expect(v2, f2)
        assert 0 < kept < n
        ps.same_words(got["mvp"], ps.History(twin).expect(v2, f2)[0], "mvp beside prevMvp")  # (an empty history is a cut: VP * M)
        items, counts = vis.previous(0, stride=128)
        assert counts.tolist() == [n, kept, n, 1]
        ps.same_words(items.reshape(-1).view(both)["prevMvp"], exp_mvp)


# ---- 4. cut --------------------------------------------------------------------------------------------------------------------------

def test_a_cut_and_an_empty_history_equal_the_mvp_of_the_instance_emission(twin):
    c = sp.CASE_BY_NAME["flat-40000"]
    sc = sp.world(c)
    v1, v2 = scene.main_camera_view(), ps.second_view()
    v2["use_hiz"] = 0
    with context(c) as vis:
        bind(vis, sc)
        vis.set_instance_layout(0, stride=64, mvp=0)
        vis.cull(0, [v1])
        vis.emit_instances(0, [0])
        mvp, _ = vis.instances(0)
        vis.emit_previous(0, 0, prev_view_proj=np.full(16, 3.0, np.float32))  # e == 0: a cut whatever is passed
        items, counts = vis.previous(0)
        assert counts.tolist() == [len(mvp), 0, len(mvp), 0] and len(mvp) > 1000
        assert items.tobytes() == mvp.tobytes()
        vis.keep_models(0, 0)
        vis.cull(0, [v2])
        vis.emit_instances(0, [0])
        mvp, _ = vis.instances(0)
        vis.emit_previous(0, 0)
        items, counts = vis.previous(0)
        assert 0 < counts[1] < counts[0] and items.tobytes() != mvp.tobytes()  # (not a cut: the kept matrix and rows)
        vis.emit_previous(0, 0, cut=True, prev_view_proj=np.full(16, 3.0, np.float32))
        items, counts = vis.previous(0)
        assert counts.tolist() == [len(mvp), 0, len(mvp), 1]
        assert items.tobytes() == mvp.tobytes()


# ---- 5. forget -----------------------------------------------------------------------------------------------------------------------

def test_forget_makes_exactly_the_range_fresh_and_count_zero_empties_the_history(twin):
    c = sp.CASE_BY_NAME["flat-40000"]
    sc = sp.world(c)
    v = scene.main_camera_view()
    h = ps.History(twin)
    with context(c) as vis:
        bind(vis, sc)
        vis.cull(0, [v])
        f = raw(vis, 0, c.n)
        slots = f["visible_idx"][:f["draw_count"]]
        vis.keep_models(0, 0)
        h.keep(v, f, c.n)
        lo, count = int(np.sort(slots)[len(slots) // 4]), c.n // 3
        assert added(vis, vis.forget_models, 0, lo, count) == {"emit": 1}
        h.forget(lo, count)
        emit(vis, FLAGGED)
        has = check(vis, FLAGGED, h, v, f, what="a forgotten range")
        inside = (slots >= lo) & (slots < lo + count)
        assert inside.sum() >= 64 and (~inside).sum() >= 64 and has.tolist() == (~inside).astype(np.uint32).tolist()
        assert added(vis, vis.forget_models, 0, c.n - 1, 0xFFFFFFFF) == {"emit": 1}   # clamped to the coverage
        h.forget(c.n - 1, 0xFFFFFFFF)
        assert added(vis, vis.forget_models, 0, c.n, 5) == {}                          # nothing of it is covered
        assert added(vis, vis.forget_models, 0, 0, 0) == {}                            # the whole history: no launch
        h.forget()
        emit(vis, FLAGGED)
        assert not check(vis, FLAGGED, h, v, f, what="an empty history").any() and h.epoch == 0
        assert code(vis.keep_models, 0, 0, add=True) == GV_E_STATE
        vis.keep_models(0, 0)
        h.keep(v, f, c.n)
        emit(vis, FLAGGED)
        assert check(vis, FLAGGED, h, v, f, what="kept again").all() and h.epoch == 1


# ---- 6. two-phase --------------------------------------------------------------------------------------------------------------------

def test_keep_add_behind_a_second_phase_keeps_the_union(twin):
    c = sp.CASE_BY_NAME["flat-40000"]
    a, b = sp.depth_images(c)
    sc = sp.world(c)
    v = sp.view()
    h = ps.History(twin)
    with context(c) as vis:
        bind(vis, sc)
        for frame in range(2):
            vis.hiz_build(a)
            vis.cull(0, [v])
            vis.hiz_build(b)
            vis.cull_second_phase(0, 1, v, pool_id=0)
            first, second = raw(vis, 0, c.n), raw(vis, 1, c.n)
            assert first["draw_count"] > 64 and second["draw_count"] > 64
            for view_index, f in ((0, first), (1, second)):
                emit(vis, FLAGGED, view_index)
                has = check(vis, FLAGGED, h, v, f, what=(frame, view_index))
                assert has.all() == (frame == 1)  # frame 2 draws what frame 1 drew, phase by phase: the union was kept
            vis.keep_models(0, 0)
            h.keep(v, first, c.n)
            vis.keep_models(0, 1, add=True)
            h.keep(v, second, c.n, add=True)
        other = dict(v, camera_position=v["camera_position"] + np.float32(1))
        vis.cull(0, [v, other])
        assert code(vis.keep_models, 0, 1, add=True) == GV_E_STATE  # another camera than the kept one
        vis.keep_models(0, 0, add=True)


# ---- 7. order ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["sort", "sort-descending", "grouped"])
def test_item_k_follows_record_k_of_the_new_order(twin, how):
    c = sp.CASE_BY_NAME["flat-40000"]
    sc = sp.world(c)
    v1, v2 = scene.main_camera_view(), ps.second_view(turn=0.05)  # (frustum only: a wider turn, so that the edges bring fresh draws)
    v2["use_hiz"] = 0
    h = ps.History(twin)
    with context(c) as vis:
        bind(vis, sc)
        if how == "grouped":
            ids = np.random.Generator(np.random.PCG64(c.n)).integers(0, 12, c.n).astype(np.uint32)
            vis.bind_geometry(0, ids, gsup.geometry_table(12))
        for v in (v1, v2):
            vis.cull(0, [v])
            if "sort" in how:
                vis.sort(0, descending=(how == "sort-descending"), pool_id=0)
            else:
                vis.group_draws(0, pool_id=0)
            emit(vis, FLAGGED)                      # (issued before the fetch: the deferred sort is flushed by the call itself)
            f = raw(vis, 0, c.n)
            assert (np.diff(f["visible_idx"].astype(np.int64)) < 0).any()  # the records are NOT in slot order
            has = check(vis, FLAGGED, h, v, f, what=how)
            vis.keep_models(0, 0)
            h.keep(v, f, c.n)
        assert 64 <= has.sum() <= len(has) - 64


# ---- 8. codes on the device (the whole list: tests/test_previous_host.py) ----------------------------------------------------------------

def test_codes_and_the_results_lifetime():
    c = sp.CASE_BY_NAME["flat-257"]
    with context(c) as vis:
        bind(vis, sp.world(c))
        vis.cull(0, [scene.main_camera_view(), dict(scene.cascade_view(index=0), emit_records=0)])
        assert code(vis.previous, 0) == GV_E_STATE
        assert code(vis.emit_previous, 0, 1) == GV_E_STATE and code(vis.keep_models, 0, 1) == GV_E_STATE  # count-only
        assert code(vis.emit_previous, 0, 5) == GV_E_ARG and code(vis.emit_previous, 0, 0, stride=72) == GV_E_ARG
        assert code(vis.emit_previous, 0, 0, device=(4096 + 4, 1 << 20)) == GV_E_ARG
        assert code(vis.previous_device, 0) == GV_E_STATE
        vis.emit_previous(0, 0)
        vis.keep_models(0, 0)
        items, counts = vis.previous(0)
        assert counts[0] == len(items) > 0
        assert code(vis.previous, 0, out=np.zeros((len(items), 64), np.uint8)[:-1]) == GV_E_ARG
        vis.cull(0, [scene.main_camera_view()])
        assert code(vis.previous, 0) == GV_E_STATE     # the result ended with the views
        vis.keep_models(0, 0, add=True)                # the history did not


# ---- 9. the shim -----------------------------------------------------------------------------------------------------------------------

def test_motion_history_shim_five_ticks_against_the_twin():
    exe = os.path.join(ROOT, "tests", "cpp", "build", "motion_history")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "motion_history.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "motion history: 5 ticks, every prevMvp equal to the twin's: ok" in run.stdout, (run.stdout + run.stderr)[-4000:]
