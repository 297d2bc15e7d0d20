"""gv_pool_emit_draw_instances on the device: draw k of a view takes its ready count of instances (gv_pool_bind_ready), read from
the count mirror, as `instanceCount.fetch_add(getInstancesAsync(view))` hands them out in the reference's draw loops (mesh.cpp:596-599).
Everything is byte-exact. Expected values: the per-record bytes of gv_pool_emit_instances (the C twin of DESIGN.md §4 item 9 over the
fetched records, instances_support.expected), expanded with np.repeat by the counts; bases by an exclusive cumsum, which must also
equal the host's gv_pool_results_instance_bases plus starts[v]; starts[v + 1] - starts[v] must equal GvResult.instance_count.
Targets are caller-owned device memory over a non-zero background, so the bytes nobody may write are compared too."""
import numpy as np
import pytest

import instances_support as isup
from garden_amd import scene
from garden_amd.lib import (GV_E_ARG, GV_E_STATE, GV_MAX_DRAW_INSTANCES, GpuVisibility, GvError)

pytestmark = pytest.mark.gpu

GV_DIRTY_MESH = 2
GV_RESULTS_MAP_RECORDS = 1
CHUNK = 4096  # kDrawChunk: records per scan chunk

SPRITE = isup.layout_dtype(96, mvp=0)  # mvp 0, colour 64, uv 80: the whole stride (staged)
SPRITE_AT = [64, 80]
# sprite + index in a 112-byte stride, every byte covered (staged): colour 64, uv 80, index 96, a 4-byte field 100, slot 104, distance 108
INDEXED = isup.layout_dtype(112, mvp=0, slot=104, distance_sq=108)
INDEXED_WIDTHS, INDEXED_AT, INDEXED_INDEX = [16, 16, 4], [64, 80, 100], 96
# gaps at 72 .. 80, 96 .. 100, 116 .. 124 (direct)
GAPS = isup.layout_dtype(128, mvp=0, slot=64, distance_sq=124)
GAPS_AT, GAPS_INDEX = [80, 100], 68


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return isup.build_twin(tmp_path_factory.mktemp("twin"))


def enclosing_ortho(half=1.0e7, shadow_pass=-1):
    """an orthographic pass that holds the whole scene: every candidate becomes a record"""
    return scene.make_view(scene.ortho_rev_z(2 * half, 2 * half, -half, half), shadow_pass=shadow_pass)


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()


def fetch_all(vis, pool_id, listed, occupancy):
    return [vis.fetch(v, write_back=False, occupancy=occupancy, order="raw", pool_id=pool_id) for v in listed]


def random_fields(n, widths, seed):
    """one C-contiguous uint32 array [n, bytes / 4] of random words per field; NaN patterns, -0 and a subnormal among them"""
    rng = np.random.Generator(np.random.PCG64(seed))
    fields = [rng.integers(0, 1 << 32, (n, w // 4), dtype=np.uint32) for w in widths]
    fields[0][:4, 0] = (0x7F800001, 0xFFC12345, 0x80000000, 0x00000001)
    return fields


def background(rows, stride, seed=7):
    block = np.random.Generator(np.random.PCG64(seed)).integers(1, 255, (4099, stride), dtype=np.uint8)
    return np.ascontiguousarray(np.resize(block, (rows, stride)))


def expected(twin, dtype, views, fetched, counts=None, fields=None, at=None, index_at=None, index_map=None):
    """(instances [total, stride] with zeros where nothing is written, the mask of written bytes, first_instance[draws + 1],
    draw_starts[views + 1], starts[views + 1]) of a draw emission of `views` over the `fetched` records with the per-slot `counts`"""
    rec, draw_starts = isup.expected(twin, dtype, views, fetched, index_map=index_map)
    mask = isup.field_mask(dtype).copy()
    slots = np.concatenate([f["visible_idx"] for f in fetched] + [np.zeros(0, np.uint32)]).astype(np.int64)
    for field, where in zip(fields or [], at or []):
        if where is not None:
            raw = np.ascontiguousarray(field).view(np.uint8).reshape(len(field), -1)
            rec[:, where:where + raw.shape[1]] = raw[slots]  # the POOL slot's row
            mask[where:where + raw.shape[1]] = True
    c = np.ones(len(slots), np.int64) if counts is None else np.asarray(counts)[slots].astype(np.int64)
    first = np.concatenate([[0], np.cumsum(c)])
    inst = np.repeat(rec, c, axis=0)
    if index_at is not None:
        j = (np.arange(first[-1]) - np.repeat(first[:-1], c)).astype(np.uint32)
        inst[:, index_at:index_at + 4] = j.view(np.uint8).reshape(-1, 4)
        mask[index_at:index_at + 4] = True
    return inst, mask, first.astype(np.uint32), draw_starts.astype(np.uint32), first[draw_starts].astype(np.uint32)


def set_layouts(vis, pool_id, dtype, at=None, index_at=None):
    vis.set_instance_index_field(pool_id, None)
    if at is not None:
        vis.set_payload_layout(pool_id, [None] * len(at))
    vis.set_instance_layout(pool_id, dtype=dtype)
    if at is not None:
        vis.set_payload_layout(pool_id, at)
    vis.set_instance_index_field(pool_id, index_at)


def check(vis, twin, views, listed, dtype, occupancy, counts=None, fields=None, at=None, index_at=None, index_map=None, pool_id=0,
          held=None, own_target=True, host_bases=True):
    """Emits `listed` with gv_pool_emit_draw_instances (own_target: into caller-owned device memory over a background, cut after
    `held` instances when given) and compares every instance byte on the device and of a host fetch, starts, first_instance[],
    draw_starts[], the host's bases and GvResult.instance_count. Returns (expected instances, first_instance, draw_starts, starts,
    the fetched results)."""
    import torch
    set_layouts(vis, pool_id, dtype, at, index_at)
    fetched = fetch_all(vis, pool_id, listed, occupancy)
    exp, mask, first, draw_starts, starts = expected(twin, dtype, [views[v] for v in listed], fetched, counts, fields, at, index_at, index_map)
    total, stride = len(exp), dtype.itemsize
    if own_target:
        rows = total + 7
        pattern = background(rows, stride)
        dev = torch.as_tensor(pattern, device="cuda:0")
        torch.cuda.synchronize()  # (torch's stream; the library's stream is non-blocking)
        room = total if held is None else held
        vis.emit_draw_instances(pool_id, listed, device=(dev.data_ptr(), rows * stride if held is None else held * stride + 5))
        assert vis.instances_device(pool_id)[0] == dev.data_ptr()
    else:
        rows, room = total, total
        pattern = np.zeros((rows, stride), np.uint8)
        vis.emit_draw_instances(pool_id, listed)
    whole = pattern.copy()
    whole[:total][:, mask] = exp[:, mask]
    host = pattern.copy()
    _, got_starts = vis.instances(pool_id, out=host)  # waits for the emission; field by field
    assert got_starts.tolist() == starts.tolist()  # (the true totals, also when the target is too small)
    assert host[:room].tobytes() == whole[:room].tobytes() and host[room:].tobytes() == pattern[room:].tobytes()
    if own_target:
        on_device = dev.cpu().numpy()
        assert on_device[:room].tobytes() == whole[:room].tobytes()  # (bytes between the fields keep the pattern in every instance)
        assert on_device[room:].tobytes() == pattern[room:].tobytes()
    got_first, got_draw_starts = vis.draw_bases(pool_id)
    assert got_draw_starts.tolist() == draw_starts.tolist()
    assert got_first.tolist() == first.tolist()
    after = fetch_all(vis, pool_id, listed, occupancy)
    for a, b in zip(fetched, after):  # the cull side is left as it was
        isup.same_results(a, b)
    for k, (v, f) in enumerate(zip(listed, after)):
        if host_bases:
            bases = vis.instance_bases(pool_id, v).astype(np.int64)
            assert (bases + int(starts[k])).tolist() == first[draw_starts[k]:draw_starts[k + 1] + 1].tolist()
            assert int(starts[k + 1]) - int(starts[k]) == int(bases[-1])
            assert int(starts[k + 1]) - int(starts[k]) == int(f["instance_count"])
    return exp, first, draw_starts, starts, fetched


def old_style_bytes(vis, pool_id, listed):
    vis.emit_instances(pool_id, listed)
    got, starts = vis.instances(pool_id)
    return got.tobytes(), starts.tolist()


def draw_style_bytes(vis, pool_id, listed):
    vis.emit_draw_instances(pool_id, listed)
    got, starts = vis.instances(pool_id)
    return got.tobytes(), starts.tolist()


def code(fn, *args, **kw):
    with pytest.raises(GvError) as e:
        fn(*args, **kw)
    return e.value.code, str(e.value)


# ---- 1. known answer ----------------------------------------------------------------------------------------------------------

def test_known_answer_written_out():
    """600 slots in slot order, counts 1, 2, 3, 0 (not drawn), 255, 256, 257, 1 repeated: every base, start and index by hand"""
    sc = scene.flat_scene(600, defects=False)
    views = [enclosing_ortho()]
    cycle = [1, 2, 3, 0, 255, 256, 257, 1]
    ready = np.array(cycle * 75, np.uint32)
    layout = isup.layout_dtype(80, mvp=0, slot=64)
    with GpuVisibility(device=0, keep_slot_order=True) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        vis.set_instance_layout(0, dtype=layout)
        vis.set_instance_index_field(0, 68)
        vis.emit_draw_instances(0, [0])
        got, starts = vis.instances(0, dtype=np.dtype(dict(names=["mvp", "slot", "index"], formats=[(np.float32, 16), np.uint32, np.uint32],
                                                           offsets=[0, 64, 68], itemsize=80)))
        first, draw_starts = vis.draw_bases(0)
        f = vis.fetch(0, write_back=False, occupancy=600, order="raw", pool_id=0)
        drawn = [s for s in range(600) if s % 8 != 3]
        assert f["visible_idx"].tolist() == drawn  # 525 draws, in slot order
        assert draw_starts.tolist() == [0, 525]
        assert starts.tolist() == [0, 75 * 775] == [0, 58125]
        within = [0, 1, 3, 6, 261, 517, 774]  # the first instance of the seven draws of a group of eight slots; a group takes 775
        assert first.tolist() == [775 * g + w for g in range(75) for w in within] + [58125]
        assert len(got) == 58125
        # group 0 by hand: slot 0 -> instance 0; slot 1 -> 1, 2; slot 2 -> 3, 4, 5; slot 4 -> 6 .. 260; slot 5 -> 261 .. 516; ...
        assert got["slot"][:7].tolist() == [0, 1, 1, 2, 2, 2, 4] and got["index"][:7].tolist() == [0, 0, 1, 0, 1, 2, 0]
        assert got["slot"][260] == 4 and got["index"][260] == 254 and got["slot"][261] == 5 and got["index"][261] == 0
        assert got["slot"][516] == 5 and got["index"][516] == 255 and got["slot"][517] == 6 and got["index"][773] == 256
        assert got["slot"][774] == 7 and got["index"][774] == 0 and got["slot"][775] == 8
        owner = np.repeat(np.array(drawn), [cycle[s % 8] for s in drawn])
        assert got["slot"].tolist() == owner.tolist()
        assert got["index"].tolist() == (np.arange(58125) - np.repeat(first[:-1], [cycle[s % 8] for s in drawn])).tolist()
        # every copy of a draw carries the draw's mvp, and draws differ
        assert (got["mvp"][6:261] == got["mvp"][6]).all() and not (got["mvp"][6] == got["mvp"][261]).all()
        assert f["instance_count"] == 58125
        # the index field in place is checked against a new layout
        assert code(vis.set_instance_layout, 0, stride=64)[0] == GV_E_ARG
        vis.set_instance_index_field(0, None)
        vis.set_instance_layout(0, stride=64)
        assert (vis.instance_bases(0, 0) == first).all()


# ---- 2. all counts 1, and no ready column --------------------------------------------------------------------------------------

@pytest.mark.parametrize("column", ["none", "ones"])
@pytest.mark.parametrize("layout", ["bare64", "full128", "sprite96"])
def test_counts_of_one_are_the_bytes_of_emit_instances(twin, layout, column):
    sc = scene.flat_scene(20_000, defects=False)
    views = [scene.main_camera_view(), enclosing_ortho(shadow_pass=0)]
    fields = random_fields(sc.count, [16, 16], 3)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        ones = np.ones(sc.count, np.uint32)
        if column == "ones":
            vis.bind_ready(0, ones)
        if layout == "sprite96":
            vis.bind_payload(0, fields)
        vis.cull(0, views)
        dtype = {"bare64": isup.BARE, "full128": isup.FULL, "sprite96": SPRITE}[layout]
        set_layouts(vis, 0, dtype, SPRITE_AT if layout == "sprite96" else None)
        old = old_style_bytes(vis, 0, [0, 1])
        new = draw_style_bytes(vis, 0, [0, 1])
        assert old[1] == new[1] and old[1][2] > 20_000 and old[1][1] > 100
        assert old[0] == new[0]
        first, draw_starts = vis.draw_bases(0)
        assert draw_starts.tolist() == new[1] and first.tolist() == list(range(new[1][2] + 1))
        check(vis, twin, views, [0, 1], dtype, sc.count, ones if column == "ones" else None,
              fields if layout == "sprite96" else None, SPRITE_AT if layout == "sprite96" else None)


# ---- 3. boundaries -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("draws", [255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_draw_counts_at_workgroup_and_chunk_edges(twin, draws):
    """the visible set is trimmed to `draws` by disabling slots; mixed counts, so that the prefix crosses every edge with a carry"""
    sc = scene.flat_scene(9_000, defects=False)
    sc.meshes["isEnabled"][draws:] = 0
    views = [enclosing_ortho(), scene.main_camera_view()]
    rng = np.random.Generator(np.random.PCG64(draws))
    ready = rng.choice(np.array([1, 1, 2, 3, 9], np.uint32), sc.count)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        _, _, draw_starts, _, _ = check(vis, twin, views, [0, 1], isup.FULL, sc.count, ready)
        assert draw_starts[1] == draws  # reached, not assumed


def test_large_draws_straddle_workgroups_among_ones(twin):
    """one draw of 5000 and one of 65535 instances among ones: their instances span many strides of a workgroup's output walk, and a
    draw's instances straddle the 256-record workgroup that owns it and its neighbours' output ranges"""
    sc = scene.flat_scene(2_000, defects=False)
    views = [enclosing_ortho()]
    ready = np.ones(sc.count, np.uint32)
    ready[300], ready[1023], ready[1024] = 5000, GV_MAX_DRAW_INSTANCES, 700
    with GpuVisibility(device=0, keep_slot_order=True) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        _, first, draw_starts, starts, fetched = check(vis, twin, views, [0], isup.BARE, sc.count, ready)
        assert draw_starts[1] == sc.count and fetched[0]["visible_idx"].tolist() == list(range(sc.count))
        assert starts[1] == sc.count - 3 + 5000 + 65535 + 700
        assert first[1024] - first[1023] == 65535 and first[1025] - first[1024] == 700  # the last draw of one workgroup, the first of the next
        check(vis, twin, views, [0], isup.FULL, sc.count, ready, index_at=120)  # the direct way


def test_zero_count_runs_and_a_first_and_last_draw_of_zero(twin):
    """300 consecutive draws, the first and the last draw made zero by marks after the cull: they take no instance and their
    first_instance equals their successor's"""
    sc = scene.flat_scene(5_000, defects=False)
    views = [enclosing_ortho()]
    rng = np.random.Generator(np.random.PCG64(11))
    ready = rng.choice(np.array([1, 2, 5], np.uint32), sc.count)
    with GpuVisibility(device=0, keep_slot_order=True) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_draw_instances(0, [0])  # the mirror exists from here on: marks feed its dirty set
        assert vis.fetch(0, write_back=False, occupancy=sc.count, order="raw", pool_id=0)["visible_idx"].tolist() == list(range(sc.count))
        for lo, n in ((0, 1), (sc.count - 1, 1), (200, 300), (4095, 2)):
            ready[lo:lo + n] = 0
            vis.mark_dirty(GV_DIRTY_MESH, lo, n, pool_id=0)
        _, first, draw_starts, starts, _ = check(vis, twin, views, [0], isup.BARE, sc.count, ready)
        assert draw_starts[1] == sc.count  # the records are those of the cull
        assert first[0] == first[1] == 0 and first[sc.count - 1] == first[sc.count] == starts[1]
        assert (first[200:501] == first[200]).all() and first[501] > first[500]
        check(vis, twin, views, [0], GAPS, sc.count, ready, index_at=GAPS_INDEX)


# ---- 4. widths and the limit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [np.uint8, np.uint32], ids=["u8", "u32"])
def test_column_widths(twin, width):
    sc = scene.flat_scene(7_000, defects=False)
    views = [enclosing_ortho(), scene.main_camera_view()]
    rng = np.random.Generator(np.random.PCG64(21))
    ready = rng.choice(np.array([0, 1, 1, 2, 3, 255], width), sc.count)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        _, _, draw_starts, starts, _ = check(vis, twin, views, [0, 1], isup.FULL, sc.count, ready)
        assert draw_starts[1] == int((ready != 0).sum()) and starts[1] == int(ready.astype(np.int64).sum())
        # a large dirty range (a contiguous copy) and scattered small ones (one packet) in one upload
        ready[1000:4000] = rng.choice(np.array([1, 4], width), 3000)
        vis.mark_dirty(GV_DIRTY_MESH, 1000, 3000, pool_id=0)
        for s in (5, 6, 4500, 6999):
            ready[s] = 7
            vis.mark_dirty(GV_DIRTY_MESH, s, 1, pool_id=0)
        before = vis.stats()["upload_bytes"]
        check(vis, twin, views, [0, 1], isup.FULL, sc.count, ready)
        assert vis.stats()["upload_bytes"] > before


def test_the_limit_holds_for_live_slots_only(twin):
    sc = scene.flat_scene(3_000, defects=False)
    sc.meshes["isEnabled"][9] = 0
    views = [enclosing_ortho()]
    ready = np.ones(sc.count, np.uint32)
    ready[9] = GV_MAX_DRAW_INSTANCES + 1   # a disabled slot: nobody's draw
    ready[10] = GV_MAX_DRAW_INSTANCES
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        _, _, draw_starts, starts, _ = check(vis, twin, views, [0], isup.BARE, sc.count, ready)
        assert draw_starts[1] == sc.count - 1 and starts[1] == sc.count - 2 + GV_MAX_DRAW_INSTANCES
        ready[20] = GV_MAX_DRAW_INSTANCES + 1  # a live one
        vis.mark_dirty(GV_DIRTY_MESH, 20, 1, pool_id=0)
        vis.cull(0, views)
        vis.set_instance_layout(0, dtype=isup.BARE)
        c, text = code(vis.emit_draw_instances, 0, [0])
        assert c == GV_E_STATE and "1 live" in text and str(GV_MAX_DRAW_INSTANCES) in text
        ready[20] = 2
        vis.mark_dirty(GV_DIRTY_MESH, 20, 1, pool_id=0)
        vis.cull(0, views)
        check(vis, twin, views, [0], isup.BARE, sc.count, ready)
        # a count put above the limit by a mark between the cull and the emission is refused too, on a live slot only
        ready[30] = ready[9] = GV_MAX_DRAW_INSTANCES + 7
        vis.mark_dirty(GV_DIRTY_MESH, 30, 1, pool_id=0)
        vis.mark_dirty(GV_DIRTY_MESH, 9, 1, pool_id=0)
        c, text = code(vis.emit_draw_instances, 0, [0])
        assert c == GV_E_STATE and "1 live" in text and str(GV_MAX_DRAW_INSTANCES) in text
        ready[30] = 3
        vis.mark_dirty(GV_DIRTY_MESH, 30, 1, pool_id=0)
        _, first, draw_starts, _, _ = check(vis, twin, views, [0], isup.BARE, sc.count, ready)
        assert draw_starts[1] == sc.count - 1


# ---- 5. views and order --------------------------------------------------------------------------------------------------------

def test_two_views_in_both_orders_and_a_shadow_view(twin):
    sc = scene.flat_scene(30_000, defects=False)
    views = [scene.main_camera_view(), enclosing_ortho(shadow_pass=0)]  # (the shadow view produces no isVisible)
    rng = np.random.Generator(np.random.PCG64(31))
    ready = rng.choice(np.array([0, 1, 2, 5], np.uint32), sc.count)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        a = check(vis, twin, views, [0, 1], isup.FULL, sc.count, ready)
        b = check(vis, twin, views, [1, 0], isup.FULL, sc.count, ready)
        assert a[3][1] > 500 and b[3][1] > 40_000 and a[3][2] == b[3][2]
        check(vis, twin, views, [1], isup.BARE, sc.count, ready, own_target=False)


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_draw_k_is_sorted_record_k(twin, descending):
    sc = scene.flat_scene(40_000, defects=False)
    views = [enclosing_ortho()]
    rng = np.random.Generator(np.random.PCG64(32))
    ready = rng.choice(np.array([1, 2, 3], np.uint32), sc.count)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        vis.sort(0, descending=descending, pool_id=0)
        vis.set_instance_layout(0, dtype=isup.FULL)
        vis.emit_draw_instances(0, [0])  # the first read: the deferred sort is launched first
        _, _, _, _, fetched = check(vis, twin, views, [0], isup.FULL, sc.count, ready)
        d = fetched[0]["distance_sq"]
        assert len(d) == sc.count and ((np.diff(d) <= 0).all() if descending else (np.diff(d) >= 0).all())
        assert len(np.unique(d)) > len(d) // 2


# ---- 6. targets ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [isup.BARE, isup.layout_dtype(80, mvp=16, slot=0, distance_sq=8), GAPS], ids=["bare64", "stride80", "gaps128"])
def test_a_target_cut_inside_one_draw_and_a_small_host_array(twin, dtype):
    sc = scene.flat_scene(6_000, defects=False)
    views = [enclosing_ortho(), scene.main_camera_view()]
    ready = np.full(sc.count, 3, np.uint32)
    ready[::7] = 40
    with GpuVisibility(device=0, keep_slot_order=True) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        exp, first, _, starts, _ = check(vis, twin, views, [0, 1], dtype, sc.count, ready)
        k = 2800  # slot 2800 = 7 x 400: a draw of 40 instances; the cut falls 13 instances into it
        assert first[k + 1] - first[k] == 40
        check(vis, twin, views, [0, 1], dtype, sc.count, ready, held=int(first[k]) + 13)
        # a host array that is too small: GV_E_ARG, nothing written
        total = int(starts[-1])
        small = np.full((total - 1, dtype.itemsize), 0x5A, np.uint8)
        with pytest.raises(GvError) as e:
            vis.instances(0, out=small)
        assert e.value.code == GV_E_ARG and (small == 0x5A).all()
        import ctypes as C
        few, few_starts = np.full(int(first.shape[0]) - 1, 0xAAAAAAAA, np.uint32), np.full(3, 0xAAAAAAAA, np.uint32)
        rc = vis.lib.gv_pool_draw_bases_fetch(vis.ctx, 0, few.ctypes.data_as(C.POINTER(C.c_uint32)), len(few),
                                              few_starts.ctypes.data_as(C.POINTER(C.c_uint32)), 3)
        assert rc == GV_E_ARG and (few == 0xAAAAAAAA).all() and (few_starts == 0xAAAAAAAA).all()
        rc = vis.lib.gv_pool_draw_bases_fetch(vis.ctx, 0, None, 0, few_starts.ctypes.data_as(C.POINTER(C.c_uint32)), 2)
        assert rc == GV_E_ARG and (few_starts == 0xAAAAAAAA).all()
        # afterwards the library-owned target
        check(vis, twin, views, [0, 1], dtype, sc.count, ready, own_target=False)


# ---- 7. fields -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("way", ["staged", "direct"])
def test_index_field_slot_through_an_index_map_and_opaque_payload(twin, way):
    sc = scene.flat_scene(12_000, defects=False)
    views = [enclosing_ortho(), scene.main_camera_view()]
    rng = np.random.Generator(np.random.PCG64(41))
    ready = rng.choice(np.array([0, 1, 2, 3, 17], np.uint32), sc.count)
    ready[:4] = (3, 2, 5, 2)  # the NaN patterns, -0 and the subnormal of the payload's first rows are drawn several times
    index_map = (rng.permutation(sc.count) + 1000).astype(np.uint32)
    dtype, widths, at, index_at = (INDEXED, INDEXED_WIDTHS, INDEXED_AT, INDEXED_INDEX) if way == "staged" else (GAPS, [16, 16], GAPS_AT, GAPS_INDEX)
    fields = random_fields(sc.count, widths, 42)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.bind_payload(0, fields)
        vis.set_index_map(0, index_map)
        vis.cull(0, views)
        exp, first, _, _, fetched = check(vis, twin, views, [0, 1], dtype, sc.count, ready, fields, at, index_at, index_map)
        k = int(np.flatnonzero(fetched[0]["visible_idx"] == 0)[0])  # slot 0: a signalling NaN in its first payload word, three copies
        rows = exp[first[k]:first[k + 1]]
        assert len(rows) == 3 and (rows[:, at[0]:at[0] + 4].view(np.uint32) == 0x7F800001).all()
        assert rows[:, index_at:index_at + 4].view(np.uint32).ravel().tolist() == [0, 1, 2]
        assert (rows[:, dtype.fields["slot"][1]:dtype.fields["slot"][1] + 4].view(np.uint32) == index_map[0]).all()
        # the index field is checked where the payload destinations are
        assert code(vis.set_instance_index_field, 0, at[0] + 4)[0] == GV_E_ARG      # inside a payload destination
        assert code(vis.set_instance_index_field, 0, 4)[0] == GV_E_ARG              # inside mvp
        assert code(vis.set_instance_index_field, 0, index_at + 2)[0] == GV_E_ARG   # misaligned
        assert code(vis.set_instance_index_field, 0, dtype.itemsize)[0] == GV_E_ARG  # beyond the stride
        assert code(vis.set_instance_layout, 0, stride=64)[0] == GV_E_ARG           # a layout the field in place does not fit
        vis.set_payload_layout(0, [None] * len(at))
        moved = list(at)
        moved[-1] = index_at
        assert code(vis.set_payload_layout, 0, moved)[0] == GV_E_ARG                # a destination on the field in place
        check(vis, twin, views, [0, 1], dtype, sc.count, ready, fields, at, index_at, index_map)
        # gv_pool_emit_instances ignores the field entirely (counts of 0 / 1 only)
        ready[ready > 1] = 1
        vis.mark_dirty(GV_DIRTY_MESH, 0, sc.count, pool_id=0)
        vis.cull(0, views)
        fetched = fetch_all(vis, 0, [0, 1], sc.count)
        import torch
        total = sum(int(f["draw_count"]) for f in fetched)
        pattern = background(total, dtype.itemsize)
        dev = torch.as_tensor(pattern, device="cuda:0")
        torch.cuda.synchronize()
        vis.emit_instances(0, [0, 1], device=(dev.data_ptr(), pattern.nbytes))
        vis.instances(0)
        assert (dev.cpu().numpy()[:, index_at:index_at + 4] == pattern[:, index_at:index_at + 4]).all()


# ---- 8. marks ------------------------------------------------------------------------------------------------------------------

def test_a_marked_count_is_seen_by_the_emission_an_unmarked_one_is_not(twin):
    sc = scene.flat_scene(8_000, defects=False)
    views = [enclosing_ortho()]
    ready = np.full(sc.count, 2, np.uint32)
    with GpuVisibility(device=0, keep_slot_order=True) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        check(vis, twin, views, [0], isup.FULL, sc.count, ready)
        mirrored = ready.copy()
        ready[100], ready[4096] = 9, 0
        vis.mark_dirty(GV_DIRTY_MESH, 100, 1, pool_id=0)
        vis.mark_dirty(GV_DIRTY_MESH, 4096, 1, pool_id=0)
        mirrored[100], mirrored[4096] = 9, 0
        ready[200] = 50  # changed, NOT marked: the mirror keeps 2
        _, first, draw_starts, starts, _ = check(vis, twin, views, [0], isup.FULL, sc.count, mirrored, host_bases=False)
        assert draw_starts[1] == sc.count  # the records are those of the cull: slot 4096 is still a draw, of no instance
        assert first[101] - first[100] == 9 and first[4097] == first[4096] and first[201] - first[200] == 2
        assert starts[1] == 2 * sc.count + 7 - 2
        # gv_sync consumes the dirty set as well: marked now, uploaded by the cull's sync, seen by the emission behind it
        vis.mark_dirty(GV_DIRTY_MESH, 200, 1, pool_id=0)
        vis.cull(0, views)
        _, first, draw_starts, _, _ = check(vis, twin, views, [0], isup.FULL, sc.count, ready)
        assert draw_starts[1] == sc.count - 1 and first[201] - first[200] == 50
        # rebinding the column resets the mirror: everything is read again, marks or not
        other = np.full(sc.count, 3, np.uint32)
        vis.bind_ready(0, other)
        vis.cull(0, views)
        check(vis, twin, views, [0], isup.FULL, sc.count, other)


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------

def test_errors_each_followed_by_a_correct_emission(twin):
    sc = scene.flat_scene(10_000, defects=False)
    views = [scene.main_camera_view(), enclosing_ortho(shadow_pass=0)]
    count_only = [dict(views[0]), dict(views[1], emit_records=0)]
    rng = np.random.Generator(np.random.PCG64(51))
    ready = rng.choice(np.array([1, 2, 4], np.uint32), sc.count)
    fields = random_fields(sc.count, [16, 16], 52)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)

        def good():
            vis.cull(0, views)
            check(vis, twin, views, [0, 1], isup.FULL, sc.count, ready)

        emit = vis.emit_draw_instances
        vis.cull(0, views)
        assert code(emit, 0, [0])[0] == GV_E_STATE             # no layout
        good()
        vis.cull(0, views)
        assert code(emit, 1, [0])[0] == GV_E_ARG               # an unbound pool
        assert code(emit, 0, [])[0] == GV_E_ARG                # no view
        assert code(emit, 0, [0, 1, 2])[0] == GV_E_ARG         # more views than were culled
        assert code(emit, 0, [1, 1])[0] == GV_E_ARG            # a view twice
        assert code(emit, 0, [8])[0] == GV_E_ARG               # no such view
        assert code(emit, 0, [5])[0] == GV_E_STATE             # a view with no results
        assert code(emit, 0, [0], device=(4096 + 4, 1 << 20))[0] == GV_E_ARG  # a misaligned target
        good()
        vis.cull(0, count_only)
        assert code(emit, 0, [0, 1])[0] == GV_E_STATE          # a count-only view
        good()
        vis.set_index_map(0, np.arange(sc.count - 1, dtype=np.uint32))
        vis.cull(0, views)
        assert code(emit, 0, [0, 1])[0] == GV_E_STATE          # an index map that does not cover the pool
        # a ready column AND a result mapping
        vis.set_index_map(0, np.arange(sc.count, dtype=np.uint32))
        vis.set_result_mapping(0, GV_RESULTS_MAP_RECORDS)
        c, text = code(emit, 0, [0, 1])
        assert c == GV_E_STATE and "result mapping" in text
        vis.set_result_mapping(0, 0)
        vis.set_index_map(0, None)
        good()
        vis.bind_payload(0, [f[:sc.count - 1] for f in fields])
        set_layouts(vis, 0, SPRITE, SPRITE_AT)
        vis.cull(0, views)
        assert code(emit, 0, [0, 1])[0] == GV_E_STATE          # a payload that does not cover the pool
        vis.bind_payload(0, None)
        good()
        # a library-owned target whose bound does not fit 32 bits of instances: 2 views x 40 000 slots x 65 535
        wide = scene.flat_scene(40_000, defects=False)
        big = np.full(wide.count, GV_MAX_DRAW_INSTANCES, np.uint32)
        vis.bind_ready(0, big)  # (in front of the larger pool: the column covers every slot the next sync reads)
        bind(vis, wide)
        away = [scene.make_view(scene.ortho_rev_z(1.0, 1.0, 0.0, 1.0), camera_position=(3.0e6, 0.0, 0.0))] * 2  # nothing in sight
        vis.cull(0, away)
        c, text = code(emit, 0, [0, 1])
        assert c == GV_E_STATE and "caller-owned" in text
        check(vis, twin, away, [0, 1], isup.FULL, wide.count, big)  # a caller-owned target works: nothing is drawn
        bind(vis, sc)
        vis.bind_ready(0, ready)
        good()


def test_the_last_emission_is_the_one_described(twin):
    sc = scene.flat_scene(5_000, defects=False)
    views = [enclosing_ortho()]
    ones = np.ones(sc.count, np.uint32)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ones)
        vis.cull(0, views)
        vis.set_instance_layout(0, dtype=isup.FULL)
        assert code(vis.draw_bases_device, 0)[0] == GV_E_STATE   # nothing emitted
        vis.emit_instances(0, [0])
        assert code(vis.draw_bases_device, 0)[0] == GV_E_STATE   # an old-style emission
        assert code(vis.draw_bases, 0)[0] == GV_E_STATE
        old = vis.instances(0)
        vis.emit_draw_instances(0, [0])
        first_ptr, starts_ptr = vis.draw_bases_device(0)
        assert first_ptr and starts_ptr
        new = vis.instances(0)
        assert vis.instances_info(0) == (1, 128, sc.count)
        assert old[0].tobytes() == new[0].tobytes() and old[1].tolist() == new[1].tolist() == [0, sc.count]
        assert vis.draw_bases(0)[0].tolist() == list(range(sc.count + 1))
        vis.emit_instances(0, [0])
        assert code(vis.draw_bases_device, 0)[0] == GV_E_STATE   # ... describes the last one again
        assert vis.instances(0)[0].tobytes() == old[0].tobytes()
        vis.emit_draw_instances(0, [0])
        vis.cull(0, views)
        assert code(vis.draw_bases_device, 0)[0] == GV_E_STATE   # the emission ended with the pool's next cull
        assert code(vis.instances_device, 0)[0] == GV_E_STATE
        check(vis, twin, views, [0], isup.FULL, sc.count, ones)


# ---- 10. a random world --------------------------------------------------------------------------------------------------------

def test_random_world_over_four_frames(twin):
    """60 000 slots, counts from {0, 1, 1, 1, 2, 3, 7, 40}, two views, a payload, 2 % of the slots marked per frame between the frame's
    cull and its emission: a marked slot that draws goes to 0 (its resources were unloaded: a draw of the cull that takes no instance
    at the emission), one that was at 0 gets a count from the set (seen by the next cull)."""
    sc = scene.flat_scene(60_000, defects=False)
    views = [enclosing_ortho(), scene.main_camera_view()]
    rng = np.random.Generator(np.random.PCG64(2026))
    values = np.array([0, 1, 1, 1, 2, 3, 7, 40], np.uint32)
    ready = rng.choice(values, sc.count)
    fields = random_fields(sc.count, [16, 16], 61)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.bind_payload(0, fields)
        vis.cull(0, views)
        check(vis, twin, views, [0, 1], SPRITE, sc.count, ready, fields, SPRITE_AT)  # (the mirror exists from here on)
        for frame in range(4):
            vis.cull(0, views)
            marked = rng.choice(sc.count, sc.count // 50, replace=False)
            ready[marked] = np.where(ready[marked] != 0, 0, rng.choice(values[1:], len(marked))).astype(np.uint32)
            for f in fields:
                f[marked] = rng.integers(0, 1 << 32, (len(marked), f.shape[1]), dtype=np.uint32)
            for s in marked:
                vis.mark_dirty(GV_DIRTY_MESH, int(s), 1, pool_id=0)
            listed = [0, 1] if frame % 2 == 0 else [1, 0]
            _, first, draw_starts, starts, fetched = check(vis, twin, views, listed, SPRITE, sc.count, ready, fields, SPRITE_AT)
            taken = np.diff(first.astype(np.int64))
            assert len(taken) == draw_starts[-1] > 50_000
            assert (taken > 1).sum() >= 0.25 * len(taken), (frame, (taken > 1).mean())
            assert (taken == 0).sum() >= 0.01 * len(taken), (frame, (taken == 0).mean())
