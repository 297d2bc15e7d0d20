"""gv_pool_emit_instances on the device: the instance array of the reference's draw loops (mesh.cpp:556-770 -> drawAsync ->
instanceData[instanceIndex].mvp = viewProj * model, sprite.cpp:107-108,122-126), checked bit for bit against the C twin of DESIGN.md
§4 item 9 (tests/instance_twin.h) fed with the fetched records, through its order, target, layout and error rules, and against
the cull results it must leave alone."""
import json
import os
import subprocess

import numpy as np
import pytest

import instances_support as isup
from garden_amd import scene
from garden_amd.lib import GV_E_ARG, GV_E_STATE, GpuVisibility, GvError

pytestmark = pytest.mark.gpu

GV_DIRTY_TRANSFORM, GV_DIRTY_MESH = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return isup.build_twin(tmp_path_factory.mktemp("twin"))


def enclosing_ortho(half=1.0e7, shadow_pass=0):
    """an orthographic pass that holds the whole scene: every candidate becomes a record"""
    return scene.make_view(scene.ortho_rev_z(2 * half, 2 * half, -half, half), shadow_pass=shadow_pass)


def two_views():
    """a perspective main pass and an orthographic pass, one camera position: one gv_cull"""
    return [scene.main_camera_view(), enclosing_ortho()]


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()


def fetch_all(vis, pool_id, listed, occupancy):
    return [vis.fetch(v, write_back=False, occupancy=occupancy, order="raw", pool_id=pool_id) for v in listed]


def check_emission(vis, twin, pool_id, views, listed, dtype, occupancy, index_map=None, fetch_first=True, min_total=None):
    """Emits `listed` and compares starts and every instance byte with the twin over the fetched records; the fetched cull results
    are the same bytes before and after the emission (fetch_first=False: the emission is the first read, results compared after)."""
    before = fetch_all(vis, pool_id, listed, occupancy) if fetch_first else None
    vis.set_instance_layout(pool_id, dtype=dtype)
    vis.emit_instances(pool_id, listed)
    got, starts = vis.instances(pool_id)
    after = fetch_all(vis, pool_id, listed, occupancy)
    if before is not None:
        for a, b in zip(before, after):
            isup.same_results(a, b)
    exp, exp_starts = isup.expected(twin, dtype, [views[v] for v in listed], after, index_map=index_map)
    assert starts.tolist() == exp_starts.tolist()
    assert got.shape == exp.shape
    assert got.tobytes() == exp.tobytes()
    if min_total is not None:
        assert int(starts[-1]) >= min_total, starts
    return got, starts, after


def column_binds(vis, sc):
    t, m = sc.transforms, sc.meshes
    xf = dict(entity=t["entity"].copy(), parent=t["parent"].copy(), position=np.ascontiguousarray(t["position"][:, :3]),
              scale=np.ascontiguousarray(t["scale"][:, :3]), rotation=t["rotation"].copy(),
              self_active=t["selfActive"].copy(), ancestors_active=t["ancestorsActive"].copy(),
              model_with_ancestors=t["modelWithAncestors"].copy())
    mesh = dict(entity=m["entity"].copy(), is_enabled=m["isEnabled"].copy(),
                aabb_min=np.ascontiguousarray(m["aabbMin"][:, :3]), aabb_max=np.ascontiguousarray(m["aabbMax"][:, :3]),
                is_visible=np.zeros(sc.count, np.uint8))
    vis.bind_transform_columns(xf, sc.entity_to_transform)
    vis.bind_pool_columns(0, mesh)
    vis.hierarchy_rebuild()


SIZES = [1, 63, 64, 65, 255, 257, 4096, 32768, 300_000, 2_000_000]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("kind", ["flat", "hierarchy", "shuffled", "columns", "index_map"])
def test_bits_against_the_twin(twin, kind, size):
    """every instance's mvp == twin(view_proj, fetched baked_model[k]) as uint32, slot / model / distance_sq == the fetched arrays,
    starts == the prefix of the fetched draw counts; perspective and orthographic views in one emission"""
    if kind == "hierarchy":
        sc = scene.hierarchy_scene(size)
    elif kind == "shuffled":
        sc = scene.shuffled_scene(scene.flat_scene(size), drop_transforms=0.02 if size >= 64 else 0.0)
    else:
        sc = scene.flat_scene(size)
    views = two_views()
    index_map = None
    with GpuVisibility(device=0) as vis:
        if kind == "columns":
            column_binds(vis, sc)
        else:
            bind(vis, sc)
        if kind == "index_map":
            rng = np.random.Generator(np.random.PCG64(size))
            index_map = (rng.permutation(size) + 1000).astype(np.uint32)
            index_map[rng.random(size) < 0.1] = isup.NONE
            vis.set_index_map(0, index_map)
        vis.cull(0, views)
        _, starts, _ = check_emission(vis, twin, 0, views, [0, 1], isup.FULL, sc.count, index_map=index_map)
        if size >= 4096:
            assert starts[1] > 0 and starts[2] - starts[1] > size // 4, starts
        # the bare layout, each view alone
        check_emission(vis, twin, 0, views, [1], isup.BARE, sc.count)
        check_emission(vis, twin, 0, views, [0], isup.BARE, sc.count)


@pytest.mark.parametrize("size", [12_000, 100_000, 400_000], ids=["small", "mid", "large"])
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_instance_order_is_the_sorted_record_order(twin, size, descending):
    """gv_pool_sort, then the emission as the first read: a deferred sort is launched first, instance k belongs to sorted record k"""
    sc = scene.flat_scene(size, defects=False)
    views = [enclosing_ortho(shadow_pass=-1)]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, views)
        vis.sort(0, descending=descending, pool_id=0)
        _, starts, fetched = check_emission(vis, twin, 0, views, [0], isup.FULL, sc.count, fetch_first=False, min_total=size // 2)
        d = fetched[0]["distance_sq"]
        assert (np.diff(d) <= 0).all() if descending else (np.diff(d) >= 0).all()
        assert len(np.unique(d)) > len(d) // 2


def test_inside_a_batch_the_same_bytes_as_outside(twin):
    sc = scene.flat_scene(9_000)
    views = two_views()
    pools = []
    for k in range(3):
        m = sc.meshes.copy()
        m["isEnabled"][k::5] = 0
        pools.append(m)
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        for k, m in enumerate(pools):
            vis.bind_pool(k, m)
            vis.set_instance_layout(k, dtype=isup.FULL)
        vis.hierarchy_rebuild()
        outside = []
        for k in range(3):
            vis.cull(k, views)
            outside.append(check_emission(vis, twin, k, views, [0, 1], isup.FULL, sc.count, min_total=4000)[0].tobytes())
        assert len(set(outside)) == 3
        sorted_outside = []
        for k in range(3):
            vis.cull(k, views)
            vis.sort(1, pool_id=k)
            sorted_outside.append(check_emission(vis, twin, k, views, [0, 1], isup.FULL, sc.count, fetch_first=False)[0].tobytes())
        assert sorted_outside != outside
        for sort_them in (False, True):
            vis.cull_batch_begin()
            for k in range(3):
                vis.cull(k, views)
                if sort_them:
                    vis.sort(1, pool_id=k)
            inside = []
            for k in range(3):  # the first emission is the batch's first read: it launches what has been recorded
                vis.emit_instances(k, [0, 1])
            for k in range(3):
                inside.append(vis.instances(k)[0].tobytes())
            vis.cull_batch_end()
            assert inside == (sorted_outside if sort_them else outside)


def test_main_pass_and_three_cascades_from_one_cull(twin):
    sc = scene.flat_scene(200_000)
    views = [scene.main_camera_view()] + [scene.cascade_view(index=k, size=4000.0 * (k + 1)) for k in range(3)]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, views)
        _, shadow_starts, _ = check_emission(vis, twin, 0, views, [1, 2, 3], isup.FULL, sc.count)
        assert shadow_starts[-1] > 0 and (np.diff(shadow_starts.astype(np.int64)) >= 0).all(), shadow_starts
        _, base_starts, _ = check_emission(vis, twin, 0, views, [0], isup.BARE, sc.count, min_total=1000)
        assert len(base_starts) == 2
        # any order of the listed views is the caller's
        check_emission(vis, twin, 0, views, [3, 0, 2], isup.FULL, sc.count)


LAYOUTS = [
    isup.layout_dtype(64, mvp=0),
    isup.layout_dtype(80, mvp=16, slot=0, distance_sq=8),
    isup.layout_dtype(80, mvp=0, slot=76),
    isup.layout_dtype(128, mvp=64, model=4, slot=56),        # a model that is only 4-byte aligned
    isup.layout_dtype(128, mvp=0, model=64, slot=112, distance_sq=124),
    isup.layout_dtype(128, mvp=48, model=0, distance_sq=112),
]


@pytest.mark.parametrize("dtype", LAYOUTS, ids=[f"stride{d.itemsize}_{i}" for i, d in enumerate(LAYOUTS)])
def test_only_the_fields_are_written_on_the_device_and_on_the_host(twin, dtype):
    import torch
    sc = scene.flat_scene(50_000)
    views = two_views()
    stride = dtype.itemsize
    rng = np.random.Generator(np.random.PCG64(stride))
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, views)
        fetched = fetch_all(vis, 0, [0, 1], sc.count)
        total = sum(f["draw_count"] for f in fetched)
        assert total > 25_000
        rows = total + 7
        pattern = rng.integers(1, 255, (rows, stride), dtype=np.uint8)
        exp, exp_starts = isup.expected(twin, dtype, views, fetched, background=pattern)
        mask = isup.field_mask(dtype)
        assert not mask.all() or stride == 64
        vis.set_instance_layout(0, dtype=dtype)
        # a caller-owned device target with room to spare
        dev = torch.as_tensor(pattern, device="cuda:0")
        torch.cuda.synchronize()  # (the copy runs on torch's stream; the library's stream is non-blocking: no implicit order between them)
        vis.emit_instances(0, [0, 1], device=(dev.data_ptr(), rows * stride))
        assert vis.instances_device(0)[0] == dev.data_ptr()
        host = pattern.copy()
        got, starts = vis.instances(0, out=host)  # (waits for the emission) into pageable memory, field by field
        assert starts.tolist() == exp_starts.tolist()
        on_device = dev.cpu().numpy()
        assert on_device[:total].tobytes() == exp.tobytes()
        assert on_device[total:].tobytes() == pattern[total:].tobytes()
        assert (on_device[:total][:, ~mask] == pattern[:total][:, ~mask]).all()
        assert host[:total].tobytes() == exp.tobytes() and host[total:].tobytes() == pattern[total:].tobytes()
        # one instance too small: nothing beyond capacity_bytes is written, the true total is still reported
        dev = torch.as_tensor(pattern, device="cuda:0")
        torch.cuda.synchronize()
        vis.emit_instances(0, [0, 1], device=(dev.data_ptr(), (total - 1) * stride + stride - 1))
        host = pattern.copy()
        got, starts = vis.instances(0, out=host)
        assert starts.tolist() == exp_starts.tolist()
        on_device = dev.cpu().numpy()
        assert on_device[:total - 1].tobytes() == exp[:total - 1].tobytes()
        assert on_device[total - 1:].tobytes() == pattern[total - 1:].tobytes()
        assert host[:total - 1].tobytes() == exp[:total - 1].tobytes() and host[total - 1:].tobytes() == pattern[total - 1:].tobytes()
        # a host array that is too small: GV_E_ARG, nothing written
        small = pattern[:total - 1].copy()
        with pytest.raises(GvError) as e:
            vis.instances(0, out=small)
        assert e.value.code == GV_E_ARG and small.tobytes() == pattern[:total - 1].tobytes()
        # the library's own buffer afterwards
        check_emission(vis, twin, 0, views, [0, 1], dtype, sc.count)


@pytest.mark.parametrize("width", [np.uint8, np.uint32], ids=["u8", "u32"])
def test_ready_column_counts_of_zero_and_one_work_and_two_is_refused(twin, width):
    sc = scene.flat_scene(60_000, defects=False)
    views = two_views()
    rng = np.random.Generator(np.random.PCG64(5))
    ready = (rng.random(sc.count) < 0.7).astype(width)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.cull(0, views)
        _, starts, fetched = check_emission(vis, twin, 0, views, [0, 1], isup.FULL, sc.count, min_total=30_000)
        assert (ready[fetched[1]["visible_idx"]] == 1).all() and starts[2] - starts[1] == int(ready.sum())
        live = int(fetched[1]["visible_idx"][17])
        ready[live] = 2
        vis.mark_dirty(GV_DIRTY_MESH, live, 1, pool_id=0)
        vis.cull(0, views)
        with pytest.raises(GvError) as e:
            vis.emit_instances(0, [0, 1])
        assert e.value.code == GV_E_STATE and "above 1" in str(e.value)
        kept = fetch_all(vis, 0, [0, 1], sc.count)  # the cull results are there all the same
        assert kept[1]["draw_count"] == int((ready != 0).sum())
        # a count of 2 on a slot that is not live is nobody's draw
        ready[live] = 1
        vis.mark_dirty(GV_DIRTY_MESH, live, 1, pool_id=0)
        sc.meshes["isEnabled"][5] = 0
        ready[5] = 2
        vis.mark_dirty(GV_DIRTY_MESH, 5, 1, pool_id=0)
        vis.cull(0, views)
        check_emission(vis, twin, 0, views, [0, 1], isup.FULL, sc.count, min_total=30_000)
        vis.bind_ready(0, None)
        vis.cull(0, views)
        _, starts, _ = check_emission(vis, twin, 0, views, [0, 1], isup.FULL, sc.count)
        assert starts[2] - starts[1] == sc.count - 1


def test_error_codes_each_followed_by_a_correct_emission(twin):
    sc = scene.flat_scene(40_000)
    views = two_views()
    count_only = [dict(views[0]), dict(views[1], emit_records=0)]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)

        def good():
            vis.cull(0, views)
            check_emission(vis, twin, 0, views, [0, 1], isup.FULL, sc.count, min_total=20_000)

        def code(fn, *args, **kw):
            with pytest.raises(GvError) as e:
                fn(*args, **kw)
            return e.value.code

        vis.cull(0, views)
        assert code(vis.emit_instances, 0, [0]) == GV_E_STATE  # no layout
        good()
        for bad in (dict(stride=48), dict(stride=72), dict(stride=272), dict(stride=64, mvp=8), dict(stride=64, mvp=16),
                    dict(stride=128, mvp=0, model=32), dict(stride=128, mvp=0, model=84), dict(stride=128, mvp=0, slot=126),
                    dict(stride=128, mvp=0, slot=128), dict(stride=128, mvp=0, slot=64, distance_sq=64),
                    dict(stride=128, mvp=0, model=64, distance_sq=108)):
            assert code(vis.set_instance_layout, 0, **bad) == GV_E_ARG, bad
            good()  # (the layout of the good emission is still in place after a refused one)
        vis.set_instance_layout(0, dtype=isup.FULL)
        vis.cull(0, views)
        assert code(vis.emit_instances, 1, [0]) == GV_E_ARG        # an unbound pool
        assert code(vis.emit_instances, 0, []) == GV_E_ARG         # no view
        assert code(vis.emit_instances, 0, [0, 1, 2]) == GV_E_ARG  # more views than were culled
        assert code(vis.emit_instances, 0, [1, 1]) == GV_E_ARG     # a view twice
        assert code(vis.emit_instances, 0, [8]) == GV_E_ARG        # no such view
        assert code(vis.emit_instances, 0, [5]) == GV_E_STATE      # a view with no results
        assert code(vis.emit_instances, 0, [0], device=(4096 + 4, 1 << 20)) == GV_E_ARG  # a misaligned target
        good()
        vis.cull(0, count_only)
        assert code(vis.emit_instances, 0, [0, 1]) == GV_E_STATE   # a count-only view
        check_emission(vis, twin, 0, count_only, [0], isup.FULL, sc.count, min_total=100)
        good()
        assert code(vis.instances_device, 3) == GV_E_STATE         # nothing emitted for that pool
        vis.cull(0, views)
        assert code(vis.instances_device, 0) == GV_E_STATE         # the emission ended with the pool's next cull
        assert code(vis.instances, 0) == GV_E_STATE
        vis.set_index_map(0, np.arange(sc.count - 1, dtype=np.uint32))
        assert code(vis.emit_instances, 0, [0, 1]) == GV_E_STATE   # an index map that does not cover the pool
        vis.set_index_map(0, None)
        good()
        vis.set_instance_layout(0, stride=None)
        assert code(vis.emit_instances, 0, [0]) == GV_E_STATE      # the layout was removed
        good()


def test_empty_result_and_reemission_after_churn_and_growth(twin):
    import torch
    full = scene.flat_scene(260_000)

    def cut(k):
        e2t = full.entity_to_transform.copy()
        e2t[e2t >= k] = 0xFFFFFFFF
        return scene.Scene(full.meshes[:k].copy(), full.transforms[:k].copy(), e2t)

    away = [scene.make_view(scene.ortho_rev_z(1.0, 1.0, 0.0, 1.0), camera_position=(3.0e6, 0.0, 0.0))]  # nothing of the scene in sight
    views = two_views()
    with GpuVisibility(device=0, linear_scan=True) as vis:
        sc = cut(150_000)
        bind(vis, sc)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.cull(0, away)
        pattern = np.full((64, 64), 0xA5, np.uint8)
        dev = torch.as_tensor(pattern, device="cuda:0")
        torch.cuda.synchronize()
        vis.emit_instances(0, [0], device=(dev.data_ptr(), pattern.nbytes))
        got, starts = vis.instances(0)
        assert starts.tolist() == [0, 0] and got.shape == (0, 64)
        assert dev.cpu().numpy().tobytes() == pattern.tobytes()
        vis.emit_instances(0, [0])
        assert vis.instances(0)[1].tolist() == [0, 0]
        vis.cull(0, views)
        check_emission(vis, twin, 0, views, [0, 1], isup.FULL, sc.count, min_total=75_000)
        # movers through dirty marks
        moved = np.arange(1000, 1400)
        sc.transforms["position"][moved, :3] += np.float32(25.0)
        vis.mark_dirty(GV_DIRTY_TRANSFORM, 1000, 400)
        vis.cull(0, views)
        check_emission(vis, twin, 0, views, [0, 1], isup.FULL, sc.count, min_total=75_000)
        # the pool grows, the mirror is re-ordered
        before = vis.stats()["mirror_reorders"]
        for k in (160_000, 175_000, 200_000, 230_000, 260_000):
            sc = cut(k)
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            vis.cull(0, views)
            check_emission(vis, twin, 0, views, [0, 1], isup.FULL, sc.count, min_total=k // 4)
        assert vis.stats()["mirror_reorders"] > before


def test_the_fourth_term_decides_the_sign_of_a_zero_on_the_device_too(twin):
    """Models scaled down to subnormals under the enclosing orthographic view (a.c2[2] = -1 / (far - near) < 0, a.c3[2] = 1/2 > 0):
    element [2][2] is fma(1/2, 0, fma(a.c2[2], c2.z, +0)); for a tiny positive c2.z the inner product underflows to -0 and the
    kept fourth term turns it into +0 — without the term it would stay -0. Kernel == twin on every bit, and the case occurs."""
    sc = scene.flat_scene(4096, defects=False)
    sc.transforms["rotation"] = (0, 0, 0, 1)
    sc.transforms["scale"][::2, :3] = np.float32(1e-39)
    views = [enclosing_ortho(shadow_pass=-1)]
    a22 = float(views[0]["view_proj"][10])
    assert a22 < 0 and views[0]["view_proj"][14] > 0
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, views)
        got, starts, fetched = check_emission(vis, twin, 0, views, [0], isup.FULL, sc.count, min_total=4000)
        c2z = fetched[0]["baked_model"][:, 8].astype(np.float64)
        hit = (c2z > 0) & (c2z * -a22 < 1e-46)  # the product lies below half the smallest subnormal: it rounds to -0
        assert hit.sum() >= 1000, int(hit.sum())
        mvp = got.view(isup.FULL)["mvp"].reshape(-1, 16).view(np.uint32)
        assert (mvp[hit, 10] == 0x00000000).all()  # +0, not 0x80000000


@pytest.fixture(scope="module")
def instance_writer(tmp_path_factory):
    """tests/cpp/instance_writer.cpp, built with the flags of the headless_tick rule of tests/cpp/Makefile"""
    cpp, lib = os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "garden_amd", "lib")
    exe = str(tmp_path_factory.mktemp("instance_writer") / "instance_writer")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-invalid-offsetof", "-fno-strict-aliasing", "-march=haswell",
                    "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(cpp, "instance_writer.cpp"),
                    "-o", exe, "-L" + lib, "-lgarden_vis", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64",
                    "-lm", "-lpthread"], check=True)
    return exe


def test_instance_writer_shim_matches_the_draw_loop(instance_writer):
    """GpuInstanceWriter of the drop-in against the draw loop restated from mesh.cpp:589-601 + sprite.cpp:126 (twin arithmetic):
    30 000 entities in three mesh systems, main pass + three cascades, 20 ticks with movers — every instance array byte for byte."""
    p = subprocess.run([instance_writer, "--entities", "30000", "--ticks", "20"], capture_output=True, text=True, timeout=300)
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert p.returncode == 0 and line["ok"], (p.stdout[-2000:], p.stderr[-2000:])
    assert line["systems"] == 3 and line["passes"] == 4 and line["ticks"] == 20, line
    assert line["instances"] >= 20 * 3 * 1000, line
