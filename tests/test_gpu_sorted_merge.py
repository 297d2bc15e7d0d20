"""gv_merge_sorted on the device: the shared sorted arrays of the reference (every sorted mesh system appends its records to one
array per sorted kind, one sort orders the whole array: mesh.cpp:247-261, 296-326), made by one merge launch from the lists
gv_pool_sort has ordered. Every case compares every byte of the merged array and the counts with the members' records, fetched
through the existing API, packed and merged by the C twin (tests/merge_twin.h), and checks that the members' fetched results are
the same bytes before and after the merge."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import merge_support as msup
from instances_support import same_results
from garden_amd import scene
from garden_amd.lib import GV_E_ARG, GV_E_STATE, GV_MAX_MERGE_GROUPS, GpuVisibility, GvError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_RESULTS_MAP_RECORDS = 1
EMPTY = "0-visible"  # a pool of 64 slots none of which is enabled


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return msup.build_twin(tmp_path_factory.mktemp("merge_twin"))


def enclosing_ortho(half=1.0e7, shadow_pass=-1, distance_2d=0):
    """an orthographic pass that holds the whole scene: every candidate becomes a record"""
    return scene.make_view(scene.ortho_rev_z(2 * half, 2 * half, -half, half), shadow_pass=shadow_pass, distance_2d=distance_2d)


def split_pools(sizes, seed=7):
    """One transform pool and one mesh pool per entry of `sizes`, over disjoint entities."""
    counts = [64 if s == EMPTY else s for s in sizes]
    sc = scene.flat_scene(sum(counts), seed=seed, defects=False)
    pools, at = [], 0
    for s, n in zip(sizes, counts):
        m = sc.meshes[at:at + n].copy()
        if s == EMPTY:
            m["isEnabled"] = 0
        pools.append(m)
        at += n
    return sc, pools


def bind_all(vis, sc, pools):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    for k, m in enumerate(pools):
        vis.bind_pool(k, m)
    vis.hierarchy_rebuild()


def cull_and_sort(vis, pools, views, descending):
    """descending: one flag, or one per view"""
    for k in range(len(pools)):
        vis.cull(k, views)
        for v in range(len(views)):
            vis.sort(v, descending=descending[v] if isinstance(descending, (list, tuple)) else descending, pool_id=k)


def fetch_members(vis, groups, pools):
    return [[vis.fetch(it[1], write_back=False, occupancy=len(pools[it[0]]), order="raw", pool_id=it[0]) for it in g["items"]] for g in groups]


def check_merge(vis, twin, groups, pools, fetch_first=True, slot_maps=None):
    """One gv_merge_sorted of `groups`; every group's merged bytes and counts against expected(), the members' fetched results the
    same bytes before and after (fetch_first=False: the merge is the first read, results compared afterwards only)."""
    before = fetch_members(vis, groups, pools) if fetch_first else None
    vis.merge_sorted(groups)
    got = [vis.merged(g["group_id"], g["dtype"]) for g in groups]
    after = fetch_members(vis, groups, pools)
    if before is not None:
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                same_results(x, y)
    totals = []
    for g, (records, counts), fetched in zip(groups, got, after):
        exp, exp_counts = msup.expected(twin, g["dtype"], fetched, g["items"], g.get("descending"), slot_maps)
        assert counts.tolist() == exp_counts.tolist()
        assert records.view(np.uint8).tobytes() == exp.tobytes()
        totals.append(int(counts[-1]))
    return totals


def one_group(pools, dtype=msup.SORTED_MESH, descending=True, view=0, group_id=0):
    return dict(group_id=group_id, items=[(k, view, 10 + k, 48 + 16 * k) for k in range(len(pools))], descending=descending, dtype=dtype)


SHAPES = {
    "one": [4097],
    "two": [1023, 1025],
    "three_with_an_empty_one_between": [65, EMPTY, 257],
    "eight": [1, 63, 64, 65, 255, 256, 257, 4095],
    "one_long_and_fifteen_single_records": [70_000] + [1] * 15,
    "sixteen": [EMPTY, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4097, 20_000, 1, 64, 257],
    "every_sort_path": [20_000, 70_000, 300_000],   # past the batch sort, past the rank-only sort, the radix path
    "all_empty": [EMPTY, EMPTY, EMPTY],
}


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_merged_bytes_against_the_twin(twin, shape, descending):
    sizes = SHAPES[shape]
    sc, pools = split_pools(sizes)
    with GpuVisibility(device=0) as vis:
        bind_all(vis, sc, pools)
        cull_and_sort(vis, pools, [enclosing_ortho()], descending)
        total, = check_merge(vis, twin, [one_group(pools, descending=descending)], pools)
        assert total == sum(s for s in sizes if s != EMPTY)  # every candidate is a record
        # again with the items the other way round: another tie order, another array
        g = one_group(pools, descending=descending)
        g["items"].reverse()
        check_merge(vis, twin, [g], pools)


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("copies", [2, 4, 16])
def test_ties_across_lists_go_to_the_list_in_front(twin, copies, descending):
    """the same scene bound as several pools: every key is tied across every list"""
    sc = scene.flat_scene(3000, defects=False)
    pools = [sc.meshes.copy() for _ in range(copies)]
    with GpuVisibility(device=0) as vis:
        bind_all(vis, sc, pools)
        cull_and_sort(vis, pools, [enclosing_ortho()], descending)
        g = one_group(pools, descending=descending)
        total, = check_merge(vis, twin, [g], pools)
        assert total == copies * 3000
        records, _ = vis.merged(0, msup.SORTED_MESH)
        tied = records["distanceSq"][1:] == records["distanceSq"][:-1]
        assert tied.sum() >= (copies - 1) * 3000 and (np.diff(records["bufferIndex"].astype(np.int64))[tied] >= 0).all()


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_negative_keys_of_distance_2d_views(twin, descending):
    sc, pools = split_pools([1025, 4097, 257, 20_000])
    with GpuVisibility(device=0) as vis:
        bind_all(vis, sc, pools)
        cull_and_sort(vis, pools, [enclosing_ortho(distance_2d=1)], descending)
        check_merge(vis, twin, [one_group(pools, descending=descending)], pools)
        keys = vis.merged(0, msup.SORTED_MESH)[0]["distanceSq"]
        assert (keys < 0).sum() > 5000 and (keys > 0).sum() > 5000  # entities on both sides of z = -1
        assert (np.diff(keys) <= 0).all() if descending else (np.diff(keys) >= 0).all()


def test_first_read_inside_a_batch_launches_the_deferred_sorts(twin):
    sc, pools = split_pools([4095, 257, 9000])
    with GpuVisibility(device=0) as vis:
        bind_all(vis, sc, pools)
        cull_and_sort(vis, pools, [enclosing_ortho()], True)
        vis.merge_sorted([one_group(pools)])
        outside = vis.merged(0, msup.SORTED_MESH)[0].tobytes()
        vis.cull_batch_begin()
        cull_and_sort(vis, pools, [enclosing_ortho()], True)
        total, = check_merge(vis, twin, [one_group(pools)], pools, fetch_first=False)
        vis.cull_batch_end()
        assert total == 4095 + 257 + 9000
        assert vis.merged(0, msup.SORTED_MESH)[0].tobytes() == outside


def test_several_groups_in_one_launch(twin):
    """two main-pass groups (translucent descending, UI ascending) and two shadow-pass groups in ONE call: one launch, counted as a sort"""
    sc, pools = split_pools([4097, 1023, 257, 65, 9000])
    views = [enclosing_ortho(), enclosing_ortho(half=2.0e7, shadow_pass=0), enclosing_ortho(half=3.0e7, shadow_pass=1)]
    with GpuVisibility(device=0) as vis:
        bind_all(vis, sc, pools)
        cull_and_sort(vis, pools, views, [True, True, True])
        for k in (3, 4):  # the UI systems sort their main pass the other way
            vis.sort(0, descending=False, pool_id=k)
        trans = [(k, 0, k, 64) for k in (0, 1, 2)]
        groups = [dict(group_id=0, items=trans, descending=True, dtype=msup.SORTED_MESH),
                  dict(group_id=1, items=[(3, 0, 3, 32), (4, 0, 4, 32)], descending=False, dtype=msup.SORTED_MESH),
                  dict(group_id=5, items=[(k, 1, 0, 64) for k in (0, 1, 2)], descending=True, dtype=msup.SORTED_MESH),
                  dict(group_id=6, items=[(k, 2, 1, 64) for k in (2, 0, 1)], descending=True, dtype=msup.WIDE)]
        before = fetch_members(vis, groups, pools)
        vis.wait()
        vis.stats_reset()
        vis.merge_sorted(groups)
        vis.wait()
        launches = vis.stats()["launches"]
        assert launches["sort"] == 1 and sum(launches.values()) == 1, launches
        totals = check_merge(vis, twin, groups, pools)
        assert totals == [4097 + 1023 + 257, 65 + 9000, 4097 + 1023 + 257, 4097 + 1023 + 257]
        for a, b in zip(before, fetch_members(vis, groups, pools)):
            for x, y in zip(a, b):
                same_results(x, y)


def test_caller_owned_target_holding_half_the_total(twin):
    import torch
    sc, pools = split_pools([4097, 1025, 257])
    g = one_group(pools)
    stride = g["dtype"].itemsize
    with GpuVisibility(device=0) as vis:
        bind_all(vis, sc, pools)
        cull_and_sort(vis, pools, [enclosing_ortho()], True)
        fetched, = fetch_members(vis, [g], pools)
        exp, exp_counts = msup.expected(twin, g["dtype"], fetched, g["items"], True)
        total = int(exp_counts[-1])
        half = total // 2
        pattern = np.random.Generator(np.random.PCG64(3)).integers(1, 255, (total + 9, stride), dtype=np.uint8)
        dev = torch.as_tensor(pattern, device="cuda:0")
        torch.cuda.synchronize()  # (the copy runs on torch's stream; the library's stream is non-blocking)
        vis.merge_sorted([dict(g, device=(dev.data_ptr(), half * stride + stride - 1))])
        assert vis.merge_device(0)[0] == dev.data_ptr()
        host = pattern.copy()
        counts = np.zeros(len(pools) + 1, np.uint32)
        cp = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        vis._check(vis.lib.gv_merge_fetch(vis.ctx, 0, host.ctypes.data, host.nbytes, cp, len(counts)))
        assert counts.tolist() == exp_counts.tolist()  # the true total
        on_device = dev.cpu().numpy()
        assert on_device[:half].tobytes() == exp[:half * stride].tobytes()
        assert on_device[half:].tobytes() == pattern[half:].tobytes()  # the guard bytes behind the target
        assert host[:half].tobytes() == exp[:half * stride].tobytes() and host[half:].tobytes() == pattern[half:].tobytes()
        # a host array or a counts array that is too small: GV_E_ARG, nothing written
        small = pattern[:total - 1].copy()
        counts[:] = 77
        assert vis.lib.gv_merge_fetch(vis.ctx, 0, small.ctypes.data, small.nbytes, cp, len(counts)) == GV_E_ARG
        assert vis.lib.gv_merge_fetch(vis.ctx, 0, host.ctypes.data, host.nbytes, cp, len(counts) - 1) == GV_E_ARG
        assert small.tobytes() == pattern[:total - 1].tobytes() and counts.tolist() == [77] * len(counts)
        # the library's own buffer afterwards
        check_merge(vis, twin, [g], pools)


@pytest.mark.parametrize("dtype", [msup.SORTED_MESH, msup.WIDE, msup.record_dtype(stride=128, component_offset=8, baked_model=32, distance_sq=100, buffer_index=0)],
                         ids=["sorted_mesh_64", "wide_80_no_buffer_index", "stride_128"])
def test_layouts_and_a_slot_map(twin, dtype):
    sc, pools = split_pools([4097, 1025, 300])
    rng = np.random.Generator(np.random.PCG64(11))
    index_map = (rng.permutation(len(pools[1])) + 100_000).astype(np.uint32)
    with GpuVisibility(device=0) as vis:
        bind_all(vis, sc, pools)
        vis.set_index_map(1, index_map)
        vis.set_result_mapping(1, GV_RESULTS_MAP_RECORDS)  # pool 1 delivers records in world slots
        cull_and_sort(vis, pools, [enclosing_ortho()], True)
        check_merge(vis, twin, [one_group(pools, dtype=dtype)], pools, slot_maps={1: index_map})
        records, _ = vis.merged(0, dtype)
        offsets = records["componentOffset"]
        assert (offsets >= 100_000 * 64).sum() == len(pools[1])  # (pool 1's component stride is 48 + 16)


def code(call, *args, **kwargs):
    with pytest.raises(GvError) as e:
        call(*args, **kwargs)
    return e.value.code


def test_errors_leave_the_context_usable(twin):
    sc, pools = split_pools([300, 257, 65, 64])
    M = msup.SORTED_MESH
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        for k in range(3):
            vis.bind_pool(k, pools[k])  # (pool 3 stays unbound)
        vis.hierarchy_rebuild()
        views = [enclosing_ortho(), enclosing_ortho(half=2.0e7, shadow_pass=0)]
        for k in range(3):
            vis.cull(k, views)
            vis.sort(0, descending=True, pool_id=k)
        vis.cull(2, [views[0], dict(views[1], emit_records=0)])
        vis.sort(0, descending=True, pool_id=2)
        good = dict(group_id=0, items=[(0, 0, 0, 64), (1, 0, 1, 64)], descending=True, dtype=M)
        bad = lambda **kw: [dict(good, **kw)]
        # GV_E_ARG
        assert vis.lib.gv_merge_sorted(vis.ctx, vis.merge_groups([good])[0], 0) == GV_E_ARG
        assert code(vis.merge_sorted, [dict(good, group_id=k, items=[(0, 0, 0, 64), (1, 0, 0, 64), (2, 0, 0, 64)]) for k in range(11)]) == GV_E_ARG  # 33 items
        assert code(vis.merge_sorted, bad(group_id=GV_MAX_MERGE_GROUPS)) == GV_E_ARG
        assert code(vis.merge_sorted, [good, good]) == GV_E_ARG  # a group id listed twice
        assert code(vis.merge_sorted, bad(items=[])) == GV_E_ARG
        assert code(vis.merge_sorted, bad(items=[(0, 0, 0, 64)] * 17)) == GV_E_ARG
        assert code(vis.merge_sorted, bad(items=[(0, 0, 0, 64), (3, 0, 0, 64)])) == GV_E_ARG  # an unbound pool
        assert code(vis.merge_sorted, bad(items=[(0, 0, 0, 64), (16, 0, 0, 64)])) == GV_E_ARG
        assert code(vis.merge_sorted, bad(items=[(0, 0, 0, 64), (1, 2, 0, 64)])) == GV_E_ARG  # a view beyond the pool's last cull
        assert code(vis.merge_sorted, bad(items=[(0, 0, 0, 64), (1, 0, 0, 64), (0, 0, 1, 64)])) == GV_E_ARG  # the same (pool, view) twice
        for stride in (0, 8, 72, 144):
            assert code(vis.merge_sorted, bad(dtype=None, stride=stride, component_offset=0, baked_model=8, distance_sq=56, buffer_index=60)) == GV_E_ARG
        layout = dict(dtype=None, stride=64, component_offset=0, baked_model=8, distance_sq=56, buffer_index=60)
        assert code(vis.merge_sorted, bad(**dict(layout, baked_model=4))) == GV_E_ARG    # overlaps componentOffset
        assert code(vis.merge_sorted, bad(**dict(layout, buffer_index=56))) == GV_E_ARG  # overlaps distanceSq
        assert code(vis.merge_sorted, bad(**dict(layout, baked_model=20))) == GV_E_ARG   # leaves the stride
        assert code(vis.merge_sorted, bad(**dict(layout, distance_sq=64))) == GV_E_ARG
        assert code(vis.merge_sorted, bad(**dict(layout, distance_sq=58))) == GV_E_ARG   # misaligned field
        assert code(vis.merge_sorted, bad(device=(4096 + 4, 1 << 20))) == GV_E_ARG       # a misaligned target
        # GV_E_STATE
        assert code(vis.merge_sorted, bad(items=[(0, 0, 0, 64), (2, 1, 0, 64)])) == GV_E_STATE  # a count-only member
        assert code(vis.merge_sorted, bad(items=[(0, 0, 0, 64), (1, 1, 0, 64)])) == GV_E_STATE  # never sorted since its cull
        assert code(vis.merge_sorted, bad(descending=False)) == GV_E_STATE                      # sorted the other way
        vis.set_index_map(1, np.arange(100, dtype=np.uint32))
        vis.set_result_mapping(1, GV_RESULTS_MAP_RECORDS)
        assert code(vis.merge_sorted, [good]) == GV_E_STATE  # a slot map that does not cover the pool
        vis.set_result_mapping(1, 0)
        assert code(vis.merge_device, 0) == GV_E_STATE and code(vis.merged, 0, M) == GV_E_STATE  # nothing merged yet
        assert code(vis.merge_device, GV_MAX_MERGE_GROUPS) == GV_E_ARG and code(vis.merged, GV_MAX_MERGE_GROUPS, M) == GV_E_ARG
        # after all that: the merge works
        check_merge(vis, twin, [good], pools)
        assert vis.merge_device(0)[0] and vis.merge_device(0)[1]
        # a gv_cull of one member ends the group's result; the other pool's cull results are not concerned
        vis.cull(1, views)
        assert code(vis.merge_device, 0) == GV_E_STATE and code(vis.merged, 0, M) == GV_E_STATE
        assert code(vis.merge_sorted, [good]) == GV_E_STATE  # pool 1 is not sorted any more
        vis.sort(0, descending=True, pool_id=1)
        check_merge(vis, twin, [good], pools)


@pytest.fixture(scope="module")
def sorted_merge_driver(tmp_path_factory):
    """tests/cpp/sorted_merge.cpp, built with the headless-tick flags (as pick_select.cpp and sprite_instances.cpp are)"""
    cpp, lib = os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "garden_amd", "lib")
    exe = str(tmp_path_factory.mktemp("sorted_merge") / "sorted_merge")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-invalid-offsetof", "-fno-strict-aliasing", "-march=haswell",
                    "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(cpp, "sorted_merge.cpp"),
                    "-o", exe, "-L" + lib, "-lgarden_vis", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64",
                    "-lm", "-lpthread"], check=True)
    return exe


def test_the_shim_delivers_the_same_shared_arrays_with_the_merge_on_the_device(sorted_merge_driver):
    """two Translucent, two UI and one Opaque system, a main pass and two cascades, 30 000 entities, 20 animated ticks through two
    GpuVisibilitySystems (mergeOnDevice off / on): draw indices, counters, isVisible and the shared arrays byte for byte, and
    sortedArraysHold's conditions in both modes"""
    p = subprocess.run([sorted_merge_driver, "--entities", "30000", "--ticks", "20"], capture_output=True, text=True, timeout=300)
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert p.returncode == 0 and line["ok"], (p.stdout[-2000:], p.stderr[-2000:])
    assert line["systems"] == 5 and line["passes"] == 3 and line["ticks"] == 20, line
    assert line["sorted_records"] >= 20 * 5000, line
