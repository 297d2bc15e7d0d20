"""The linear-scan cull hands its work units (256-entry tiles, or super-tiles of K tiles) to the workgroups in an order that depends
on the view (garden_amd/csrc/gv_tile_order.hpp: XCD runs for frustum-only views, the identity for Hi-Z views), and a Hi-Z view of a
large flat pool takes fewer tiles per workgroup than a frustum-only view of the same pool (hot_tiles_per_workgroup_hiz). Whatever the order
and K, every entry gets the decision of the CPU oracle, bit for bit: visible_idx, isVisible, bakedModel and drawCount — for pools
with fewer units than one XCD run or one workgroup, for K = 1, 2 and 4 with a partial last super-tile, with views where everything
is inside, everything is outside, or a mix, count-only views whose cull writes isVisible itself, and an edit between two culls."""
import numpy as np
import pytest

from garden_amd import scene
from hiz_paths_support import header_constant

pytestmark = pytest.mark.gpu

GV_DIRTY_TRANSFORM = 0
# 1, 255, 257: fewer units than anything the orders are cut into; 65 537: K = 1, 257 tiles; 2 097 665: 8194 tiles, K = 2, the last
# super-tile holds one entry; 4 195 000: 16 387 tiles, K = 4 for a frustum-only view and K = 2 for a Hi-Z view, the last tile partial
# (2 097 665 is K = 2 for a frustum-only view and K = 1 for a Hi-Z view)
SIZES = [1, 255, 257, 65_537, 2_097_665, 4_195_000]


def identity_view(width, cam=(0.0, 0.0, 0.0), **kw):
    """An axis-aligned orthographic main-pass view `width` across, centred on `cam`."""
    proj = scene.ortho_rev_z(width, width, -width * 0.5, width * 0.5)
    return scene.make_view(scene.mul_cm(proj, scene.view_from_quat(np.array([0, 0, 0, 1], np.float32))), camera_position=cam, **kw)


def expected(oracle, sc, view, hz=None):
    """the oracle's frame of one view (a count-only view of the same camera has the same one): computed once, shared"""
    m2 = sc.meshes.copy()
    exp = oracle.prepare_meshes(m2, sc.transforms, sc.entity_to_transform, view, hiz=hz)
    o = np.argsort(exp["visible_idx"], kind="stable")
    return dict(draw_count=exp["draw_count"], is_visible=m2["isVisible"], visible_idx=exp["visible_idx"][o], baked_model=exp["baked_model"][o])


def check(gpu, sc, view, exp):
    gpu.cull(0, [view])
    got = gpu.fetch(0, write_back=False, occupancy=sc.count)
    assert got["draw_count"] == exp["draw_count"]
    assert np.array_equal(got["is_visible"], exp["is_visible"])
    if view.get("emit_records", 1):
        assert np.array_equal(got["visible_idx"], exp["visible_idx"])
        assert np.array_equal(got["baked_model"].view(np.uint32), exp["baked_model"].view(np.uint32))
    return exp["draw_count"]


@pytest.fixture(scope="module")
def pyramid():
    depth = scene.synthetic_depth(1024, 512)
    depth[:, :400] = np.maximum(depth[:, :400], np.float32(0.3))
    return depth


@pytest.mark.parametrize("n", SIZES)
def test_every_order_and_k_matches_the_oracle(gpu_linear, oracle, pyramid, n):
    gpu = gpu_linear
    sc = scene.flat_scene(n, defects=False)  # flat and exactly paired: the large pools take the sphere stream
    rng = np.random.Generator(np.random.PCG64(n))
    gpu.hiz_build(pyramid)
    hz = oracle.Hiz(pyramid)
    gpu.bind_transforms(sc.transforms, sc.entity_to_transform)
    gpu.bind_pool(0, sc.meshes)
    gpu.hierarchy_rebuild()
    main = scene.main_camera_view()
    side = 400.0 * max(n, 1000) ** (1.0 / 3.0)
    inside, outside = identity_view(side), identity_view(1.0, cam=(1e6, 1e6, 1e6))
    # Hi-Z views: a mix, everything inside the frustum, everything outside, and count-only (the cull writes isVisible)
    mixed_hiz, main_hiz = expected(oracle, sc, dict(main, use_hiz=1), hz), dict(main, use_hiz=1)
    mixed = check(gpu, sc, main_hiz, mixed_hiz)
    check(gpu, sc, dict(inside, use_hiz=1), expected(oracle, sc, dict(inside, use_hiz=1), hz))
    assert check(gpu, sc, dict(outside, use_hiz=1), expected(oracle, sc, dict(outside, use_hiz=1), hz)) == 0
    check(gpu, sc, dict(main_hiz, emit_records=0), mixed_hiz)
    # a frustum-only view of the same pool (XCD runs, K from the pool's size alone), with records and count-only
    frustum = expected(oracle, sc, main)
    survivors = check(gpu, sc, main, frustum)
    check(gpu, sc, dict(main, emit_records=0), frustum)
    if n > 1000:
        assert 0 < mixed < survivors < n
    # an edit between two culls: entries move to where visible ones are (none visible: they only change their active flag)
    vis = frustum["visible_idx"]
    moved = np.sort(rng.choice(n, min(64, n), replace=False))
    if vis.size:
        sc.transforms["position"][moved, :3] = sc.transforms["position"][rng.choice(vis, moved.size), :3]
    sc.transforms["selfActive"][moved[::2]] = 0
    for s in moved:
        gpu.mark_dirty(GV_DIRTY_TRANSFORM, int(s), 1)
    check(gpu, sc, main_hiz, expected(oracle, sc, main_hiz, hz))
    check(gpu, sc, main, expected(oracle, sc, main))


def test_a_hiz_view_of_a_very_large_pool_takes_four_tiles_per_workgroup(gpu_linear, oracle, pyramid):
    """cull_hot_kernel<true, 4> starts at kHizHotK4Tiles tiles for a Hi-Z view: one tile more, the last super-tile holding one
    partial tile. The size is the threshold's, so the case takes longer than the others: one oracle frame, shared by both views."""
    gpu, n = gpu_linear, header_constant("gv_kernels.hpp", "kHizHotK4Tiles") * 256 + 84
    sc = scene.flat_scene(n, defects=False)
    gpu.hiz_build(pyramid)
    gpu.bind_transforms(sc.transforms, sc.entity_to_transform)
    gpu.bind_pool(0, sc.meshes)
    gpu.hierarchy_rebuild()
    main_hiz = scene.main_camera_view(use_hiz=1)
    exp = expected(oracle, sc, main_hiz, oracle.Hiz(pyramid))
    assert 0 < check(gpu, sc, main_hiz, exp) < n
    check(gpu, sc, dict(main_hiz, emit_records=0), exp)
