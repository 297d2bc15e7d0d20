"""The sphere-stream cull of large flat pools covers K 256-entry tiles per workgroup (cull_hot_kernel, K chosen from the pool
size: 1 = cull_kernel, 2 from 8 Ki tiles, 4 from 16 Ki tiles). Every entry must get the decision it gets from one tile per
workgroup: visible_idx, bakedModel, distanceSq, isVisible and drawCount against the CPU oracle, for pool sizes whose last
super-tile is partial, with views where everything is inside, everything is outside, or a mix, with and without Hi-Z."""
import numpy as np
import pytest

from garden_amd import scene

pytestmark = pytest.mark.gpu

GV_DIRTY_TRANSFORM = 0
# K = 1 (just above the sphere-stream threshold / around 1 M), K = 2 (8194 tiles, the last holding one entry),
# K = 4 (16 387 tiles: the last super-tile has three tiles, the third partial)
SIZES = [65_537, 1_000_003, 2_097_665, 4_195_000]


def identity_view(width, cam=(0.0, 0.0, 0.0), **kw):
    """An axis-aligned orthographic main-pass view `width` across, centred on `cam`."""
    proj = scene.ortho_rev_z(width, width, -width * 0.5, width * 0.5)
    return scene.make_view(scene.mul_cm(proj, scene.view_from_quat(np.array([0, 0, 0, 1], np.float32))), camera_position=cam, **kw)


def check(gpu, oracle, sc, view, hz=None):
    gpu.cull(0, [view])
    got = gpu.fetch(0, write_back=False, occupancy=sc.count)
    m2 = sc.meshes.copy()
    exp = oracle.prepare_meshes(m2, sc.transforms, sc.entity_to_transform, view, hiz=hz)
    assert got["draw_count"] == exp["draw_count"]
    assert np.array_equal(got["is_visible"], m2["isVisible"])
    if view.get("emit_records", 1):
        o = np.argsort(exp["visible_idx"], kind="stable")
        assert np.array_equal(got["visible_idx"], exp["visible_idx"][o])
        assert np.array_equal(got["baked_model"].view(np.uint32), exp["baked_model"][o].view(np.uint32))
        assert np.array_equal(got["distance_sq"].view(np.uint32), exp["distance_sq"][o].view(np.uint32))
    return exp["draw_count"]


@pytest.fixture(scope="module")
def pyramid():
    depth = scene.synthetic_depth(1024, 512)
    depth[:, :400] = np.maximum(depth[:, :400], np.float32(0.3))
    return depth


@pytest.mark.parametrize("n", SIZES)
def test_hot_tiles_match_the_oracle(gpu_linear, oracle, pyramid, n):
    gpu = gpu_linear
    sc = scene.flat_scene(n)
    rng = np.random.Generator(np.random.PCG64(n))
    # non-finite positions and scales (they reach the exact test), inactive transforms, at both ends and in between
    odd = np.unique(np.concatenate([np.arange(40), np.arange(n - 300, n), rng.choice(n, 200, replace=False)]))
    sc.transforms["position"][odd[0::4], 0] = np.nan
    sc.transforms["position"][odd[1::4], 1] = np.inf
    sc.transforms["scale"][odd[2::4], 2] = -np.inf
    sc.transforms["selfActive"][odd[3::4]] = 0
    gpu.hiz_build(pyramid)
    hz = oracle.Hiz(pyramid)
    gpu.bind_transforms(sc.transforms, sc.entity_to_transform)
    gpu.bind_pool(0, sc.meshes)
    gpu.hierarchy_rebuild()
    main = scene.main_camera_view()
    mixed = check(gpu, oracle, sc, main)
    assert 0 < mixed < n
    assert check(gpu, oracle, sc, dict(main, use_hiz=1), hz) < mixed
    check(gpu, oracle, sc, dict(main, emit_records=0))  # the cull writes isVisible itself
    check(gpu, oracle, sc, dict(main, emit_records=0, use_hiz=1), hz)
    side = 400.0 * n ** (1.0 / 3.0)
    inside = identity_view(side)
    assert check(gpu, oracle, sc, inside) > n // 2
    check(gpu, oracle, sc, dict(inside, use_hiz=1), hz)
    outside = identity_view(1.0, cam=(1e6, 1e6, 1e6))
    assert check(gpu, oracle, sc, outside) < odd.size  # (only non-finite entries: their exact test cannot reject them)
    assert check(gpu, oracle, sc, dict(outside, use_hiz=1), hz) < odd.size
    # an edit between two culls: the sphere-stream patch runs in front of the cull
    vis = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, main)["visible_idx"]
    hidden = np.setdiff1d(np.arange(40, n), vis)
    moved = np.sort(rng.choice(hidden, 64, replace=False))
    sc.transforms["position"][moved, :3] = sc.transforms["position"][rng.choice(vis, 64), :3]
    sc.transforms["selfActive"][moved] = 1
    for s in moved:
        gpu.mark_dirty(GV_DIRTY_TRANSFORM, int(s), 1)
    assert check(gpu, oracle, sc, main) > mixed
    check(gpu, oracle, sc, dict(main, use_hiz=1), hz)
