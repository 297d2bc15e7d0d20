"""Census of the sphere-entry occlusion proof (hiz_sphere_occluded, restated in tests/hiz_sphere_twin.h) against the oracle, on the
CPU: over the cfg3 bench scene (make_tile_scene, main_camera_view) and seeded random cameras, the twin's verdict per entry is set
against the oracle's isVisible. CONDITION: no entry the twin calls occluded is visible to the oracle. The share of the oracle's
"frustum survivor but occluded" entries the twin settles is printed (profiles/r12_hiz_sphere.md records the 10 M figures: walls
95.5 %, noise 27.7 %, 0 wrong; run once by hand at full size, the sizes here keep the file within the non-GPU tier's time)."""
import math

import numpy as np
import pytest

import hiz_sphere_support as hs
from garden_amd import scene
from garden_amd.benchlib.workloads import HIZ_SIZE, WORKLOADS, make_tile_scene

THREADS = 4


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return hs.build_twin(tmp_path_factory.mktemp("hiz_sphere_twin"))


@pytest.fixture(scope="module")
def bench_scene(twin, oracle):
    sc = make_tile_scene(WORKLOADS["cfg3"], 2_000_000, 0, 1)
    return sc, hs.hot_entries(twin, oracle, sc, threads=THREADS)


def random_camera(seed, side):
    """a perspective main-pass camera somewhere inside the world cube, looking anywhere"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q = rng.normal(size=4)
    q = (q / np.linalg.norm(q)).astype(np.float32)
    proj = scene.persp_inf_rev_z(math.radians(float(rng.uniform(40.0, 110.0))), float(rng.uniform(1.0, 2.0)), float(rng.choice([0.01, 0.1, 1.0])))
    pos = rng.uniform(-0.4 * side, 0.4 * side, 3)
    return scene.make_view(scene.mul_cm(proj, scene.view_from_quat(q)), camera_position=tuple(float(x) for x in pos), use_hiz=1)


@pytest.mark.parametrize("depth_name", ["walls", "noise"])
@pytest.mark.parametrize("rg16f", [False, True])
def test_bench_scene_census(twin, oracle, bench_scene, depth_name, rg16f):
    sc, hot = bench_scene
    depth = scene.synthetic_depth(HIZ_SIZE, HIZ_SIZE) if depth_name == "walls" else scene.noise_depth(HIZ_SIZE, HIZ_SIZE)
    hz = oracle.Hiz(depth, threads=THREADS, rg16f=rg16f)
    r = hs.census(twin, oracle, sc, hz, scene.main_camera_view(use_hiz=1), hot, threads=THREADS)
    print(f"census {depth_name} rg16f={rg16f}: {r}")
    assert r["occluded"] > 0 and r["visible"] > 0
    assert r["wrong"][hs.STEP] == 0
    if depth_name == "walls":
        assert r["settled"][hs.STEP] > 0  # (the go/no-go share, >= one half, is a 10 M figure: profiles/r12_hiz_sphere.md)


@pytest.mark.parametrize("seed", range(8))
def test_random_camera_census(twin, oracle, seed):
    n = 1_000_000
    sc = scene.flat_scene(n, seed=scene.SEED + 100 + seed)
    hot = hs.hot_entries(twin, oracle, sc, threads=THREADS)
    depth = scene.synthetic_depth(1024, 512, seed=scene.SEED + seed) if seed % 2 == 0 else scene.noise_depth(1024, 512, seed=scene.SEED + seed)
    hz = oracle.Hiz(depth, threads=THREADS, rg16f=seed % 4 >= 2)
    r = hs.census(twin, oracle, sc, hz, random_camera(seed, 100.0 * n ** (1.0 / 3.0)), hot, threads=THREADS)
    print(f"census camera {seed}: {r}")
    assert r["wrong"][hs.STEP] == 0


def test_a_pyramid_that_is_not_nested_declines(twin, oracle):
    sc = scene.flat_scene(100_000)
    hot = hs.hot_entries(twin, oracle, sc)
    hz = oracle.Hiz(scene.synthetic_depth(1000, 500))  # 125 wide at level 3: the reference rule skips texels there
    assert not hs.nested(hz)
    assert not hs.verdicts(twin, hz, scene.main_camera_view(use_hiz=1), hot).any()
