"""GPU parity of the Hi-Z pyramid over every build path: hiz_reduce (garden_amd/csrc/gv_context.cpp) picks the kernel for each
group of levels from the level sizes alone, so the sizes here (tests/hiz_paths_support.py SIZES) are chosen by that dispatch,
restated as hiz_plan and proved to cover it by tests/test_hiz_plan_census.py on the CPU. Also: pyramids of one or two levels,
occlusion queries against pyramids of every class, many builds on one context, and a device-resident depth image rebuilt in place.

Bar, as in test_hiz_pyramid_parity: every level >= 1 equals the oracle's bit for bit (no tolerance), both rules, both formats."""
import numpy as np
import pytest

import hiz_paths_support as hp
from garden_amd import scene

pytestmark = pytest.mark.gpu

ENTITIES = 20_000


def pyramid_cases():
    """(size, rule, rg16f): both formats always; both rules where some level is odd (sizes that are even at every level do not
    read the rule). The largest image (34 * 10^6 texels) is even throughout: one rule, both formats — its oracle pyramid takes
    well under 2 s on one CPU core in either format."""
    out = []
    for size in hp.SIZES:
        rules = (0, 1) if hp.reads_rule(hp.mip_sizes(*size)) else (0,)
        out += [pytest.param(size, rule, rg16f, id=f"{size[0]}x{size[1]}-rule{rule}-{'rg16f' if rg16f else 'rg32f'}")
                for rule in rules for rg16f in (False, True)]
    return out


@pytest.mark.parametrize("size,rule,rg16f", pyramid_cases())
def test_pyramid_parity(oracle, size, rule, rg16f):
    from garden_amd.lib import GpuVisibility
    w, h = size
    depth = hp.special_depth(w, h)
    exp = oracle.Hiz(depth, rule=rule, rg16f=rg16f, threads=4 if w * h > 1 << 22 else 1)
    with GpuVisibility(device=0, hiz_rule=rule, hiz_rg16f=rg16f) as vis:
        vis.hiz_build(depth)
        hp.assert_pyramid_equal(vis, exp, f"{w} x {h} {hp.plan_of(size)}")


@pytest.mark.parametrize("size", hp.REFUSED, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sides_beyond_the_limit_are_refused(size):
    """(so the single-level kernel never reads pairs inside hiz_reduce: tests/test_hiz_plan_census.py pins that as unreachable)"""
    from garden_amd.lib import GV_E_ARG, GpuVisibility, GvError
    with GpuVisibility(device=0) as vis:
        with pytest.raises(GvError) as refused:
            vis.hiz_build(np.zeros((size[1], size[0]), dtype=np.float32))
        assert refused.value.code == GV_E_ARG


@pytest.fixture(scope="module")
def flat():
    return scene.flat_scene(ENTITIES)


@pytest.fixture(scope="module")
def frustum_only(oracle, flat):
    return oracle.prepare_meshes(flat.meshes.copy(), flat.transforms, flat.entity_to_transform, scene.main_camera_view())["draw_count"]


@pytest.fixture(scope="module", params=[False, True], ids=["rg32f", "rg16f"])
def bound(request, flat):
    """a context of its own per format with the 20 000 entities bound: every query test and every build of it reuses that mirror"""
    from garden_amd.lib import GpuVisibility
    with GpuVisibility(device=0, hiz_rg16f=request.param) as vis:
        vis.bind_transforms(flat.transforms, flat.entity_to_transform)
        vis.bind_pool(0, flat.meshes)
        yield vis, request.param


@pytest.mark.parametrize("size", hp.QUERY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_query_parity(oracle, flat, frustum_only, bound, size):
    """The occlusion query against a pyramid of every build path and of one and two levels: level selection and the clamps of the
    footprint on images one texel high or wide. Where the image has an area, the query must reject some survivors of the frustum
    and keep others (tests/test_hiz_plan_census.py checks that with the oracle alone)."""
    vis, rg16f = bound
    depth = hp.base_depth(*size)
    vis.hiz_build(depth)
    hz = oracle.Hiz(depth, rg16f=rg16f)
    view = scene.main_camera_view(use_hiz=1)
    got, exp, exp_vis = hp.cull_both(vis, oracle, flat, view, hz)
    if min(size) > 1 and size not in hp.DEGENERATE:
        assert 0 < exp["draw_count"] < frustum_only
    hp.assert_cull_equal(got, exp, exp_vis, f"{size}")
    hp.assert_pyramid_equal(vis, hz, f"{size}")


def check_build(vis, oracle, flat, depth, rg16f, what):
    """after a build from `depth`: cull (level 1 still virtual where it can be), every level, cull again (level 1 now stored)"""
    hz = oracle.Hiz(depth, rg16f=rg16f, threads=4)
    view = scene.main_camera_view(use_hiz=1)
    hp.assert_cull_equal(*hp.cull_both(vis, oracle, flat, view, hz), f"{what}: cull after the build")
    hp.assert_pyramid_equal(vis, hz, what)
    hp.assert_cull_equal(*hp.cull_both(vis, oracle, flat, view, hz), f"{what}: cull after reading every level")
    return hz


def test_many_builds_on_one_context(oracle, flat, bound):
    """hp.SEQUENCE on one context: the level-1 flags, the level offsets and the allocation carry over from build to build."""
    vis, rg16f = bound
    view = scene.main_camera_view(use_hiz=1)
    for step, (size, seed) in enumerate(hp.SEQUENCE):
        depth = hp.base_depth(*size, seed=scene.SEED + seed)
        vis.hiz_build(depth)
        hz = check_build(vis, oracle, flat, depth, rg16f, f"step {step} {size}")
        if hp.level1_virtual(hp.mip_sizes(*size)):
            # level 1 has just been materialised (hiz_level1_stored): the next reduction must not leave that flag standing over a
            # level it did not write — rebuild, query, read level 1 alone, then go on to a size that stores its level 1
            vis.hiz_rebuild()
            hp.assert_cull_equal(*hp.cull_both(vis, oracle, flat, view, hz), f"step {step} {size}: cull after hiz_rebuild")
            e = hz.level(1)
            assert np.array_equal(vis.hiz_read_level(1, e.shape[1], e.shape[0]).view(np.uint32), e.view(np.uint32))


def test_device_resident_depth_rebuilt_in_place(oracle, flat, bound):
    """The same sequence with the depth image left where it is (GV_MEM_DEVICE: a tensor on the GPU): after each build the image is
    overwritten in place, gv_hiz_rebuild reduces it again, and the pyramid and the cull are those of the new image."""
    import torch
    from garden_amd.lib import GV_MEM_DEVICE
    vis, rg16f = bound
    for step, (size, seed) in enumerate(hp.SEQUENCE):
        depth = hp.base_depth(*size, seed=scene.SEED + seed)
        resident = torch.from_numpy(depth).to("cuda:0")
        torch.cuda.synchronize()
        vis.hiz_build(resident, mem_kind=GV_MEM_DEVICE)
        check_build(vis, oracle, flat, depth, rg16f, f"step {step} {size} resident")
        again = hp.base_depth(*size, seed=scene.SEED + 100 + seed)
        assert not np.array_equal(again, depth)
        resident.copy_(torch.from_numpy(again))  # (every read of the old image has been waited for: the fetches and level reads above)
        torch.cuda.synchronize()
        vis.hiz_rebuild()
        check_build(vis, oracle, flat, again, rg16f, f"step {step} {size} resident, overwritten")
    # the context must not keep reading freed memory: leave it with an image of its own
    vis.hiz_build(hp.base_depth(64, 64))
