"""Test helpers of the sphere-entry occlusion proof (hiz_sphere_occluded): the C twin (tests/hiz_sphere_twin.h) built into a shared
library, the sphere-stream entries of a flat scene as the device derives them, and the twin's verdicts over a scene.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEP = 2  # kHizSphereStep

_TWIN_SRC = """#include "hiz_sphere_twin.h"
void twin_hot(uint32_t n, const float* world, const float* boxes, float* hot)
{
    for (uint32_t k = 0; k < n; k++) {
        hot[4 * (size_t)k + 0] = world[12 * (size_t)k + 9];
        hot[4 * (size_t)k + 1] = world[12 * (size_t)k + 10];
        hot[4 * (size_t)k + 2] = world[12 * (size_t)k + 11];
        hot[4 * (size_t)k + 3] = hiz_sphere_twin_radius(world + 12 * (size_t)k, boxes + 6 * (size_t)k);
    }
}
void twin_verdicts(const float* mips, const uint64_t* mip_offset, uint32_t width, uint32_t height, uint32_t mip_count, uint32_t nested,
                   const float* vp, const float* cam, uint32_t n, const float* hot, uint32_t step, uint8_t* out)
{
    const HizSphereTwinPyramid hz = {mips, mip_offset, width, height, mip_count, nested};
    for (uint32_t k = 0; k < n; k++) {
        const float* h = hot + 4 * (size_t)k;
        const float tx = h[0] - cam[0], ty = h[1] - cam[1], tz = h[2] - cam[2];
        out[k] = h[3] < 0.0f ? 0 : (uint8_t)hiz_sphere_twin_at(&hz, vp, tx, ty, tz, hiz_sphere_twin_reach(h[3], tx, ty, tz), step);
    }
}
"""


def build_twin(directory):
    """gcc -O2 -ffp-contract=off of the twin into `directory`; returns the ctypes library."""
    src = os.path.join(str(directory), "hiz_sphere_twin.c")
    out = os.path.join(str(directory), "libhiz_sphere_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out, "-lm"],
                   check=True)
    lib = C.CDLL(out)
    P, u32 = C.c_void_p, C.c_uint32
    lib.twin_hot.argtypes = [u32, P, P, P]
    lib.twin_hot.restype = None
    lib.twin_verdicts.argtypes = [P, P, u32, u32, u32, u32, P, P, u32, P, u32, P]
    lib.twin_verdicts.restype = None
    return lib


def nested(hz):
    """HizDevice::nested of the oracle pyramid `hz` under the reference rule: no level that is reduced has an odd size"""
    return all((hz.c.mip_w[k] <= 1 or hz.c.mip_w[k] % 2 == 0) and (hz.c.mip_h[k] <= 1 or hz.c.mip_h[k] % 2 == 0)
               for k in range(hz.c.mip_count - 1))


def hot_entries(twin, oracle, sc, chunk=1 << 20, threads=1):
    """(pos.xyz, r) of every entry of a flat, exactly paired scene, as hot_entry derives them: the world matrix's translation and
    sphere_radius of its columns and the box. (The filter chain is not applied: every entry gets a computed r, so the twin is asked
    about a superset of what the kernel asks it about.)"""
    n = sc.count
    hot = np.empty((n, 4), dtype=np.float32)
    for first in range(0, n, chunk):
        count = min(chunk, n - first)
        world = oracle.world_matrices(sc.transforms, sc.entity_to_transform, first, count, threads=threads)
        boxes = np.ascontiguousarray(np.concatenate([sc.meshes["aabbMin"][first:first + count, :3], sc.meshes["aabbMax"][first:first + count, :3]],
                                                    axis=1), dtype=np.float32)
        twin.twin_hot(count, world.ctypes.data, boxes.ctypes.data, hot[first:].ctypes.data)
    return hot


def verdicts(twin, hz, view, hot, step=STEP, is_nested=None):
    """the twin's verdict (1 = proven occluded) per entry for the oracle pyramid `hz` and `view`"""
    vp = np.ascontiguousarray(view["view_proj"], dtype=np.float32)
    cam = np.ascontiguousarray(view["camera_position"][:3], dtype=np.float32)
    offsets = np.array(list(hz.c.mip_offset), dtype=np.uint64)
    out = np.zeros(hot.shape[0], dtype=np.uint8)
    if is_nested is None:
        is_nested = nested(hz)
    hot = np.ascontiguousarray(hot, dtype=np.float32)
    twin.twin_verdicts(hz.mips.ctypes.data, offsets.ctypes.data, hz.c.width, hz.c.height, hz.c.mip_count, int(bool(is_nested)),
                       vp.ctypes.data, cam.ctypes.data, hot.shape[0], hot.ctypes.data, step, out.ctypes.data)
    return out


def census(twin, oracle, sc, hz, view, hot, threads=1, steps=(STEP,)):
    """One run of the census: the twin's verdicts against the oracle's. Returns dict(entries, survivors, visible, occluded,
    wrong[step], settled[step]): `occluded` = frustum survivors the oracle finds occluded, `wrong` = entries the twin calls occluded
    while the oracle's isVisible is 1 (must be 0), `settled` = occluded survivors the twin proves."""
    view = dict(view, use_hiz=1)
    with_hiz = sc.meshes.copy()
    with_hiz["isVisible"] = 0
    oracle.prepare_meshes(with_hiz, sc.transforms, sc.entity_to_transform, view, hiz=hz, threads=threads)
    frustum_only = sc.meshes.copy()
    frustum_only["isVisible"] = 0
    oracle.prepare_meshes(frustum_only, sc.transforms, sc.entity_to_transform, dict(view, use_hiz=0), threads=threads)
    visible = with_hiz["isVisible"] != 0
    survivor = frustum_only["isVisible"] != 0
    occluded = survivor & ~visible
    out = dict(entries=sc.count, survivors=int(survivor.sum()), visible=int(visible.sum()), occluded=int(occluded.sum()), wrong={}, settled={})
    for step in steps:
        v = verdicts(twin, hz, view, hot, step) != 0
        out["wrong"][step] = int((v & visible).sum())
        out["settled"][step] = int((v & occluded).sum())
    return out
