"""Test helpers of gv_pick: the C twin (tests/pick_twin.h) built into a shared library, the oracle's candidates of a pool and
rays aimed at them. TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MISS = 0xFFFFFFFFFFFFFFFF
NONE = 0xFFFFFFFF

_TWIN_SRC = """#include "pick_twin.h"
void twin_min(uint32_t n, const float* models, const float* boxes, const uint32_t* slots, uint32_t order, uint32_t exclude,
              const float* rays, uint32_t ray_count, uint64_t* keys)
{ pick_twin_min(n, models, boxes, slots, order, exclude, rays, ray_count, keys); }
uint64_t twin_key(const float* model, const float* box, const float* ray, uint32_t order_slot)
{ return pick_twin_key(model, box, ray, order_slot); }
"""


def build_twin(directory, march=None):
    """gcc -O2 -ffp-contract=off (optionally -march=...) of the twin into `directory`; returns the ctypes library."""
    src = os.path.join(str(directory), "pick_twin.c")
    out = os.path.join(str(directory), "libpick_twin%s.so" % ("_" + march if march else ""))
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    cmd = ["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out, "-lm"]
    if march:
        cmd.insert(3, "-march=" + march)
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    P, u32 = C.c_void_p, C.c_uint32
    lib.twin_min.argtypes = [u32, P, P, P, u32, u32, P, u32, P]
    lib.twin_min.restype = None
    lib.twin_key.argtypes = [P, P, P, u32]
    lib.twin_key.restype = C.c_uint64
    return lib


def enclosing_view(camera_position, half=1.0e7):
    """Orthographic main pass around the camera that holds the whole scene: the oracle's prepare_meshes then returns exactly the
    entries that pass the filter chain, each with its camera-relative model."""
    from garden_amd import scene
    return scene.make_view(scene.ortho_rev_z(2 * half, 2 * half, -half, half), camera_position=camera_position)


class Pool:
    """The candidates of one pool as the twin reads them: pool slots, camera-relative models (float4x3 order), model-space boxes."""

    def __init__(self, slots, models, boxes):
        self.slots = np.ascontiguousarray(slots, dtype=np.uint32)
        self.models = np.ascontiguousarray(models, dtype=np.float32).reshape(-1, 12)
        self.boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)


def candidates(sc, camera_position=(0.0, 0.0, 0.0), oracle=None, threads=1):
    if oracle is None:
        from oracle import oracle_py as oracle
    meshes = sc.meshes.copy()  # (a main pass writes isVisible)
    r = oracle.prepare_meshes(meshes, sc.transforms, sc.entity_to_transform, enclosing_view(camera_position), threads=threads)
    slots = r["visible_idx"]
    boxes = np.concatenate([sc.meshes["aabbMin"][slots, :3], sc.meshes["aabbMax"][slots, :3]], axis=1)
    return Pool(slots, r["baked_model"], boxes)


def twin_keys(twin, pools, rays, exclude=None):
    """keys of the call gv_pick(pools in this order, rays, exclude) as the twin computes them"""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    keys = np.full(len(rays), MISS, dtype=np.uint64)
    for order, p in enumerate(pools):
        ex = NONE if exclude is None or exclude[order] is None else int(exclude[order])
        twin.twin_min(len(p.slots), p.models.ctypes.data, p.boxes.ctypes.data, p.slots.ctypes.data, order, ex, rays.ctypes.data,
                      len(rays), keys.ctypes.data)
    return keys


def decode(keys, pool_ids):
    """keys -> what GpuVisibility.pick returns: (pool_id, slot, distance_sq) or None"""
    out = []
    for k in np.asarray(keys, dtype=np.uint64):
        k = int(k)
        if k == MISS:
            out.append(None)
        else:
            low = k & 0xFFFFFFFF
            d = np.array([k >> 32], dtype=np.uint32).view(np.float32)[0]
            out.append((int(pool_ids[low >> 28]), low & 0x0FFFFFFF, float(d)))
    return out


def aimed_rays(pool, count, seed, reach=(20.0, 400.0), stray=0.25):
    """`count` camera-relative rays: most from a random point `reach` away towards the pivot of a random candidate (so that they hit
    it or something in front of it), a share `stray` in random directions."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rays = np.empty((count, 6), dtype=np.float32)
    pick = rng.integers(0, len(pool.slots), count)
    pivots = pool.models[pick, 9:12].astype(np.float64)
    u = rng.normal(size=(count, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = rng.uniform(reach[0], reach[1], (count, 1))
    origins = pivots + u * dist
    dirs = (pivots - origins) * rng.uniform(0.05, 3.0, (count, 1)) + rng.normal(scale=0.02, size=(count, 3))
    stray_rows = rng.random(count) < stray
    dirs[stray_rows] = rng.normal(size=(int(stray_rows.sum()), 3))
    rays[:, :3] = origins
    rays[:, 3:] = dirs
    return rays


def gpu_pick(vis, rays, pool_ids=(0,), camera_position=(0, 0, 0), exclude=None):
    """gv_pick over any number of rays, GV_MAX_PICK_RAYS per call"""
    from garden_amd.lib import GV_MAX_PICK_RAYS
    out = []
    for k in range(0, len(rays), GV_MAX_PICK_RAYS):
        out += vis.pick(rays[k:k + GV_MAX_PICK_RAYS], pool_ids=pool_ids, camera_position=camera_position, exclude=exclude)
    return out


def as_bits(hits):
    return [None if h is None else (h[0], h[1], int(np.float32(h[2]).view(np.uint32))) for h in hits]
