"""Test helpers of gv_pool_view_bounds: the C twin (tests/bounds_twin.h) built into a shared library, the expected bounds of an item
from the records fetched in front of the call, and the case table of tests/test_gpu_view_bounds.py — whose sizes are read from the
kernel header, so they follow the kernel — with the conditions that keep a case from passing by accident. The conditions are
asserted on the oracle's records by the CPU tier (tests/test_bounds_abi.py). TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from garden_amd import scene
from hiz_paths_support import header_constant

HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS_DTYPE = np.dtype([("lo", np.float32, (3,)), ("draw_count", np.uint32), ("hi", np.float32, (3,)), ("nan_records", np.uint32)])
MAX_ITEMS = 8

R = header_constant("gv_bounds_kernels.hpp", "kBoundsRecords")   # records per workgroup of the fold
BLOCK = header_constant("gv_bounds_kernels.hpp", "kBoundsBlock")  # lanes per workgroup of both launches
# the smallest n at which a lane of the finish kernel folds more than one partial row: BLOCK rows give every lane one
FINISH_TWO_ROWS = BLOCK * R + 1
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 2 * R + 1, FINISH_TWO_ROWS)
OUTLIER_WORLD = 2 * R + 1
OUTLIER_POSITIONS = (0, 63, 64, 255, 256, R - 1, R, 2 * R)
NAN_CAP = 0.25

_TWIN_SRC = """#include "bounds_twin.h"
void twin_bounds(const float* models, const float* boxes, uint32_t n, const float* basis, BoundsTwin* out)
{
    *out = bounds_twin(models, boxes, n, basis);
}
uint32_t twin_key(float f) { return bounds_twin_key(f); }
/* every projected coordinate on its own: q[(8 k + c) * 3 + r] */
void twin_coords(const float* models, const float* boxes, uint32_t n, const float* basis, float* q)
{
    uint32_t k;
    int c, r;
    for (k = 0; k < n; k++)
        for (c = 0; c < 8; c++) {
            const float* m = models + 12 * (size_t)k;
            const float* box = boxes + 6 * (size_t)k;
            const float x = box[(c & 1) ? 3 : 0], y = box[(c & 2) ? 4 : 1], z = box[(c & 4) ? 5 : 2];
            const float px = bounds_twin_row(m, 0, x, y, z), py = bounds_twin_row(m, 1, x, y, z), pz = bounds_twin_row(m, 2, x, y, z);
            for (r = 0; r < 3; r++)
                q[((size_t)8 * k + c) * 3 + r] = bounds_twin_row(basis, r, px, py, pz);
        }
}
"""


def build_twin(directory):
    """gcc -O2 -ffp-contract=off -fno-fast-math of the twin into `directory`; returns the ctypes library."""
    src = os.path.join(str(directory), "bounds_twin.c")
    out = os.path.join(str(directory), "libbounds_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out, "-lm"],
                   check=True)
    lib = C.CDLL(out)
    P, U32 = C.c_void_p, C.c_uint32
    lib.twin_bounds.argtypes = [P, P, U32, P, P]
    lib.twin_bounds.restype = None
    lib.twin_key.argtypes = [C.c_float]
    lib.twin_key.restype = U32
    lib.twin_coords.argtypes = [P, P, U32, P, P]
    lib.twin_coords.restype = None
    return lib


def _arrays(models, boxes, basis):
    m = np.ascontiguousarray(models, dtype=np.float32).reshape(-1, 12)
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    basis = np.ascontiguousarray(basis, dtype=np.float32).reshape(12)
    assert len(m) == len(b)
    return m, b, basis


def twin_bounds(twin, models, boxes, basis):
    """the twin's answer for records given as models [n, 12] and boxes [n, 6] (min.xyz, max.xyz): one BOUNDS_DTYPE element"""
    m, b, basis = _arrays(models, boxes, basis)
    out = np.zeros(1, BOUNDS_DTYPE)
    twin.twin_bounds(m.ctypes.data, b.ctypes.data, len(m), basis.ctypes.data, out.ctypes.data)
    return out[0]


def twin_coords(twin, models, boxes, basis):
    """every projected coordinate: float32 [n, 8, 3]"""
    m, b, basis = _arrays(models, boxes, basis)
    q = np.zeros((len(m), 8, 3), np.float32)
    twin.twin_coords(m.ctypes.data, b.ctypes.data, len(m), basis.ctypes.data, q.ctypes.data)
    return q


def aabbs_by_slot(meshes):
    """[slots, 6] (min.xyz, max.xyz) as the device mirror holds them: a slot that is no candidate (no entity, or disabled) holds the
    empty box"""
    boxes = np.concatenate([meshes["aabbMin"][:, :3], meshes["aabbMax"][:, :3]], axis=1).astype(np.float32)
    boxes[(meshes["entity"] == 0) | (meshes["isEnabled"] == 0)] = 0.0
    return boxes


def expected(twin, fetched, boxes_by_slot, basis):
    """What an item over the `fetched` records (GpuVisibility.fetch(order="raw") in front of the call, or the oracle's records)
    must give: the twin over the records' own models and the boxes of their POOL slots."""
    n = int(fetched["draw_count"])
    slots = np.asarray(fetched["visible_idx"])[:n].astype(np.int64)
    models = np.asarray(fetched["baked_model"], np.float32).reshape(-1, 12)[:n]
    return twin_bounds(twin, models, np.asarray(boxes_by_slot, np.float32)[slots], basis)


def words(bounds):
    """the 8 words of every item, for an exact comparison (NaN-free by the rule, but -0 and +0 differ)"""
    return np.ascontiguousarray(bounds).view(np.uint32).reshape(-1, 8).tolist()


# ---- bases -------------------------------------------------------------------------------------------------------------------------

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def rotation_basis(seed, translation=(0.0, 0.0, 0.0)):
    """a random rotation and a translation: 12 float32, c0.xyz c1.xyz c2.xyz c3.xyz (a light view's affine part)"""
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ (0xB0B0 + seed)))
    rot = scene.quat_to_mat3(scene._unit_quats(rng, 1)[0])  # rot[r][c]
    return np.concatenate([rot.T.reshape(9), np.asarray(translation, np.float32)]).astype(np.float32)


def extreme_basis():
    """a basis with planted extremes: row 0 overflows to +-inf on both sides (3e38 x a coordinate of a few hundred), row 1 carries
    a subnormal coefficient, row 2 a NaN (no coordinate of that axis takes part, every record counts)"""
    b = rotation_basis(99).copy()
    b[0] = np.float32(3.0e38)
    b[4] = np.float32(1.0e-40)
    b[8] = np.float32(np.nan)
    return b


# ---- worlds ------------------------------------------------------------------------------------------------------------------------

def enclosing(half=1.0e7, shadow_pass=-1, camera_position=(0, 0, 0), camera_offset=(0, 0, 0)):
    """an orthographic view that holds the whole scene: every box becomes a draw"""
    return scene.make_view(scene.ortho_rev_z(2 * half, 2 * half, -half, half), camera_position=camera_position, camera_offset=camera_offset,
                           shadow_pass=shadow_pass)


def edge_world(n):
    """n boxes without defects: in the enclosing view n is the draw count"""
    return scene.flat_scene(n, seed=scene.SEED + n, defects=False)


PLANTED_N = 2 * R + 1
PLANTED_HALF = 1.0e21


def planted_world():
    """PLANTED_N boxes, under a quarter of them with extremes in what becomes their bakedModel: NaN positions and rotations (every
    coordinate of the record a NaN: counted, takes no part), infinite scales (inf - inf among the corners), subnormal scales (the box
    collapses onto the pivot, through subnormal products), pivots at +-3e19 (finite: they take part and are the extremes) and NaN box
    corners. Returns (scene, the planted slots)."""
    n = PLANTED_N
    sc = scene.flat_scene(n, seed=scene.SEED + 7, defects=False)
    rng = np.random.Generator(np.random.PCG64(scene.SEED + 8))
    planted = rng.permutation(n)[:360]
    t, m = sc.transforms, sc.meshes
    t["position"][planted[0:40], 0] = np.nan
    t["rotation"][planted[40:60], 1] = np.nan
    t["scale"][planted[60:100], 2] = np.inf
    t["scale"][planted[100:160], :3] = np.float32(1.0e-40)
    t["position"][planted[160:190], 1] = np.float32(3.0e19)
    t["position"][planted[190:220], 1] = np.float32(-3.0e19)
    t["position"][planted[220:250], 0] = np.float32(-3.0e19)
    t["position"][planted[250:280], 2] = np.float32(3.0e19)
    m["aabbMax"][planted[280:320], 0] = np.nan
    t["scale"][planted[320:360], 0] = -np.inf
    return sc, planted


@functools.lru_cache(maxsize=None)
def oracle_records(kind, n=0):
    """the oracle's records of a world in its enclosing view, with the boxes by slot; computed once, treat as read-only"""
    from oracle import oracle_py
    if kind == "planted":
        sc, _ = planted_world()
        view = enclosing(PLANTED_HALF)
    else:
        sc, view = edge_world(n), enclosing()
    records = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view)
    return records, aabbs_by_slot(sc.meshes)


def attained_by(q):
    """the records that attain each of the six extremes of coordinates q [n, 8, 3] (NaN-free): six record indices"""
    per_record_lo, per_record_hi = q.min(axis=1), q.max(axis=1)  # [n, 3]
    return [int(per_record_lo[:, r].argmin()) for r in range(3)] + [int(per_record_hi[:, r].argmax()) for r in range(3)]
