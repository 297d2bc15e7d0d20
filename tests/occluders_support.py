"""Test helpers of gv_pool_draw_occluders: the C twin (tests/occluder_twin.h) built into a shared library, the expected image and
counts of a draw from the records fetched in front of the call, the float64 model the conservativeness census holds the twin to,
and the worlds of tests/test_gpu_occluders.py. The tile size and the workgroup size are read from the kernel header, so the cases
follow the kernel. TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

from garden_amd import scene
from hiz_paths_support import header_constant

HERE = os.path.dirname(os.path.abspath(__file__))
COUNT_NAMES = ("drawn", "no_box", "behind", "range", "flat", "small")
DRAWN, NO_BOX, BEHIND, RANGE, FLAT, SMALL = range(6)

T = header_constant("gv_occluder_kernels.hpp", "kOccluderTile")
BLOCK = header_constant("gv_occluder_kernels.hpp", "kOccluderBlock")
RECORD_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1025)
IMAGE_SIZES = ((1, 1), (37, 23), (64, 48), (2 * T + 1, 2 * T + 1))

_TWIN_SRC = r"""#include "occluder_twin.h"
#include <stdlib.h>
/* info: X[8] Y[8] | active_count x0 x1 y0 y1 | positive mask | edge_a[12] edge_b[12]; words: u[8] v[8] z[8] d */
int twin_setup(const float* model, const float* box, const float* vp, uint32_t W, uint32_t H, uint32_t min_pixels, int32_t* info, float* words)
{
    OccluderTwinSetup s;
    int c, f, mask = 0;
    const int cls = occluder_twin_setup(model, box, vp, W, H, min_pixels, &s);
    for (c = 0; c < 8; c++) {
        info[c] = s.X[c], info[8 + c] = s.Y[c];
        words[c] = s.u[c], words[8 + c] = s.v[c], words[16 + c] = s.z[c];
    }
    words[24] = s.d;
    info[16] = s.active_count, info[17] = s.x0, info[18] = s.x1, info[19] = s.y0, info[20] = s.y1;
    for (f = 0; f < 6; f++)
        mask |= s.positive[f] << f;
    info[21] = mask;
    for (c = 0; c < 12; c++)
        info[22 + c] = s.edge_a[c], info[34 + c] = s.edge_b[c];
    return cls;
}
void twin_draw(const float* models, const float* boxes, uint32_t n, const float* vp, uint32_t W, uint32_t H, uint32_t min_pixels, float* depth,
               OccluderTwinCounts* counts)
{
    occluder_twin_draw(models, boxes, n, vp, W, H, min_pixels, depth, counts);
}
/* the tile paths of the drawn occluders among n records, summed */
void twin_paths(const float* models, const float* boxes, uint32_t n, const float* vp, uint32_t W, uint32_t H, uint32_t min_pixels, uint32_t T,
                uint32_t* paths)
{
    OccluderTwinSetup s;
    uint32_t k;
    for (k = 0; k < n; k++)
        if (occluder_twin_setup(models + 12 * (size_t)k, boxes + 6 * (size_t)k, vp, W, H, min_pixels, &s) == OCCLUDER_TWIN_DRAWN)
            occluder_twin_tile_paths(&s, T, paths);
}

/* what a draw moves: out[0] pixels the drawn occluders cover (with multiplicity), out[1] of those, the ones whose stored word was
 * smaller when the records are taken one after the other in delivery order (what gets past a plain-load filter in that order) */
void twin_traffic(const float* models, const float* boxes, uint32_t n, const float* vp, uint32_t W, uint32_t H, uint32_t min_pixels, float* depth,
                  uint64_t* out)
{
    OccluderTwinSetup s;
    uint32_t k, bits, held;
    int32_t px, py;
    for (k = 0; k < n; k++) {
        if (occluder_twin_setup(models + 12 * (size_t)k, boxes + 6 * (size_t)k, vp, W, H, min_pixels, &s) != OCCLUDER_TWIN_DRAWN)
            continue;
        memcpy(&bits, &s.d, 4);
        for (py = s.y0; py <= s.y1; py++)
            for (px = s.x0; px <= s.x1; px++) {
                float* at = depth + (size_t)py * W + px;
                if (!occluder_twin_covered(&s, px, py, OCCLUDER_TWIN_MARGIN))
                    continue;
                out[0]++;
                memcpy(&held, at, 4);
                if (held < bits) {
                    memcpy(at, &bits, 4);
                    out[1]++;
                }
            }
    }
}

/* ---- the float64 model of the census: the convex hull of the float64 projection of the same fp32 inputs ---- */
typedef struct { double x, y; } P2;
static int p2_less(const void* a, const void* b)
{
    const P2 *p = (const P2*)a, *q = (const P2*)b;
    return p->x < q->x ? -1 : p->x > q->x ? 1 : p->y < q->y ? -1 : p->y > q->y ? 1 : 0;
}
static double p2_cross(P2 o, P2 a, P2 b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }
/* Andrew's monotone chain: hull[0 .. returned) counter-clockwise, no point repeated */
static int hull_of(P2* pts, int n, P2* hull)
{
    int i, k = 0, lower;
    qsort(pts, (size_t)n, sizeof(P2), p2_less);
    for (i = 0; i < n; i++) {
        while (k >= 2 && p2_cross(hull[k - 2], hull[k - 1], pts[i]) <= 0)
            k--;
        hull[k++] = pts[i];
    }
    lower = k + 1;
    for (i = n - 2; i >= 0; i--) {
        while (k >= lower && p2_cross(hull[k - 2], hull[k - 1], pts[i]) <= 0)
            k--;
        hull[k++] = pts[i];
    }
    return k - 1;
}
/* out[0] occluders drawn, [1] pixels written, [2] written pixels with a corner outside the float64 hull, [3] drawn occluders the
 * float64 model cannot judge (a corner with w <= 0 in float64: none expected), [4] pixels in the ranges of the drawn occluders */
void twin_census(const float* models, const float* boxes, uint32_t n, const float* vp, uint32_t W, uint32_t H, int margin, uint64_t* out)
{
    OccluderTwinSetup s;
    uint32_t k;
    for (k = 0; k < n; k++) {
        const float* m = models + 12 * (size_t)k;
        const float* box = boxes + 6 * (size_t)k;
        P2 pts[8], hull[17];
        int c, e, r, count, judged = 1;
        int32_t px, py;
        if (occluder_twin_setup(m, box, vp, W, H, 1, &s) != OCCLUDER_TWIN_DRAWN)
            continue;
        out[0]++;
        for (c = 0; c < 8; c++) {
            const double x = box[(c & 1) ? 3 : 0], y = box[(c & 2) ? 4 : 1], z = box[(c & 4) ? 5 : 2];
            double p[3], cl[4];
            for (r = 0; r < 3; r++)
                p[r] = (double)m[r] * x + (double)m[3 + r] * y + (double)m[6 + r] * z + (double)m[9 + r];
            for (r = 0; r < 4; r++)
                cl[r] = (double)vp[r] * p[0] + (double)vp[4 + r] * p[1] + (double)vp[8 + r] * p[2] + (double)vp[12 + r];
            if (!(cl[3] > 0.0))
                judged = 0;
            pts[c].x = (cl[0] / cl[3] * 0.5 + 0.5) * (double)W;
            pts[c].y = (cl[1] / cl[3] * 0.5 + 0.5) * (double)H;
        }
        if (!judged) {
            out[3]++;
            continue;
        }
        count = hull_of(pts, 8, hull);
        out[4] += (uint64_t)(s.x1 - s.x0 + 1) * (uint64_t)(s.y1 - s.y0 + 1);
        for (py = s.y0; py <= s.y1; py++)
            for (px = s.x0; px <= s.x1; px++) {
                int inside = count >= 3;
                if (!occluder_twin_covered(&s, px, py, margin))
                    continue;
                out[1]++;
                for (c = 0; c < 4 && inside; c++) {
                    const P2 corner = {(double)(px + (c & 1)), (double)(py + (c >> 1))};
                    for (e = 0; e < count && inside; e++)
                        inside = p2_cross(hull[e], hull[(e + 1) % count], corner) >= 0.0;
                }
                out[2] += (uint64_t)!inside;
            }
    }
}
"""


def build_twin(directory):
    """gcc -O2 -ffp-contract=off -fno-fast-math of the twin into `directory`; returns the ctypes library."""
    src = os.path.join(str(directory), "occluder_twin.c")
    out = os.path.join(str(directory), "liboccluder_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out, "-lm"],
                   check=True)
    lib = C.CDLL(out)
    P, U32 = C.c_void_p, C.c_uint32
    lib.twin_setup.argtypes = [P, P, P, U32, U32, U32, P, P]
    lib.twin_setup.restype = C.c_int
    lib.twin_draw.argtypes = [P, P, U32, P, U32, U32, U32, P, P]
    lib.twin_draw.restype = None
    lib.twin_paths.argtypes = [P, P, U32, P, U32, U32, U32, U32, P]
    lib.twin_paths.restype = None
    lib.twin_traffic.argtypes = [P, P, U32, P, U32, U32, U32, P, P]
    lib.twin_traffic.restype = None
    lib.twin_census.argtypes = [P, P, U32, P, U32, U32, C.c_int, P]
    lib.twin_census.restype = None
    return lib


def _arrays(models, boxes, vp):
    m = np.ascontiguousarray(models, dtype=np.float32).reshape(-1, 12)
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    vp = np.ascontiguousarray(vp, dtype=np.float32).reshape(16)
    assert len(m) == len(b)
    return m, b, vp


def twin_setup(twin, model, box, vp, width, height, min_pixels=1):
    """items 1 - 6 and 8 of one occluder: dict(cls, X, Y, edges [(a, b)], positive [6 bools], range (x0, x1, y0, y1), u, v, z, d)"""
    m, b, vp = _arrays(model, box, vp)
    info, words = np.zeros(46, np.int32), np.zeros(25, np.float32)
    cls = twin.twin_setup(m.ctypes.data, b.ctypes.data, vp.ctypes.data, width, height, min_pixels, info.ctypes.data, words.ctypes.data)
    active = int(info[16])
    return dict(cls=cls, X=info[0:8].copy(), Y=info[8:16].copy(), edges=[(int(info[22 + e]), int(info[34 + e])) for e in range(active)],
                positive=[bool((int(info[21]) >> f) & 1) for f in range(6)], range=tuple(int(x) for x in info[17:21]),
                u=words[0:8].copy(), v=words[8:16].copy(), z=words[16:24].copy(), d=words[24])


def twin_draw(twin, models, boxes, vp, width, height, min_pixels=1, image=None, counts=None):
    """the twin's image (accumulated into `image` when one is given) and counts (added to `counts`) of n records"""
    m, b, vp = _arrays(models, boxes, vp)
    image = np.zeros((height, width), np.float32) if image is None else image
    assert image.shape == (height, width) and image.dtype == np.float32 and image.flags.c_contiguous
    c = np.zeros(6, np.uint32) if counts is None else np.array([counts[k] for k in COUNT_NAMES], np.uint32)
    twin.twin_draw(m.ctypes.data, b.ctypes.data, len(m), vp.ctypes.data, width, height, min_pixels, image.ctypes.data, c.ctypes.data)
    return image, {k: int(v) for k, v in zip(COUNT_NAMES, c)}


def twin_paths(twin, models, boxes, vp, width, height, min_pixels=1, tile=T):
    """tiles of the drawn occluders by the path the raster kernel takes for them: (inside, mixed, outside)"""
    m, b, vp = _arrays(models, boxes, vp)
    paths = np.zeros(3, np.uint32)
    twin.twin_paths(m.ctypes.data, b.ctypes.data, len(m), vp.ctypes.data, width, height, min_pixels, tile, paths.ctypes.data)
    return tuple(int(x) for x in paths)


def twin_traffic(twin, models, boxes, vp, width, height, min_pixels=1):
    """(image, covered pixels with multiplicity, of those the ones that raise the stored word in delivery order)"""
    m, b, vp = _arrays(models, boxes, vp)
    image, out = np.zeros((height, width), np.float32), np.zeros(2, np.uint64)
    twin.twin_traffic(m.ctypes.data, b.ctypes.data, len(m), vp.ctypes.data, width, height, min_pixels, image.ctypes.data, out.ctypes.data)
    return image, int(out[0]), int(out[1])


def twin_census(twin, models, boxes, vp, width, height, margin):
    """dict(drawn, written, violations, unjudged, range_pixels) of the twin's coverage against the float64 hull"""
    m, b, vp = _arrays(models, boxes, vp)
    out = np.zeros(5, np.uint64)
    twin.twin_census(m.ctypes.data, b.ctypes.data, len(m), vp.ctypes.data, width, height, margin, out.ctypes.data)
    return dict(zip(("drawn", "written", "violations", "unjudged", "range_pixels"), (int(x) for x in out)))


def words(image):
    return np.ascontiguousarray(image, np.float32).view(np.uint32)


# ---- cameras and models ---------------------------------------------------------------------------------------------------------------

def camera(aspect=4.0 / 3.0, fov=90.0, mirrored=False):
    """an infinite reversed-Z perspective looking down +z from the origin (w = z); mirrored: the x axis of the projection negated"""
    proj = scene.persp_inf_rev_z(math.radians(fov), aspect, 0.01)
    if mirrored:
        proj = proj.copy()
        proj[0] = -proj[0]
    return proj


def model_of(position, scale=(1.0, 1.0, 1.0), quat=(0.0, 0.0, 0.0, 1.0)):
    """12 floats c0.xyz c1.xyz c2.xyz c3.xyz of T * R * S, in float64 rounded once (a test input, not the canonical product)"""
    r = scene.quat_to_mat3(np.asarray(quat, np.float32)).astype(np.float64)
    cols = r * np.asarray(scale, np.float64)[None, :]
    return np.concatenate([cols.T.reshape(9), np.asarray(position, np.float64)]).astype(np.float32)


UNIT_BOX = np.array([-1, -1, -1, 1, 1, 1], np.float32)
# a thin plate turned by 45 degrees about the view axis in front of camera(1.0): a diamond of radius 1.7 (in NDC, L1) about (-0.2, -0.2).
# On a (2 T + 1)^2 image it holds the first tile whole, cuts through the second, and leaves the last pixel — a tile of its own in the
# corner of its pixel range — outside: the three paths of the raster kernel
FULL_SCREEN_PLATE = model_of((-0.6, 0.6, 3.0), (3.6, 3.6, 0.05), (0.0, 0.0, 0.38268343, 0.92387953))


# One occluder per skip class in front of camera(1.0) at the origin, identity rotation: (position, scale, occluder box). The slot's
# AABB is the unit box throughout, so every one of them is a draw of the frustum cull.
SKIP_TRS = {
    "no_box": ((0.0, 0.0, 8.0), (1.0, 1.0, 1.0), (-1, -1, -1, 1, -1, 1)),             # omin.y == omax.y
    "no_box_nan": ((0.5, 0.0, 8.0), (1.0, 1.0, 1.0), (-1, np.nan, -1, 1, 1, 1)),
    "behind": ((0.0, 0.0, 0.5), (1.0, 1.0, 1.0), (-1, -1, -1, 1, 1, 1)),              # z from -0.5 to 1.5: straddles w = 0
    "range": ((29.5, 0.0, 1.0005), (30.5, 1.0, 1.0), (-1, -1, -1, 1, 1, 1)),          # reaches x = 60 at w = 0.0005: u beyond 2^22 / (16 W)
    "flat": ((0.3, 0.2, 8.0), (0.0, 0.0, 1.0), (-1, -1, -1, 1, 1, 1)),                # collapsed onto a line
    "small": ((0.0, 0.0, 50.0), (0.1, 0.1, 0.1), (-1, -1, -1, 1, 1, 1)),              # under a pixel: small from min_pixels = 2 on
    "drawn": ((0.0, 0.0, 8.0), (2.0, 1.0, 1.0), (-1, -1, -1, 1, 1, 1)),
}


def skip_world():
    """SKIP_TRS as a world of its own, slots in sorted name order. Returns (scene, lo, hi, names)."""
    names = sorted(SKIP_TRS)
    sc = scene.flat_scene(len(names), seed=scene.SEED + 0x0CC6, defects=False)
    lo = np.zeros((len(names), 4), np.float32)
    hi = np.zeros((len(names), 4), np.float32)
    for slot, name in enumerate(names):
        position, scale, box = SKIP_TRS[name]
        sc.transforms["position"][slot, :3] = position
        sc.transforms["scale"][slot, :3] = scale
        sc.transforms["rotation"][slot] = (0.0, 0.0, 0.0, 1.0)
        sc.meshes["aabbMin"][slot, :3], sc.meshes["aabbMax"][slot, :3] = -1.0, 1.0
        lo[slot, :3], hi[slot, :3] = box[:3], box[3:]
    return sc, lo, hi, names


def census_boxes(n, seed):
    """n random occluders in front of camera(): log-uniform scales 0.02 .. 30 per axis (thin ones by the spread alone, and a tenth
    with one axis at 0.02 .. 0.05), distances 1.5 .. 60, a quarter mirrored (scale.x < 0), a tenth larger than the screen (scales 10
    .. 30 at distances below 8). Returns (models [n, 12], boxes [n, 6])."""
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ (0x0CC1 + seed)))
    quats = scene._unit_quats(rng, n)
    scales = np.exp(rng.uniform(math.log(0.02), math.log(30.0), (n, 3)))
    thin = rng.random(n) < 0.1
    scales[thin, rng.integers(0, 3, int(thin.sum()))] = np.exp(rng.uniform(math.log(0.02), math.log(0.05), int(thin.sum())))
    distance = np.exp(rng.uniform(math.log(1.5), math.log(60.0), n))
    huge = rng.random(n) < 0.1
    scales[huge] = rng.uniform(10.0, 30.0, (int(huge.sum()), 3))
    distance[huge] = rng.uniform(1.5, 8.0, int(huge.sum()))
    scales[rng.random(n) < 0.25, 0] *= -1.0
    lateral = rng.uniform(-1.2, 1.2, (n, 2)) * distance[:, None]
    models = np.stack([model_of((lateral[k, 0], lateral[k, 1], distance[k]), scales[k], quats[k]) for k in range(n)])
    half = rng.uniform(0.25, 1.0, (n, 3)).astype(np.float32)
    return models, np.concatenate([-half, half], axis=1)


# ---- worlds of the GPU tests ---------------------------------------------------------------------------------------------------------

CAMERA_BACK = 80.0


def parity_view(aspect=4.0 / 3.0, fov=90.0, **kw):
    """camera() from (0, 0, -CAMERA_BACK): every pivot of parity_world lies inside the frustum, so every slot is a draw"""
    return scene.make_view(camera(aspect, fov), camera_position=(0.0, 0.0, -CAMERA_BACK), **kw)


def parity_world(n, seed=0):
    """n boxes without defects around the origin: pivots in [-20, 20]^3, log-uniform scales 0.05 .. 150 per axis (thin, tiny, larger
    than the screen, and some that reach behind the camera plane, 80 away from the origin), a tenth mirrored"""
    sc = scene.flat_scene(n, seed=scene.SEED + 0x0CC + n + seed, defects=False)
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ (0x0CC2 + n + seed)))
    t = sc.transforms
    t["position"][:, :3] = rng.uniform(-20.0, 20.0, (n, 3)).astype(np.float32)
    t["scale"][:, :3] = np.exp(rng.uniform(math.log(0.05), math.log(150.0), (n, 3))).astype(np.float32)
    t["scale"][rng.random(n) < 0.1, 0] *= np.float32(-1.0)
    return sc


def occluder_boxes(meshes, seed=0):
    """[slots, 4] min and max: the slot's AABB shrunk per axis by 0.3 .. 1 (the binder's contract holds); a tenth of the slots without a
    box (zeros), and a few with a NaN or an inverted axis — all `no_box`"""
    n = len(meshes)
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ (0x0CC3 + n + seed)))
    shrink = rng.uniform(0.3, 1.0, (n, 3)).astype(np.float32)
    lo = np.zeros((n, 4), np.float32)
    hi = np.zeros((n, 4), np.float32)
    lo[:, :3] = meshes["aabbMin"][:, :3] * shrink
    hi[:, :3] = meshes["aabbMax"][:, :3] * shrink
    r = rng.random(n)
    none = r < 0.1
    lo[none], hi[none] = 0.0, 0.0
    if n >= 64:
        lo[(r >= 0.1) & (r < 0.12), 1] = np.nan
        inverted = (r >= 0.12) & (r < 0.14)
        lo[inverted, 2], hi[inverted, 2] = hi[inverted, 2].copy(), lo[inverted, 2].copy()
    return lo, hi


def boxes_by_slot(lo, hi):
    return np.concatenate([lo[:, :3], hi[:, :3]], axis=1).astype(np.float32)


def expected(twin, fetched, boxes, view_proj, width, height, min_pixels=1, image=None, counts=None):
    """What a draw of the `fetched` records (GpuVisibility.fetch(order="raw") in front of the call) must give: the twin over the
    records' own models and the occluder boxes of their POOL slots, in delivery order."""
    n = int(fetched["draw_count"])
    slots = np.asarray(fetched["visible_idx"])[:n].astype(np.int64)
    models = np.asarray(fetched["baked_model"], np.float32).reshape(-1, 12)[:n]
    return twin_draw(twin, models, np.asarray(boxes, np.float32)[slots], view_proj, width, height, min_pixels, image, counts)


# ---- the end-to-end scene: a few walls among small entities --------------------------------------------------------------------------

WALLS = 3


def wall_world(n=600):
    """n entities in front of the camera of parity_view(): slots 0 .. WALLS - 1 are wide, thin walls at depths 30, 45 and 60 in front of
    the camera (the nearest one is hidden by nothing), the rest small boxes between depth 20 and 140. The walls' occluder boxes are
    their AABBs shrunk to 0.9; the small entities have none."""
    sc = scene.flat_scene(n, seed=scene.SEED + 0x0CC4, defects=False)
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ 0x0CC5))
    t, m = sc.transforms, sc.meshes
    depth = rng.uniform(20.0, 140.0, n)
    t["position"][:, 0] = (rng.uniform(-0.9, 0.9, n) * depth).astype(np.float32)
    t["position"][:, 1] = (rng.uniform(-0.7, 0.7, n) * depth).astype(np.float32)
    t["position"][:, 2] = (depth - CAMERA_BACK).astype(np.float32)
    t["scale"][:, :3] = rng.uniform(0.3, 1.0, (n, 3)).astype(np.float32)
    t["rotation"][:] = (0.0, 0.0, 0.0, 1.0)
    for w, (z, x) in enumerate(((30.0, -12.0), (45.0, 14.0), (60.0, 0.0))):
        t["position"][w, :3] = (x, 0.0, z - CAMERA_BACK)
        t["scale"][w, :3] = (18.0, 14.0, 0.5)
        m["aabbMin"][w, :3], m["aabbMax"][w, :3] = -1.0, 1.0
    lo = np.zeros((n, 4), np.float32)
    hi = np.zeros((n, 4), np.float32)
    lo[:WALLS, :3], hi[:WALLS, :3] = -0.9, 0.9
    return sc, lo, hi


@functools.lru_cache(maxsize=None)
def oracle_cull(n=600, width=64, height=48, min_pixels=1):
    """the oracle's side of the end-to-end frame over wall_world(n), computed once (treat as read-only): the frustum cull, the twin's
    image of ITS records, and the Hi-Z cull against that image. Returns dict(first, image, counts, full)."""
    import tempfile

    from oracle import oracle_py
    sc, lo, hi = wall_world(n)
    twin = build_twin(tempfile.mkdtemp(prefix="occluder_twin_"))
    view = parity_view()
    first = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view)
    image, counts = expected(twin, first, boxes_by_slot(lo, hi), view["view_proj"], width, height, min_pixels)
    hiz_view = parity_view(use_hiz=1)
    full = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, hiz_view, hiz=oracle_py.Hiz(image))
    return dict(first=first, image=image, counts=counts, full=full)
