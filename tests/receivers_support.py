"""Test helpers of gv_pool_draw_receivers: the C twin (tests/receiver_twin.h) built into a shared library, the expected mask and counts
of a draw from the records fetched in front of the call, the census of the FORMS the two launches divide the records into (written by
the setup lane / listed; the three tile paths), light matrices in the shape csm::fit gives them, the worlds of
tests/test_gpu_receivers.py, and the end-to-end shadow scene with the oracle's side of it and the ray caster that holds the masked cull
to the geometry. The tile, workgroup and small-range sizes are read from the kernel header. TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

import occluders_support as osup
from garden_amd import scene
from hiz_paths_support import header_constant

HERE = os.path.dirname(os.path.abspath(__file__))
COUNT_NAMES = ("drawn", "flat", "behind", "range", "outside", "reserved")
DRAWN, FLAT, BEHIND, RANGE, OUTSIDE = range(5)
INF_WORD = 0x7F800000

T = osup.T
BLOCK = osup.BLOCK
SMALL_PIXELS = header_constant("gv_receiver_kernels.hpp", "kReceiverSmallPixels")
RECORD_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1025)
IMAGE_SIZES = ((1, 1), (31, 33), (2 * T + 1, 2 * T + 1), (512, 256), (1000, 600))

_TWIN_SRC = r"""#include "receiver_twin.h"
/* info: X[8] Y[8] | active_count x0 x1 y0 y1 | edge_a[12] edge_b[12]; words: u[8] v[8] z[8] d */
int rtwin_setup(const float* model, const float* box, const float* light, uint32_t W, uint32_t H, int32_t* info, float* words)
{
    ReceiverTwinSetup s;
    int c;
    const int cls = receiver_twin_setup(model, box, light, W, H, &s);
    for (c = 0; c < 8; c++) {
        info[c] = s.X[c], info[8 + c] = s.Y[c];
        words[c] = s.u[c], words[8 + c] = s.v[c], words[16 + c] = s.z[c];
    }
    words[24] = s.d;
    info[16] = s.active_count, info[17] = s.x0, info[18] = s.x1, info[19] = s.y0, info[20] = s.y1;
    for (c = 0; c < 12; c++)
        info[21 + c] = s.edge_a[c], info[33 + c] = s.edge_b[c];
    return cls;
}
void rtwin_clear(float* mask, uint32_t W, uint32_t H) { receiver_twin_clear(mask, W, H); }
void rtwin_draw(const float* models, const float* boxes, uint32_t n, const float* light, uint32_t W, uint32_t H, float* mask, ReceiverTwinCounts* counts)
{
    receiver_twin_draw(models, boxes, n, light, W, H, mask, counts);
}
/* the pixels one record writes: out[W H] bytes set to 1; returns the class */
int rtwin_pixels(const float* model, const float* box, const float* light, uint32_t W, uint32_t H, uint8_t* out)
{
    ReceiverTwinSetup s;
    int32_t px, py;
    const int cls = receiver_twin_setup(model, box, light, W, H, &s);
    if (cls == RECEIVER_TWIN_OUTSIDE)
        return cls;
    for (py = s.y0; py <= s.y1; py++)
        for (px = s.x0; px <= s.x1; px++)
            if (cls != RECEIVER_TWIN_DRAWN || receiver_twin_touched(&s, px, py, RECEIVER_TWIN_MARGIN))
                out[(size_t)py * W + px] = 1;
    return cls;
}
/* the forms of the launches over n records: out[0] records written by the setup lane (a range of at most `small` pixels), out[1]
 * records listed, out[2] their tiles; of those out[3] with every pixel of the clipped tile written, out[4] some, out[5] none;
 * out[6] tiles of listed records that write the whole mask (behind, range) */
void rtwin_forms(const float* models, const float* boxes, uint32_t n, const float* light, uint32_t W, uint32_t H, uint32_t small, uint32_t T,
                 uint64_t* out)
{
    ReceiverTwinSetup s;
    uint32_t k;
    for (k = 0; k < n; k++) {
        const int cls = receiver_twin_setup(models + 12 * (size_t)k, boxes + 6 * (size_t)k, light, W, H, &s);
        int32_t tx, ty, px, py;
        if (cls == RECEIVER_TWIN_OUTSIDE)
            continue;
        if ((uint64_t)(s.x1 - s.x0 + 1) * (uint64_t)(s.y1 - s.y0 + 1) <= small) {
            out[0]++;
            continue;
        }
        out[1]++;
        for (ty = s.y0 / (int32_t)T; ty <= s.y1 / (int32_t)T; ty++)
            for (tx = s.x0 / (int32_t)T; tx <= s.x1 / (int32_t)T; tx++) {
                const int32_t rx0 = tx * (int32_t)T > s.x0 ? tx * (int32_t)T : s.x0, ry0 = ty * (int32_t)T > s.y0 ? ty * (int32_t)T : s.y0;
                const int32_t rx1 = (tx + 1) * (int32_t)T - 1 < s.x1 ? (tx + 1) * (int32_t)T - 1 : s.x1;
                const int32_t ry1 = (ty + 1) * (int32_t)T - 1 < s.y1 ? (ty + 1) * (int32_t)T - 1 : s.y1;
                uint64_t written = 0;
                for (py = ry0; py <= ry1; py++)
                    for (px = rx0; px <= rx1; px++)
                        written += cls != RECEIVER_TWIN_DRAWN || receiver_twin_touched(&s, px, py, RECEIVER_TWIN_MARGIN);
                out[2]++;
                out[written == (uint64_t)(rx1 - rx0 + 1) * (uint64_t)(ry1 - ry0 + 1) ? 3 : written ? 4 : 5]++;
                out[6] += cls == RECEIVER_TWIN_BEHIND || cls == RECEIVER_TWIN_RANGE;
            }
    }
}
"""


def build_twin(directory):
    """gcc -O2 -ffp-contract=off -fno-fast-math of the twin into `directory`; returns the ctypes library."""
    src = os.path.join(str(directory), "receiver_twin.c")
    out = os.path.join(str(directory), "libreceiver_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out, "-lm"],
                   check=True)
    lib = C.CDLL(out)
    P, U32 = C.c_void_p, C.c_uint32
    lib.rtwin_setup.argtypes = [P, P, P, U32, U32, P, P]
    lib.rtwin_setup.restype = C.c_int
    lib.rtwin_clear.argtypes = [P, U32, U32]
    lib.rtwin_clear.restype = None
    lib.rtwin_draw.argtypes = [P, P, U32, P, U32, U32, P, P]
    lib.rtwin_draw.restype = None
    lib.rtwin_pixels.argtypes = [P, P, P, U32, U32, P]
    lib.rtwin_pixels.restype = C.c_int
    lib.rtwin_forms.argtypes = [P, P, U32, P, U32, U32, U32, U32, P]
    lib.rtwin_forms.restype = None
    return lib


@functools.lru_cache(maxsize=None)
def shared_twin():
    """one twin per process for the cached oracle sides (treat as read-only)"""
    import tempfile
    return build_twin(tempfile.mkdtemp(prefix="receiver_twin_"))


_arrays = osup._arrays
words = osup.words


def twin_setup(twin, model, box, light, width, height):
    """steps 1 - 6 of one record: dict(cls, X, Y, edges [(a, b)], range (x0, x1, y0, y1), u, v, z, d)"""
    m, b, light = _arrays(model, box, light)
    info, out = np.zeros(45, np.int32), np.zeros(25, np.float32)
    cls = twin.rtwin_setup(m.ctypes.data, b.ctypes.data, light.ctypes.data, width, height, info.ctypes.data, out.ctypes.data)
    active = int(info[16])
    return dict(cls=cls, X=info[0:8].copy(), Y=info[8:16].copy(), edges=[(int(info[21 + e]), int(info[33 + e])) for e in range(active)],
                range=tuple(int(x) for x in info[17:21]), u=out[0:8].copy(), v=out[8:16].copy(), z=out[16:24].copy(), d=out[24])


def clear_mask(width, height):
    return np.full((height, width), np.inf, np.float32)


def twin_draw(twin, models, boxes, light, width, height, image=None, counts=None):
    """the twin's mask (accumulated into `image` when one is given, a cleared one otherwise) and counts (added to `counts`)"""
    m, b, light = _arrays(models, boxes, light)
    image = clear_mask(width, height) if image is None else image
    assert image.shape == (height, width) and image.dtype == np.float32 and image.flags.c_contiguous
    c = np.zeros(6, np.uint32) if counts is None else np.array([counts[k] for k in COUNT_NAMES], np.uint32)
    twin.rtwin_draw(m.ctypes.data, b.ctypes.data, len(m), light.ctypes.data, width, height, image.ctypes.data, c.ctypes.data)
    return image, {k: int(v) for k, v in zip(COUNT_NAMES, c)}


def twin_pixels(twin, model, box, light, width, height):
    """(class, bool [height, width]: the pixels one record writes)"""
    m, b, light = _arrays(model, box, light)
    out = np.zeros((height, width), np.uint8)
    cls = twin.rtwin_pixels(m.ctypes.data, b.ctypes.data, light.ctypes.data, width, height, out.ctypes.data)
    return cls, out.astype(bool)


FORM_NAMES = ("small", "listed", "tiles", "tiles_all", "tiles_some", "tiles_none", "tiles_whole_mask")


def twin_forms(twin, models, boxes, light, width, height):
    """how the launches divide n records: dict over FORM_NAMES (see rtwin_forms)"""
    m, b, light = _arrays(models, boxes, light)
    out = np.zeros(7, np.uint64)
    twin.rtwin_forms(m.ctypes.data, b.ctypes.data, len(m), light.ctypes.data, width, height, SMALL_PIXELS, T, out.ctypes.data)
    return dict(zip(FORM_NAMES, (int(x) for x in out)))


def aabbs_by_slot(meshes):
    """[slots, 6] (min.xyz, max.xyz) as the device mirror holds them: a slot that is no candidate holds the empty box"""
    boxes = np.concatenate([meshes["aabbMin"][:, :3], meshes["aabbMax"][:, :3]], axis=1).astype(np.float32)
    boxes[(meshes["entity"] == 0) | (meshes["isEnabled"] == 0)] = 0.0
    return boxes


def records(fetched):
    n = int(fetched["draw_count"])
    return np.asarray(fetched["visible_idx"])[:n].astype(np.int64), np.asarray(fetched["baked_model"], np.float32).reshape(-1, 12)[:n]


def expected(twin, fetched, boxes, light, width, height, image=None, counts=None):
    """What a draw of the `fetched` records (GpuVisibility.fetch(order="raw") in front of the call, or the oracle's records) must
    give: the twin over the records' own models and the cull AABBs of their POOL slots, in delivery order."""
    slots, models = records(fetched)
    return twin_draw(twin, models, np.asarray(boxes, np.float32)[slots], light, width, height, image, counts)


def forms(twin, fetched, boxes, light, width, height):
    slots, models = records(fetched)
    return twin_forms(twin, models, np.asarray(boxes, np.float32)[slots], light, width, height)


# ---- light matrices, in the conventions of csm_lite.hpp (column-major, +Z forward, reversed Z, Y flipped by the projection) ------------

def _cm(m):
    """a 4x4 in mathematical layout (row, column) as column-major float32 [16]"""
    return np.asarray(m, np.float64).T.reshape(16).astype(np.float32)


def look_at(eye, center):
    """csm::lookAt as a (row, column) float64 4x4"""
    eye, center = np.asarray(eye, np.float64), np.asarray(center, np.float64)
    f = center - eye
    f /= np.linalg.norm(f)
    up = np.array([0.0, 1.0, 0.0]) if abs(f[1]) <= 0.999 else np.array([1.0, 0.0, 0.0])
    s = np.cross(up, f)
    s /= np.linalg.norm(s)
    u = np.cross(f, s)
    v = np.eye(4)
    v[0, :3], v[1, :3], v[2, :3] = s, u, f
    v[:3, 3] = -s @ eye, -u @ eye, -f @ eye
    return v


def ortho_rev_z(x0, x1, y0, y1, z0, z1):
    """csm::orthoRevZ as a (row, column) float64 4x4: depth 1 at z0 and 0 at z1"""
    p = np.zeros((4, 4))
    p[0, 0], p[1, 1], p[2, 2] = 2.0 / (x1 - x0), -2.0 / (y1 - y0), -1.0 / (z1 - z0)
    p[0, 3], p[1, 3], p[2, 3], p[3, 3] = -(x1 + x0) / (x1 - x0), (y1 + y0) / (y1 - y0), z1 / (z1 - z0), 1.0
    return p


def ortho_light(direction, center, half_width, half_height, depth_lo, depth_hi):
    """an orthographic cascade: a light looking along `direction` at `center`, its box half_width x half_height about the centre
    and depth_lo .. depth_hi along the light (float32 [16], column-major)"""
    d = np.asarray(direction, np.float64)
    d /= np.linalg.norm(d)
    view = look_at(np.asarray(center, np.float64) - d, center)
    return _cm(ortho_rev_z(-half_width, half_width, -half_height, half_height, depth_lo, depth_hi) @ view)


def slice_light(rotation3, fov_y, aspect, near, far, direction, z_coeff=10.0):
    """csm::fit without the texel snapping: the cascade of the main camera's slice near .. far. `rotation3` is the camera's
    rotation (columns: its right, up and forward in the camera-relative world). Returns (L float32 [16], dict(view, lo, hi))."""
    ty, tx = math.tan(fov_y * 0.5), math.tan(fov_y * 0.5) * aspect
    r = np.asarray(rotation3, np.float64)
    corners = np.array([r @ np.array([sx * tx * d, sy * ty * d, d]) for d in (near, far) for sy in (-1, 1) for sx in (-1, 1)])
    center = corners.mean(axis=0)
    d = np.asarray(direction, np.float64)
    d /= np.linalg.norm(d)
    view = look_at(center - d, center)
    t = corners @ view[:3, :3].T + view[:3, 3]
    lo, hi = t.min(axis=0), t.max(axis=0)
    lo[2] = lo[2] * z_coeff if lo[2] < 0 else lo[2] / z_coeff
    hi[2] = hi[2] / z_coeff if hi[2] < 0 else hi[2] * z_coeff
    return _cm(ortho_rev_z(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]) @ view), dict(view=view, lo=lo, hi=hi)


# ---- worlds of the parity tests -------------------------------------------------------------------------------------------------------

parity_view = osup.parity_view


def parity_world(n, seed=0):
    """osup.parity_world (pivots in [-20, 20]^3, a tenth mirrored) with scales 0.05 .. 10 log-uniform per axis and a quarter of the
    boxes a hundred times smaller again — from sub-pixel to a good part of any mask; a twentieth of the cull AABBs collapsed onto a
    segment (two extents 0: `flat` from wherever it is seen) and a twentieth onto a plate (one extent 0: `flat` only edge-on); and
    one slot in 32 a slab larger than the mask, 40 to 60 above the cloud: nearer the light than nearly everything, so that the
    minimum under it keeps the words of what lies below (a box that reaches far along the light floors every texel it touches).
    Every slot stays a candidate and a draw of parity_view()."""
    sc = osup.parity_world(n, seed)
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ (0x5EC1 + n + seed)))
    r = rng.random(n)
    t, m = sc.transforms, sc.meshes
    mirrored = t["scale"][:, 0] < 0
    t["scale"][:, :3] = np.exp(rng.uniform(math.log(0.05), math.log(10.0), (n, 3))).astype(np.float32)
    t["scale"][mirrored, 0] *= np.float32(-1.0)
    segment, plate = r < 0.05, (r >= 0.05) & (r < 0.10)
    for axis in (0, 2):
        m["aabbMin"][segment, axis] = 0.0
        m["aabbMax"][segment, axis] = 0.0
    m["aabbMin"][plate, 1] = 0.0
    m["aabbMax"][plate, 1] = 0.0
    t["scale"][(r >= 0.10) & (r < 0.35), :3] *= np.float32(0.01)
    slab = np.nonzero((r >= 0.35) & (r < 0.35 + 1.0 / 32.0))[0]
    t["scale"][slab, :3] = (60.0, 2.0, 60.0)
    t["rotation"][slab] = (0.0, 0.0, 0.0, 1.0)
    t["position"][slab, :3] = np.stack([rng.uniform(-10.0, 10.0, len(slab)), rng.uniform(40.0, 60.0, len(slab)),
                                        rng.uniform(-10.0, 10.0, len(slab))], axis=1).astype(np.float32)
    return sc


def parity_light():
    """an orthographic cascade over the middle of parity_world as parity_view() delivers it (camera-relative: the cloud is around
    (0, 0, CAMERA_BACK)): 30 x 24 about the centre, so pivots out to +-20 leave records wholly outside, and a light direction that is
    no axis of the world and not the source view's"""
    return ortho_light((0.4, -1.0, 0.3), (0.0, 0.0, osup.CAMERA_BACK), 15.0, 12.0, -400.0, 400.0)


def perspective_light_inside():
    """a perspective light in the middle of the cloud looking along +z: about half of the records reach behind it"""
    return scene.mul_cm(scene.persp_inf_rev_z(math.radians(70.0), 1.0, 0.05),
                        _cm(look_at((0.0, 0.0, osup.CAMERA_BACK), (0.0, 0.0, osup.CAMERA_BACK + 1.0))))


def perspective_light_outside():
    """... and one well outside it, looking at it: a few of the largest boxes still reach behind it"""
    return scene.mul_cm(scene.persp_inf_rev_z(math.radians(50.0), 1.0, 0.05),
                        _cm(look_at((45.0, 35.0, osup.CAMERA_BACK - 30.0), (0.0, 0.0, osup.CAMERA_BACK))))


# ---- the end-to-end scene: entities over a floor slab, the main camera and one cascade -------------------------------------------------

SHADOW_N = 20_000
SHADOW_MASK = (256, 256)
CAMERA = (0.0, 8.0, -20.0)
LIGHT_DIR = (0.1, -1.0, 0.3)
FOV_Y, ASPECT, SLICE_FAR = math.radians(60.0), 16.0 / 9.0, 300.0
# planted by hand in the last slots (world positions; unit cull AABB, identity rotation): what each exists for is in its name
PLANTED = {
    "floor": ((0.0, -1.0, 130.0), (150.0, 1.0, 150.0)),            # the slab: x -150 .. 150, y -2 .. 0, z -20 .. 280
    # under the slab, beside the main frustum, and deeper than the slab's one depth — that of its farthest corner from the slanted
    # light, some 90 units under the near end: dropped
    "under_floor_0": ((140.0, -200.0, 100.0), (1.5, 1.5, 1.5)),
    "under_floor_1": ((-140.0, -200.0, 140.0), (2.0, 1.0, 2.0)),
    "under_floor_2": ((145.0, -180.0, 90.0), (1.0, 1.0, 1.0)),
    "off_floor_0": ((-230.0, 20.0, 100.0), (0.5, 0.5, 0.5)),       # over no receiver at all: dropped
    "off_floor_1": ((-240.0, 30.0, 90.0), (0.4, 0.4, 0.4)),
    "above_floor_0": ((140.0, 10.0, 100.0), (1.5, 1.5, 1.5)),      # beside the main frustum, but over the slab the camera sees: kept
    "above_floor_1": ((-140.0, 25.0, 110.0), (2.0, 1.0, 2.0)),
}
# no random entity within this distance (x, z) of an off_floor caster or inside the strip the light carries its footprint along:
# the mask around them holds no receiver, by construction and asserted
OFF_FLOOR_CLEARING = 60.0


def shadow_world(n=SHADOW_N, seed=3):
    """scene.flat_scene(n) reshaped: entities of 1 .. 6 units in x -320 .. 320, y 0.5 .. 40, z -40 .. 320 around and over the floor
    slab, with PLANTED in the last slots. Returns (scene, {name: slot})."""
    sc = scene.flat_scene(n, seed=scene.SEED + 0x5EC0 + seed, defects=False)
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ (0x5EC2 + seed)))
    t, m = sc.transforms, sc.meshes
    t["position"][:, 0] = rng.uniform(-320.0, 320.0, n).astype(np.float32)
    t["position"][:, 1] = rng.uniform(0.5, 40.0, n).astype(np.float32)
    t["position"][:, 2] = rng.uniform(-40.0, 320.0, n).astype(np.float32)
    t["scale"][:, :3] = rng.uniform(1.0, 6.0, (n, 3)).astype(np.float32)
    names = sorted(PLANTED)
    slots = {name: n - len(names) + i for i, name in enumerate(names)}
    clear = [np.asarray(PLANTED[k][0]) for k in names if k.startswith("off_floor")]
    for c in clear:  # the clearing: entities near an off_floor caster move to the far side of the world
        near = np.hypot(t["position"][:, 0] - c[0], t["position"][:, 2] - c[2]) < OFF_FLOOR_CLEARING
        t["position"][near, 0] = np.float32(300.0)
    for name, slot in slots.items():
        position, scale = PLANTED[name]
        t["position"][slot, :3] = position
        t["scale"][slot, :3] = scale
        t["rotation"][slot] = (0.0, 0.0, 0.0, 1.0)
        m["aabbMin"][slot, :3], m["aabbMax"][slot, :3] = -1.0, 1.0
    return sc, slots


def shadow_views():
    """(main perspective view, the cascade's light matrix L, the cascade as a frustum-only view, the cascade as a Hi-Z view): all
    share the camera position, so a slot's record model is the same in every one of them"""
    main = scene.make_view(scene.persp_inf_rev_z(FOV_Y, ASPECT, 0.1), camera_position=CAMERA)
    light, _ = slice_light(np.eye(3), FOV_Y, ASPECT, 0.1, SLICE_FAR, LIGHT_DIR)
    plain = scene.make_view(light, camera_position=CAMERA, shadow_pass=0)
    masked = scene.make_view(light, camera_position=CAMERA, shadow_pass=0, use_hiz=1)
    return main, light, plain, masked


@functools.lru_cache(maxsize=None)
def shadow_oracle(rg16f=False):
    """the oracle's side of the end-to-end frame, computed once (treat as read-only): the main view's cull, the twin's mask of ITS
    records, the cascade's frustum-only cull and its cull against the pyramid of that mask.
    Returns dict(main, image, counts, plain, masked)."""
    from oracle import oracle_py
    sc, _ = shadow_world()
    main_view, light, plain_view, masked_view = shadow_views()
    main = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, main_view)
    width, height = SHADOW_MASK
    image, counts = expected(shared_twin(), main, aabbs_by_slot(sc.meshes), light, width, height)
    plain = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, plain_view)
    masked = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, masked_view,
                                      hiz=oracle_py.Hiz(image, rg16f=rg16f))
    return dict(main=main, image=image, counts=counts, plain=plain, masked=masked)


# ---- soundness against the geometry: rays from the receivers towards the light ---------------------------------------------------------

def _affine(models):
    """[n, 12] c0.xyz c1.xyz c2.xyz c3.xyz -> (A [n, 3, 3], t [n, 3]) in float64: p = A x + t"""
    m = np.asarray(models, np.float64).reshape(-1, 4, 3)
    return np.transpose(m[:, :3, :], (0, 2, 1)), m[:, 3, :]


def sample_points(main, boxes, light, width, height, count=4096, seed=11, floor_slot=None):
    """`count` points inside the cull AABBs of the main view's records (camera-relative world, float64) that project at least two
    texels inside the mask; half of them in the record of `floor_slot` when one is given"""
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ (0x5EC3 + seed)))
    slots, models = records(main)
    a, t = _affine(models)
    lm = np.asarray(light, np.float64).reshape(4, 4).T
    out = []
    floor_record = None if floor_slot is None else int(np.nonzero(slots == floor_slot)[0][0])
    while sum(len(o) for o in out) < count:
        k = rng.integers(0, len(slots), 4 * count)
        if floor_record is not None:
            k[::2] = floor_record
        b = np.asarray(boxes, np.float64)[slots[k]]
        x = b[:, :3] + rng.random((len(k), 3)) * (b[:, 3:] - b[:, :3])
        p = np.einsum("nij,nj->ni", a[k], x) + t[k]
        cl = p @ lm[:, :3].T + lm[:, 3]
        u, v = (cl[:, 0] / cl[:, 3] * 0.5 + 0.5) * width, (cl[:, 1] / cl[:, 3] * 0.5 + 0.5) * height
        inside = (u >= 2) & (u <= width - 2) & (v >= 2) & (v <= height - 2) & (cl[:, 3] > 0)
        out.append(p[inside])
    return np.concatenate(out)[:count]


def rays_hit(points, direction, models, boxes, light, chunk=128):
    """bool [len(points)]: the ray from the point along `direction` (towards the light) hits one of the boxes — each shrunk by 1e-3
    of its size, slab-tested in its model space — at a point nearer the light than the origin by more than 1e-4 in L's z"""
    points = np.asarray(points, np.float64)
    d = np.asarray(direction, np.float64)
    lm = np.asarray(light, np.float64).reshape(4, 4).T
    assert abs(lm[3, :3]).max() == 0.0 and lm[3, 3] == 1.0  # (an orthographic L: z is affine, so z gained = t * dz)
    dz = lm[2, :3] @ d
    hit = np.zeros(len(points), bool)
    a, t = _affine(models)
    b = np.asarray(boxes, np.float64)
    size = b[:, 3:] - b[:, :3]
    lo, hi = b[:, :3] + 1e-3 * size, b[:, 3:] - 1e-3 * size
    for s in range(0, len(a), chunk):
        inv = np.linalg.inv(a[s:s + chunk])                                  # [c, 3, 3]
        o = np.einsum("cij,cpj->cpi", inv, points[None, :, :] - t[s:s + chunk, None, :])   # [c, p, 3]
        e = np.einsum("cij,j->ci", inv, d)[:, None, :]                        # [c, 1, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            t0 = (lo[s:s + chunk, None, :] - o) / e
            t1 = (hi[s:s + chunk, None, :] - o) / e
        enter = np.nanmax(np.minimum(t0, t1), axis=2)
        leave = np.nanmin(np.maximum(t0, t1), axis=2)
        parallel_out = ((e == 0) & ((o < lo[s:s + chunk, None, :]) | (o > hi[s:s + chunk, None, :]))).any(axis=2)
        ok = (enter <= leave) & (leave * dz > 1e-4) & ~parallel_out & (leave > 0)
        hit |= ok.any(axis=0)
    return hit
