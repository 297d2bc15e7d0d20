"""Test helpers of gv_pool_bind_cluster_cones / gv_pool_cull_cluster_cones: the C twin (tests/cluster_cone_twin.h — which cluster
passes the frustum and the pyramid is decided by cluster_twin.h, that is by the oracle's two tests; it restates the cone test, the
conjunction and the second phase's pending set under it, and counts the census) built into a shared library; outward cones for the
cluster tables of cluster_runs_support.geometry() plus one geometry of DESIGNED cones; the designed draws; the CASE TABLE the GPU
tests (tests/test_gpu_cluster_cones.py) and the oracle-only census (tests/test_cluster_cones_census.py) share. World, cameras, wall
and placement are clusters_support's. TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import math
import os
import subprocess
from collections import namedtuple

import numpy as np

import cluster_runs_support as rsup
import clusters_support as ksup
from garden_amd import scene
from garden_amd.lib import CLUSTER_CONE_DTYPE, CLUSTER_DTYPE, CLUSTER_RANGE_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS_FIELDS = ("tested", "frustum_kept", "base_kept", "cone_rejected", "cone_only", "hiz_only", "survivors", "partial")
FRUSTUM, BASE, CONE, PENDING, SECOND = 1, 2, 4, 8, 16   # verdict bits
PLAIN_FORM, RUN_FORM, SECOND_PHASE = 0, 1, 2

_TWIN_SRC = """#include "cluster_cone_twin.h"
uint32_t cone_twin_view(const float* models, const uint32_t* g, const uint32_t* first, uint32_t n, const void* table, uint32_t table_count,
                        const void* ranges, uint32_t range_count, const void* clusters, const void* cones, const float* eye,
                        const float* view_proj, const GvoHiz* hiz, const GvoHiz* hiz2, int mode, void* out, uint32_t* tested, uint8_t* verdict,
                        uint32_t* census)
{
    return cluster_cone_twin_view(models, g, first, n, (const ClusterTwinGeometry*)table, table_count, (const ClusterTwinRange*)ranges,
                                  range_count, (const ClusterTwinCluster*)clusters, (const ClusterConeTwinCone*)cones, eye, view_proj, hiz, hiz2,
                                  mode, (ClusterTwinCommand*)out, tested, verdict, (ClusterConeCensus*)census);
}
uint32_t cone_twin_census_words(void) { return (uint32_t)(sizeof(ClusterConeCensus) / sizeof(uint32_t)); }
uint32_t cone_twin_cone_bytes(void) { return (uint32_t)sizeof(ClusterConeTwinCone); }
"""


@functools.lru_cache(maxsize=None)
def twin():
    """gcc -O2 -ffp-contract=off -fno-fast-math of the twin against the oracle's library; the ctypes library (built once)."""
    import tempfile

    from oracle import oracle_py
    oracle_py.load()
    directory = tempfile.mkdtemp(prefix="cluster_cone_twin_")
    src, out = os.path.join(directory, "cluster_cone_twin.c"), os.path.join(directory, "libcluster_cone_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    build = os.path.dirname(oracle_py.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out,
                    "-L" + build, "-Wl,-rpath," + build, "-lgv_oracle", "-lm"], check=True)
    lib = C.CDLL(out)
    P, U32 = C.c_void_p, C.c_uint32
    lib.cone_twin_view.argtypes = [P, P, P, U32, P, U32, P, U32, P, P, P, P, P, P, C.c_int, P, P, P, P]
    lib.cone_twin_view.restype = U32
    lib.cone_twin_census_words.restype = U32
    lib.cone_twin_cone_bytes.restype = U32
    assert lib.cone_twin_census_words() == len(CENSUS_FIELDS) and lib.cone_twin_cone_bytes() == CLUSTER_CONE_DTYPE.itemsize
    return lib


# ---- cones --------------------------------------------------------------------------------------------------------------------------
def outward_cones(clusters, seed=77):
    """One cone per cluster: axis = the normalised centre of the cluster's cell (zero where the centre is zero or not finite), apex =
    centre - axis * half the cell's diagonal, cutoff uniform in [0.1, 0.8]. A cell of a box around the model's origin faces outward."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cones = np.zeros(len(clusters), CLUSTER_CONE_DTYPE)
    lo, hi = clusters["box_min"].astype(np.float32), clusters["box_max"].astype(np.float32)
    centre = (np.float32(0.5) * (lo + hi)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        length = np.linalg.norm(centre, axis=1).astype(np.float32)
        usable = np.isfinite(length) & (length > 0)
        axis = np.where(usable[:, None], centre / np.where(usable, length, 1)[:, None], 0).astype(np.float32)
        half_diagonal = (np.float32(0.5) * np.linalg.norm(hi - lo, axis=1)).astype(np.float32)
        cones["apex"] = (centre - axis * half_diagonal[:, None]).astype(np.float32)
    cones["axis"] = axis
    cones["cutoff"] = rng.uniform(0.1, 0.8, len(clusters)).astype(np.float32)
    cones["reserved"] = 0xDEADBEEF  # not read
    return cones


# the designed cones: the clusters of ONE extra geometry (id ksup.RANGED, which clusters_support's ranges leave whole). Every box lies
# inside a unit entity; every cone but the named ones has apex 0 and axis +z. Seen from the origin by an unrotated entity of unit
# scale at DESIGN_PLACE (below), apex - eye is the entity's place: the cosine to +z is 120 / |place|, about 0.9997, below 1.
DESIGNED = (
    # name, apex, axis, cutoff, cone-rejected by the point eye at the origin
    ("cutoff-0", (0, 0, 0), (0, 0, 1), 0.0, True),            # q >= 0
    ("cutoff-1", (0, 0, 0), (0, 0, 1), 1.0, False),           # the eye is not exactly on the axis
    ("cutoff-1.5", (0, 0, 0), (0, 0, 1), 1.5, False),
    ("cutoff-minus-0.5", (0, 0, 0), (0, 0, 1), -0.5, True),   # cutoff enters squared: as 0.5
    ("cutoff-0.5", (0, 0, 0), (0, 0, 1), 0.5, True),          # the control
    ("axis-away", (0, 0, 0), (0, 0, -1), 0.5, False),         # s < 0: the cone faces the eye
    ("axis-zero", (0, 0, 0), (0, 0, 0), 0.5, False),          # meshoptimizer's degenerate cone
    ("apex-nan", (np.nan, 0, 0), (0, 0, 1), 0.5, False),
    ("axis-nan", (0, 0, 0), (0, np.nan, 1), 0.5, False),
    ("cutoff-nan", (0, 0, 0), (0, 0, 1), np.nan, False),
    ("apex-1e30", (0, 0, 1e30), (0, 0, 1), 0.5, False),       # q overflows
)
DESIGNED_ID = ksup.RANGED
DESIGNED_NAMES = tuple(d[0] for d in DESIGNED)


@functools.lru_cache(maxsize=None)
def geometry():
    """(geometry table, ranges, clusters, cones): cluster_runs_support.geometry()'s tables (contiguous index ranges, so that the run
    form merges) with the designed geometry appended as id DESIGNED_ID, and one cone per cluster; read-only."""
    table, _, ranges, clusters = rsup.geometry()
    assert len(ranges) == DESIGNED_ID and len(table) > DESIGNED_ID
    designed = np.zeros(len(DESIGNED), CLUSTER_DTYPE)
    designed_cones = np.zeros(len(DESIGNED), CLUSTER_CONE_DTYPE)
    at = 70000
    for j, (_, apex, axis, cutoff, _) in enumerate(DESIGNED):
        designed[j]["box_min"], designed[j]["box_max"] = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
        designed[j]["first"], designed[j]["count"] = at, 3 + j
        at += 3 + j
        designed_cones[j]["apex"], designed_cones[j]["axis"], designed_cones[j]["cutoff"] = apex, axis, cutoff
    all_ranges = np.zeros(len(ranges) + 1, CLUSTER_RANGE_DTYPE)
    all_ranges[:len(ranges)] = ranges
    all_ranges[DESIGNED_ID] = (len(clusters), len(DESIGNED))
    return table, all_ranges, np.concatenate([clusters, designed]), np.concatenate([outward_cones(clusters), designed_cones])


# ---- eyes ---------------------------------------------------------------------------------------------------------------------------
POINT_EYE = (0.0, 0.0, 0.0, 1.0)   # the camera of clusters_support.camera(): at the origin of the records' space
ZERO_EYE = (0.0, 0.0, 0.0, 0.0)    # no cone test


def direction_eye(yaw):
    """parallel rays that travel along the viewing direction of clusters_support.camera(yaw)"""
    return (math.sin(yaw), 0.0, math.cos(yaw), 0.0)


def eyes_of(case):
    """the eyes of a case's views: 'P' the point eye, 'D' the direction eye of the view's yaw, 'Z' all zero"""
    return np.array([{"P": POINT_EYE, "Z": ZERO_EYE, "D": direction_eye(yaw)}[kind] for kind, yaw in zip(case.eyes, case.yaws)], np.float32)


# ---- expected values ---------------------------------------------------------------------------------------------------------------
def view_commands(models, g, first, view_proj, eye, hiz, mode=PLAIN_FORM, hiz2=None, tables=None):
    """(commands of ONE view as a COMMAND_DTYPE array, tested — second phase: pending —, the census as a dict, the verdict bytes) by
    the twin. tables: None for geometry(), or (table, ranges, clusters, cones)."""
    table, ranges, clusters, cones = geometry() if tables is None else tables
    assert len(cones) == len(clusters)
    n = len(g)
    m = np.ascontiguousarray(models, np.float32).reshape(-1, 12)[:n]
    g = np.ascontiguousarray(g, np.uint32)
    first = np.ascontiguousarray(first, np.uint32)
    vp = np.ascontiguousarray(view_proj, np.float32)
    eye = np.ascontiguousarray(eye, np.float32)
    assert len(first) == n + 1 and len(m) == n and eye.shape == (4,)
    per_draw = np.where(g < len(ranges), ranges["count"][np.minimum(g, len(ranges) - 1)], 0)
    room = int(np.maximum(per_draw, 1).sum(dtype=np.int64)) + 1
    out = np.zeros(room, ksup.COMMAND_DTYPE)
    verdict = np.zeros(int(per_draw.sum(dtype=np.int64)) + 1, np.uint8)
    tested = C.c_uint32()
    census = np.zeros(len(CENSUS_FIELDS), np.uint32)
    count = twin().cone_twin_view(m.ctypes.data, g.ctypes.data, first.ctypes.data, n, table.ctypes.data, len(table), ranges.ctypes.data,
                                  len(ranges), clusters.ctypes.data, cones.ctypes.data, eye.ctypes.data, vp.ctypes.data,
                                  C.addressof(hiz.c) if hiz is not None else None, C.addressof(hiz2.c) if hiz2 is not None else None, int(mode),
                                  out.ctypes.data, C.addressof(tested), verdict.ctypes.data, census.ctypes.data)
    return out[:count], tested.value, dict(zip(CENSUS_FIELDS, (int(x) for x in census))), verdict[:-1]


def commands_of(fetched, starts, bases, draw_ids, views, eyes, hizzes, mode=PLAIN_FORM, hiz2s=None, tables=None):
    """(the commands of every view, counts[views], tested[views], the census summed over the views, the verdicts per view) of a cone
    cull; arguments as clusters_support.commands_of, eyes [views, 4]. mode SECOND_PHASE: hizzes are K1's (None: the view was not
    queried and nothing is pending), hiz2s the pyramids in force at the second phase; tested is the pending count."""
    per_view, tested, verdicts = [], [], []
    total = dict.fromkeys(CENSUS_FIELDS, 0)
    for v, (f, first) in enumerate(zip(fetched, ksup.firsts(fetched, starts, bases))):
        n = int(f["draw_count"])
        if mode == SECOND_PHASE and hizzes[v] is None:
            per_view.append(np.zeros(0, ksup.COMMAND_DTYPE))
            tested.append(0)
            verdicts.append(np.zeros(0, np.uint8))
            continue
        commands, t, census, verdict = view_commands(np.asarray(f["baked_model"]).reshape(-1, 12)[:n], draw_ids[v], first, views[v]["view_proj"],
                                                     eyes[v], hizzes[v], mode, None if hiz2s is None else hiz2s[v], tables)
        per_view.append(commands)
        tested.append(t)
        verdicts.append(verdict)
        for name in CENSUS_FIELDS:
            total[name] += census[name]
    return per_view, np.array([len(c) for c in per_view], np.uint32), np.array(tested, np.uint32), total, verdicts


# ---- the designed draws --------------------------------------------------------------------------------------------------------------
# cluster_runs_support.design_scene(): 258 unrotated entities of unit scale on a grid 120 units in front of the camera, every one
# wholly inside the frustum. Three of them draw the designed geometry; the others draw nothing.
DESIGN_IDENTITY, DESIGN_MIRRORED, DESIGN_FLAT = 40, 41, 42   # slots: unit scale; scale (-1, 1, 1): det < 0; scale (1, 0, 1): det = 0
VOID_ID = ksup.VOID_IDS[0]


@functools.lru_cache(maxsize=None)
def design_scene():
    """(Scene, ids per slot, the place of the identity draw); read-only"""
    base = rsup.design_scene()
    sc = scene.flat_scene(base.count, defects=False)
    for name in ("position", "scale", "rotation"):
        sc.transforms[name][:] = base.transforms[name]
    sc.meshes["aabbMin"][:], sc.meshes["aabbMax"][:] = base.meshes["aabbMin"], base.meshes["aabbMax"]
    sc.transforms["scale"][DESIGN_MIRRORED, :3] = (-1.0, 1.0, 1.0)
    sc.transforms["scale"][DESIGN_FLAT, :3] = (1.0, 0.0, 1.0)
    ids = np.full(sc.count, VOID_ID, np.uint32)
    ids[[DESIGN_IDENTITY, DESIGN_MIRRORED, DESIGN_FLAT]] = DESIGNED_ID
    place = tuple(float(x) for x in sc.transforms["position"][DESIGN_IDENTITY, :3])
    assert place[0] != 0.0 or place[1] != 0.0  # off the axis: cutoff 1 keeps
    return sc, ids, place


def design_eyes():
    """name -> the eye: the camera; a point eye exactly at the apex of the identity draw's apex-0 cones (its translation: w = 0)"""
    _, _, place = design_scene()
    return {"camera": np.array(POINT_EYE, np.float32), "at-apex": np.array(place + (1.0,), np.float32)}


# ---- the case table ------------------------------------------------------------------------------------------------------------------
# name, draws under camera(), yaws of the views, which views query the wall, the anchor's geometry, the eye of every view (P point, D
# direction, Z all zero)
Case = namedtuple("Case", "name draws yaws hiz anchor eyes")
CASES = (
    Case("draws-0", 0, (0.0,), (False,), ksup.ANCHOR_DEFAULT, "P"),
    Case("draws-1-of-1", 1, (0.0,), (False,), 2, "P"),          # a geometry of 1 cluster
    Case("draws-1-of-63", 1, (0.0,), (False,), 5, "P"),         # ... of 63, 64 and 65: the wave's edge
    Case("draws-1-of-64", 1, (0.0,), (False,), 0, "D"),
    Case("draws-1-of-65", 1, (0.0,), (False,), 6, "P"),
    Case("draws-2", 2, (0.0,), (False,), ksup.ANCHOR_DEFAULT, "P"),
    Case("draws-256", 256, (0.0,), (False,), ksup.ANCHOR_DEFAULT, "D"),
    Case("draws-257", 257, (0.0,), (True,), ksup.ANCHOR_DEFAULT, "P"),
    Case("tile-minus-1", 1, (0.0,), (False,), 12, "P"),         # one draw of 255, 256, 257 clusters: the candidate total at a tile's edge
    Case("tile", 1, (0.0,), (False,), 13, "P"),
    Case("tile-plus-1", 1, (0.0,), (False,), 7, "D"),
    Case("two-tiles-plus-1", 1, (0.0,), (True,), 8, "P"),       # 513 clusters
    Case("views-2", 64, (0.0, 0.4), (True, False), ksup.ANCHOR_DEFAULT, "PD"),
    Case("views-8", 64, ksup.EIGHT, (True, False, True, False, False, False, False, True), ksup.ANCHOR_DEFAULT, "PDZPDZPD"),
)
CASE = {c.name: c for c in CASES}
SHARE_FROM = 63   # the census holds a case's share of cone-rejected clusters to [1/10, 1/2] from this many tested clusters on


def case_views(case):
    return ksup.case_views(case)
