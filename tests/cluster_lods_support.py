"""Test helpers of gv_pool_bind_cluster_lods / gv_pool_cull_cluster_lods: the C twin (tests/cluster_lod_twin.h — which cluster
passes the frustum and the pyramid is decided by cluster_twin.h, that is by the oracle's two tests, the cone by cluster_cone_twin.h,
the runs by cluster_runs_twin.h; it restates the LOD cut, the conjunction and the second phase's pending set under it, and counts the
census) built into a shared library; the DAG FIXTURE — binary cluster DAGs over the cells of a geometry's box, with nested spheres
and doubling errors, padded to the range sizes the walks have edges at; one geometry of DESIGNED entries and the designed draws and
views; the CASE TABLE the GPU tests (tests/test_gpu_cluster_lods.py) and the oracle-only census (tests/test_cluster_lods_census.py)
share. World, cameras, wall and placement are clusters_support's. TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import math
import os
import subprocess
from collections import namedtuple

import numpy as np

import cluster_cones_support as nsup
import cluster_runs_support as rsup
import clusters_support as ksup
from garden_amd import scene
from garden_amd.lib import CLUSTER_CONE_DTYPE, CLUSTER_DTYPE, CLUSTER_LOD_DTYPE, CLUSTER_LOD_VIEW_DTYPE, CLUSTER_RANGE_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS_FIELDS = ("tested", "lod_kept", "lod_frustum", "lod_hiz", "lod_cone", "base_kept", "survivors", "eyes_disagree")
FRUSTUM, BASE, CONE, PENDING, SECOND, KEPT = 1, 2, 4, 8, 16, 32   # verdict bits
PLAIN_FORM, RUN_FORM, SECOND_PHASE = 0, 1, 2

_TWIN_SRC = """#include "cluster_lod_twin.h"
uint32_t lod_twin_view(const float* models, const uint32_t* g, const uint32_t* first, uint32_t n, const void* table, uint32_t table_count,
                       const void* ranges, uint32_t range_count, const void* clusters, const void* lods, const void* lod_view, const void* cones,
                       const float* eye, const float* view_proj, const GvoHiz* hiz, const GvoHiz* hiz2, int mode, void* out, uint32_t* tested,
                       uint8_t* verdict, uint32_t* census)
{
    return cluster_lod_twin_view(models, g, first, n, (const ClusterTwinGeometry*)table, table_count, (const ClusterTwinRange*)ranges,
                                 range_count, (const ClusterTwinCluster*)clusters, (const ClusterLodTwinLod*)lods,
                                 (const ClusterLodTwinView*)lod_view, (const ClusterConeTwinCone*)cones, eye, view_proj, hiz, hiz2, mode,
                                 (ClusterTwinCommand*)out, tested, verdict, (ClusterLodCensus*)census);
}
uint32_t lod_twin_census_words(void) { return (uint32_t)(sizeof(ClusterLodCensus) / sizeof(uint32_t)); }
uint32_t lod_twin_lod_bytes(void) { return (uint32_t)sizeof(ClusterLodTwinLod); }
uint32_t lod_twin_view_bytes(void) { return (uint32_t)sizeof(ClusterLodTwinView); }
"""


@functools.lru_cache(maxsize=None)
def twin():
    """gcc -O2 -ffp-contract=off -fno-fast-math of the twin against the oracle's library; the ctypes library (built once)."""
    import tempfile

    from oracle import oracle_py
    oracle_py.load()
    directory = tempfile.mkdtemp(prefix="cluster_lod_twin_")
    src, out = os.path.join(directory, "cluster_lod_twin.c"), os.path.join(directory, "libcluster_lod_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    build = os.path.dirname(oracle_py.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out,
                    "-L" + build, "-Wl,-rpath," + build, "-lgv_oracle", "-lm"], check=True)
    lib = C.CDLL(out)
    P, U32 = C.c_void_p, C.c_uint32
    lib.lod_twin_view.argtypes = [P, P, P, U32, P, U32, P, U32, P, P, P, P, P, P, P, P, C.c_int, P, P, P, P]
    lib.lod_twin_view.restype = U32
    for name in ("lod_twin_census_words", "lod_twin_lod_bytes", "lod_twin_view_bytes"):
        getattr(lib, name).restype = U32
    assert lib.lod_twin_census_words() == len(CENSUS_FIELDS)
    assert lib.lod_twin_lod_bytes() == CLUSTER_LOD_DTYPE.itemsize == 48 and lib.lod_twin_view_bytes() == CLUSTER_LOD_VIEW_DTYPE.itemsize == 32
    return lib


# ---- the DAG fixture ----------------------------------------------------------------------------------------------------------------
# A range of `count` clusters over a geometry's box is the largest binary DAG that fits — 2^L - 1 clusters: 2^(L-1) leaves, the cells
# of a grid over the box in bit-interleaved order (bit b of the leaf index goes to axis b % 3, so that the two children of every
# inner cluster are neighbours and a cluster's region is a box), level l holding leaves >> l clusters, each the parent group of two
# clusters of level l - 1 — followed by PADS: clusters of their own (a DAG of one: error 0, parent_error +inf), small boxes in the
# middle of the geometry. In the table the levels follow each other, leaves first; every cluster's indices follow its predecessor's
# (leaves are contiguous, so runs merge; inner clusters have index ranges of their own behind them).
# Self error: 0 at the leaves, ERROR_BASE of the box's smallest half-extent at level 1, doubling per level. Spheres: a leaf's is
# around its cell, an inner cluster's around its region with the radius that holds both children's spheres; each with MARGIN.
# geometry id -> clusters (0: drawn whole). The ids are clusters_support's, so that its world() and anchors serve: 0 is the 127-DAG
# over 4^3 cells; 9, 10, 11 are the levels of one model (gv_pool_select_lods).
GEOMETRY_CLUSTERS = (127, 3, 1, 0, 7, 63, 65, 257, 513, 64, 8, 1, 255, 256)
MARGIN = np.float32(1.03)
ERROR_BASE = 0.02
DAG_ID, DESIGNED_ID = 0, ksup.RANGED
assert len(GEOMETRY_CLUSTERS) == ksup.RANGED


def dag_size(count):
    """(clusters of the DAG, its levels) of a range of `count` clusters"""
    levels = int(math.floor(math.log2(count + 1)))
    return (1 << levels) - 1, levels


def dag_level(count, j):
    """the DAG level of cluster j of a range of `count` clusters (leaves 0), or -1 for a pad"""
    size, levels = dag_size(count)
    if j >= size:
        return -1
    at, level = 0, 0
    while j >= at + (1 << (levels - 1 - level)):
        at += 1 << (levels - 1 - level)
        level += 1
    return level


def dag_leaves(count, j):
    """the leaves (their indices among the leaves) that cluster j of the DAG covers"""
    size, levels = dag_size(count)
    level = dag_level(count, j)
    at = sum(1 << (levels - 1 - l) for l in range(level))
    i = j - at
    return range(i << level, (i + 1) << level)


def _dag(half, count, rng, at):
    """(clusters, lods) of one range; `at`: where its indices begin"""
    size, levels = dag_size(count)
    leaves = 1 << (levels - 1)
    bits = [sum(1 for b in range(levels - 1) if b % 3 == axis) for axis in range(3)]
    grid = np.array([1 << b for b in bits])
    cell = (2.0 * half / grid).astype(np.float32)
    clusters = np.zeros(count, CLUSTER_DTYPE)
    lods = np.zeros(count, CLUSTER_LOD_DTYPE)
    lods["reserved"] = 0xDEADBEEF  # not read
    boxes, spheres, index = {}, {}, {}
    j = 0
    for level in range(levels):
        for i in range(leaves >> level):
            if level == 0:
                ix = [sum(((i >> b) & 1) << (b // 3) for b in range(levels - 1) if b % 3 == axis) for axis in range(3)]
                lo = (-half + cell * np.array(ix, np.float32)).astype(np.float32)
                hi = (-half + cell * (np.array(ix, np.float32) + 1)).astype(np.float32)
                centre = (np.float32(0.5) * (lo + hi)).astype(np.float32)
                radius = np.float32(0.5) * np.float32(np.linalg.norm(hi - lo)) * MARGIN
            else:
                (lo0, hi0), (lo1, hi1) = boxes[level - 1, 2 * i], boxes[level - 1, 2 * i + 1]
                lo, hi = np.minimum(lo0, lo1), np.maximum(hi0, hi1)
                centre = (np.float32(0.5) * (lo + hi)).astype(np.float32)
                radius = max(np.float32(np.linalg.norm(centre - spheres[level - 1, 2 * i + s][0])) + spheres[level - 1, 2 * i + s][1]
                             for s in (0, 1)) * MARGIN
            boxes[level, i], spheres[level, i], index[level, i] = (lo, hi), (centre, np.float32(radius)), j
            clusters[j]["box_min"], clusters[j]["box_max"] = lo, hi
            j += 1
    error = lambda level: np.float32(0.0 if level == 0 else ERROR_BASE * float(half.min()) * 2.0 ** (level - 1))
    for (level, i), j in index.items():
        lods[j]["self_center"], lods[j]["self_radius"] = spheres[level, i]
        lods[j]["self_error"] = error(level)
        if level == levels - 1:  # the root: its own sphere again, refined-from at any distance
            lods[j]["parent_center"], lods[j]["parent_radius"], lods[j]["parent_error"] = spheres[level, i][0], spheres[level, i][1], np.inf
        else:
            lods[j]["parent_center"], lods[j]["parent_radius"] = spheres[level + 1, i >> 1]
            lods[j]["parent_error"] = error(level + 1)
    for j in range(size, count):  # the pads
        lo = np.float32(0.05 * (j - size)) * half.astype(np.float32)
        clusters[j]["box_min"], clusters[j]["box_max"] = lo - np.float32(0.1) * half, lo + np.float32(0.1) * half
        lods[j]["self_center"] = lods[j]["parent_center"] = lo
        lods[j]["self_radius"] = lods[j]["parent_radius"] = np.float32(0.2) * np.float32(np.linalg.norm(half))
        lods[j]["self_error"], lods[j]["parent_error"] = 0.0, np.inf
    for j in range(count):
        level = dag_level(count, j)
        clusters[j]["first"], clusters[j]["count"] = at, 3 * int(rng.integers(1, 40)) * (1 + max(level, 0))
        at += int(clusters[j]["count"])
    return clusters, lods


# the designed entries: the clusters of ONE extra geometry (id DESIGNED_ID, which the ranges above leave whole). Every box lies
# inside a unit entity and every centre is the model's origin, so that C is the draw's translation. Seen by design_view() (a point
# eye at the origin, scale 1, near_distance 1) from an unrotated draw of unit scale about 120 units away, D is about 14 400.
DESIGNED = (
    # name, self (radius, error), parent (centre x, radius, error), LOD-kept by the point eye of design_view(), by its parallel twin
    ("root-inf", (1.0, 0.0), (0.0, 2.0, np.inf), True, True),             # refined-from at any distance
    ("self-error-nan", (1.0, np.nan), (0.0, 2.0, np.inf), True, True),    # a NaN in the self triple: fine enough
    ("parent-centre-nan", (1.0, 0.0), (np.nan, 2.0, 1000.0), False, True),  # a NaN in the parent triple rejects — through D only
    ("parent-error-nan", (1.0, 0.0), (0.0, 2.0, np.nan), False, False),
    ("self-above-parent", (1.0, 1000.0), (0.0, 2.0, 0.001), False, False),  # not monotone: the builder's business; by the rule, rejected
    ("radius-0", (0.0, 0.0), (0.0, 0.0, 1000.0), True, True),
    ("fine-parent", (1.0, 0.01), (0.0, 2.0, 0.02), False, False),         # the parent is fine enough: something coarser is drawn
    ("at-the-near-clamp", (1.0, 1.0), (0.0, 2.0, 1000.0), True, True),    # Q == N: not above, so not exceeded
    ("near-only", (1.0, 0.0), (0.0, 2.0, 2.0), False, True),              # Q > N but A < D: the parallel eye disagrees
)
DESIGNED_NAMES = tuple(d[0] for d in DESIGNED)


@functools.lru_cache(maxsize=None)
def geometry():
    """(geometry table, ranges, clusters, cones, lods): the DAG fixture over the boxes of clusters_support.geometry() with the
    designed geometry appended as id DESIGNED_ID; outward cones on the DAGs' leaves, zero-axis cones elsewhere; read-only."""
    table, half, _, _ = ksup.geometry()
    table = table.copy()
    table[6]["first"] = 12345  # (the wrapping uint32 add is the run form's own test)
    rng = np.random.Generator(np.random.PCG64(39))
    ranges = np.zeros(ksup.RANGED + 1, CLUSTER_RANGE_DTYPE)
    clusters, lods, cones = [], [], []
    total = 0
    for g, count in enumerate(GEOMETRY_CLUSTERS):
        ranges[g] = (total, count)
        if not count:
            continue
        c, l = _dag(half[g], count, rng, 1000 * (g + 1))
        cone = np.zeros(count, CLUSTER_CONE_DTYPE)
        leaves = (dag_size(count)[0] + 1) // 2
        if leaves > 1:
            cone[:leaves] = nsup.outward_cones(c[:leaves], seed=100 + g)
        clusters.append(c), lods.append(l), cones.append(cone)
        total += count
    designed = np.zeros(len(DESIGNED), CLUSTER_DTYPE)
    designed_lods = np.zeros(len(DESIGNED), CLUSTER_LOD_DTYPE)
    at = 70000
    for j, (_, (radius, error), (px, parent_radius, parent_error), _, _) in enumerate(DESIGNED):
        designed[j]["box_min"], designed[j]["box_max"] = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
        designed[j]["first"], designed[j]["count"] = at, 3 + j
        at += 3 + j
        designed_lods[j]["self_radius"], designed_lods[j]["self_error"] = radius, error
        designed_lods[j]["parent_center"][0] = px
        designed_lods[j]["parent_radius"], designed_lods[j]["parent_error"] = parent_radius, parent_error
    ranges[DESIGNED_ID] = (total, len(DESIGNED))
    clusters.append(designed), lods.append(designed_lods), cones.append(np.zeros(len(DESIGNED), CLUSTER_CONE_DTYPE))
    return table, ranges, np.concatenate(clusters), np.concatenate(cones), np.concatenate(lods)


# ---- LOD views ----------------------------------------------------------------------------------------------------------------------
def lod_view(eye=(0.0, 0.0, 0.0, 1.0), scale=1.0, near=1.0):
    v = np.zeros((), CLUSTER_LOD_VIEW_DTYPE)
    v["eye"], v["scale"], v["near_distance"] = eye, scale, near
    v["reserved"] = np.nan  # not read
    return v


def lod_scale(fovy, height, pixels):
    """k of a perspective view: the projection factor divided by the pixel threshold"""
    return (0.5 * height) / math.tan(0.5 * fovy) / pixels


CAMERA_SCALE = lod_scale(math.radians(90.0), 1080.0, 1.0)   # 540: clusters_support.camera() at 1080 rows and one pixel
PARALLEL_SCALE = 3.0                                        # pixels per world unit over tau of the parallel views


ANCHOR_EYE = (ksup.ASPECT * 34.0 - 6.0, 1.0, 34.0 - 5.0, 1.0)   # a point inside the anchor's box (clusters_support.world())


def lod_views_of(case):
    """the LOD views of a case's views: 'P' the camera's point eye, 'A' a point eye inside the anchor's box (one draw then spans
    several levels), 'O' a parallel projection, 'Z' scale 0 (the test switched off)"""
    kinds = {"P": lod_view(scale=CAMERA_SCALE * case.scale), "A": lod_view(eye=ANCHOR_EYE, scale=CAMERA_SCALE * case.scale),
             "O": lod_view(eye=(0.0, 0.0, 0.0, 0.0), scale=PARALLEL_SCALE * case.scale), "Z": lod_view(scale=0.0)}
    return np.array([kinds[kind] for kind in case.lods], CLUSTER_LOD_VIEW_DTYPE)


def eyes_of(case):
    """cluster_cones_support.eyes_of, or None for a case without cone eyes"""
    return nsup.eyes_of(case) if case.eyes else None


# ---- expected values ---------------------------------------------------------------------------------------------------------------
def view_commands(models, g, first, view_proj, lod, eye, hiz, mode=PLAIN_FORM, hiz2=None, tables=None):
    """(commands of ONE view as a COMMAND_DTYPE array, tested — second phase: pending —, the census as a dict, the verdict bytes, the
    first verdict of every draw) by the twin. eye: None for no cone test."""
    table, ranges, clusters, cones, lods = geometry() if tables is None else tables
    assert len(cones) == len(clusters) == len(lods)
    n = len(g)
    m = np.ascontiguousarray(models, np.float32).reshape(-1, 12)[:n]
    g = np.ascontiguousarray(g, np.uint32)
    first = np.ascontiguousarray(first, np.uint32)
    vp = np.ascontiguousarray(view_proj, np.float32)
    lod = np.ascontiguousarray(lod)
    eye = None if eye is None else np.ascontiguousarray(eye, np.float32)
    assert len(first) == n + 1 and len(m) == n and lod.dtype == CLUSTER_LOD_VIEW_DTYPE
    instances = np.diff(first.astype(np.int64)) if n else np.zeros(0, np.int64)
    per_draw = np.where((g < len(ranges)) & (instances != 0), ranges["count"][np.minimum(g, len(ranges) - 1)], 0)
    room = int(np.maximum(per_draw, 1).sum(dtype=np.int64)) + 1
    out = np.zeros(room, ksup.COMMAND_DTYPE)
    verdict = np.zeros(int(per_draw.sum(dtype=np.int64)) + 1, np.uint8)
    tested = C.c_uint32()
    census = np.zeros(len(CENSUS_FIELDS), np.uint32)
    count = twin().lod_twin_view(m.ctypes.data, g.ctypes.data, first.ctypes.data, n, table.ctypes.data, len(table), ranges.ctypes.data,
                                 len(ranges), clusters.ctypes.data, lods.ctypes.data, lod.ctypes.data, None if eye is None else cones.ctypes.data,
                                 None if eye is None else eye.ctypes.data, vp.ctypes.data, C.addressof(hiz.c) if hiz is not None else None,
                                 C.addressof(hiz2.c) if hiz2 is not None else None, int(mode), out.ctypes.data, C.addressof(tested),
                                 verdict.ctypes.data, census.ctypes.data)
    return out[:count], tested.value, dict(zip(CENSUS_FIELDS, (int(x) for x in census))), verdict[:-1], np.concatenate([[0], np.cumsum(per_draw)])


def commands_of(fetched, starts, bases, draw_ids, views, lod_views, eyes, hizzes, mode=PLAIN_FORM, hiz2s=None, tables=None):
    """(the commands of every view, counts[views], tested[views], the census summed over the views, per view (verdicts, the first
    verdict of every draw, g per draw)) of a LOD cull; arguments as cluster_cones_support.commands_of, lod_views one per view, eyes
    [views, 4] or None."""
    per_view, tested, verdicts = [], [], []
    total = dict.fromkeys(CENSUS_FIELDS, 0)
    for v, (f, first) in enumerate(zip(fetched, ksup.firsts(fetched, starts, bases))):
        n = int(f["draw_count"])
        if mode == SECOND_PHASE and hizzes[v] is None:
            per_view.append(np.zeros(0, ksup.COMMAND_DTYPE))
            tested.append(0)
            verdicts.append((np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.uint32)))
            continue
        commands, t, census, verdict, at = view_commands(np.asarray(f["baked_model"]).reshape(-1, 12)[:n], draw_ids[v], first, views[v]["view_proj"],
                                                         lod_views[v], None if eyes is None else eyes[v], hizzes[v], mode,
                                                         None if hiz2s is None else hiz2s[v], tables)
        per_view.append(commands)
        tested.append(t)
        verdicts.append((verdict, at, np.asarray(draw_ids[v], np.uint32)))
        for name in CENSUS_FIELDS:
            total[name] += census[name]
    return per_view, np.array([len(c) for c in per_view], np.uint32), np.array(tested, np.uint32), total, verdicts


def cut_statistics(verdicts, ranges=None):
    """Over the tested draws of the views: (kept clusters per DAG level — pads under -1 —, draws whose leaves are not each covered by
    exactly one kept cluster of the DAG, draws whose cut is only leaves, draws whose cut is only the root), DAGs of 3 clusters and
    more."""
    ranges = geometry()[1] if ranges is None else ranges
    levels, uncovered, only_leaves, only_root = {}, 0, 0, 0
    for verdict, at, g in verdicts:
        for k, gk in enumerate(g):
            a, b = int(at[k]), int(at[k + 1])
            if a == b or int(gk) == DESIGNED_ID:
                continue
            count = b - a
            size, depth = dag_size(count)
            kept = [j for j in range(count) if verdict[a + j] & KEPT]
            cover = np.zeros((size + 1) // 2, np.int64)
            for j in kept:
                level = dag_level(count, j)
                levels[level] = levels.get(level, 0) + 1
                if level >= 0:
                    cover[list(dag_leaves(count, j))] += 1
            uncovered += not np.all(cover == 1)
            if size >= 3:
                in_dag = [dag_level(count, j) for j in kept if j < size]
                only_leaves += all(level == 0 for level in in_dag)
                only_root += in_dag == [depth - 1]
    return levels, uncovered, only_leaves, only_root


# ---- the designed draws and views ------------------------------------------------------------------------------------------------------
# cluster_runs_support.design_scene(): 258 unrotated entities of unit scale on a grid 120 units in front of the camera, every one wholly
# inside the frustum. Some draw the designed geometry, the rest of the first 64 draw the 127-DAG; the others draw nothing.
DESIGN_IDENTITY, DESIGN_MIRRORED, DESIGN_ZERO, DESIGN_FAR, DESIGN_DAG_FAR, DESIGN_DAG_ZERO = 40, 41, 42, 43, 44, 45
VOID_ID = ksup.VOID_IDS[0]


@functools.lru_cache(maxsize=None)
def design_scene():
    """(Scene, ids per slot, the place of the identity draw, the place of a DAG draw); read-only. DESIGN_MIRRORED: scale -1 on one
    axis (s2 = 1); DESIGN_ZERO and DESIGN_DAG_ZERO: a zero-scale model (s2 = 0: nothing exceeds); DESIGN_FAR and DESIGN_DAG_FAR: a
    translation of 1e30 along the viewing direction (inside the frustum, which has no far plane; D overflows: nothing exceeds)."""
    base = rsup.design_scene()
    sc = scene.flat_scene(base.count, defects=False)
    for name in ("position", "scale", "rotation"):
        sc.transforms[name][:] = base.transforms[name]
    sc.meshes["aabbMin"][:], sc.meshes["aabbMax"][:] = base.meshes["aabbMin"], base.meshes["aabbMax"]
    sc.transforms["scale"][DESIGN_MIRRORED, :3] = (-1.0, 1.0, 1.0)
    sc.transforms["scale"][[DESIGN_ZERO, DESIGN_DAG_ZERO], :3] = 0.0
    sc.transforms["position"][[DESIGN_FAR, DESIGN_DAG_FAR], :3] = (0.0, 0.0, 1e30)
    ids = np.full(sc.count, VOID_ID, np.uint32)
    ids[:64] = DAG_ID
    ids[[DESIGN_IDENTITY, DESIGN_MIRRORED, DESIGN_ZERO, DESIGN_FAR]] = DESIGNED_ID
    place = tuple(float(x) for x in sc.transforms["position"][DESIGN_IDENTITY, :3])
    dag_place = tuple(float(x) for x in sc.transforms["position"][7, :3])
    return sc, ids, place, dag_place


def design_views():
    """name -> the LOD view of the designed draws' one view"""
    _, _, place, dag_place = design_scene()
    return {
        "camera": lod_view(),                                                   # DESIGNED's fourth column
        "parallel": lod_view(eye=(0.0, 0.0, 0.0, 0.0)),                         # ... and its fifth
        "near-0": lod_view(near=0.0),
        "scale-1e30": lod_view(scale=1e30),                                     # every error but 0 exceeds: the cut of a DAG is its leaves
        "scale-tiny": lod_view(scale=1e-30),                                    # only +inf exceeds: the cut of a DAG is its root
        "at-a-centre": lod_view(eye=place + (1.0,)),                            # D == 0 for the identity draw's entries
        "inside-the-root": lod_view(eye=(dag_place[0] + 3.0, dag_place[1], dag_place[2] - 2.0, 1.0), scale=0.5),
        "off": lod_view(scale=-0.0),                                            # -0 switches the test off, as +0
    }


# ---- the case table ------------------------------------------------------------------------------------------------------------------
# name, draws under camera(), yaws of the views, which views query the wall, the anchor's geometry, the LOD view of every view (P the
# camera's point eye, A a point eye inside the anchor's box, O a parallel projection, Z scale 0), the cone eye of every view ("" for a call without eyes; P, D, Z as
# cluster_cones_support), the factor on the views' scale (chosen on the twin so that the census holds its conditions)
Case = namedtuple("Case", "name draws yaws hiz anchor lods eyes scale")
CASES = (
    Case("draws-0", 0, (0.0,), (False,), ksup.ANCHOR_DEFAULT, "P", "", 0.1),
    Case("draws-1-of-1", 1, (0.0,), (False,), 2, "P", "P", 0.1),           # a DAG of 1 cluster
    Case("draws-1-of-3", 1, (0.0,), (False,), 1, "P", "", 0.1),            # ... of 3
    Case("draws-1-of-63", 1, (0.0,), (False,), 5, "A", "P", 0.02),          # ... of 63, and padded to 64 and 65: the wave's edge
    Case("draws-1-of-64", 1, (0.0,), (False,), 9, "O", "", 0.1),
    Case("draws-1-of-65", 1, (0.0,), (False,), 6, "P", "D", 0.1),
    Case("draws-1-of-127", 1, (0.0,), (True,), 0, "A", "", 0.02),           # the 127-DAG over 4^3 cells
    Case("draws-2", 2, (0.0,), (False,), ksup.ANCHOR_DEFAULT, "A", "P", 0.02),
    Case("draws-256", 256, (0.0,), (False,), ksup.ANCHOR_DEFAULT, "P", "", 0.1),
    Case("draws-257", 257, (0.0,), (True,), ksup.ANCHOR_DEFAULT, "P", "P", 0.1),
    Case("tile-minus-1", 1, (0.0,), (False,), 12, "A", "", 0.02),           # one draw of 255, 256, 257 clusters: the candidate total at a tile's edge
    Case("tile", 1, (0.0,), (False,), 13, "A", "P", 0.02),
    Case("tile-plus-1", 1, (0.0,), (False,), 7, "A", "D", 0.02),
    Case("two-tiles-plus-1", 1, (0.0,), (True,), 8, "A", "", 0.02),         # 513 clusters
    Case("views-2", 64, (0.0, 0.4), (True, False), ksup.ANCHOR_DEFAULT, "PO", "PD", 0.1),
    Case("views-8", 64, ksup.EIGHT, (True, False, True, False, False, False, False, True), ksup.ANCHOR_DEFAULT, "POZPOZPO", "", 0.1),
    Case("views-8-eyes", 64, ksup.EIGHT, (True, False, True, False, False, False, False, True), ksup.ANCHOR_DEFAULT, "PPZOPZPO", "PDZPDZPD", 0.1),
)
CASE = {c.name: c for c in CASES}
SHARE_FROM = 127   # the census holds a case's LOD-kept share to [1/20, 1/2] and its level spread from this many tested clusters on


def case_views(case):
    return ksup.case_views(case)
