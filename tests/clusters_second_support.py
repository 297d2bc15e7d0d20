"""Test helpers of gv_pool_cull_clusters_second_phase: the C twin (tests/cluster_second_twin.h over tests/cluster_twin.h, which calls
the oracle's gvo_is_behind_frustum and gvo_hiz_occluded) built into a shared library, and the CASE TABLE the GPU tests
(tests/test_gpu_clusters_second.py) and the oracle-only census (tests/test_clusters_second_census.py) share. World, geometry, camera,
wall_depth, place and firsts are clusters_support's. TEST INFRASTRUCTURE ONLY.

A case names three depth images: the one in force at the cull (which decides the draws), the one at the cluster cull K1 (hiz1: what it
leaves out is pending) and the one at the second phase (hiz2). "near" hides everything: with it at K1 every tested cluster of a
queried view is pending, which pins the pending total to the cluster count of the draws."""
import ctypes as C
import functools
import os
import subprocess
from collections import namedtuple

import numpy as np

import clusters_support as ksup
from garden_amd import scene

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = ksup.TILE  # pending candidates per pending tile, as candidates per candidate tile

_TWIN_SRC = """#include "cluster_second_twin.h"
uint32_t second_twin_view(const float* models, const uint32_t* g, const uint32_t* first, uint32_t n, const void* table, uint32_t table_count,
                          const void* ranges, uint32_t range_count, const void* clusters, const float* view_proj, const GvoHiz* hiz1,
                          const GvoHiz* hiz2, void* out, uint32_t* stats)
{
    return cluster_second_twin_view(models, g, first, n, (const ClusterTwinGeometry*)table, table_count, (const ClusterTwinRange*)ranges,
                                    range_count, (const ClusterTwinCluster*)clusters, view_proj, hiz1, hiz2, (ClusterTwinCommand*)out,
                                    (ClusterSecondTwinStats*)stats);
}
"""
STATS = ("pending", "frustum_rejects", "rejected_in_view", "both_phases")


@functools.lru_cache(maxsize=None)
def twin():
    """gcc -O2 -ffp-contract=off -fno-fast-math of the twin against the oracle's library; the ctypes library (built once)."""
    import tempfile

    from oracle import oracle_py
    oracle_py.load()
    directory = tempfile.mkdtemp(prefix="cluster_second_twin_")
    src, out = os.path.join(directory, "cluster_second_twin.c"), os.path.join(directory, "libcluster_second_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    build = os.path.dirname(oracle_py.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out,
                    "-L" + build, "-Wl,-rpath," + build, "-lgv_oracle", "-lm"], check=True)
    lib = C.CDLL(out)
    P, U32 = C.c_void_p, C.c_uint32
    lib.second_twin_view.argtypes = [P, P, P, U32, P, U32, P, U32, P, P, P, P, P, P]
    lib.second_twin_view.restype = U32
    return lib


def second_view_commands(models, g, first, view_proj, hiz1, hiz2, tables=None):
    """(second-phase commands of ONE view K1 queried as a COMMAND_DTYPE array, the twin's stats as a dict). hiz1 / hiz2: the
    oracle_py.Hiz in force at K1 and at the second phase; tables: (table, ranges, clusters), default clusters_support.geometry()'s."""
    t, _, r, c = ksup.geometry()
    table, ranges, clusters = (t, r, c) if tables is None else tables
    n = len(g)
    m = np.ascontiguousarray(models, np.float32).reshape(-1, 12)[:n]
    g = np.ascontiguousarray(g, np.uint32)
    first = np.ascontiguousarray(first, np.uint32)
    vp = np.ascontiguousarray(view_proj, np.float32)
    assert len(first) == n + 1 and len(m) == n
    per_draw = np.where(g < len(ranges), ranges["count"][np.minimum(g, len(ranges) - 1)], 0)
    out = np.zeros(int(per_draw.sum(dtype=np.int64)) + 1, ksup.COMMAND_DTYPE)
    stats = np.zeros(len(STATS), np.uint32)
    count = twin().second_twin_view(m.ctypes.data, g.ctypes.data, first.ctypes.data, n, table.ctypes.data, len(table), ranges.ctypes.data,
                                    len(ranges), clusters.ctypes.data, vp.ctypes.data, C.addressof(hiz1.c), C.addressof(hiz2.c),
                                    out.ctypes.data, stats.ctypes.data)
    return out[:count], dict(zip(STATS, (int(x) for x in stats)))


def second_commands_of(fetched, starts, bases, draw_ids, views, hiz1s, hiz2s, tables=None):
    """(the second-phase commands of every view, counts[views], pending[views], the stats summed) — hiz1s[v] None: K1 did not
    query for view v (frustum only, or use_hiz == 0), nothing is pending there."""
    per_view, pending = [], []
    total = dict.fromkeys(STATS, 0)
    for v, (f, first) in enumerate(zip(fetched, ksup.firsts(fetched, starts, bases))):
        if hiz1s[v] is None:
            per_view.append(np.zeros(0, ksup.COMMAND_DTYPE))
            pending.append(0)
            continue
        n = int(f["draw_count"])
        commands, stats = second_view_commands(np.asarray(f["baked_model"]).reshape(-1, 12)[:n], draw_ids[v], first, views[v]["view_proj"],
                                               hiz1s[v], hiz2s[v], tables)
        per_view.append(commands)
        pending.append(stats["pending"])
        for name in STATS:
            total[name] += stats[name]
    return per_view, np.array([len(c) for c in per_view], np.uint32), np.array(pending, np.uint32), total


# ---- depth images --------------------------------------------------------------------------------------------------------------
def image(name):
    """far: nothing drawn; near: everything hidden; the walls of clusters_support.wall_depth at several places and distances"""
    if name == "far":
        return np.zeros((64, 128), np.float32)
    if name == "near":
        return np.ones((64, 128), np.float32)
    return ksup.wall_depth(**{"wall": {}, "wide": dict(x0=0.0), "narrow": dict(x0=0.7), "close": dict(x0=0.0, distance=14.0),
                              "deep": dict(x0=0.0, distance=300.0), "deep-right": dict(x0=0.5, distance=300.0)}[name])


# ---- a world in front of the camera -------------------------------------------------------------------------------------------
SPARSE_GEOMETRY, SPARSE_CLUSTER, SPARSE_SHIFT = 0, 17, 400.0


@functools.lru_cache(maxsize=None)
def sparse_tables():
    """clusters_support.geometry()'s tables with ONE cluster of geometry 0 (4^3 clusters) moved 400 units down the model's z: in a
    front_world it lies far behind a wall at 300 units that the other 63 stand in front of"""
    table, _, ranges, clusters = ksup.geometry()
    clusters = clusters.copy()
    at = int(ranges[SPARSE_GEOMETRY]["first"]) + SPARSE_CLUSTER
    clusters[at]["box_min"][2] += np.float32(SPARSE_SHIFT)
    clusters[at]["box_max"][2] += np.float32(SPARSE_SHIFT)
    return table, ranges, clusters


@functools.lru_cache(maxsize=None)
def front_world(draws, geometry_id=SPARSE_GEOMETRY):
    """`draws` entities of geometry `geometry_id`, unrotated and unscaled, spread 100 to 140 units in front of camera() with every box
    well inside its frustum: every one is a draw and no cluster is a frustum reject. Returns (Scene, ids); read-only."""
    _, half, _, _ = ksup.geometry()
    rng = np.random.Generator(np.random.PCG64(977 + draws))
    sc = scene.flat_scene(draws, defects=False)
    pos = np.stack([rng.uniform(-100.0, 100.0, draws), rng.uniform(-40.0, 40.0, draws), rng.uniform(100.0, 140.0, draws)], axis=1)
    sc.transforms["position"][:, :3] = pos.astype(np.float32)
    sc.transforms["scale"][:, :3] = 1.0
    sc.transforms["rotation"] = np.array([0.0, 0.0, 0.0, 1.0], np.float32)
    sc.meshes["aabbMin"][:, :3] = -half[geometry_id]
    sc.meshes["aabbMax"][:, :3] = half[geometry_id]
    return sc, np.full(draws, geometry_id, np.uint32)


# ---- the case table ------------------------------------------------------------------------------------------------------------
# name; the world ("mix": clusters_support.world(draws, anchor), "front": front_world(draws, anchor)); draws; the views' yaws; which
# views query; the anchor's / the world's geometry; the images at the cull, at K1 and at the second phase; the pending total and the
# second-phase survivor total the case NAMES (None: not named; the census holds them on the oracle); edge: a 0 / all edge, which need
# not both keep and reject a pending cluster; tables: "sparse" for sparse_tables()
Case = namedtuple("Case", "name world draws yaws hiz anchor images pending kept edge tables", defaults=(None, None, False, None))
A = ksup.ANCHOR_DEFAULT
ONE = (0.0,)
CASES = (
    # pending totals at a pending tile's edges: "near" at K1 makes every cluster of the one clustered draw pending
    Case("pending-0", "mix", 0, ONE, (True,), A, ("far", "far", "wall"), 0, 0, True),
    Case("pending-1", "mix", 1, ONE, (True,), 2, ("far", "near", "wall"), 1, 1, True),
    Case("pending-255", "mix", 1, ONE, (True,), 12, ("far", "near", "wall"), 255),
    Case("pending-256", "mix", 1, ONE, (True,), 13, ("far", "near", "wall"), 256),
    Case("pending-257", "mix", 1, ONE, (True,), 7, ("far", "near", "wall"), 257),   # one draw whose pending spans two pending tiles
    Case("pending-513", "mix", 1, ONE, (True,), 8, ("far", "near", "wall"), 513),   # ... and three
    # survivor totals of 0 (the pyramid K1 queried) and of all pending (nothing is a frustum reject, nothing is hidden any more)
    Case("kept-0", "mix", 64, ONE, (True,), A, ("wall", "wall", "wall"), None, 0, True),
    Case("kept-all", "front", 2, ONE, (True,), 0, ("far", "near", "far"), 128, 128, True),
    # draws: whole, void and clustered draws side by side, a wall that comes closer at K1 and goes back
    Case("draws-1", "mix", 1, ONE, (True,), A, ("far", "close", "wall")),
    Case("draws-2", "mix", 2, ONE, (True,), A, ("far", "close", "wall")),
    Case("draws-255", "mix", 255, ONE, (True,), A, ("far", "close", "wall")),
    Case("draws-256", "mix", 256, ONE, (True,), A, ("far", "close", "wall")),
    Case("draws-257", "mix", 257, ONE, (True,), A, ("wall", "wide", "narrow")),
    # one pending cluster per draw of 64 over 257 draws: a pending tile spans 64 candidate tiles
    Case("sparse", "front", 257, ONE, (True,), 0, ("far", "deep", "deep-right"), 257, None, False, "sparse"),
    # several views, mixed query bits
    Case("views-2", "mix", 64, (0.0, 0.4), (True, False), A, ("far", "close", "wall")),
    Case("views-2-second", "mix", 64, (0.0, 0.4), (False, True), A, ("far", "close", "wall")),
    Case("views-8", "mix", 64, ksup.EIGHT, (True, False, True, False, False, False, False, True), A, ("far", "close", "wall")),
)
CASE = {c.name: c for c in CASES}


def case_world(case):
    """(Scene, ids per slot, the tables or None)"""
    tables = sparse_tables() if case.tables == "sparse" else None
    if case.world == "front":
        return front_world(case.draws, case.anchor) + (tables,)
    return ksup.world(case.draws, anchor=case.anchor) + (tables,)


def case_views(case):
    return ksup.case_views(case)


def case_census(case, oracle):
    """The case on the ORACLE ALONE: the records are the oracle's cull against the image in force at the cull, the clusters are
    decided by the twins. Returns (the stats summed over the queried views, kept = second-phase commands, K1's commands, per queried
    view (view number, pending))."""
    sc, ids, tables = case_world(case)
    hiz0, hiz1, hiz2 = (oracle.Hiz(image(name)) for name in case.images)
    total = dict.fromkeys(STATS, 0)
    kept = first_phase = 0
    per_view = []
    for v, (view, query) in enumerate(zip(case_views(case), case.hiz)):
        got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view, hiz=hiz0 if query else None)
        n = int(got["draw_count"])
        g = ids[got["visible_idx"][:n]]
        extra = {} if tables is None else dict(table=tables[0], ranges=tables[1], clusters=tables[2])
        first_phase += len(ksup.view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], hiz1 if query else None, **extra)[0])
        if not query:
            continue
        commands, stats = second_view_commands(got["baked_model"], g, np.arange(n + 1), view["view_proj"], hiz1, hiz2, tables)
        kept += len(commands)
        per_view.append((v, stats["pending"]))
        for name in STATS:
            total[name] += stats[name]
    return total, kept, first_phase, per_view
