"""Test helpers of gv_pool_cull_cluster_runs: the C twin (tests/cluster_runs_twin.h — which cluster survives is decided by
cluster_twin.h, that is by the oracle's two tests; it restates linked, head, run and the run's command, and counts the census) built
into a shared library; cluster tables with the boxes of clusters_support.geometry() and CONTIGUOUS index ranges per geometry with
designed breaks; the designed single-draw scenes of the rule's edges. World, cameras, wall and CASES are clusters_support's. TEST
INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import clusters_support as ksup
import commands_support as csup
from garden_amd import scene
from garden_amd.lib import CLUSTER_DTYPE, CLUSTER_RANGE_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
SPAN = 256  # GV_CLUSTER_RUN_SPAN
CENSUS_FIELDS = ("candidates", "survivors", "runs", "whole", "longest", "break_nonsurvivor", "break_gap", "break_span", "cross_word",
                 "cross_tile")

_TWIN_SRC = """#include "cluster_runs_twin.h"
uint32_t runs_twin_view(const float* models, const uint32_t* g, const uint32_t* first, uint32_t n, const void* table, uint32_t table_count,
                        const void* ranges, uint32_t range_count, const void* clusters, const float* view_proj, const GvoHiz* hiz,
                        uint64_t candidate_base, void* out, uint32_t* tested, uint32_t* census)
{
    return cluster_runs_twin_view(models, g, first, n, (const ClusterTwinGeometry*)table, table_count, (const ClusterTwinRange*)ranges,
                                  range_count, (const ClusterTwinCluster*)clusters, view_proj, hiz, candidate_base, (ClusterTwinCommand*)out,
                                  tested, (ClusterRunsCensus*)census);
}
uint32_t runs_twin_census_words(void) { return (uint32_t)(sizeof(ClusterRunsCensus) / sizeof(uint32_t)); }
uint32_t runs_twin_span(void) { return CLUSTER_RUNS_TWIN_SPAN; }
"""


@functools.lru_cache(maxsize=None)
def twin():
    """gcc -O2 -ffp-contract=off -fno-fast-math of the twin against the oracle's library; the ctypes library (built once)."""
    import tempfile

    from oracle import oracle_py
    oracle_py.load()
    directory = tempfile.mkdtemp(prefix="cluster_runs_twin_")
    src, out = os.path.join(directory, "cluster_runs_twin.c"), os.path.join(directory, "libcluster_runs_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    build = os.path.dirname(oracle_py.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out,
                    "-L" + build, "-Wl,-rpath," + build, "-lgv_oracle", "-lm"], check=True)
    lib = C.CDLL(out)
    P, U32 = C.c_void_p, C.c_uint32
    lib.runs_twin_view.argtypes = [P, P, P, U32, P, U32, P, U32, P, P, P, C.c_uint64, P, P, P]
    lib.runs_twin_view.restype = U32
    lib.runs_twin_census_words.restype = U32
    lib.runs_twin_span.restype = U32
    assert lib.runs_twin_census_words() == len(CENSUS_FIELDS) and lib.runs_twin_span() == SPAN
    return lib


# ---- cluster tables with contiguous index ranges and designed breaks --------------------------------------------------------------
GAP_GEOMETRIES, GAP_EVERY, GAP = (0, 5), 11, 7       # a hole of 7 indices behind every 11th cluster of geometries 0 and 5
OVERLAP_GEOMETRY, OVERLAP_AT, OVERLAP = 1, 4, 5      # cluster 4 of geometry 1 begins 5 indices before cluster 3 ends
ZERO_GEOMETRY, ZERO_AT = 10, (2, 5)                  # clusters of geometry 10 with count 0, inside a run (never two in a row: a
                                                     # command names its cluster by first and count in coalesce() below)
WRAP_GEOMETRY, WRAP_AT = 6, 20                       # cluster 20 of geometry 6 ends at exactly 2^32: no link; its successor begins at 0x40


def contiguous(clusters, ranges):
    """`first` of every cluster rewritten so that a geometry's clusters lie back to back from 1000 * (g + 1), with the designed
    breaks; boxes and counts stay. Returns a new cluster table."""
    out = clusters.copy()
    for g, r in enumerate(ranges):
        at = 1000 * (g + 1)
        a, n = int(r["first"]), int(r["count"])
        if g == ZERO_GEOMETRY:
            for j in ZERO_AT:
                out[a + j]["count"] = 0
        if g == WRAP_GEOMETRY:  # the clusters up to WRAP_AT end at exactly 2^32
            at = (1 << 32) - int(out[a:a + WRAP_AT + 1]["count"].sum(dtype=np.int64))
        for j in range(n):
            if g in GAP_GEOMETRIES and j and j % GAP_EVERY == 0:
                at += GAP
            if g == OVERLAP_GEOMETRY and j == OVERLAP_AT:
                at -= OVERLAP
            if g == WRAP_GEOMETRY and j == WRAP_AT + 1:
                assert at == 1 << 32
                at = 0x40
            out[a + j]["first"] = at
            at += int(out[a + j]["count"])
    return out


@functools.lru_cache(maxsize=None)
def geometry():
    """(geometry table, box half-extents, ranges, clusters) as clusters_support.geometry() with contiguous index ranges; read-only."""
    table, half, ranges, clusters = ksup.geometry()
    assert int(table[WRAP_GEOMETRY]["first"]) == 0xFFFFFF00  # the head's uint32 add wraps
    return table, half, ranges, contiguous(clusters, ranges)


# ---- expected values ---------------------------------------------------------------------------------------------------------------
def view_commands(models, g, first, view_proj, hiz, candidate_base=0, table=None, ranges=None, clusters=None):
    """(commands of ONE view as a COMMAND_DTYPE array, tested, the census as a dict) by the twin"""
    t, _, r, c = geometry()
    table = t if table is None else table
    ranges, clusters = (r if ranges is None else ranges), (c if clusters is None else clusters)
    n = len(g)
    m = np.ascontiguousarray(models, np.float32).reshape(-1, 12)[:n]
    g = np.ascontiguousarray(g, np.uint32)
    first = np.ascontiguousarray(first, np.uint32)
    vp = np.ascontiguousarray(view_proj, np.float32)
    assert len(first) == n + 1 and len(m) == n
    per_draw = np.where(g < len(ranges), np.maximum(ranges["count"][np.minimum(g, len(ranges) - 1)], 1), 1)
    out = np.zeros(int(per_draw.sum(dtype=np.int64)) + 1, ksup.COMMAND_DTYPE)
    tested = C.c_uint32()
    census = np.zeros(len(CENSUS_FIELDS), np.uint32)
    count = twin().runs_twin_view(m.ctypes.data, g.ctypes.data, first.ctypes.data, n, table.ctypes.data, len(table), ranges.ctypes.data,
                                  len(ranges), clusters.ctypes.data, vp.ctypes.data, C.addressof(hiz.c) if hiz is not None else None,
                                  int(candidate_base), out.ctypes.data, C.addressof(tested), census.ctypes.data)
    return out[:count], tested.value, dict(zip(CENSUS_FIELDS, (int(x) for x in census)))


def add_census(total, one):
    for name in CENSUS_FIELDS:
        total[name] = max(total.get(name, 0), one[name]) if name == "longest" else total.get(name, 0) + one[name]
    return total


def commands_of(fetched, starts, bases, draw_ids, views, hizzes, tables=None):
    """(the commands of every view, counts[views], tested[views], the census summed over the views) of a run cull; arguments as
    clusters_support.commands_of. tables: None for geometry(), or (table, ranges, clusters)."""
    table, ranges, clusters = (None, None, None) if tables is None else tables
    per_view, tested, census, base = [], [], {}, 0
    for v, (f, first) in enumerate(zip(fetched, ksup.firsts(fetched, starts, bases))):
        n = int(f["draw_count"])
        commands, t, one = view_commands(np.asarray(f["baked_model"]).reshape(-1, 12)[:n], draw_ids[v], first, views[v]["view_proj"], hizzes[v],
                                         base, table, ranges, clusters)
        base += one["candidates"]
        add_census(census, one)
        per_view.append(commands)
        tested.append(t)
    return per_view, np.array([len(c) for c in per_view], np.uint32), np.array(tested, np.uint32), census


def coalesce(plain, clusters_of_draw):
    """The run commands that the plain form's commands of ONE view coalesce into, by the rule restated over the commands alone.
    plain: the view's per-cluster commands (COMMAND_DTYPE) in order; clusters_of_draw(k) -> (G.first, the draw's cluster rows, or
    None for a draw drawn whole). A plain command is matched to its cluster j by walking the draw's clusters in order."""
    out = []
    at = 0
    while at < len(plain):
        k = int(plain[at]["draw"])
        end = at
        while end < len(plain) and int(plain[end]["draw"]) == k:
            end += 1
        gfirst, cl = clusters_of_draw(k)
        if cl is None:
            assert end == at + 1
            out.append(plain[at].copy())
            at = end
            continue
        # which clusters survived: the plain commands are a subsequence of the draw's clusters, in order
        kept, j = [], 0
        for row in plain[at:end]:
            while not (((gfirst + int(cl[j]["first"])) & 0xFFFFFFFF) == int(row["first"]) and int(cl[j]["count"]) == int(row["count"])):
                j += 1
            kept.append(j)
            j += 1
        previous = None
        for row, j in zip(plain[at:end], kept):
            linked = (j > 0 and j % SPAN != 0 and int(cl[j - 1]["first"]) + int(cl[j - 1]["count"]) == int(cl[j]["first"])
                      and int(cl[j]["first"]) + int(cl[j]["count"]) <= 0xFFFFFFFF)
            if linked and previous == j - 1:
                out[-1]["count"] = (int(cl[j]["first"]) + int(cl[j]["count"]) - head_first) & 0xFFFFFFFF
            else:
                out.append(row.copy())
                head_first = int(cl[j]["first"])
            previous = j
        at = end
    return np.array(out, ksup.COMMAND_DTYPE) if out else np.zeros(0, ksup.COMMAND_DTYPE)


# ---- the designed scenes: one clustered draw behind `lead` whole draws -----------------------------------------------------------
DESIGN_ENTITIES = 258          # every one unrotated, unit scale, wholly inside camera()'s frustum
CLUSTERED_ID, WHOLE_ID, VOID_ID = 0, 1, 7
INSIDE, BEHIND = 0.0, -1000.0  # model-space z of a cluster box's centre: inside the entity, or far behind the camera
LEADS = (0, 1, 63, 64, 255)


@functools.lru_cache(maxsize=None)
def design_scene():
    """DESIGN_ENTITIES entities on a grid in front of the camera (which looks along +z from the origin), boxes of half-extent 1"""
    sc = scene.flat_scene(DESIGN_ENTITIES, defects=False)
    i = np.arange(DESIGN_ENTITIES)
    sc.transforms["position"][:, 0] = (i % 16 - 7.5) * 3.0
    sc.transforms["position"][:, 1] = ((i // 16) % 17 - 8.0) * 3.0
    sc.transforms["position"][:, 2] = 120.0
    sc.transforms["scale"][:, :3] = 1.0
    sc.transforms["rotation"] = (0.0, 0.0, 0.0, 1.0)
    sc.meshes["aabbMin"][:, :3] = -1.0
    sc.meshes["aabbMax"][:, :3] = 1.0
    return sc


def design_tables(survive, firsts_counts=None, gfirst=5000):
    """(geometry table, ranges, clusters) of a designed scene: geometry CLUSTERED_ID has len(survive) clusters — cluster j's box lies
    inside the entity where survive[j], far behind the camera otherwise; index ranges back to back from 100 with counts 3 + j % 5,
    or the rows (first, count) given. Geometry WHOLE_ID has no range: drawn whole."""
    n = len(survive)
    table = csup.geometry_table([(9999, gfirst, -3), (77, 123456, 11)])
    table[CLUSTERED_ID]["first"] = gfirst
    ranges = np.zeros(1, CLUSTER_RANGE_DTYPE)
    ranges[0] = (0, n)
    clusters = np.zeros(n, CLUSTER_DTYPE)
    at = 100
    for j in range(n):
        z = INSIDE if survive[j] else BEHIND
        clusters[j]["box_min"] = (-0.5, -0.5, z - 0.5)
        clusters[j]["box_max"] = (0.5, 0.5, z + 0.5)
        if firsts_counts is None:
            clusters[j]["first"], clusters[j]["count"] = at, 3 + j % 5
            at += 3 + j % 5
        else:
            clusters[j]["first"], clusters[j]["count"] = firsts_counts[j]
    return table, ranges, clusters


def rows_of_geometry(g):
    """(first, count) of every cluster of geometry g of geometry(), and its G.first"""
    table, _, ranges, clusters = geometry()
    a, n = int(ranges[g]["first"]), int(ranges[g]["count"])
    return [(int(c["first"]), int(c["count"])) for c in clusters[a:a + n]], int(table[g]["first"])


def design_patterns():
    """name -> (survive per cluster, (first, count) rows or None, G.first, what the census must hold: a dict of exact values)"""
    p = {}
    for n, runs in ((1, 1), (2, 1), (255, 1), (256, 1), (257, 2), (513, 3)):
        p[f"all-{n}"] = ([True] * n, None, 5000, {"survivors": n, "runs": runs, "longest": min(n, SPAN), "break_span": runs - 1, "break_gap": 0,
                                                 "break_nonsurvivor": 0})
    alternating = [j % 2 == 0 for j in range(130)]
    p["alternating"] = (alternating, None, 5000, {"survivors": 65, "runs": 65, "longest": 1, "break_nonsurvivor": 64})
    for j in (0, 63, 64, 255, 256):
        survive = [True] * 300
        survive[j] = False
        # (the span breaks the survivors at 256 too, unless 256 is the rejected one or its predecessor is)
        runs = {0: 2, 63: 3, 64: 3, 255: 2, 256: 2}[j]
        p[f"reject-{j}"] = (survive, None, 5000, {"survivors": 299, "runs": runs})
    gaps = []
    at = 100
    for j in range(40):
        at += 4 if j and j % 7 == 0 else 0
        gaps.append((at, 6))
        at += 6
    p["gaps-only"] = ([True] * 40, gaps, 5000, {"survivors": 40, "runs": 6, "break_gap": 5, "break_nonsurvivor": 0, "break_span": 0, "longest": 7})
    rows, gfirst = rows_of_geometry(OVERLAP_GEOMETRY)
    p["overlap"] = ([True] * len(rows), rows, gfirst, {"survivors": 8, "runs": 2, "break_gap": 1, "longest": 4})
    rows, gfirst = rows_of_geometry(ZERO_GEOMETRY)
    p["zero-count"] = ([True] * len(rows), rows, gfirst, {"survivors": 8, "runs": 1, "longest": 8})
    rows, gfirst = rows_of_geometry(WRAP_GEOMETRY)
    p["wrap"] = ([True] * len(rows), rows, gfirst, {"survivors": 65, "runs": 3, "break_gap": 2, "longest": 44})
    return p
