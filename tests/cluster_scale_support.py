"""Test helpers of the cluster cull AT SCALE: two designed worlds that take the index machinery of garden_amd/csrc/gv_clusters.hip
past its first iteration — scan_table's second turn, the strided per-view sums and table fills, locate / find_pending with a search
width, the second and third pass of every grid-stride walk, the strided padding loops — and a numpy restatement of
clusters_support.firsts / place, which loop per draw and per command. The GPU tests (tests/test_gpu_cluster_scale.py) and the
oracle-only census (tests/test_cluster_scale_census.py) share them. Expected values come from the C twins of the cluster tests
(cluster_twin.h and its siblings over the oracle's gvo_is_behind_frustum / gvo_hiz_occluded). TEST INFRASTRUCTURE ONLY.

WORLD A, "wide and sparse" — the COUNT side. S = 262 401 slots on a grid in front of clusters_support.camera(), five views: 1026
count workgroups per view, 5130 in all, so cluster_scan_kernel<0> scans block_total in two turns, the second through its scalar
tail. Views 0, 1, 3 and 4 see all but a corner of the grid (the top and bottom planes of a slightly yawed view cut a thin triangle
off the rim); view 2 looks away. Most slots hold the void id; a random 1 / 128 of them (and a quarter of the last 4096, so that
the draws behind index 262 144 of every view have clusters) hold a whole id or a range of 1, 2 or 3 clusters, so a candidate tile
spans dozens of count workgroups and many count workgroups hold nothing. The slots lie in the mirror's own order (the Morton order
of their cells, reorder_support.codes), so that the oracle's slot order is the order the device delivers.

WORLD B, "deep" — the TILE side. 300 slots, two views, ranges of 4096 and 4097 clusters (16^3 cells of the entity's box and one
more), one of 1000, a whole id and a void one. THE SPLIT: view 0 (which queries the pyramid) sees nearly every slot and alone has
more than 2^20 tested clusters — what the dense second phase needs —; view 1 (frustum only) is turned away and keeps a quarter of
the draws, which puts its first candidate mid-tile far behind tile 2048. T is about 1.4 x 10^6: more than 4096 tiles, more than two
passes of a grid of 8 x 256 workgroups."""
import functools
import math
from collections import namedtuple

import numpy as np

import cluster_cones_support as nsup
import cluster_lods_support as lsup
import clusters_support as ksup
import commands_support as csup
import reorder_support as rosup
from garden_amd import scene
from garden_amd.lib import CLUSTER_CONE_DTYPE, CLUSTER_DTYPE, CLUSTER_LOD_DTYPE, CLUSTER_RANGE_DTYPE

# thresholds of garden_amd/csrc/gv_cluster_kernels.hpp, restated
SCAN_TURN = 4096    # 4 * kClusterScanBlock: entries of one turn of scan_table
SCAN_BLOCK = 1024   # kClusterScanBlock: lanes of the scanning workgroup; the stride of its sums and fills
TILE = 256          # kClusterTile (and kClusterBlock: draws per count workgroup)
GRID_PER_CU = 8     # kClusterGridPerCu
CUS = 256           # compute units of an MI355X (the census; the GPU tests read the device)
SPAN = 256          # kClusterRunSpan


def tiles_of(total):
    return -(-int(total) // TILE)


# ---- placement and firsts, in numpy ------------------------------------------------------------------------------------------------
def firsts(fetched, starts, bases):
    """clusters_support.firsts as arrays: per view first[0 .. n] with the closing word behind the last draw"""
    out = []
    for v, f in enumerate(fetched):
        n = int(f["draw_count"])
        if bases is None:
            head = np.uint32(starts[v]) + np.arange(n, dtype=np.uint32)
        else:
            first_instance, draw_starts = bases
            head = np.asarray(first_instance, np.uint32)[int(draw_starts[v]):int(draw_starts[v]) + n]
        out.append(np.concatenate([head, np.array([starts[v + 1]], np.uint32)]).astype(np.uint32))
    return out


def place(per_view, dtype, region, capacity, pattern):
    """clusters_support.place without a Python loop over commands: a prefix over the per-view counts, one fancy-index store per
    view, the padding by slice. Returns the bytes [rows, stride]."""
    stride = dtype.itemsize
    rows = len(pattern)
    room = rows if capacity is None else int(capacity)
    counts = np.array([len(c) for c in per_view], np.int64)
    packed_at = np.concatenate([[0], np.cumsum(counts)])
    out = pattern.copy()
    for v, commands in enumerate(per_view):
        base = v * region if region else int(packed_at[v])
        n = min(len(commands), region) if region else len(commands)
        positions = base + np.arange(n, dtype=np.int64)
        positions = positions[positions < room]
        if len(positions):
            assert int(positions[-1]) < rows, "the pattern is too small for the test's own target"
            laid = np.zeros(len(positions), dtype)
            for name in dtype.names:
                laid[name] = commands[name][:len(positions)]
            out[positions] = laid.view(np.uint8).reshape(len(positions), stride)
        if region:
            lo, hi = base + n, min(base + region, room)
            if hi > lo:
                assert hi <= rows, "the pattern is too small for the test's own target"
                out[lo:hi] = 0
    return out


# ---- what both worlds share --------------------------------------------------------------------------------------------------------
def _grid_scene(x, y, z, half):
    """a flat scene of unrotated entities of unit scale at (x, y, z) with boxes of half-extents `half`, its slots in the mirror's own
    order: sorted (stably) by the Morton code the mirror gives them"""
    n = len(x)
    sc = scene.flat_scene(n, defects=False)
    sc.transforms["position"][:, 0], sc.transforms["position"][:, 1], sc.transforms["position"][:, 2] = x, y, z
    sc.transforms["scale"][:, :3] = 1.0
    sc.transforms["rotation"] = np.array([0.0, 0.0, 0.0, 1.0], np.float32)
    order = np.argsort(rosup.codes(sc.transforms, sc.entity_to_transform), kind="stable")
    sc.transforms["position"][:, :3] = sc.transforms["position"][order, :3].copy()
    code = rosup.codes(sc.transforms, sc.entity_to_transform)
    assert np.all(code[1:] >= code[:-1])  # (a permutation keeps the box, hence the cells)
    sc.meshes["aabbMin"][:, :3] = -np.asarray(half, np.float32)
    sc.meshes["aabbMax"][:, :3] = np.asarray(half, np.float32)
    return sc


def _index_ranges(clusters, a, n, at, rng, breaks):
    """first / count of clusters [a, a + n): back to back from `at`, a hole of 5 indices in front of every 37th cluster and in front
    of the clusters listed in `breaks`"""
    count = rng.integers(3, 384, n).astype(np.int64)
    hole = np.zeros(n, np.int64)
    hole[37::37] = 5
    hole[list(breaks)] = 5
    first = at + np.cumsum(hole) + np.concatenate([[0], np.cumsum(count)[:-1]])
    clusters["first"][a:a + n], clusters["count"][a:a + n] = first.astype(np.uint32), count.astype(np.uint32)


World = namedtuple("World", "scene ids tables yaws hiz occupancy")


def views_of(world):
    return [ksup.camera(yaw, use_hiz=1 if h else 0, shadow_pass=-1 if k == 0 else k) for k, (yaw, h) in enumerate(zip(world.yaws, world.hiz))]


# ---- world A -------------------------------------------------------------------------------------------------------------------------
A_SLOTS = 262401                       # 1025 * 256 + 1: 1026 count workgroups per view
A_COLUMNS, A_ROWS = 513, 512
A_DISTANCE = 200.0
A_HALF_WIDTH, A_HALF_HEIGHT = 0.5 * A_DISTANCE, 0.9952 * A_DISTANCE   # the grid's extent at that distance: inside the side planes, at the top and bottom ones
A_YAWS = (0.012, -0.012, math.pi, 0.016, -0.016)
A_HIZ = (False, True, False, False, True)
A_SHARE, A_TAIL, A_TAIL_SHARE = 1.0 / 128.0, 4096, 0.25
A_TABLE_COUNT = 8                      # ids 0 .. 7 are in the table; 0, 6, 7 have no range and are drawn whole
A_VOID = (A_TABLE_COUNT, A_TABLE_COUNT + 3)
A_RANGES = (0, 1, 2, 3, 1, 2)          # clusters of ids 0 .. 5
A_MAX_RANGE = 3
A_BEHIND = -2.0 * A_DISTANCE           # model-space z of a cluster that lies behind every camera


@functools.lru_cache(maxsize=None)
def world_a():
    i = np.arange(A_SLOTS)
    column, row = i % A_COLUMNS, i // A_COLUMNS
    x = (column - 0.5 * (A_COLUMNS - 1)) * (2.0 * A_HALF_WIDTH / (A_COLUMNS - 1))
    y = (row - 0.5 * (A_ROWS - 1)) * (2.0 * A_HALF_HEIGHT / (A_ROWS - 1))
    h = 0.3 * 2.0 * A_HALF_WIDTH / (A_COLUMNS - 1)
    sc = _grid_scene(x, y, np.full(A_SLOTS, A_DISTANCE), (h, h, h))
    # ids: void, but for a random share — denser in the last slots, which are the last draws of every view
    rng = np.random.Generator(np.random.PCG64(20260))
    ids = np.where(rng.random(A_SLOTS) < 0.5, A_VOID[0], A_VOID[1]).astype(np.uint32)
    share = np.full(A_SLOTS, A_SHARE)
    share[A_SLOTS - A_TAIL:] = A_TAIL_SHARE
    held = rng.random(A_SLOTS) < share
    ids[held] = rng.choice(np.arange(A_TABLE_COUNT), int(held.sum()), p=[0.06, 0.3, 0.25, 0.15, 0.08, 0.1, 0.03, 0.03]).astype(np.uint32)
    # the tables: a cluster lies INSIDE the entity's box (one of its octants' slabs) or far BEHIND the cameras
    table = csup.geometry_table([(int(rng.integers(1, 1 << 20)), int(rng.integers(0, 1 << 30)), int(rng.integers(-(1 << 20), 1 << 20)))
                                 for _ in range(A_TABLE_COUNT)])
    ranges = np.zeros(len(A_RANGES), CLUSTER_RANGE_DTYPE)
    clusters = np.zeros(sum(A_RANGES), CLUSTER_DTYPE)
    inside = {1: (True,), 2: (True, False), 3: (True, False, True), 4: (False,), 5: (True, True)}
    at = 0
    for g, count in enumerate(A_RANGES):
        ranges[g] = (at, count)
        for j in range(count):
            z = 0.0 if inside[g][j] else A_BEHIND
            lo = -h + (2.0 * h * j) / count
            clusters[at + j]["box_min"], clusters[at + j]["box_max"] = (lo, -h, z - h), (lo + 2.0 * h / count, h, z + h)
        if count:
            _index_ranges(clusters, at, count, 1000 * (g + 1), rng, ())
        at += count
    return World(sc, ids, (table, ranges, clusters), A_YAWS, A_HIZ, A_SLOTS)


def a_image(name):
    """the depth images of world A: "wall" hides the right half of the screen at mid-scene depth (the grid fills its middle), "narrow"
    its right quarter — the pyramid rebuilt in front of the second phase"""
    return ksup.wall_depth(x0={"wall": 0.5, "narrow": 0.75}[name])


# ---- world B -------------------------------------------------------------------------------------------------------------------------
B_COLUMNS, B_ROWS = 20, 15
B_SLOTS = B_COLUMNS * B_ROWS
B_DISTANCE = 100.0
B_HALF = (8.0, 6.0, 6.0)
B_YAWS = (0.0, 1.8)
B_HIZ = (True, False)
B_CELLS = 16
B_RANGES = (B_CELLS ** 3, B_CELLS ** 3 + 1, 1000)   # ids 0, 1, 2; id 3 is drawn whole, id 4 is void
B_TABLE_COUNT, B_VOID = 4, 4
B_MAX_RANGE = B_CELLS ** 3 + 1
B_BREAKS = ((SPAN - 1,), (SPAN + 1,), (2 * SPAN - 1,))   # a hole in front of cluster 255, 257, 511 of the three ranges
B_WRAP_GEOMETRY = 2                    # table.first + cluster.first wraps 32 bits, as geometry 6 of clusters_support.geometry()
B_BAD_GEOMETRY, B_NAN_CLUSTER, B_INVERTED_CLUSTER = 0, 3, 7


def _cells(half, grid, count):
    """(box_min, box_max) of the first `count` cells of a grid^3 sub-grid of the box; the cells behind them: a small box in the middle"""
    half = np.asarray(half, np.float32)
    j = np.arange(count)
    ix = np.stack([j % grid, (j // grid) % grid, j // (grid * grid)], axis=1).astype(np.float32)
    cell = (np.float32(2.0) * half / np.float32(grid)).astype(np.float32)
    lo, hi = -half + cell * ix, -half + cell * (ix + np.float32(1.0))
    extra = j >= grid ** 3
    lo[extra], hi[extra] = -np.float32(0.1) * half, np.float32(0.1) * half
    return lo.astype(np.float32), hi.astype(np.float32)


@functools.lru_cache(maxsize=None)
def world_b():
    i = np.arange(B_SLOTS)
    column, row = i % B_COLUMNS, i // B_COLUMNS
    x = (column - 0.5 * (B_COLUMNS - 1)) * 17.8
    y = (row - 0.5 * (B_ROWS - 1)) * 13.3
    z = B_DISTANCE + 3.0 * ((column + 2 * row) % 5)
    sc = _grid_scene(x, y, z, B_HALF)
    rng = np.random.Generator(np.random.PCG64(20261))
    ids = (np.arange(B_SLOTS) % 2).astype(np.uint32)           # ranges of 4096 and 4097 in turn
    ids[5::16] = 2
    ids[11::41] = 3
    ids[17::53] = B_VOID
    ids[B_SLOTS - 1] = 0                                       # the last draw of both views: its last clusters are linked
    table = csup.geometry_table([(int(rng.integers(1, 1 << 20)), int(rng.integers(0, 1 << 30)), int(rng.integers(-(1 << 20), 1 << 20)))
                                 for _ in range(B_TABLE_COUNT)])
    table[B_WRAP_GEOMETRY]["first"] = 0xFFFFFF00
    ranges = np.zeros(len(B_RANGES), CLUSTER_RANGE_DTYPE)
    clusters = np.zeros(sum(B_RANGES), CLUSTER_DTYPE)
    at = 0
    for g, count in enumerate(B_RANGES):
        ranges[g] = (at, count)
        lo, hi = _cells(B_HALF, B_CELLS if g < 2 else 10, count)
        clusters["box_min"][at:at + count], clusters["box_max"][at:at + count] = lo, hi
        _index_ranges(clusters, at, count, 1000 * (g + 1) + 0x200 * (g == B_WRAP_GEOMETRY), rng, B_BREAKS[g])
        at += count
    bad = int(ranges[B_BAD_GEOMETRY]["first"])
    clusters[bad + B_NAN_CLUSTER]["box_min"][0] = np.nan
    lo, hi = clusters[bad + B_INVERTED_CLUSTER]["box_min"].copy(), clusters[bad + B_INVERTED_CLUSTER]["box_max"].copy()
    clusters[bad + B_INVERTED_CLUSTER]["box_min"], clusters[bad + B_INVERTED_CLUSTER]["box_max"] = hi, lo
    return World(sc, ids, (table, ranges, clusters), B_YAWS, B_HIZ, B_SLOTS)


# B's cones and LOD entries, designed directly over its cell grid: outward cones (cluster_cones_support.outward_cones); a LOD entry
# per cluster whose self sphere holds the cell and whose parent sphere holds the box, the errors spread so that a point eye at the
# camera with B_LOD_SCALE keeps some clusters of every draw and cuts others
B_LOD_SCALE = 540.0   # cluster_lods_support.CAMERA_SCALE: the camera at 1080 rows and one pixel
B_EYE = (0.0, 0.0, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def b_wide_tables():
    """(table, ranges, clusters, cones, lods) of world B"""
    table, ranges, clusters = world_b().tables
    cones = nsup.outward_cones(clusters, seed=311)
    assert cones.dtype == CLUSTER_CONE_DTYPE
    rng = np.random.Generator(np.random.PCG64(20262))
    lods = np.zeros(len(clusters), CLUSTER_LOD_DTYPE)
    lods["reserved"] = 0xDEADBEEF  # not read
    lo, hi = clusters["box_min"].astype(np.float32), clusters["box_max"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        centre = np.nan_to_num(np.float32(0.5) * (lo + hi)).astype(np.float32)
        radius = np.nan_to_num(np.float32(0.5) * np.linalg.norm(hi - lo, axis=1)).astype(np.float32)
    lods["self_center"], lods["self_radius"] = centre, radius
    lods["parent_center"], lods["parent_radius"] = 0.0, np.float32(np.linalg.norm(np.asarray(B_HALF, np.float32)))
    # about B_DISTANCE away a pixel is B_DISTANCE / B_LOD_SCALE units: errors around it, so that both EXCEEDS decide both ways
    pixel = B_DISTANCE / B_LOD_SCALE
    lods["self_error"] = (pixel * rng.uniform(0.0, 1.3, len(clusters))).astype(np.float32)
    lods["parent_error"] = (pixel * rng.uniform(0.7, 4.0, len(clusters))).astype(np.float32)
    return table, ranges, clusters, cones, lods


def b_lod_views(scale=B_LOD_SCALE):
    return [lsup.lod_view(eye=B_EYE, scale=scale), lsup.lod_view(eye=B_EYE, scale=scale)]


B_EYES = np.array([B_EYE, B_EYE], np.float32)


# ---- depth images of B's second phases -----------------------------------------------------------------------------------------------
def image(name):
    """clusters_second_support.image's, and "dots": far but for two small near patches in opposite corners of view 0's grid, which
    hide about one in a hundred of its clusters — the pending of a pending tile then lie thousands of candidate tiles apart"""
    import clusters_second_support as ssup
    if name == "dots":
        d = np.zeros((64, 128), np.float32)
        d[6:11, 20:30] = 1.0
        d[52:57, 96:106] = 1.0
        return d
    return ssup.image(name)


# ---- the candidates of a world by the twins ------------------------------------------------------------------------------------------
def records_of(world, oracle):
    """the oracle's own cull of the world per view (no pyramid: the tests cull under the far image): (models, g, first)"""
    sc = world.scene
    out = []
    for view in views_of(world):
        got = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view)
        n = int(got["draw_count"])
        out.append((got["baked_model"], world.ids[got["visible_idx"][:n]].astype(np.uint32), np.arange(n + 1, dtype=np.uint32)))
    return out


def candidates_per_draw(g, table, ranges):
    """candidates of every draw: 0 for a void id, 1 for a draw drawn whole, the range's count otherwise"""
    count = np.where(g < len(ranges), ranges["count"][np.minimum(g, len(ranges) - 1)], 0).astype(np.int64)
    return np.where(g < len(table), np.maximum(count, 1), 0)


class Candidates:
    """The candidate numbering of a call over `records` (per view (models, g, first)), with per candidate its view, its draw, its
    cluster number, whether it is a tested cluster and the twin's verdict. The verdicts are cluster_lod_twin.h's — with a LOD scale
    of 0 and no eye they are cluster_twin_survives' alone."""

    def __init__(self, records, views, hizzes, tables, occupancy, lod_views=None, eyes=None):
        table, ranges, clusters = tables[:3]
        wide = tables if len(tables) == 5 else (table, ranges, clusters, np.zeros(len(clusters), CLUSTER_CONE_DTYPE), np.zeros(len(clusters), CLUSTER_LOD_DTYPE))
        per_view_blocks = -(-occupancy // TILE)
        view_of, draw, number, tested, frustum, base, survives, block = [], [], [], [], [], [], [], []
        self.start, self.draws, self.tested, self.commands = [0], [], [], []
        self.lod_kept = self.cone_seen = self.cone_rejected = 0   # clusters on the cut; of those, kept by the unchanged test; of those, cone-rejected
        for v, ((models, g, first), view) in enumerate(zip(records, views)):
            lod = lsup.lod_view(scale=0.0) if lod_views is None else lod_views[v]
            eye = None if eyes is None else eyes[v]
            commands, t, _, verdict, _ = lsup.view_commands(models, g, first, view["view_proj"], lod, eye, hizzes[v], tables=wide)
            per_draw = candidates_per_draw(g, table, ranges)
            is_cluster = np.repeat((g < len(ranges)) & (per_draw > 0) & (ranges["count"][np.minimum(g, len(ranges) - 1)] > 0), per_draw)
            k = np.repeat(np.arange(len(g)), per_draw)
            at = np.concatenate([[0], np.cumsum(per_draw)])
            j = np.arange(int(at[-1])) - at[k]
            s = np.ones(len(k), bool)
            f, b = s.copy(), s.copy()
            kept = (verdict & lsup.KEPT) != 0
            f[is_cluster] = (verdict & lsup.FRUSTUM) != 0
            b[is_cluster] = (verdict & lsup.BASE) != 0
            s[is_cluster] = kept & ((verdict & lsup.BASE) != 0) & ((verdict & lsup.CONE) == 0)
            self.lod_kept += int(kept.sum())
            self.cone_seen += int((kept & ((verdict & lsup.BASE) != 0)).sum())
            self.cone_rejected += int((kept & ((verdict & lsup.BASE) != 0) & ((verdict & lsup.CONE) != 0)).sum())
            assert int(is_cluster.sum()) == t == len(verdict) and int(s.sum()) == len(commands)
            view_of.append(np.full(len(k), v)), draw.append(k), number.append(j), tested.append(is_cluster)
            frustum.append(f), base.append(b), survives.append(s), block.append(v * per_view_blocks + k // TILE)
            self.start.append(self.start[-1] + len(k))
            self.draws.append(len(g)), self.tested.append(t), self.commands.append(len(commands))
        cat = np.concatenate
        self.view, self.draw, self.number, self.is_cluster = cat(view_of), cat(draw), cat(number), cat(tested)
        self.frustum, self.base, self.survives, self.block = cat(frustum), cat(base), cat(survives), cat(block)
        self.total, self.tiles, self.blocks = len(self.view), tiles_of(len(self.view)), per_view_blocks * len(views)
        self.g = [g for _, g, _ in records]
        self.ranges, self.clusters = ranges, clusters

    def widest_tile(self):
        """the largest number of different count workgroups among the candidates of one tile"""
        tile = np.arange(self.total) // TILE
        pairs = np.unique(tile.astype(np.int64) * self.blocks + self.block)
        return int(np.bincount(pairs // self.blocks).max())

    def emptied_blocks(self):
        """count workgroups with candidates directly followed by one with none"""
        has = np.bincount(self.block, minlength=self.blocks) > 0
        return int(np.count_nonzero(has[:-1] & ~has[1:]))

    def pending(self, queried):
        """the pending candidates of a second phase behind this call: tested, not kept, in a view that queried"""
        return self.is_cluster & ~self.survives & np.asarray(queried, bool)[self.view]

    def widest_pending_tile(self, queried):
        """(P, the largest number of candidate tiles between the first and the last pending of one pending tile)"""
        at = np.nonzero(self.pending(queried))[0]
        if not len(at):
            return 0, 0
        tile = at // TILE
        first, last = tile[::TILE], tile[np.minimum(np.arange(0, len(at), TILE) + TILE - 1, len(at) - 1)]
        return len(at), int((last - first + 1).max())

    def heads(self):
        """(head bits, run ends) of the run form: a survivor is a head iff it is not linked or its predecessor did not survive"""
        linked = np.zeros(self.total, bool)
        c = np.nonzero(self.is_cluster & (self.number > 0) & (self.number % SPAN != 0))[0]
        views = self.view[c]
        index = np.zeros(len(c), np.int64)
        for v, g in enumerate(self.g):
            mine = views == v
            index[mine] = self.ranges["first"][g[self.draw[c[mine]]]].astype(np.int64) + self.number[c[mine]]
        first, count = self.clusters["first"].astype(np.int64), self.clusters["count"].astype(np.int64)
        linked[c] = (first[index - 1] + count[index - 1] == first[index]) & (first[index] + count[index] <= 0xFFFFFFFF)
        before = np.concatenate([[False], self.survives[:-1]])
        head = self.survives & ~(linked & before)
        member = self.survives & ~head            # a candidate that continues a run
        ends = np.nonzero(self.survives & ~np.concatenate([member[1:], [False]]))[0]   # the last candidate of every run
        return head, ends
