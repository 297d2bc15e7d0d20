"""Test helpers of gv_pool_group_draws: the case table of tests/test_gpu_group_draws.py, the keys of DESIGN.md §4 item 12 restated
with numpy (kappa = min(g, K); with GV_GROUP_BY_LOD g comes from the C twin of the LOD rule, tests/lod_twin.h, through lod_support),
the conditions that keep a case from passing by accident, and the flat world of tests/test_gpu_lod_select.py re-stated. The CPU tier
(tests/test_group_abi.py) checks the table against the kernel header's constants and every case's restatement against the
conditions; the GPU tier asserts the same conditions again on the order the device really delivered. TEST INFRASTRUCTURE ONLY."""
import collections

import numpy as np

import lod_support as lsup
from hiz_paths_support import header_constant

# the constants the counts below are built around; test_group_abi.py compares them with garden_amd/csrc/gv_group_kernels.hpp
BLOCK = 256
TILE = 2048
GROUP_TILES = 32
HEADER = "gv_group_kernels.hpp"
HEADER_NAMES = {"kGroupBlock": BLOCK, "kGroupTileKeys": TILE, "kGroupGroupTiles": GROUP_TILES, "kGroupMaxDigits": 3}
BATCH_SORT_MAX = 16384       # kBatchSortMaxSlots: up to here a gv_pool_sort is deferred into the frame's one-launch batch
PUBLISH_MAX = 262144         # kPublishMaxSlots: above it the engine-sized publish no longer delivers the view
SORT_AT_ONCE = (1 << 20) + 3  # above kMidSortMaxSlots gv_pool_sort launches at once
SPECIAL_IDS = (0, 255, 256, 65535, 65536, 0xFFFFFFFF)  # planted on three slots each where the column's width holds them


def header_constants():
    return {name: header_constant(HEADER, name) for name in HEADER_NAMES}


def digits(table_count):
    """8-bit digits of the VALUE K: what fixes the launches of a call (2 per digit)"""
    return 1 if table_count <= 255 else 2 if table_count <= 65535 else 3


# n: entities (all visible); K: geometry table entries; width: bytes of an id (None: no id column); spread: ids are drawn from
# [0, spread); by_lod: GV_GROUP_BY_LOD with the LOD world (4 levels, 7 bases; K = 28); presort: gv_pool_sort in front of the call
Case = collections.namedtuple("Case", "name n K width spread by_lod presort")


def _count_case(n, presort=False):
    if n < BATCH_SORT_MAX:  # one digit: 12 (below a tile) or 48 geometries of a table of 200, so that every key has several members
        return Case(f"count-{n}" + ("-sorted" if presort else ""), n, 200, 4, 12 if n < TILE - 1 else 48, False, presort)
    return Case(f"count-{n}" + ("-sorted" if presort else ""), n, 4096, 2, 4200, False, presort)  # two digits, some void ids


COUNTS = (1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, BATCH_SORT_MAX, BATCH_SORT_MAX + 1, 40000, 300000)
CASES = [_count_case(n) for n in COUNTS] + [
    _count_case(BATCH_SORT_MAX, presort=True),       # a deferred sort is pending when the call is issued
    _count_case(BATCH_SORT_MAX + 1, presort=True),
    _count_case(SORT_AT_ONCE, presort=True),         # the sort was launched at once; 513 tiles in 17 groups
    # key widths at 5000 draws (three tiles): ids beyond K are void and share the last bucket
    Case("K-1", 5000, 1, 4, 3, False, False),
    Case("K-200-u8", 5000, 200, 1, 256, False, False),
    Case("K-256", 5000, 256, 4, 300, False, False),
    Case("K-257-u16", 5000, 257, 2, 300, False, False),
    Case("K-65535-u16", 5000, 65535, 2, 65536, False, False),
    Case("K-65535", 5000, 65535, 4, 70000, False, False),
    Case("K-65536", 5000, 65536, 4, 70000, False, False),
    Case("K-65536-few", 5000, 65536, 4, 40, False, False),   # three digits, two of them constant
    Case("no-ids-lod", 5000, 28, None, 0, True, False),     # b = 0 everywhere: the keys are the levels of geometry 0
    Case("lod", 5000, 28, 4, 0, True, False),
    Case("lod-sorted", 5000, 28, 4, 0, True, True),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def case_ids(c):
    """the id column of a case (per POOL slot), or None; the LOD cases take their ids from LodWorld"""
    if c.width is None or c.by_lod:
        return None
    dtype = {1: np.uint8, 2: np.uint16, 4: np.uint32}[c.width]
    rng = np.random.Generator(np.random.PCG64(7919 * c.K + c.n))
    ids = rng.integers(0, c.spread, c.n).astype(dtype)
    if c.n >= 256:
        at = rng.permutation(c.n)
        fit = [s for s in SPECIAL_IDS if s <= np.iinfo(dtype).max]
        for k, special in enumerate(fit):
            ids[at[3 * k:3 * k + 3]] = special
    return ids


def geometry_table(count, seed=11):
    """`count` rows of (count, first, vertex_offset), vectorised (65 536 rows in the widest case)"""
    rng = np.random.Generator(np.random.PCG64(seed + count))
    table = np.zeros(count, np.dtype([("count", np.uint32), ("first", np.uint32), ("vertex_offset", np.int32)]))
    table["count"] = rng.integers(1, 1 << 20, count)
    table["first"] = rng.integers(0, 1 << 30, count)
    table["vertex_offset"] = rng.integers(-(1 << 20), 1 << 20, count)
    return table


class LodWorld:
    """the World of tests/test_gpu_lod_select.py: `bases` geometries of `levels` levels each, base ids at stride `levels`, sizes
    in [0.5, 4), the thresholds the positions' own quantiles of distance / size"""

    def __init__(self, positions, levels=4, bases=7, seed=0):
        n = len(positions)
        self.levels, self.bases = levels, bases
        rng = np.random.Generator(np.random.PCG64(1000 * levels + n + seed))
        self.ids = (rng.integers(0, bases, n) * levels).astype(np.uint32)
        self.sizes = rng.uniform(0.5, 4.0, n).astype(np.float32)
        self.switch_at = lsup.quantile_thresholds(positions, self.sizes, levels)
        self.lod = lsup.lod_table([(levels, self.switch_at) if g % levels == 0 else (1, []) for g in range(bases * levels)])
        self.table = geometry_table(bases * levels)


def keys(visible_idx, ids, table_count, lod=None):
    """kappa of every record in delivery order. ids: per POOL slot or None. lod: None, or (twin, baked_model [n, 12], sizes per
    slot or None, scale, lod table)."""
    slots = np.asarray(visible_idx).astype(np.int64)
    base = np.zeros(len(slots), np.uint32) if ids is None else np.asarray(ids)[slots].astype(np.uint32)
    if lod is None:
        g = base
    else:
        twin, models, sizes, scale, table = lod
        size = np.ones(len(slots), np.float32) if sizes is None else np.asarray(sizes, np.float32)[slots]
        g, _ = lsup.twin_many(twin, np.asarray(models, np.float32).reshape(-1, 12)[:len(slots)], base, size, scale, table)
    return np.minimum(g.astype(np.uint64), table_count).astype(np.uint32)


def order_of(kappa):
    """pi: record j after the call is the old record pi(j)"""
    return np.argsort(kappa, kind="stable")


def check_conditions(kappa, visible_idx, identity_allowed=False):
    """what keeps a case from passing by accident (the issue's list), on kappa in delivery order"""
    n = len(kappa)
    if n >= 256:
        assert (np.diff(kappa.astype(np.int64)) < 0).any(), "the pre-call order is already grouped"
        present, members = np.unique(kappa, return_counts=True)
        if len(present) <= 64:
            assert (members >= 2).all(), "a key with a single member: an unstable scatter could pass"
    if n > 2 and not identity_allowed:  # (one record has no other order, and which of two comes first is the mirror's choice)
        assert order_of(kappa).tolist() != list(range(n)), "the expected permutation is the identity"
    if n > 2 and visible_idx is not None:
        assert np.asarray(visible_idx).tolist() != list(range(n)), "visible_idx is the identity"


def stand_in_order(n, seed=5):
    """The CPU tier has no device: a seeded permutation stands in for the mirror's Morton order, which like it does not depend on
    the ids. (The GPU tier repeats check_conditions on the order the device delivered.)"""
    return np.random.Generator(np.random.PCG64(seed + n)).permutation(n).astype(np.uint32)


def expected_results(before, order):
    """the three record arrays after the call, from the fetch in front of it"""
    return dict(visible_idx=before["visible_idx"][order], baked_model=before["baked_model"][order],
                distance_sq=before["distance_sq"][order])


def same_records(got, exp, n):
    """all three arrays; the floats as bit patterns"""
    assert int(got["draw_count"]) == n
    if n == 0:
        return
    assert got["visible_idx"][:n].tolist() == exp["visible_idx"].tolist()
    assert np.ascontiguousarray(got["baked_model"][:n]).view(np.uint32).tobytes() == \
        np.ascontiguousarray(exp["baked_model"]).view(np.uint32).tobytes()
    assert np.ascontiguousarray(got["distance_sq"][:n]).view(np.uint32).tobytes() == \
        np.ascontiguousarray(exp["distance_sq"]).view(np.uint32).tobytes()

