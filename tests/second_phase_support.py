"""Test helpers of gv_pool_cull_second_phase: the case table of tests/test_gpu_second_phase.py and the expected values, which are exact
and come from the oracle unchanged — oracle.prepare_meshes(..., view, hiz=Hiz(A)) gives S1 (what phase 1 drew against the old pyramid),
the same call with Hiz(B) gives R (what a cull against the new pyramid delivers); the second view holds the records of R whose slot
is not in S1. The condition that keeps a case from passing by accident (check_condition) is asserted by the CPU tier
(tests/test_second_phase_abi.py) for every case of the table and again by the GPU tier on the case it runs.
TEST INFRASTRUCTURE ONLY."""
import collections
import functools

import numpy as np

from garden_amd import scene
from hiz_paths_support import header_constant

SEED = scene.SEED
SIZES = ((512, 256), (135, 77))  # an even pyramid, and the odd, non-nested one
MIN_SHARE = 0.02                 # of the view's frustum survivors, for each of new / gone / both

# the sizes at which phase 1 changes its launch form; test_second_phase_abi.py compares them with garden_amd/csrc/gv_kernels.hpp
EMIT_CHUNK = 4096         # kEmitChunk
FUSED_EMIT_MAX = 32768    # kFusedEmitMaxSlots: up to here phase 1 is the one-launch cull + emit, which keeps no ballot words
HOT_MIN = 65536           # kHotMinSlots: above it phase 1 culls from the sphere stream
AUTO_BOUNDS_MIN = 262144  # kAutoBoundsMinSlots: above it phase 1 goes through block bounds
HEADER_NAMES = {"kEmitChunk": EMIT_CHUNK, "kFusedEmitMaxSlots": FUSED_EMIT_MAX, "kHotMinSlots": HOT_MIN,
                "kAutoBoundsMinSlots": AUTO_BOUNDS_MIN, "kCullBlock": 256}

# kind: flat | hierarchy | shuffled; (w, h): the depth images' size; keep_slot_order / rg16f: the context's configuration;
# scene_seed / depth_seed: added to SEED (+ n for the scene) — what to change if a case misses the condition, never the threshold
Case = collections.namedtuple("Case", "name kind n w h keep_slot_order rg16f scene_seed depth_seed empty")


def _case(name, kind, n, size=SIZES[0], keep_slot_order=False, rg16f=False, scene_seed=0, depth_seed=0, empty=False):
    return Case(name, kind, n, size[0], size[1], keep_slot_order, rg16f, scene_seed, depth_seed, empty)


FLAT_COUNTS = (1, 64, 257, EMIT_CHUNK + 1, 40000, 100003, 270000)
CASES = [_case(f"flat-{n}", "flat", n, empty=(n == 1)) for n in FLAT_COUNTS] + [
    _case(f"flat-{n}-135x77", "flat", n, SIZES[1]) for n in (257, EMIT_CHUNK + 1, 40000)] + [
    _case("hierarchy-50000", "hierarchy", 50000),
    _case("shuffled-4097", "shuffled", EMIT_CHUNK + 1),
    _case("keep-slot-order-4097", "flat", EMIT_CHUNK + 1, keep_slot_order=True),
    _case("rg16f-4097", "flat", EMIT_CHUNK + 1, rg16f=True),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def header_constants():
    return {name: header_constant("gv_kernels.hpp", name) for name in HEADER_NAMES}


def world(c):
    """a fresh copy of the case's pools (the oracle and a write-back both write isVisible in place)"""
    seed = SEED + c.n + c.scene_seed
    if c.kind == "hierarchy":
        return scene.hierarchy_scene(c.n, depth=4, seed=seed)
    sc = scene.flat_scene(c.n, seed=seed)
    return scene.shuffled_scene(sc, seed=seed) if c.kind == "shuffled" else sc


def view(shadow_pass=-1):
    v = scene.main_camera_view(use_hiz=1)
    v["shadow_pass"] = int(shadow_pass)
    return v


def depth_images(c):
    return (scene.synthetic_depth(c.w, c.h, seed=SEED + c.depth_seed), scene.synthetic_depth(c.w, c.h, seed=SEED + c.depth_seed + 1))


def oracle_cull(sc, v, depth=None, rg16f=False):
    """the oracle's records of one cull, ascending slots; the pools are left as they were (the oracle writes isVisible in place)"""
    from oracle import oracle_py
    hiz = None if depth is None else oracle_py.Hiz(depth, rg16f=rg16f)
    return oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, v, hiz=hiz)


def second_of(first, full, n):
    """what the second view holds: the records of `full` (R) whose slot is not in `first` (S1), and the union bytes"""
    s1 = np.asarray(first["visible_idx"], np.uint32)
    keep = ~np.isin(full["visible_idx"], s1)
    union = np.zeros(n, np.uint8)
    union[s1] = 1
    union[full["visible_idx"][keep]] = 1
    return dict(visible_idx=full["visible_idx"][keep], baked_model=full["baked_model"][keep], distance_sq=full["distance_sq"][keep],
                draw_count=int(keep.sum()), is_visible=union)


Expected = collections.namedtuple("Expected", "frustum first full second new gone both")


def expected_of(sc, v, depth_a, depth_b, rg16f=False, first=None):
    """first: S1 from somewhere else (the pools as they were before an edit); default: the oracle on `sc` with A"""
    n = sc.count
    frustum = int(oracle_cull(sc, v)["draw_count"]) if first is None else 0
    first = oracle_cull(sc, v, depth_a, rg16f) if first is None else first
    full = oracle_cull(sc, v, depth_b, rg16f)
    s1, r = set(first["visible_idx"].tolist()), set(full["visible_idx"].tolist())
    return Expected(frustum, first, full, second_of(first, full, n), len(r - s1), len(s1 - r), len(s1 & r))


@functools.lru_cache(maxsize=None)
def expected(name):
    """computed once per case and shared by every test that needs it; treat as read-only"""
    c = CASE_BY_NAME[name]
    a, b = depth_images(c)
    return expected_of(world(c), view(), a, b, c.rg16f)


def check_condition(c, e):
    """each of R \\ S1 (new), S1 \\ R (must NOT reappear) and S1 & R (must not be duplicated) holds at least one slot and at least
    2 % of the view's frustum survivors; n = 1 sees nothing and is the declared empty case"""
    if c.empty:
        assert (e.frustum, e.new, e.gone, e.both) == (0, 0, 0, 0), (c.name, e.frustum, e.new, e.gone, e.both)
        return
    for what, count in (("new", e.new), ("gone", e.gone), ("both", e.both)):
        assert count >= 1 and count >= MIN_SHARE * e.frustum, (c.name, what, count, e.frustum)


def same_records(got, exp):
    """a fetch in ascending slot order against expected records: slots, and models and distances as bit patterns"""
    n = int(exp["draw_count"])
    assert int(got["draw_count"]) == n
    if n == 0:
        return
    assert got["visible_idx"][:n].tolist() == np.asarray(exp["visible_idx"]).tolist()
    assert np.ascontiguousarray(got["baked_model"][:n]).view(np.uint32).tobytes() == \
        np.ascontiguousarray(exp["baked_model"]).view(np.uint32).tobytes()
    assert np.ascontiguousarray(got["distance_sq"][:n]).view(np.uint32).tobytes() == \
        np.ascontiguousarray(exp["distance_sq"]).view(np.uint32).tobytes()
