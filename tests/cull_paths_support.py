"""Test helpers of the cull dispatch: which launches one gv_cull takes (gv_cull, plan_cull, cull_launch and flush_culls in
garden_amd/csrc/gv_context.cpp; launch_cull, launch_cull_listed, launch_cull_multi and launch_emit* in gv_cull.hip), restated in
plain Python (cull_plan over a PoolModel), and the table of GPU cases (CASES) that tests/test_cull_plan_census.py proves to
cover every reachable cell and tests/test_gpu_cull_paths.py runs against the oracle. TEST INFRASTRUCTURE ONLY.

A CELL is (cull form, HIZ, MAP, emit form): the template instantiation that culls a view and the launch that writes its records.
The plan depends on sizes, the mapping, the views' flags, the context flags and on what is current of the pool's derived state
(sphere stream, block bounds, emit seeds); never on the entities themselves."""
import collections
import functools
import math
import re

import numpy as np

from garden_amd import scene
from hiz_paths_support import header_constant, source_text

K = "gv_kernels.hpp"
CULL_BLOCK = header_constant(K, "kCullBlock")
FUSED_EMIT_MAX = header_constant(K, "kFusedEmitMaxSlots")
HOT_MIN = header_constant(K, "kHotMinSlots")
AUTO_BOUNDS_MIN = header_constant(K, "kAutoBoundsMinSlots")
EMIT_SEED_MIN = header_constant(K, "kEmitSeedMinSlots")
EMIT_CHUNK = header_constant(K, "kEmitChunk")
SELF_PREFIX_MAX_CHUNKS = header_constant(K, "kSelfPrefixMaxChunks")
MAX_BATCH_VIEWS = header_constant(K, "kMaxBatchViews")
TABLE_MAX_SLOTS = header_constant("gv_sort_kernels.hpp", "kSmallSortMaxSlots")
MIN_SMALL_STREAK = header_constant("gv_context.cpp", "kMinSmallStreak")


def _hot_tile_steps():
    """(tiles from which K = 4, tiles from which K = 2) of hot_tiles_per_workgroup, read from its text"""
    m = re.search(r"return tiles >= (\d+)u \? 4u : \(tiles >= (\d+)u \? 2u : 1u\);", source_text(K))
    assert m, "hot_tiles_per_workgroup no longer reads as restated"
    return int(m.group(1)), int(m.group(2))


HOT_K4_TILES, HOT_K2_TILES = _hot_tile_steps()

# Lines of the dispatch that the restatement below follows (test_cull_plan_census.py checks that the library still holds them).
LITERAL_LINES = {
    "gv_context.cpp": [
        "const bool exact = p.mapping == kMapExact, flat = xf.max_depth == 0, paired = exact && p.occupancy <= xf.count;",
        "plan.batched = batched && p.occupancy != 0;",
        "plan.self_prefix = (p.occupancy + kEmitChunk - 1) / kEmitChunk <= kSelfPrefixMaxChunks;",
        "plan.emit_batched = plan.batched && plan.self_prefix && all_emit;",
        "plan.fused = ctx->sweep_with_cull && !plan.batched && p.occupancy != 0 && paired;",
        "plan.patchable = paired && flat;",
        "((ctx->config.flags & GV_CONFIG_BLOCK_BOUNDS) || (!(ctx->config.flags & GV_CONFIG_LINEAR_SCAN) && p.occupancy > kAutoBoundsMinSlots));",
        "plan.hot_wanted = !plan.batched && !plan.fused && !plan.bounds_wanted && p.occupancy > kHotMinSlots && exact && flat;",
        "plan.seeds_wanted = emits != 0 && !plan.batched && p.occupancy >= kEmitSeedMinSlots && plan.patchable;",
        "plan.cull_emit = !plan.batched && !plan.fused && view_count == 1 && all_emit && p.occupancy != 0 && p.occupancy <= kFusedEmitMaxSlots;",
        "const bool may_rebuild = !(changed && p.changed_prev) || (patchable && changed && p.small_streak >= kMinSmallStreak);",
        "if (!current && p.hot_patch_valid && p.d_hot.cap >= p.occupancy && p.d_blk_dirty.ptr) {",
        "if (!current && p.patch_valid && patchable && p.d_blk_lo.ptr && p.d_blk_dirty.ptr) {",
        "const bool seeds_in_step = p.d_seed.ptr && p.d_seed.cap >= p.occupancy && p.seed_at == p.bounds_at;",
        "const float4* emit_world = (ctx->world_valid && !ctx->world_partial && ctx->max_depth != 0) ? ctx->d_world.ptr : nullptr;",
        "const bool one_launch = plan.cull_emit && !use_bounds;",
        "bool batched = view_count > 1 && view_count <= kMaxBatchViews && p.occupancy > 0;",
        "batched = memcmp(views[v].camera_position, views[0].camera_position, 12) == 0 && !views[v].use_hiz;",
        "bool eligible = p.occupancy != 0 && p.occupancy <= kSmallSortMaxSlots && !ctx->sweep_with_cull &&",
        "!(ctx->config.flags & GV_CONFIG_BLOCK_BOUNDS) && (view_count == 1 || batched) &&",
        "if (jobs.size() == 1) {  // nothing to batch: the ordinary launches (cull + emit in one for a single view) are shorter",
    ],
    "gv_cull.hip": [
        "const bool window_test = vp.use_hiz && hiz.nested;",
        "const uint32_t k = mesh.hot && mesh.mapping == kMapExact ? hot_tiles_per_workgroup(a.nblocks) : 1u;",
        "hipLaunchKernelGGL((cull_kernel<hiz, kMapExact, true>), grid, block, 0, stream, a);",
        "hipLaunchKernelGGL((cull_multi_kernel<hiz, map, true>), grid, block, 0, stream, a);",
        "if (use_seed) {",
        "} else if (args.world) {  // uniform",
    ],
    "gv_mirror.cpp": [
        "const bool dense = most_of_pool(total, n);",
        "const bool few = !dense && !ctx->xf_links_dirty && few_enough_to_patch_blocks(total, blocks_of(q.occupancy));",
        "if (!few || ctx->max_depth != 0 || q.mapping != kMapExact || !q.d_blk_dirty.ptr) {",
        "p.mapping = mesh_mapping_of(own, candidates);",
    ],
    "gv_dirty_ranges.hpp": [  # the rules themselves (tabulated by tests/cpp/dirty_ranges_test.cpp)
        "inline bool most_of_pool(uint64_t total, uint32_t occupancy) { return total * 2 > occupancy; }",
        "inline bool few_enough_to_patch_blocks(uint64_t total, uint64_t nblocks) { return total * 16 <= nblocks + 16 * 64; }",
        "return own == candidates ? kPairedExact : (own * 10 >= candidates * 9 ? kPairedSpeculate : kPairedGeneral);",
    ],
}

CULL_FORMS = ("plain", "plain_hot", "hot_k2", "hot_k4", "listed", "listed_window", "one_launch", "multi", "multi_bounds", "fused_mfma",
              "fused_valu", "table")
EMIT_FORMS = ("none_scan", "self", "self_seeds", "self_world", "scan_emit", "batch", "batch_world", "table", "in_cull")
MAPS = ("general", "speculate", "exact")
UPKEEP = ("sweep_mfma", "sweep_valu", "hot_build", "hot_patch", "block_bounds", "block_patch", "block_patch_seeds", "emit_seeds")

# the context flags of the four fixtures of tests/conftest.py
Flags = collections.namedtuple("Flags", "block_bounds linear_scan slot_order")
FIXTURE_FLAGS = {"gpu": Flags(False, False, False), "gpu_slot_order": Flags(False, False, True),
                 "gpu_bounds": Flags(True, False, False), "gpu_linear": Flags(False, True, False)}

# emit: records wanted; hiz: use_hiz; shared: same camera position as view 0 (view 0 itself: True)
View = collections.namedtuple("View", "emit hiz shared")
View.__new__.__defaults__ = (True, False, True)

Plan = collections.namedtuple("Plan", "cull_form HIZ MAP cull_forms hiz emit_forms upkeep launches bounds_blocks cells")


def blocks_of(n):
    return (n + CULL_BLOCK - 1) // CULL_BLOCK


def chunks_of(n):
    return (n + EMIT_CHUNK - 1) // EMIT_CHUNK


def hot_tiles(tiles):
    return 4 if tiles >= HOT_K4_TILES else (2 if tiles >= HOT_K2_TILES else 1)


class PoolModel:
    """What cull_launch keeps of one pool between culls (PoolState's stamps and recording flags) and of the context (the world
    cache, a pending sweep request). Stamps are counted as the library's: a change of the pool's mirror gives a new one."""

    def __init__(self):
        self.stamp = 1
        self.seen_at = self.hot_at = self.bounds_at = self.seed_at = 0
        self.hot_patch_valid = self.patch_valid = False
        self.changed_prev = False
        self.small_streak = 0
        self.world = False

    def edit(self, occupancy, count, mapping="exact", max_depth=0):
        """`count` transforms re-mirrored by the sync in front of the next cull (gv_mirror.cpp: remirror_dirty_transforms, dense or
        itemised by most_of_pool; pools_that_keep_flagging with few_enough_to_patch_blocks — the rules of gv_dirty_ranges.hpp)"""
        dense = count * 2 > occupancy
        few = not dense and count * 16 <= blocks_of(occupancy) + 16 * 64
        self.small_streak = min(self.small_streak + 1, 1000) if few else 0
        if (self.patch_valid or self.hot_patch_valid) and (not few or max_depth != 0 or mapping != "exact"):
            self.patch_valid = self.hot_patch_valid = False
        self.world = False
        self.stamp += 1

    def rebind(self):
        """a full gather of the mirror (bind, gv_hierarchy_rebuild)"""
        self.patch_valid = self.hot_patch_valid = False
        self.world = False
        self.stamp += 1

    def sweep(self):
        """gv_sweep(VALU / MFMA) of the current mirror"""
        self.world = True


def is_batched(occupancy, views):
    return (1 < len(views) <= MAX_BATCH_VIEWS and occupancy > 0 and all(v.shared and not v.hiz for v in views[1:]))


def table_eligible(occupancy, views, flags, sweep=0):
    """gv_cull records the cull instead of launching it (inside gv_cull_batch_begin / _end)"""
    return (occupancy != 0 and occupancy <= TABLE_MAX_SLOTS and not sweep and not flags.block_bounds and
            (len(views) == 1 or is_batched(occupancy, views)) and all(v.emit for v in views))


def table_plan(jobs):
    """flush_culls over two or more recorded jobs [(occupancy, mapping, views)]: ONE cull launch and ONE emit launch for all"""
    assert len(jobs) >= 2
    cells = set()
    for occupancy, mapping, views in jobs:
        for _v in views:
            cells.add(("table", bool(views[0].hiz), mapping, "table"))
    return Plan("table", None, None, ("table",), None, ("table",), (), dict(cull=1, scan=0, emit=1, sweep=0), False, frozenset(cells))


def cull_plan(occupancy, transforms, mapping, max_depth, views, flags, sweep=0, state=None, changed=None, pyramid=True, nested=True):
    """The launches of ONE gv_cull of a pool that is not being recorded into a batch.
    occupancy / transforms: entries of the mesh pool and of the transform pool; mapping: one of MAPS; views: [View];
    flags: Flags; sweep: 0, or the pending GV_SWEEP_WITH_CULL (2) / GV_SWEEP_WITH_CULL_VALU (3); state: the PoolModel (updated);
    changed: the pool's mirror changed since the previous cull (default: state.stamp tells); pyramid / nested: gv_hiz_build has
    run / every level of it is nested. Returns a Plan, or None where gv_cull refuses (Hi-Z asked for without a pyramid)."""
    st = state if state is not None else PoolModel()
    if any(v.hiz for v in views) and not pyramid:
        return None
    n = len(views)
    exact, flat = mapping == "exact", max_depth == 0
    paired = exact and occupancy <= transforms
    emits = sum(v.emit for v in views)
    all_emit = emits == n
    batched = is_batched(occupancy, views)
    self_prefix = chunks_of(occupancy) <= SELF_PREFIX_MAX_CHUNKS
    emit_batched = batched and self_prefix and all_emit
    fused = bool(sweep) and not batched and occupancy != 0 and paired
    patchable = paired and flat
    bounds_wanted = occupancy != 0 and not fused and (flags.block_bounds or (not flags.linear_scan and occupancy > AUTO_BOUNDS_MIN))
    hot_wanted = not batched and not fused and not bounds_wanted and occupancy > HOT_MIN and exact and flat
    seeds_wanted = emits != 0 and not batched and occupancy >= EMIT_SEED_MIN and patchable
    cull_emit = not batched and not fused and n == 1 and all_emit and occupancy != 0 and occupancy <= FUSED_EMIT_MAX

    upkeep = []
    if sweep:
        if not fused:
            upkeep.append("sweep_mfma" if sweep == 2 else "sweep_valu")
        st.world = True
    now = st.stamp
    if changed is None:
        changed = st.seen_at != now
    may_rebuild = not (changed and st.changed_prev) or (patchable and changed and st.small_streak >= MIN_SMALL_STREAK)
    st.changed_prev = changed
    st.seen_at = now

    hot = use_bounds = seeds = False
    if hot_wanted:
        current = st.hot_at == now
        if not current and st.hot_patch_valid:
            upkeep.append("hot_patch")
            current = True
        if not current and may_rebuild:
            upkeep.append("hot_build")
            st.hot_patch_valid = True
            current = True
        if current:
            st.hot_at = now
            hot = True
    if bounds_wanted:
        current = st.bounds_at == now
        if not current and st.patch_valid and patchable:
            in_step = st.seed_at == st.bounds_at and st.seed_at != 0
            upkeep.append("block_patch_seeds" if in_step else "block_patch")
            if in_step:
                st.seed_at = now
            st.bounds_at = now
            current = True
        if not current and may_rebuild:
            upkeep.append("block_bounds")
            st.hot_patch_valid = False
            st.bounds_at = now
            st.patch_valid = patchable
            current = True
        use_bounds = current
    if seeds_wanted:
        if st.seed_at != now and may_rebuild:
            upkeep.append("emit_seeds")
            st.seed_at = now
        seeds = st.seed_at == now
    emit_world = st.world and max_depth != 0
    one_launch = cull_emit and not use_bounds

    launches = dict(cull=0, scan=0, emit=0, sweep=len(upkeep))
    cull_forms, emit_forms = [], []

    def emit_view(v):
        if v.emit and self_prefix:
            launches["emit"] += 1
            return "self_seeds" if seeds else ("self_world" if emit_world else "self")
        launches["scan"] += 1
        if v.emit:
            launches["emit"] += 1
            return "scan_emit"
        return "none_scan"

    if occupancy == 0:
        pass
    elif batched:
        launches["cull"] += 1
        cull_forms = ["multi_bounds" if use_bounds else "multi"] * n
        if emit_batched:
            launches["emit"] += 1
            emit_forms = ["batch_world" if emit_world else "batch"] * n
        else:
            emit_forms = [emit_view(v) for v in views]
    elif one_launch:
        launches["cull"] += 1
        cull_forms, emit_forms = ["one_launch"], ["in_cull"]
    else:
        for i, v in enumerate(views):
            launches["cull"] += 1
            if fused and i == 0:
                cull_forms.append("fused_mfma" if sweep == 2 else "fused_valu")
            elif use_bounds:
                cull_forms.append("listed_window" if v.hiz and nested else "listed")
            elif hot:
                cull_forms.append({4: "hot_k4", 2: "hot_k2", 1: "plain_hot"}[hot_tiles(blocks_of(occupancy))])
            else:
                cull_forms.append("plain")
            emit_forms.append(emit_view(v))
    # the kernel's HIZ: the view's own flag; the batched forms take view 0's for all; its MAP: the pool's mapping, except that
    # the sphere-stream and the fused forms exist for exactly paired pools only
    hiz = [bool(views[0].hiz if batched else v.hiz) for v in views] if occupancy else []
    cells = frozenset((c, h, mapping, e) for c, h, e in zip(cull_forms, hiz, emit_forms))
    return Plan(cull_forms[0] if cull_forms else None, hiz[0] if hiz else None, mapping, tuple(cull_forms), tuple(hiz), tuple(emit_forms),
                tuple(upkeep), launches, use_bounds, cells)


# ---------------------------------------------------------------------------------------------------------------------------
# The GPU cases. A case binds ONE scene to one of the four contexts and runs a PROGRAM: a list of steps, each a cull (its views
# as a string of view codes, an optional sweep request in front) or a change of the pool. Every cull's launch counts are
# compared with cull_plan's and every view's outputs with the oracle's.
#   view codes: E emit, C count-only; h = Hi-Z; s = shadow pass (a cascade) at the main camera's position; x = a camera of its own
#   ("Eh,Es" = an occlusion view and a cascade sharing its camera: batched; "E,Ex" = two separate views)
# ---------------------------------------------------------------------------------------------------------------------------
Step = collections.namedtuple("Step", "kind views sweep")
EDIT_SLOTS = 64  # "few": 64 * 16 <= blocks + 1024 for every pool size


def cull(views, sweep=0):
    return Step("cull", views, sweep)


FEW, DENSE, SWEEP = Step("few", None, 0), Step("dense", None, 0), Step("sweep", None, 0)
NON_NESTED = (250, 130)  # 125 x 65 at level 1: odd, so the pyramid is not nested and the listed cull goes without its window test
REBUILD_NOT_NESTED = Step("hiz", NON_NESTED, 0)  # gv_hiz_build of another image: every Hi-Z cull from here on queries that one

# programs, by name. Every one starts from a pool whose mirror has just changed after a quiet cull (the GPU test brings that
# about: two culls, then every transform marked dirty), so the first cull builds what it wants of the derived state.
_SINGLE = [cull("E"), cull("C"), cull("Eh"), cull("Ch"), FEW, cull("E"), FEW, cull("Ch"), cull("Eh"), REBUILD_NOT_NESTED, cull("Eh"), cull("Ch")]
_SHARED = [cull("E,Es"), cull("Eh,Es,Es,Es"), cull("C,Cs"), cull("Ch,Cs"), cull("E,Cs"), cull("Eh,Cs,Es,Cs"), FEW, cull("E,Es"), cull("Eh,Cs")]
_SEPARATE = [cull("E,Ex"), cull("Eh,Cx"), cull("C,Exh"), cull("Ch,Ex,Exh,Cx")]
_WORLD = [SWEEP, cull("E"), cull("Eh"), cull("E,Es"), cull("Eh,Es"), cull("E,Cs"), cull("Eh,Cs"), cull("E,Ex"), cull("Eh,Exh"),
          DENSE, cull("E", sweep=2), cull("Eh,Cs", sweep=3), DENSE, cull("Eh", sweep=3), cull("C,Ex", sweep=2), REBUILD_NOT_NESTED, cull("Eh")]
_FUSED = [cull("E", sweep=2), cull("Eh", sweep=3), cull("C", sweep=3), cull("Ch", sweep=2), cull("C", sweep=2), cull("Ch", sweep=3), cull("E,Ex", sweep=3), cull("Eh,Exh", sweep=2),
          cull("E,Es", sweep=2), FEW, cull("Eh", sweep=2), cull("E")]
_CHURN = [DENSE, cull("E"), DENSE, cull("Eh"), DENSE, cull("C"), DENSE, cull("Ch"), DENSE, cull("E,Ex"), DENSE, cull("Eh,Es")]
_STREAK = [FEW, cull("E"), FEW, cull("Eh"), FEW, cull("E"), FEW, cull("Eh"), FEW, cull("E"), FEW, cull("Ch")]
PROGRAMS = {
    "single": _SINGLE,
    "shared": _SHARED,
    "separate": _SEPARATE,
    "all": _SINGLE + _SHARED + _SEPARATE,
    "world": _WORLD,
    "fused": _FUSED,
    "churn": _CHURN,
    "streak": _STREAK,
    "large": _SINGLE + _SHARED + _SEPARATE + _FUSED + _CHURN[:8],
}

Case = collections.namedtuple("Case", "name fixture kind n transforms MAP depth hiz program exact_threshold")


def case(name, fixture, kind, n, program, transforms=None, hiz=(256, 256), exact_threshold=False):
    MAP = {"flat": "exact", "hier": "exact", "spec": "speculate", "gen": "general", "hier_spec": "speculate", "hier_gen": "general"}[kind]
    depth = 3 if kind.startswith("hier") else 0
    return Case(name, fixture, kind, n, transforms or n, MAP, depth, hiz, program, exact_threshold)


# Sizes: the smallest at which each form exists, never a multiple of 64 (the last wave is partial) and, above one chunk, never
# of 4096 (the last emit chunk is partial) — except the cases named for a threshold, which sit exactly on it for the comparison.
# Non-exact mappings come from shuffled pools and are bound to the slot-order context only: there the mirror is the pools' own
# order and the mapping follows from them (mirror_mapping); a spatially ordered mirror re-pairs a shuffled pool in ways that
# cannot be told from outside. Flat and hierarchy scenes pair slot for slot and are exact in every context.
CASES = [
    # ---- one launch / plain, small pools ----
    case("one-launch-exact-333", "gpu", "flat", 333, "all"),
    case("one-launch-at-32768", "gpu_linear", "flat", FUSED_EMIT_MAX, "single", exact_threshold=True),
    case("plain-exact-32769", "gpu", "flat", FUSED_EMIT_MAX + 1, "all"),
    case("one-launch-speculate-4097", "gpu_slot_order", "spec", 4097, "all"),
    case("one-launch-general-4099", "gpu_slot_order", "gen", 4099, "all"),
    case("plain-speculate-33001", "gpu_slot_order", "spec", 33_001, "all"),
    case("plain-general-33003", "gpu_slot_order", "gen", 33_003, "all"),
    case("plain-at-65536", "gpu_linear", "flat", HOT_MIN, "single", exact_threshold=True),
    # ---- the sphere stream (K = 1), its patch, a pool that keeps changing ----
    case("hot-65537", "gpu_linear", "flat", HOT_MIN + 1, "all"),
    case("hot-churn-70001", "gpu", "flat", 70_001, "churn"),
    case("hot-streak-70003", "gpu", "flat", 70_003, "streak"),
    # ---- hierarchies: records from the world cache, the sweep riding on the cull ----
    case("world-exact-5003", "gpu", "hier", 5003, "world"),
    case("world-exact-40001", "gpu", "hier", 40_001, "world"),
    case("world-speculate-5005", "gpu_slot_order", "hier_spec", 5005, "world"),
    case("world-general-5007", "gpu_slot_order", "hier_gen", 5007, "world"),
    case("world-speculate-40003", "gpu_slot_order", "hier_spec", 40_003, "world"),
    case("world-general-40005", "gpu_slot_order", "hier_gen", 40_005, "world"),
    case("hier-plain-exact-40007", "gpu_slot_order", "hier", 40_007, "all"),
    case("hier-plain-general-40009", "gpu_slot_order", "hier_gen", 40_009, "all"),
    case("hier-plain-speculate-40011", "gpu_slot_order", "hier_spec", 40_011, "all"),
    # ---- fused sweep + cull; a mesh pool smaller than its transform pool (the workgroups past the mesh range only sweep) ----
    case("fused-flat-9001", "gpu_slot_order", "flat", 9001, "fused"),
    case("fused-mesh-smaller-3001-of-9001", "gpu_slot_order", "flat", 3001, "fused", transforms=9001),
    case("fused-hier-mesh-smaller-5001-of-9003", "gpu_slot_order", "hier", 5001, "fused", transforms=9003),
    case("fused-flat-70005", "gpu_linear", "flat", 70_005, "fused"),
    # ---- block bounds by flag: the listed cull, with and without the window test, batched views behind boxes ----
    case("listed-exact-5009", "gpu_bounds", "flat", 5009, "all"),
    case("listed-exact-70007-not-nested", "gpu_bounds", "flat", 70_007, "all", hiz=NON_NESTED),
    case("listed-hier-40013", "gpu_bounds", "hier", 40_013, "world"),
    case("listed-churn-5011", "gpu_bounds", "flat", 5011, "churn"),
    case("listed-streak-5013", "gpu_bounds", "flat", 5013, "streak"),
    # ---- block bounds by size, seeds ----
    case("auto-bounds-at-262144", "gpu", "flat", AUTO_BOUNDS_MIN, "single", exact_threshold=True),
    case("auto-bounds-262145", "gpu", "flat", AUTO_BOUNDS_MIN + 1, "large"),
    case("seeds-linear-at-262144", "gpu_linear", "flat", EMIT_SEED_MIN, "large", exact_threshold=True),
    case("seeds-linear-262143", "gpu_linear", "flat", EMIT_SEED_MIN - 1, "single"),
    case("listed-speculate-262147", "gpu_slot_order", "spec", 262_147, "all"),
    case("listed-general-262149", "gpu_slot_order", "gen", 262_149, "all"),
    case("listed-speculate-262151-not-nested", "gpu_slot_order", "spec", 262_151, "single", hiz=NON_NESTED),
    case("listed-hier-speculate-262153", "gpu_slot_order", "hier_spec", 262_153, "world"),
    case("listed-hier-general-262155", "gpu_slot_order", "hier_gen", 262_155, "world"),
    case("listed-hier-exact-300001", "gpu", "hier", 300_001, "world"),
]

# The table form: several recorded pools of one context in one gv_cull_batch_begin / _end. Pools of a table case share the
# transform pool of a flat scene of `n` entries: (pool id, mapping, entries, views of the first batch, of the second batch)
TableCase = collections.namedtuple("TableCase", "name fixture n hiz pools")
TABLE_CASES = [
    TableCase("table-three-mappings", "gpu_slot_order", 20_001, (256, 256),
              [(0, "exact", 333, "E", "Eh"), (1, "general", 20_001, "E,Es", "Eh,Es"), (2, "speculate", 9001, "Eh,Es,Es", "E")]),
]


def parse_views(code):
    """"Eh,Cs,Ex" -> [View]"""
    out = []
    for i, c in enumerate(code.split(",")):
        assert c[0] in "EC" and set(c[1:]) <= set("hsx") and not (i == 0 and set(c[1:]) & set("sx")), code
        out.append(View(c[0] == "E", "h" in c, "x" not in c))
    return out


def make_views(code, salt, side):
    """the scene.make_view dicts of a view code; salt: a number that differs from cull to cull (another camera orientation)"""
    out = []
    for i, c in enumerate(code.split(",")):
        if "s" in c:
            v = scene.cascade_view(seed=scene.SEED + 31 * salt, size=0.4 * side, depth=2.0 * side, index=i - 1)
        else:
            v = scene.main_camera_view(seed=scene.SEED + 17 * salt + i, camera_position=(0.03 * side * i, 0.0, -0.02 * side * i) if "x" in c else (0.0, 0.0, 0.0))
        v["use_hiz"] = int("h" in c)
        v["emit_records"] = int(c[0] == "E")
        out.append(v)
    return out


def scene_side(n):
    return 100.0 * n ** (1.0 / 3.0)


@functools.lru_cache(maxsize=2)
def build_scene(kind, n, transforms):
    """The pools of a case (the generators' defects on). kind: flat / hier (pools pair slot for slot), spec / gen (the transform
    pool shuffled for 5 % / all of the slots), hier_spec / hier_gen. transforms > n: the mesh pool holds the first n entities."""
    total = max(n, transforms)
    sc = scene.hierarchy_scene(total, depth=4, fanout=10) if kind.startswith("hier") else scene.flat_scene(total)
    if kind.endswith("spec"):
        sc = scene.shuffled_scene(sc, fraction=0.05)
    elif kind.endswith("gen"):
        sc = scene.shuffled_scene(sc, fraction=1.0)
    if n < total:
        sc = scene.Scene(sc.meshes[:n].copy(), sc.transforms, sc.entity_to_transform)
    return sc


def mirror_mapping(sc):
    """MeshMapping of a pool whose mirror is in pool-slot order (gv_mirror.cpp: rebuild_meshes counts, mesh_mapping_of in
    gv_dirty_ranges.hpp decides): candidates = live, enabled meshes with a transform; exact when each sits at its transform's
    slot, speculate when 90 % do"""
    ent = sc.meshes["entity"].astype(np.int64)
    e2t = np.asarray(sc.entity_to_transform, dtype=np.int64)
    slot = np.where(ent < e2t.size, e2t[np.minimum(ent, e2t.size - 1)], int(scene.GV_NONE))
    slot = np.where(ent == 0, int(scene.GV_NONE), slot)
    candidate = (ent != 0) & (sc.meshes["isEnabled"] != 0) & (slot != int(scene.GV_NONE))
    own = int(np.count_nonzero(candidate & (slot == np.arange(ent.size))))
    total = int(np.count_nonzero(candidate))
    return "exact" if own == total else ("speculate" if own * 10 >= total * 9 else "general")


def candidates(sc):
    ent = sc.meshes["entity"]
    return int(np.count_nonzero((ent != 0) & (sc.meshes["isEnabled"] != 0)))


def hiz_is_nested(size):
    import hiz_paths_support as hp
    sizes = hp.mip_sizes(*size)
    return not any((w > 1 and w % 2) or (h > 1 and h % 2) for w, h in sizes[:-1])


def run_program(c, on_cull=None):
    """Walks the case's program over a PoolModel in the state the GPU test starts from; yields / returns [(step index, Step, Plan)]
    of its culls."""
    st = PoolModel()
    st.seen_at = st.stamp  # two quiet culls ...
    st.edit(c.transforms, c.transforms, c.MAP, c.depth)  # ... then every transform marked dirty
    flags = FIXTURE_FLAGS[c.fixture]
    nested = hiz_is_nested(c.hiz)
    out = []
    for i, step in enumerate(PROGRAMS[c.program]):
        if step.kind == "few":
            st.edit(c.transforms, EDIT_SLOTS, c.MAP, c.depth)
        elif step.kind == "dense":
            st.edit(c.transforms, c.transforms, c.MAP, c.depth)
        elif step.kind == "sweep":
            st.sweep()
        elif step.kind == "hiz":
            nested = hiz_is_nested(step.views)
        else:
            out.append((i, step, cull_plan(c.n, c.transforms, c.MAP, c.depth, parse_views(step.views), flags, sweep=step.sweep, state=st,
                                           nested=nested)))
    return out


def case_cells(c):
    cells, upkeep = set(), set()
    for _i, _step, plan in run_program(c):
        cells |= plan.cells
        upkeep |= set(plan.upkeep)
    return cells, upkeep


def table_pools(t):
    """(scene of the shared transform pool, {pool id: mesh array}) of a table case: the first entities in place (exact), a
    random selection in random order (general), the first entities with one in twenty swapped about (speculate)"""
    sc = build_scene("flat", t.n, t.n)
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ 0x7AB1E))
    pools = {}
    for pool_id, mapping, n, _a, _b in t.pools:
        idx = np.arange(n)
        if mapping == "general":
            idx = rng.permutation(t.n)[:n]
        elif mapping == "speculate":
            chosen = rng.choice(n, size=n // 20, replace=False)
            idx[chosen] = chosen[rng.permutation(chosen.size)]
        pools[pool_id] = sc.meshes[idx].copy()
    return sc, pools


def table_jobs(t, batch):
    return [(n, mapping, parse_views(first if batch == 0 else second)) for _id, mapping, n, first, second in t.pools]


def all_case_cells():
    cells, upkeep = set(), set()
    for c in CASES:
        cc, uu = case_cells(c)
        cells |= cc
        upkeep |= uu
    for t in TABLE_CASES:
        for batch in (0, 1):
            cells |= table_plan(table_jobs(t, batch)).cells
    return cells, upkeep
