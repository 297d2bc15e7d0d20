"""Test helpers of the results delivery: which route hands every (pool, view) of a frame to the host (gv_pool_results_fetch,
flush_mid_sorts, sort_publishes, flush_small_sorts, publish_args_of, deliver_small and deliver_large in
garden_amd/csrc/gv_results.cpp), restated in plain Python (delivery_plan over a Frame), the record layouts the GPU tests deliver
in (LAYOUTS), and the table of GPU cases (CASES) that tests/test_delivery_census.py proves to hold every reachable cell and
tests/test_gpu_delivery_forms.py runs against the oracle. TEST INFRASTRUCTURE ONLY.

A CELL is (route, records, visibility):
  route       sort    the small-pool sort publishes what it has sorted (publish_visibility / publish_record in gv_sort.hip)
              publish the publish launch (publish_kernel = publish_block + pack_records_chunk in gv_cull.hip)
              copies  deliver_large: the count read back, pack_records_kernel or three copies, unpermute_bytes_kernel
              found   an earlier fetch of the frame has delivered the view already: its own fetch only looks the results up
  records     structs (the pool's record layout), arrays (visible_idx / baked_model / distance_sq) or none (a count-only view)
  visibility  lds (un-permuted in LDS by the delivering kernel), device (un-permuted by unpermute_bytes_kernel in front),
              straight (the mirror is in pool-slot order: copied as it is) or none (a shadow pass)
The plan depends on sizes, flags and the order of the fetches; never on the entities themselves.

The library has no counter that tells which route delivered a view, so no GPU test observes a cell: that a case holds a cell
rests on this model — on delivery_plan following the lines of LITERAL_LINES, and on frame_model's claim, restated from
gv_mirror.cpp, that a pool's mirror is permuted exactly in a spatially ordered context from two slots on. What the GPU tests
confirm of it is indirect: mutants of one route's kernel fail exactly the cases the model puts on that route
(profiles/r21_delivery_forms.md)."""
import collections

import numpy as np

from hiz_paths_support import header_constant, source_text  # noqa: F401  (source_text: for the census)

BATCH_SORT_MAX = header_constant("gv_sort_kernels.hpp", "kBatchSortMaxSlots")
PUBLISH_LDS = header_constant("gv_kernels.hpp", "kPublishLdsSlots")
PUBLISH_MAX = header_constant("gv_kernels.hpp", "kPublishMaxSlots")
MAX_PUBLISH_VIEWS = header_constant("gv_kernels.hpp", "kMaxPublishViews")
MAX_RECORD_STRIDE = header_constant("gv_kernels.hpp", "kMaxRecordStride")
MID_SORT_MAX = 1 << 20  # (not a plain number in its header: LITERAL_LINES holds the line)
GV_MAX_POOLS, GV_MAX_VIEWS = 16, 8  # include/garden_vis.h, as garden_amd/lib.py has them

# Lines of the dispatch that the restatement below follows (test_delivery_census.py checks that the library still holds them).
LITERAL_LINES = {
    "gv_results.cpp": [
        "const bool small = vs.occupancy != 0 && vs.occupancy <= kPublishMaxSlots;",
        # sort_publishes: the two `return false` conditions
        "if (w.valid && !w.published && !w.sort_pending && w.occupancy != 0 && w.occupancy <= kPublishMaxSlots)",
        "if (w.valid && w.sort_pending && w.occupancy <= kBatchSortMaxSlots && !ctx->pools[pool].record_layout.stride)",
        # publish_args_of
        "const bool wperm = !wp.perm.empty() && wp.perm.size() == w.occupancy;",
        "if (w.emitted && wp.record_layout.stride) {",
        "if (wperm && w.occupancy > kPublishLdsSlots) {  // too large for the in-LDS un-permutation",
        # flush_mid_sorts, flush_small_sorts
        "if (!vs.valid || !vs.sort_pending || vs.occupancy <= kBatchSortMaxSlots)",
        "for (uint32_t pool = 0; pool < GV_MAX_POOLS && views < kMaxPublishViews; pool++)",
        "const bool fuse_publish = sort_publishes(ctx);",
        # deliver_small
        "if (vs.published && !ctx->publish_sync_pending)",
        "const uint32_t pid = (pool_id + q) % GV_MAX_POOLS;  // the pool asked for first: it always fits",
        "if (!w.valid || w.published || w.occupancy == 0 || w.occupancy > kPublishMaxSlots)",
        # deliver_large
        "const bool as_records = vs.emitted && pool.record_layout.stride;",
        "if (!pool.perm.empty() && pool.perm.size() == vs.occupancy)",
        # gv_pool_sort: every pool a case may bind waits for the frame's flush
        "if (vs.occupancy <= kMidSortMaxSlots) {",
    ],
    "gv_sort_kernels.hpp": ["constexpr uint32_t kMidSortMaxSlots = 1u << 20;"],
    "gv_cull.hip": [  # the grids the record-count edges of the GPU tests are chosen for (publish_grid, PACK_GRID)
        "const uint32_t blocks = std::max(1u, std::min(256u, (occupancy + 255u) / 256u));",
        "const uint32_t blocks = std::max(1u, std::min(2048u, (capacity + 63u) / 64u));",
        "for (uint32_t first = block * 64; first < n; first += nblocks * 64)  // workgroup-uniform",
    ],
    "gv_mirror.cpp": [  # when a pool's mirror is permuted: a spatially ordered context, two slots or more
        "if ((ctx->config.flags & GV_CONFIG_KEEP_SLOT_ORDER) || n < 2)",
        "if (ctx->xinv.empty() || n < 2)",
    ],
}

ROUTES = ("sort", "publish", "copies", "found")
RECORDS = ("structs", "arrays", "none")
VISIBILITY = ("lds", "device", "straight", "none")
RECORD_CHUNK = 64  # records per pack_records_chunk
PACK_GRID = 2048   # most workgroups of pack_records_kernel


def publish_grid(widest):
    """workgroups per view of launch_publish"""
    return max(1, min(256, (widest + 255) // 256))


# ---- the model ----
# View.sort: 0, or 1 ascending / 2 descending (gv_sort asks for emitted views only)
View = collections.namedtuple("View", "emitted main sort")
# permuted: the pool's perm is non-empty and of the view's size; layout: the pool has a record layout
Pool = collections.namedtuple("Pool", "occupancy permuted layout views")
# fetches: [(pool, view)] in the order gv_pool_results_fetch is called, every view at most once
Frame = collections.namedtuple("Frame", "pools fetches")


def _records_of(pool, view):
    return "structs" if view.emitted and pool.layout else ("arrays" if view.emitted else "none")


def _publish_args_of(pool, view):
    """(records, visibility) as publish_args_of sets a view up, for the publish launch and for the publishing sort alike"""
    wperm = pool.permuted
    visibility = "none"
    if view.main:
        visibility = "device" if wperm and pool.occupancy > PUBLISH_LDS else ("lds" if wperm else "straight")
    return _records_of(pool, view), visibility


def delivery_plan(frame, trace=None):
    """{(pool, view): CELL} of every view the frame's fetches deliver or look up, all views freshly culled (unpublished) and
    their sorts asked for. A view delivered by a sibling's fetch and then fetched itself is `found` (in the form it was
    delivered in); one that is never fetched keeps the route that delivered it. trace: a list that receives
    (fetch number, "mid_sort" / "small_sort" / "publishing_sort" / "publish" / "copies" / "found", [(pool, view)])."""
    pools = frame.pools
    assert len(pools) <= GV_MAX_POOLS and all(len(p.views) <= GV_MAX_VIEWS for p in pools)
    keys = [(p, v) for p, pool in enumerate(pools) for v in range(len(pool.views))]  # the loops' order: pool, then view
    occ = {k: pools[k[0]].occupancy for k in keys}
    assert all(o <= MID_SORT_MAX for o in occ.values())
    published = dict.fromkeys(keys, False)
    pending = {k: (pools[k[0]].views[k[1]].sort if occ[k] else 0) for k in keys}
    assert all(pools[p].views[v].emitted for (p, v) in keys if pending[(p, v)])
    cells = {}
    sync_pending = False

    def note(f, what, views):
        if trace is not None and views:
            trace.append((f, what, list(views)))

    def sort_publishes():
        for k in keys:
            if not published[k] and not pending[k] and occ[k] != 0 and occ[k] <= PUBLISH_MAX:
                return False
            if pending[k] and occ[k] <= BATCH_SORT_MAX and not pools[k[0]].layout:
                return False
        return True

    for f, (p, v) in enumerate(frame.fetches):
        # flush_mid_sorts: every pending list beyond the one-launch batch; its view is delivered afterwards like an unsorted one
        mid = [k for k in keys if pending[k] and occ[k] > BATCH_SORT_MAX]
        for k in mid:
            pending[k] = 0
            published[k] = False
        note(f, "mid_sort", mid)
        # flush_small_sorts: up to kMaxPublishViews views per launch
        while True:
            fuse = sort_publishes()
            taken = [k for k in keys if pending[k]][:MAX_PUBLISH_VIEWS]
            if not taken:
                break
            for k in taken:
                pending[k] = 0
                published[k] = fuse
                if fuse:
                    cells[k] = ("sort",) + _publish_args_of(pools[k[0]], pools[k[0]].views[k[1]])
                    sync_pending = True
            note(f, "publishing_sort" if fuse else "small_sort", taken)
        pool, view = pools[p], pools[p].views[v]
        small = pool.occupancy != 0 and pool.occupancy <= PUBLISH_MAX
        if small and published[(p, v)] and not sync_pending:
            cells[(p, v)] = ("found",) + cells[(p, v)][1:]
            note(f, "found", [(p, v)])
        elif small:  # deliver_small: every unpublished small view, the pool asked for first
            sent = []
            for q in range(GV_MAX_POOLS):
                pid = (p + q) % GV_MAX_POOLS
                for w in range(len(pools[pid].views) if pid < len(pools) else 0):
                    if len(sent) < MAX_PUBLISH_VIEWS and not published[(pid, w)] and occ[(pid, w)] != 0 and occ[(pid, w)] <= PUBLISH_MAX:
                        sent.append((pid, w))
            for k in sent:
                cells[k] = ("publish",) + _publish_args_of(pools[k[0]], pools[k[0]].views[k[1]])
                published[k] = True
            sync_pending = False
            note(f, "publish", sent)
        else:  # deliver_large
            visibility = "none"
            if view.main and pool.occupancy:
                visibility = "device" if pool.permuted else "straight"
            cells[(p, v)] = ("copies", _records_of(pool, view), visibility)
            note(f, "copies", [(p, v)])
    return cells


# ---- record layouts of the GPU tests: name -> (numpy dtype, bufferIndex value or None) ----
def _layout(stride, component_offset, baked_model, distance_sq, buffer_index=None):
    names, formats, offsets = ["componentOffset", "bakedModel", "distanceSq"], ["<u8", ("<f4", 12), "<f4"], [component_offset, baked_model, distance_sq]
    if buffer_index is not None:
        names, formats, offsets = names + ["bufferIndex"], formats + ["<u4"], offsets + [buffer_index]
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": stride})


LAYOUTS = {
    # the four of RECORD_DTYPES (tests/test_gpu_cull.py): 64 bytes packed, 80 bytes under a 16-byte-aligned matrix
    "packed": (_layout(64, 0, 8, 56), None),
    "packed_sorted": (_layout(64, 0, 8, 56, 60), 5),
    "simd": (_layout(80, 0, 16, 64), None),
    "simd_sorted": (_layout(80, 0, 16, 64, 68), 5),
    "index_last": (_layout(64, 0, 8, 56, 60), 0x80000001),  # bufferIndex in the record's last word, its top bit set
    "reversed_96": (_layout(96, 80, 16, 12, 8), 7),          # the fields in reverse order, padding in front, between and behind
    "offset4_112": (_layout(112, 4, 16, 64, 68), 9),         # componentOffset 4- but not 8-aligned
    "wide_128": (_layout(128, 0, 64, 124, 8), 11),           # the widest stride, distanceSq in the last word
}


def covered_bytes(dtype):
    """which bytes of a record a field owns (every other one leaves as zero)"""
    covered = np.zeros(dtype.itemsize, bool)
    for name in dtype.names:
        sub, at = dtype.fields[name][:2]
        covered[at:at + sub.itemsize] = True
    return covered


# ---------------------------------------------------------------------------------------------------------------------------
# The GPU cases. A case binds pools of the given sizes (the first entities of ONE flat scene, sharing its transform pool) to a
# context that keeps the mirror in spatial order ("spatial": permuted from two slots on) or in pool-slot order ("slot") and
# runs FRAMES: per pool a layout name (or None: three arrays) and a string of view codes, then the order of the fetches.
#   view codes: M main pass, S shadow pass, m / s the same count-only; a / d behind it: sorted ascending / descending; a digit:
#   the camera (0 the whole cube — the default of a main pass —, 1 .. 7 slabs of it, 1 the default of a shadow pass)
#   order: "forward" (pool by pool, view by view), "reverse", a pool to fetch first ("from 2": pool 2, then forward) or the
#   forward order begun at its k-th fetch ("rotate 2")
# ---------------------------------------------------------------------------------------------------------------------------
Frm = collections.namedtuple("Frm", "layouts views order")
Case = collections.namedtuple("Case", "name context sizes frames")

ViewCode = collections.namedtuple("ViewCode", "emitted main sort camera")


def parse_views(code):
    out = []
    for c in code.split(","):
        assert c[0] in "MSms" and set(c[1:]) <= set("ad01234567"), code
        sort = 1 if "a" in c else (2 if "d" in c else 0)
        digits = [int(x) for x in c[1:] if x.isdigit()]
        out.append(ViewCode(c[0] in "MS", c[0] in "Mm", sort, digits[0] if digits else (0 if c[0] in "Mm" else 1)))
    return out


def fetch_order(frm):
    keys = [(p, v) for p, code in enumerate(frm.views) for v in range(len(code.split(",")))]
    if frm.order == "forward":
        return keys
    if frm.order == "reverse":
        return keys[::-1]
    what, number = frm.order.split()
    if what == "rotate":
        return keys[int(number):] + keys[:int(number)]
    return [k for k in keys if k[0] == int(number)] + [k for k in keys if k[0] != int(number)]


def frame_model(c, frm):
    """the Frame of one of a case's frames"""
    total = max(c.sizes)
    pools = [Pool(n, c.context == "spatial" and n >= 2 and total >= 2, layout is not None,
                  tuple(View(v.emitted, v.main, v.sort) for v in parse_views(code)))
             for n, layout, code in zip(c.sizes, frm.layouts, frm.views)]
    return Frame(tuple(pools), tuple(fetch_order(frm)))


# the occupancies on either side of every handover of the path, and the byte tails of the isVisible copies below and beside 4
EDGE_OCCUPANCIES = (1, 2, 3, 5, 255, BATCH_SORT_MAX - 1, BATCH_SORT_MAX, BATCH_SORT_MAX + 1, PUBLISH_LDS - 1, PUBLISH_LDS, PUBLISH_LDS + 1,
                    PUBLISH_MAX - 1, PUBLISH_MAX, PUBLISH_MAX + 1)
_ALL_KINDS = "M,S,m,s"
EDGE_FRAMES = (
    # a main and a shadow pass and a count-only main and shadow pass, as arrays and as structs; each kind of view is fetched
    # first once (its fetch delivers all four) and found by its own fetch otherwise
    Frm((None,), (_ALL_KINDS,), "forward"),
    Frm(("packed",), (_ALL_KINDS,), "rotate 1"),
    Frm(("simd_sorted",), (_ALL_KINDS,), "rotate 2"),
    Frm((None,), (_ALL_KINDS,), "reverse"),
    Frm(("packed_sorted",), ("Ma,Sd",), "forward"),    # sorted with a layout: the sort publishes up to 16 384 slots
    Frm(("simd",), ("Md,Sa1,Sd2",), "from 0"),
)
_SORTED_PAIR = (("packed_sorted", "simd_sorted"), ("Ma,Sd", "Md0,Sa1,Sa2"))
CASES = [Case(f"edge-{n}-{context}", context, (n,), EDGE_FRAMES) for n in EDGE_OCCUPANCIES for context in ("spatial", "slot")] + [
    # who publishes: two sorted pools with layouts (the sort) / plus an unsorted small view, or a sorted pool without a layout
    # (the publish launch takes all); every frame twice
    Case("who-publishes-spatial", "spatial", (3001, 9001, 5003), [
        Frm(_SORTED_PAIR[0], _SORTED_PAIR[1], "forward"), Frm(_SORTED_PAIR[0], _SORTED_PAIR[1], "reverse"),
        Frm(_SORTED_PAIR[0] + ("packed",), _SORTED_PAIR[1] + ("M",), "forward"), Frm(_SORTED_PAIR[0] + ("packed",), _SORTED_PAIR[1] + ("M",), "from 1"),
        Frm(_SORTED_PAIR[0] + (None,), _SORTED_PAIR[1] + ("Ma",), "forward"), Frm(_SORTED_PAIR[0] + (None,), _SORTED_PAIR[1] + ("Ma",), "from 2")]),
    Case("who-publishes-slot", "slot", (3001, 9001, 5003), [
        Frm(_SORTED_PAIR[0], _SORTED_PAIR[1], "forward"), Frm(_SORTED_PAIR[0], _SORTED_PAIR[1], "forward"),
        Frm(_SORTED_PAIR[0] + ("packed",), _SORTED_PAIR[1] + ("s",), "forward"), Frm(_SORTED_PAIR[0] + ("packed",), _SORTED_PAIR[1] + ("s",), "reverse"),
        Frm(_SORTED_PAIR[0] + (None,), _SORTED_PAIR[1] + ("Sd",), "forward"), Frm(_SORTED_PAIR[0] + (None,), _SORTED_PAIR[1] + ("Sd",), "reverse")]),
    # more unpublished small views than one PublishBatch holds: 40, pool 2 fetched first (pools 2, 3, 4 and 0 fill the launch,
    # pool 1 waits for a fetch of its own)
    Case("forty-views-spatial", "spatial", (3, 3000, 3001, 20_000, 200_000), [
        Frm(("packed", None, "wide_128", None, "simd_sorted"), ("M0,S1,S2,S3,M4,S5,s6,S7",) * 5, "from 2")]),
    Case("forty-views-slot", "slot", (3, 3000, 3001, 20_000, 200_000), [
        Frm((None, "reversed_96", None, "offset4_112", None), ("M0,S1,S2,S3,m4,S5,S6,S7",) * 5, "from 2")]),
]


def case_cells(c):
    cells = set()
    for frm in c.frames:
        cells |= set(delivery_plan(frame_model(c, frm)).values())
    return cells


def all_case_cells():
    """{cell: the name of the first case that holds it}"""
    held = {}
    for c in CASES:
        for cell in sorted(case_cells(c)):
            held.setdefault(cell, c.name)
    return held
