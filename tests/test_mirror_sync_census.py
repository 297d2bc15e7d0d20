"""Census of the mirror sync, on the CPU: sync_plan (tests/mirror_sync_support.py) restates sync_mirror and its steps
(garden_amd/csrc/gv_mirror.cpp) and the rules of gv_dirty_ranges.hpp. A search over pool sizes beside every threshold, mark sets
(one range, 32 / 33 / many ranges, ranges beside kDeviceGatherMinSlots, totals beside half the pool and beside the flagging limit,
large and small ranges mixed), the state flags and the start states that a previous sync of every form leaves collects every
reachable CELL (side, form, order, binding, flagging, cache) and every hand-over cell; the cases of CASES (run by
tests/test_gpu_mirror_sync_forms.py against the oracle) must between them hold each one, and every cell a case claims is the one
sync_plan gives for its program.

CONDITION, not a measurement: cells whose smallest shape exceeds SIZE_CAP slots get no small case. The census derives their minimal
size (LARGE_MIN, LARGE_BOTH) and tests/test_gpu_fullsize.py runs ONE case at that size for the transform-side cells among them."""
import itertools
import os
import re

import pytest

import mirror_sync_support as ms
from mirror_sync_support import Marks, every

SIZE_CAP = 1_000_000
G = ms.DEVICE_GATHER_MIN


few_limit = ms.few_limit


def smallest_pool_patching(total):
    """the smallest pool on which a sync of `total` slots is still few enough to patch blocks"""
    blocks = max(total * ms.FEW_SHARE - ms.FEW_FREE, 0)
    n = (blocks - 1) * ms.CULL_BLOCK + 1 if blocks else 1
    assert ms.few_enough_to_patch_blocks(total, ms.blocks_of(n)) and (n == 1 or not ms.few_enough_to_patch_blocks(total, ms.blocks_of(n - 1)))
    return n


LARGE_MIN = smallest_pool_patching(G)       # a device-gathered range that still keeps the pools flagging
LARGE_BOTH = smallest_pool_patching(G + 3)  # ... with three slots in the packet beside it
# beside every threshold on the pool's own size: an order table from two slots on, the sphere stream above kHotMinSlots, block boxes of
# their own accord above kAutoBoundsMinSlots, the smallest pool on which a device-gathered range goes on flagging
SIZES = (1, 2, 300, 4099, 12 * G + 257, ms.HOT_MIN, ms.HOT_MIN + 7, ms.AUTO_BOUNDS_MIN + 1, LARGE_MIN - 1, LARGE_MIN, LARGE_BOTH)


def mark_sets(n, cap):
    """name -> (first, count) marks on a pool of n slots; cap: the entity capacity (the mesh device gather's other threshold)"""
    few = few_limit(n)
    share = -(-cap // ms.MESH_GATHER_ENTITY_SHARE)  # the shortest range with count * 12 >= cap
    sets = {
        "none": (),
        "one": ((n // 3, 1),),
        "below-gather": ((n // 4, G - 1),),
        "gather": ((n // 4, G),),
        "r32": every(5, 7, 32),
        "r33": every(5, 7, 33),
        "many": every(3, 5, 200, 2),
        "half": ((1, n // 2),),
        "half+1": ((1, n // 2 + 1),),
        "half+1-small": every(0, n // 8 + 1, 7, min(n // 14 + 1, G - 1)),
        "gather+small": ((n // 4, G), (n // 4 + G + 50, 3)),
        "gather+r33": ((300, G),) + every(300 + G + 9, 7, 33),
        "two-gathers": ((10, G), (20 + G, G + 1)),
        "few": every(1, 3, few),
        "few+1": every(1, 3, few + 1),
        "few-range": ((2, few),),
        "few-range+1": ((2, few + 1),),
        "share-1": ((7, share - 1),),
        "share": ((7, share),),
        "share+small": ((7, share), (share + 40, 2)),
        "share+half+1-small": ((7, share),) + every(share + 100, max((n - share - 100) // 7, 1), 7, max(min((n - share - 100) // 7 - 1, n // 14 + 1, G - 1), 1)),
    }
    return {k: v for k, v in sets.items() if all(f + c <= n for f, c in v)}


# what the transform side can change for the mesh side of the same sync: nothing, or every recording ended
XF_REPRESENTATIVES = ("none", "half+1")
# what a first sync can leave for the second: nothing; stale staging on both sides; recordings ended
FIRST_SYNCS = (("none", "none"), ("gather", "share"), ("half+1", "half+1-small"))
# (binding, chained, the mapping the rebuild finds)
KINDS = (("aos", False, ms.MAP_EXACT), ("aos", True, ms.MAP_EXACT), ("aos", False, ms.MAP_SPECULATE), ("columns", False, ms.MAP_EXACT),
         ("ready", False, ms.MAP_EXACT), ("columns", True, ms.MAP_EXACT))
CONTEXTS = tuple(itertools.product((False, True), (False, True), (False,)))  # (keep_slot_order, block_bounds, linear_scan)


def start_states():
    """(n, the plan of the bind's own sync, the state at rest behind it): every context, binding and size without a cull in front
    (nobody records); with two culls in front (boxes or the sphere stream built, one quiet frame) where that makes a pool record"""
    for n, context, (binding, chained, mapping) in itertools.product(SIZES, CONTEXTS, KINDS):
        if n > SIZE_CAP and (chained or mapping != ms.MAP_EXACT or binding == "ready"):
            continue  # (beyond the cap only what can go on flagging is of interest)
        # (beyond the cap also with few entities: the mesh device gather then applies from kDeviceGatherMinSlots slots on)
        for cap in ((None,) if n <= SIZE_CAP else (None, ms.MESH_GATHER_ENTITY_SHARE * G)):
            state = ms.bound(context, n, [(n, binding, mapping)], chained=chained, xf_binding="columns" if binding == "columns" else "aos", entity_capacity=cap)
            plan = ms.sync_plan(state)
            rest = ms.cull(ms.cull(plan.state))
            if not context[1] and not chained and mapping == ms.MAP_EXACT:  # (without a cull the flags of the context and the pairing change nothing)
                yield n, plan, plan.state
            if rest.pools[0].has_flags:
                yield n, plan, rest


def syncs_from(n, state, xf_only):
    sets = mark_sets(n, state.xf.entity_capacity)
    pairs = [(x, "none") for x in sets] + ([] if xf_only else [(x, m) for x in XF_REPRESENTATIVES if x in sets for m in sets if m != "none"])
    for x, m in pairs:
        links = (False, True) if x in ("one", "half+1", "gather", "r33") and m == "none" else (False,)
        for link in links:
            for demote in ((False, True) if m in ("one", "share", "half+1-small", "share+small") else (False,)):
                yield (x, m, link, demote), Marks(sets[x], link, {0: sets[m]}, (0,) if demote else (), True if link else None)


@pytest.fixture(scope="module")
def reachable():
    """({cell: (smallest pool size, how)}, {hand-over cell: likewise}, number of syncs searched)"""
    cells, handovers, count = {}, {}, 0

    def note(plan, n, how):
        for found, into in ((plan.cells, cells), (plan.handovers, handovers)):
            for cell in found:
                if cell not in into or n < into[cell][0]:
                    into[cell] = (n, how)

    for n, plan, state in start_states():
        note(plan, n, "bind")
        sets = mark_sets(n, state.xf.entity_capacity)
        for x1, m1 in FIRST_SYNCS:
            if x1 not in sets or m1 not in sets:
                continue
            first = ms.sync_plan(state, Marks(sets[x1], False, {0: sets[m1]}))
            for swept in (True, False):  # (the world cache matters to the transform side alone)
                mid = ms.cull(first.state)
                mid = ms.swept(mid) if swept else mid
                for how, marks in syncs_from(n, mid, xf_only=not swept):
                    note(ms.sync_plan(mid, marks), n, (x1, m1, swept) + how)
                    count += 1
                # growth: a few slots, and enough of them that the tail is due for its re-order
                for extra in (3, n // 7 + 2):
                    grown = ms.resized(mid, n + extra, {0: n + extra})
                    note(ms.sync_plan(grown, Marks(sets["one"], False, {0: sets["one"]})), n + extra, (x1, m1, swept, "grow", extra))
                    count += 1
    return cells, handovers, count


@pytest.fixture(scope="module")
def held():
    """({cell: the first case that holds it}, {hand-over cell: likewise})"""
    cells, handovers = {}, {}
    for c in ms.CASES:
        for plan in [ms.case_bind(c)] + [run[2] for run in ms.case_states(c)]:
            for cell in plan.cells:
                cells.setdefault(cell, c.name)
            for cell in plan.handovers:
                handovers.setdefault(cell, c.name)
    return cells, handovers


def test_the_sync_still_reads_as_restated():
    for name, lines in ms.LITERAL_LINES.items():
        text = ms.source_text(name)
        for line in lines:
            assert line in text, f"{name} no longer holds `{line}`: the mirror sync changed, restate sync_plan"
    assert (ms.DEVICE_GATHER_MIN, ms.CULL_BLOCK, ms.HOT_MIN, ms.AUTO_BOUNDS_MIN) == (2048, 256, 65536, 262144)  # (the sizes of CASES were chosen for these)
    assert (ms.XF_STRIDE, ms.XF_EXTENT, ms.MESH_STRIDE, ms.MESH_EXTENT) == (80, 75, 48, 44)
    m = re.search(r"constexpr uint32_t kMinSmallStreak = (\d+);", ms.source_text("gv_context.cpp"))
    assert m and int(m.group(1)) == ms.MIN_SMALL_STREAK


# Cells the search finds only above SIZE_CAP slots: a device-gathered range (kDeviceGatherMinSlots slots at least) of a sync that is
# still few enough to patch blocks (16 * total <= blocks + 1024) needs 31 744 blocks. cell -> the test that runs it.
LARGE_CASE = "tests.test_gpu_fullsize::test_marks_through_the_order_table_at_the_smallest_pool_that_has_them"


def test_every_reachable_cell_has_a_case(reachable, held):
    cells, handovers, count = reachable
    print(f"census: {count} syncs searched, {len(cells)} cells, {len(handovers)} hand-over cells; LARGE_MIN = {LARGE_MIN}")
    large = {c: where for c, where in cells.items() if where[0] > SIZE_CAP}
    for cell in sorted(cells):
        n, how = cells[cell]
        where = "LARGE ONLY" if cell in large else ("case " + held[0][cell] if cell in held[0] else "MISSING")
        print(f"census {str(cell):<76} {where}; smallest: {n} slots, {how}")
    for cell in sorted(handovers):
        n, how = handovers[cell]
        print(f"census hand-over {str(cell):<44} {'case ' + held[1][cell] if cell in held[1] else 'MISSING'}; smallest: {n} slots, {how}")
    missing = sorted(c for c in cells if c not in large and c not in held[0])
    assert not missing, f"no case of mirror_sync_support.CASES takes: {missing}"
    missing = sorted(c for c in handovers if handovers[c][0] <= SIZE_CAP and c not in held[1])
    assert not missing, f"no case of mirror_sync_support.CASES takes the hand-over: {missing}"
    unknown = sorted(c for c in held[0] if c not in cells) + sorted(c for c in held[1] if c not in handovers)
    assert not unknown, f"cells of CASES that the search never found (extend the search): {unknown}"
    # the large-only cells: all of them device gathers that go on flagging, each from LARGE_MIN slots on
    assert large and all(where[0] in (LARGE_MIN, LARGE_BOTH) for where in large.values())
    assert all((where[0] == LARGE_BOTH) == c[1].startswith("mixed") for c, where in large.items())
    assert all(c[1] in ("device", "mixed+packet", "mixed+ranged") and c[4] in ("marks", "both") for c in large)
    assert LARGE_MIN == 8_126_209  # 31 744 blocks less 255 slots: "about 8.13 M"
    xf_large = {c for c in large if c[0] == "xf"}
    assert ("xf", "device", "permuted", "aos", "marks", "tracked") in xf_large  # mark_dirty_blocks_kernel through d_xinv
    module, name = LARGE_CASE.split("::")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), module.split(".")[1] + ".py")) as f:
        assert f"def {name}(" in f.read(), "the one case at LARGE_MIN slots is gone"
    assert LARGE_BOTH == LARGE_MIN + 3 * ms.FEW_SHARE * ms.CULL_BLOCK
    for cell in sorted(large):
        print(f"census large-only {cell}: from {large[cell][0]} slots")


def test_cells_proven_unreachable(reachable):
    cells = set(reachable[0])
    # a dense sync is never few (2 * total > occupancy and 16 * total <= blocks + 1024 only meet below 2 slots... where nothing records):
    # it never goes on flagging
    assert not {c for c in cells if c[1] in ("device_dense", "pipelined", "whole", "mixed+whole") and c[4] in ("packet", "marks", "both")}
    # rebuilds and growth end every recording
    assert not {c for c in cells if c[1] in ("rebuild", "grow") and c[4] not in ("none", "stopped")}
    # a permuted transform mirror sends host ranges as the packet, never as ranged copies
    assert not {c for c in cells if c[0] == "xf" and c[1] in ("ranged", "mixed+ranged") and c[2] == "permuted"}
    # column binds and pools with a ready column have no device gather
    assert not {c for c in cells if c[3] != "aos" and (c[1].startswith("device") or c[1].startswith("mixed"))}
    # only a permuted mesh pool goes up whole
    assert not {c for c in cells if c[0] == "mesh" and c[1] in ("whole", "mixed+whole") and c[2] == "slot"}
    # a rebuild or growth leaves the world cache invalid: no tracked cell
    assert not {c for c in cells if c[0] == "xf" and c[1] in ("rebuild", "grow") and c[5] == "tracked"}
    # the transform packet alone keeps the bit-plane (nothing else flags): `both` on the transform side is a mixed sync
    assert not {c for c in cells if c[0] == "xf" and c[4] == "both" and not c[1].startswith("mixed")}


def test_every_case_claims_what_the_model_gives():
    names = [c.name for c in ms.CASES]
    assert len(set(names)) == len(names)
    for c in ms.CASES:
        assert c.n % ms.CULL_BLOCK != 0 and c.n <= SIZE_CAP, c.name
        runs = ms.case_states(c)
        assert len(runs) == len(c.syncs), c.name
        for k, ((_state, _marks, plan, after), claim) in enumerate(zip(runs, (s.claim for s in c.syncs))):
            forms = tuple((cell[0], cell[1], cell[4]) for cell in plan.cells)
            assert forms == tuple(claim), f"{c.name} sync {k}: the model gives {forms}, the case claims {claim}"
            # every sync leaves room for decoys on both sides
            ms.decoy_slots(plan, "xf", c.n)
            ms.decoy_slots(plan, 0, c.n)
            # what bounds_blocks_total must show behind a flagging sync of a block-bounds context
            if "+bounds" in c.context and not c.chained:
                for cell in plan.cells:
                    if cell[4] in ("packet", "marks", "both"):
                        assert after.pools[0].boxes, f"{c.name} sync {k}: flagged, but the boxes would be rebuilt or dropped"
                if any(cell[4] == "stopped" for cell in plan.cells):
                    assert not after.pools[0].boxes, f"{c.name} sync {k}: the recording ends, but the cull behind it rebuilds the boxes"


def test_the_thresholds_sit_where_the_cases_put_them():
    """one sync each, either side of every threshold of the issue's list"""
    def forms(n, context, marks, binding="aos", prep="ccs", cap=None):
        state = ms.bound(context, n, [(n, binding, ms.MAP_EXACT)], xf_binding="columns" if binding == "columns" else "aos", entity_capacity=cap)
        state = ms.sync_plan(state).state
        for step in prep:
            state = ms.cull(state) if step == "c" else ms.swept(state)
        plan = ms.sync_plan(state, marks)
        return [(c[0], c[1], c[4]) for c in plan.cells], ms.upload_bytes(plan)

    spatial, slot, slot_bounds = (False, False, False), (True, False, False), (True, True, False)
    n = 9001
    assert forms(n, spatial, Marks(((100, G - 1),))) == ([("xf", "packet", "none")], 64 * (G - 1))
    assert forms(n, spatial, Marks(((100, G),))) == ([("xf", "device", "none")], (G - 1) * 80 + 75)
    assert forms(n, slot, Marks(((100, G - 1),))) == ([("xf", "ranged", "none")], 45 * (G - 1))
    assert forms(n, slot, Marks(every(5, 7, 32))) == ([("xf", "ranged", "none")], 45 * 32)
    assert forms(n, slot, Marks(every(5, 7, 33))) == ([("xf", "packet", "none")], 64 * 33)
    assert forms(n, spatial, Marks(((1, 4500),))) == ([("xf", "device", "none")], 4499 * 80 + 75)           # 9000 is not more than 9001
    assert forms(n, spatial, Marks(((1, 4501),))) == ([("xf", "device_dense", "none")], 4500 * 80 + 75)
    assert forms(n, spatial, Marks(((1, 4501),)), binding="columns") == ([("xf", "pipelined", "none")], 45 * n)
    assert forms(n, spatial, Marks(((1, 4501),), links=True)) == ([("xf", "pipelined", "none")], 45 * n)
    # the mesh device gather: 2048 slots and 1/12 of the entity capacity
    assert forms(n, spatial, Marks(pools={0: ((7, G),)}), cap=12 * G) == ([("mesh", "device", "none")], (G - 1) * 48 + 44 + 4 * 12 * G)
    assert forms(n, spatial, Marks(pools={0: ((7, G),)}), cap=12 * G + 1) == ([("mesh", "packet", "none")], 32 * G)
    assert forms(n, spatial, Marks(pools={0: ((7, G - 1),)}), cap=1000) == ([("mesh", "packet", "none")], 32 * (G - 1))
    assert forms(n, spatial, Marks(pools={0: ((7, G),)}), cap=12 * G, binding="ready") == ([("mesh", "packet", "none")], 32 * G)
    assert forms(n, spatial, Marks(pools={0: every(0, 1200, 7, 643)})) == ([("mesh", "whole", "none")], 28 * n)   # 4501 slots
    assert forms(n, spatial, Marks(pools={0: every(0, 1200, 6, 643) + ((7200, 642),)})) == ([("mesh", "packet", "none")], 32 * 4500)
    assert forms(n, slot, Marks(pools={0: every(0, 1200, 7, 643)})) == ([("mesh", "ranged", "none")], 28 * 4501)
    # few enough to patch blocks: 36 blocks + 1024 -> 66 slots
    assert few_limit(n) == 66
    assert forms(n, slot_bounds, Marks(every(1, 3, 66))) == ([("xf", "packet", "packet")], 64 * 66)
    assert forms(n, slot_bounds, Marks(every(1, 3, 67))) == ([("xf", "packet", "stopped")], 64 * 67)
    assert forms(n, slot_bounds, Marks(((2, 66),))) == ([("xf", "ranged", "marks")], 45 * 66)
    assert forms(n, slot_bounds, Marks(pools={0: ((2, 66),)})) == ([("mesh", "ranged", "marks")], 28 * 66)
    assert forms(n, slot_bounds, Marks(pools={0: every(1, 3, 66)})) == ([("mesh", "packet", "packet")], 32 * 66)
    assert forms(n, slot_bounds, Marks(pools={0: every(1, 3, 67)})) == ([("mesh", "packet", "stopped")], 32 * 67)


def test_the_rules_agree_with_the_table_of_the_cpp_test():
    """normalise and the four rules against the values tests/cpp/dirty_ranges_test.cpp tabulates (read from its text), so that the
    two restatements cannot drift apart"""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "cpp", "dirty_ranges_test.cpp")) as f:
        text = f.read()
    number = lambda s: int(re.sub(r"(ull|u)$", "", s.replace("1ull << 40", str(1 << 40))))  # noqa: E731
    truth = {"true": True, "false": False}

    def table(name):
        body = text[text.index(name + "[] = {"):]
        return body[:body.index("};")]

    tails = re.findall(r"\{(\d+u?), (\d+u?), (\d+u?), (true|false)\}", table("tails"))
    fews = re.findall(r"\{(1ull << 40|\d+), (\d+), (true|false)\}", table("fews"))
    mosts = re.findall(r"\{(\d+u?), (\d+u?), (true|false)\}", table("mosts"))
    maps = re.findall(r"\{(\d+), (\d+), (\d)\}", table("maps"))
    assert (len(tails), len(fews), len(mosts), len(maps)) == (16, 10, 10, 12)  # as its own summary line says
    for a, b, c, due in tails:
        assert ms.tail_due_for_reorder(number(a), number(b), number(c)) == truth[due], (a, b, c)
    for total, blocks, few in fews:
        assert ms.few_enough_to_patch_blocks(number(total), number(blocks)) == truth[few], (total, blocks)
    for total, occupancy, most in mosts:
        assert ms.most_of_pool(number(total), number(occupancy)) == truth[most], (total, occupancy)
    for own, candidates, mapping in maps:
        assert ms.mesh_mapping_of(int(own), int(candidates)) == int(mapping), (own, candidates)
    # normalise: the invariants its random rounds check, on the same generator and seed, against a bitmap
    seed = [12345]

    def rnd():
        seed[0] = (seed[0] * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return seed[0] >> 33

    for rounds in range(60):
        limit = 1000 + rnd() % 60000
        marked = bytearray(limit)
        marks = []
        for _ in range(1 + rnd() % 300):
            first, count = rnd() % (limit + 50), rnd() % 40
            if rnd() % 50 == 0:
                count = 0xFFFFFFFF - rnd() % 3
            marks.append((first, count))
            for i in range(first, min(first + count, limit)):
                marked[i] = 1
        gap = 0 if rounds % 3 == 0 else rnd() % 64
        got = ms.normalise(ms.add_marks(marks), limit, gap)
        covered = bytearray(limit)
        for (lo, hi), nxt in zip(got, got[1:] + [(limit + gap + 1, 0)]):
            assert lo < hi <= limit and hi + gap < nxt[0]
            covered[lo:hi] = b"\x01" * (hi - lo)
        assert all(c or not m for c, m in zip(covered, marked))
        if gap == 0:
            assert covered == marked
    # beyond kMax ranges the gap doubles until they fit
    got = ms.normalise([(4 * k, 4 * k + 1) for k in range(40)], 1000, 0, kmax=8)
    assert len(got) <= 8 and got[0][0] == 0 and got[-1][1] == 157
