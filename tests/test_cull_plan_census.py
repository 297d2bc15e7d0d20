"""Census of the cull dispatch, on the CPU: cull_plan (tests/cull_paths_support.py) restates gv_cull, plan_cull, cull_launch and the
kernel picks of gv_cull.hip. A search over pool sizes, mappings, view sets, context flags, sweep requests and pool histories
collects every reachable CELL (cull form, HIZ, MAP, emit form); the programs of CASES (run by tests/test_gpu_cull_paths.py against
the oracle) must between them hold each one. What the search reaches only beyond the size cap of the GPU cases is pinned with the
existing test that covers it: a change of the dispatch that makes a pinned cell reachable below the cap, or creates a new cell,
fails here and asks for a case.

CONDITIONS, none measured: GPU cases hold at most 300 001 entries and a depth image of at most 256 x 256."""
import itertools

import numpy as np
import pytest

import cull_paths_support as cp
import test_gpu_hot_tiles
from garden_amd import scene

SIZE_CAP = 300_001

OCCUPANCIES = sorted({1, 255, 256, 257, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65536, 65537, 262143, 262144, 262145, 300_001} |
                     set(test_gpu_hot_tiles.SIZES))
# beyond every size a test may bind; stands for "more than kSelfPrefixMaxChunks chunks" in the search
BEYOND_SELF_PREFIX = cp.SELF_PREFIX_MAX_CHUNKS * cp.EMIT_CHUNK + 1

# Cells that exist only above SIZE_CAP: (cull form, emit form) -> (why, the test that covers it)
PINNED = {
    "scan_emit": ("the scan in front of the emit is taken beyond kSelfPrefixMaxChunks = 4096 chunks = 16 777 216 slots",
                  "tests/test_gpu_fullsize.py::test_cfg2_shape_at_10_to_the_8_on_one_gpu"),
    "hot_k2": ("two tiles per workgroup from 8192 tiles = 2 Mi entries", "tests/test_gpu_hot_tiles.py::test_hot_tiles_match_the_oracle"),
    "hot_k4": ("four tiles per workgroup from 16384 tiles = 4 Mi entries", "tests/test_gpu_hot_tiles.py::test_hot_tiles_match_the_oracle"),
}


def is_pinned(cell):
    return cell[0] in PINNED or cell[3] in PINNED


def view_sets():
    """1, 2 and 4 views; shared camera or separate; emitting, count-only or mixed; Hi-Z on view 0 or not (and on a later, separate one)"""
    out = []
    for hiz in (False, True):
        out += [[cp.View(True, hiz, True)], [cp.View(False, hiz, True)]]
        for n, shared in itertools.product((2, 4), (True, False)):
            for kinds in ("E" * n, "C" * n, "EC" * (n // 2), "CE" * (n // 2)):
                out.append([cp.View(k == "E", hiz and i == 0, shared or i == 0) for i, k in enumerate(kinds)])
                if not shared and hiz:
                    out.append([cp.View(k == "E", True, i == 0) for i, k in enumerate(kinds)])
    return out


# pool histories: what happens in front of each of a run of culls ("" nothing, F a few transforms change, D most of them do,
# S a gv_sweep of the whole pool)
HISTORIES = {"at rest": ["", "", ""], "changed once": ["", "", "F", ""], "changed once, much": ["", "", "D", ""],
             "changing every frame": ["D", "D", "D"], "changing a little every frame": ["F"] * 6, "swept": ["S", ""]}


@pytest.fixture(scope="module")
def reachable():
    """{cell: (occupancy, mapping, depth, fixture, views, sweep, history) of the smallest pool found that takes it}"""
    found = {}
    views = view_sets()
    for occ in OCCUPANCIES + [BEYOND_SELF_PREFIX]:
        for mapping, depth, (fixture, flags), sweep in itertools.product(cp.MAPS, (0, 3), cp.FIXTURE_FLAGS.items(), (0, 2, 3)):
            xfs = (occ,) if not sweep else (occ, 2 * occ, max(1, occ // 2))
            for xf, vs, (hname, history), nested in itertools.product(xfs, views, HISTORIES.items(), (True, False)):
                # (the window test is the only thing `nested` decides, the pools' sizes relative to each other matter to the fused
                # form alone: those axes are not crossed with every history)
                if not nested and not (any(v.hiz for v in vs) and hname in ("at rest", "swept")):
                    continue
                if xf != occ and hname not in ("at rest", "changed once"):
                    continue
                st = cp.PoolModel()
                for event in history:
                    if event in "FD" and event:
                        st.edit(xf, cp.EDIT_SLOTS if event == "F" else xf, mapping, depth)
                    elif event == "S":
                        st.sweep()
                    plan = cp.cull_plan(occ, xf, mapping, depth, vs, flags, sweep=sweep, state=st, nested=nested)
                    for cell in plan.cells:
                        found.setdefault(cell, (occ, mapping, depth, fixture, vs, sweep, hname))
                # the same views recorded into a batch beside another pool
                if cp.table_eligible(occ, vs, flags, sweep):
                    for cell in cp.table_plan([(occ, mapping, vs), (occ, mapping, vs)]).cells:
                        found.setdefault(cell, (occ, mapping, depth, fixture, vs, sweep, "recorded"))
    return found


@pytest.fixture(scope="module")
def covered():
    return cp.all_case_cells()


def test_the_dispatch_still_reads_as_restated():
    for name, lines in cp.LITERAL_LINES.items():
        text = cp.source_text(name)
        for line in lines:
            assert line in text, f"{name} no longer holds `{line}`: the dispatch changed, restate cull_plan"
    # (the sizes of CASES were chosen for these values)
    assert (cp.FUSED_EMIT_MAX, cp.HOT_MIN, cp.AUTO_BOUNDS_MIN, cp.EMIT_SEED_MIN, cp.EMIT_CHUNK, cp.SELF_PREFIX_MAX_CHUNKS) == \
        (32768, 65536, 262144, 262144, 4096, 4096)
    assert cp.TABLE_MAX_SLOTS == 32768 and cp.CULL_BLOCK == 256 and cp.MIN_SMALL_STREAK == 4


def test_hot_tile_sizes_are_the_pinned_tests():
    """test_gpu_hot_tiles.SIZES holds K = 1, 2 and 4 of hot_tiles_per_workgroup; K > 1 starts beyond the cap of the cases here"""
    ks = [cp.hot_tiles(cp.blocks_of(n)) for n in test_gpu_hot_tiles.SIZES]
    assert sorted(set(ks)) == [1, 2, 4]
    assert cp.HOT_K2_TILES * cp.CULL_BLOCK > SIZE_CAP and cp.HOT_K4_TILES > cp.HOT_K2_TILES
    assert cp.SELF_PREFIX_MAX_CHUNKS * cp.EMIT_CHUNK > SIZE_CAP


def test_every_reachable_cell_has_a_case(reachable, covered):
    cells, _upkeep = covered
    for cell in sorted(reachable, key=str):
        where = reachable[cell]
        print(f"census {str(cell):<58} {'pinned ' if is_pinned(cell) else ('case   ' if cell in cells else 'MISSING')} smallest: {where[0]} "
              f"{where[3]} depth {where[2]} sweep {where[5]} {where[6]} {''.join(('E' if v.emit else 'C') + ('h' if v.hiz else '') + ('' if v.shared else 'x') + ' ' for v in where[4])}")
    assert all(c[0] in cp.CULL_FORMS and c[3] in cp.EMIT_FORMS and c[2] in cp.MAPS for c in reachable)
    missing = sorted((c for c in reachable if not is_pinned(c) and c not in cells), key=str)
    assert not missing, f"no case of cull_paths_support.CASES takes: {missing}"
    # nothing is claimed that the search does not know
    unknown = sorted((c for c in cells if c not in reachable), key=str)
    assert not unknown, f"cells of CASES that the search never found (extend the search): {unknown}"


def test_pinned_cells_are_out_of_reach_below_the_cap(reachable, covered):
    """every pinned form is reachable (so the pin is not stale), first at a size beyond the cap, and names its covering test"""
    import os
    root = os.path.dirname(cp.__file__)
    for form, (why, test) in PINNED.items():
        sizes = [where[0] for cell, where in reachable.items() if form in (cell[0], cell[3])]
        assert sizes, f"{form} is pinned but no longer reachable"
        assert min(sizes) > SIZE_CAP, f"{form} is reachable at {min(sizes)} entries ({why}): give it a case"
        path, name = test.split("::")
        assert why and f"def {name}(" in open(os.path.join(os.path.dirname(root), path)).read()
    assert not any(is_pinned(c) for c in covered[0])
    # every form named by the issue is either reachable or a mistake in the tables above
    assert {c[0] for c in reachable} == set(cp.CULL_FORMS) and {c[3] for c in reachable} == set(cp.EMIT_FORMS)


def test_every_upkeep_launch_has_a_case(covered):
    """hot build and patch, block bounds and its patch with and without seeds in step, seeds, both sweeps in front of a cull"""
    assert covered[1] == set(cp.UPKEEP)


def test_plans_hold_what_the_programs_ask(covered):
    for c in cp.CASES:
        assert c.n <= SIZE_CAP and c.transforms <= SIZE_CAP and c.hiz[0] <= 256 and c.hiz[1] <= 256
        culls = cp.run_program(c)
        assert len(culls) >= 3, c.name  # a first cull and at least two more with other views
        assert len({step.views for _i, step, _p in culls}) >= 3, c.name
        for _i, step, plan in culls:
            assert plan is not None and len(plan.cull_forms) == len(plan.emit_forms) == len(cp.parse_views(step.views))
    assert len({c.name for c in cp.CASES}) == len(cp.CASES)
    # one fused case whose mesh pool is smaller than its transform pool
    assert any(c.n < c.transforms and any(p.cull_form.startswith("fused") and p.HIZ for _i, _s, p in cp.run_program(c)) for c in cp.CASES)
    for t in cp.TABLE_CASES:
        sizes = [n for _id, _m, n, _a, _b in t.pools]
        assert len(set(sizes)) >= 2 and max(sizes) <= min(SIZE_CAP, cp.TABLE_MAX_SLOTS)
        assert any(len(cp.parse_views(a)) == 1 for _id, _m, _n, a, _b in t.pools)
        for batch in (0, 1):
            assert all(cp.table_eligible(n, vs, cp.FIXTURE_FLAGS[t.fixture]) for n, _m, vs in cp.table_jobs(t, batch))


def test_sizes_leave_partial_waves_and_chunks():
    for c in cp.CASES:
        if c.exact_threshold:
            assert c.n in (cp.FUSED_EMIT_MAX, cp.HOT_MIN, cp.AUTO_BOUNDS_MIN, cp.EMIT_SEED_MIN), c.name
            continue
        assert c.n % 64 != 0, c.name
        if c.n > cp.EMIT_CHUNK:
            assert c.n % cp.EMIT_CHUNK != 0, c.name


# ---- the cases are not degenerate: with the oracle alone ----

def _oracle_counts(oracle, sc, view, hz):
    plain = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, dict(view, use_hiz=0), threads=4)
    if not view["use_hiz"]:
        return plain["draw_count"], None
    with_hiz = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view, hiz=hz, threads=4)
    return plain["draw_count"], with_hiz["draw_count"]


@pytest.mark.parametrize("c", cp.CASES, ids=lambda c: c.name)
def test_case_is_not_degenerate(oracle, c):
    """every view of the case's first three culls (and its first Hi-Z view) keeps some candidates and drops some; a Hi-Z view
    drops at least one entry the frustum alone keeps; the mapping is the one the case is declared for"""
    sc = cp.build_scene(c.kind, c.n, c.transforms)
    assert sc.count == c.n and sc.transforms.shape[0] == c.transforms
    assert cp.mirror_mapping(sc) == c.MAP
    total = cp.candidates(sc)
    hz = oracle.Hiz(scene.synthetic_depth(*c.hiz))
    side = cp.scene_side(c.transforms)
    culls = cp.run_program(c)
    seen_hiz = False
    for k, (i, step, _plan) in enumerate(culls):
        has_hiz = "h" in step.views
        if k >= 3 and (seen_hiz or not has_hiz):
            continue
        seen_hiz = seen_hiz or has_hiz
        for view in cp.make_views(step.views, i, side):
            plain, with_hiz = _oracle_counts(oracle, sc, view, hz)
            print(f"{c.name} step {i} {step.views}: {plain} of {total} candidates in the frustum" + (f", {with_hiz} behind the pyramid" if with_hiz is not None else ""))
            assert 0 < plain < total
            if with_hiz is not None:
                assert 0 < with_hiz < plain
    assert seen_hiz or not any("h" in s.views for _i, s, _p in culls)


@pytest.mark.parametrize("t", cp.TABLE_CASES, ids=lambda t: t.name)
def test_table_case_is_not_degenerate(oracle, t):
    sc, pools = cp.table_pools(t)
    hz = oracle.Hiz(scene.synthetic_depth(*t.hiz))
    for pool_id, mapping, n, first, second in t.pools:
        pool = scene.Scene(pools[pool_id], sc.transforms, sc.entity_to_transform)
        assert pool.count == n and n % 64 != 0 and cp.mirror_mapping(pool) == mapping
        for batch, code in enumerate((first, second)):
            for view in cp.make_views(code, 7 + 5 * batch + pool_id, cp.scene_side(t.n)):
                plain, with_hiz = _oracle_counts(oracle, pool, view, hz)
                print(f"{t.name} pool {pool_id} {code}: {plain} of {cp.candidates(pool)} in the frustum, behind the pyramid: {with_hiz}")
                assert 0 < plain < cp.candidates(pool)
                assert with_hiz is None or 0 < with_hiz < plain
