"""The ORDER of the device mirror: after a build on the host and after every re-order on the device (gv_reorder.hip: roots and
their box, Morton codes, the radix sort on bare keys, one permuting pass per stream) the entry -> slot table must be exactly
the one the ordering rule gives — tests/reorder_support.py, a plain numpy twin of the rule, pinned by hand-computed answers in
tests/test_reorder_twin.py. The other GPU tests check a re-ordered mirror through its results, which any consistent permutation
passes; the order itself (codes of the roots inside the roots' box, bit interleave, stability of the sort) is what block bounds,
block-level Hi-Z windows and the paired fast paths live on.

What is observed: gv_pool_mirror_slots (entry -> pool slot) of the mesh pools; a pool that pairs 1:1 with its transforms shows
the transforms' order. The twin is advanced step by step beside the library (Mirror below): a build sorts the slots, growth
appends the new slots as they are, a re-order is a stable sort of the mirror as it lies. Every step asserts
  * the table of every pool, exactly (np.array_equal; the library divides with correct rounding and does not contract),
  * the rise of stats()["mirror_reorders"] (re-orders of the transforms; the contexts are shared: deltas only),
  * that gv_pool_mirror_epoch moved exactly when the table was made anew (built, grown, re-ordered) and never otherwise,
  * that the table describes what the device holds: one cull, the mask shard (a bit per mirror ENTRY) decoded through the table
    must be the oracle's visible set and count."""
import numpy as np
import pytest

from garden_amd import scene
import reorder_support as rs

pytestmark = pytest.mark.gpu

VIEW = scene.main_camera_view()
GV_NONE = rs.GV_NONE
GV_DIRTY_TRANSFORM, GV_DIRTY_HIERARCHY = 0, 1


def cut(full, n, k=None):
    """The first n transforms / k meshes (default n) of `full` in arrays of their own; entities beyond the cut have no slot."""
    e2t = full.entity_to_transform.copy()
    e2t[e2t >= n] = GV_NONE
    return scene.Scene(full.meshes[:n if k is None else k].copy(), full.transforms[:n].copy(), e2t)


def same_table(got, exp, what):
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0]) if got.shape == exp.shape else -1
        raise AssertionError(f"{what}: the table is not the rule's; first difference at entry {at}: "
                             f"slots {got[at:at + 6].tolist()} where the rule puts {exp[at:at + 6].tolist()}")


class Mirror:
    """A context and the twin's tables side by side."""

    def __init__(self, vis, oracle):
        self.vis, self.oracle = vis, oracle
        self.seen = {}  # pool -> (epoch, table) as last fetched

    def _bind(self, sc, pools, lib_e2t):
        if sc is not None:
            self.sc = sc
            # (lib_e2t: a map that still names slots beyond the pool — the library must treat them as no slot; the oracle is given sc's)
            self.e2t = sc.entity_to_transform if lib_e2t is None else lib_e2t
            self.vis.bind_transforms(sc.transforms, self.e2t)
            if pools is None:
                pools = {0: sc.meshes}
        if pools is not None:
            self.pools = dict(pools)
            for pid, meshes in self.pools.items():
                self.vis.bind_pool(pid, meshes)

    def build(self, sc, pools=None, lib_e2t=None, parity=True):
        """Bind and build on the host."""
        self._bind(sc, pools, lib_e2t)
        self.vis.hierarchy_rebuild()
        tr = self.sc.transforms
        self.xt = rs.expected_table([], tr.shape[0], rs.codes(tr, self.e2t))
        self.tables = {pid: rs.built_mesh_table(self.xt, m["entity"], tr, self.e2t) for pid, m in self.pools.items()}
        self._observe("build", set(self.pools))
        if parity:
            self.check()

    def step(self, sc=None, pools=None, reorders=0, alone=(), sync="cull", lib_e2t=None, parity=True, what="step"):
        """Re-bind what is given (no rebuild request) and sync. reorders: re-orders of the transforms this sync must make (every
        pool then follows them); alone: pools whose own tail is due. Anything else is appended as it is."""
        before = self.vis.stats()["mirror_reorders"]
        self._bind(sc, pools, lib_e2t)
        if sync == "cull":
            self.vis.cull(0, [VIEW])
        else:
            self.vis.mirror_epoch(0)  # (syncs without a cull)
        assert self.vis.stats()["mirror_reorders"] - before == reorders, what
        tr = self.sc.transforms
        n1 = tr.shape[0]
        self.xt = rs.expected_table(self.xt, n1, rs.codes(tr, self.e2t) if reorders else np.zeros(n1, np.uint32))
        remade = set()
        for pid, m in self.pools.items():
            k1 = m.shape[0]
            if reorders or pid in alone or k1 != self.tables[pid].shape[0]:
                remade.add(pid)
            key = rs.mesh_keys(m["entity"], self.e2t, self.xt) if (reorders or pid in alone) else np.zeros(k1, np.uint32)
            self.tables[pid] = rs.expected_table(self.tables[pid], k1, key)
        self._observe(what, remade)
        if parity:
            self.check()

    def _observe(self, what, remade):
        """remade: the pools whose table this sync made anew (built, grown or re-ordered) — their epoch must have moved, whatever
        the new table is; a table that changed belongs to such a pool, and every other pool keeps table and epoch."""
        for pid, m in self.pools.items():
            table = self.vis.mirror_slots(pid, m.shape[0])
            epoch = self.vis.mirror_epoch(pid)
            same_table(table, self.tables[pid], f"{what}, pool {pid}")
            if pid in self.seen:
                old_epoch, old = self.seen[pid]
                assert (epoch != old_epoch) == (pid in remade), (what, pid, epoch, old_epoch)
                assert pid in remade or np.array_equal(table, old), (what, pid)
            self.seen[pid] = (epoch, table)

    def check(self):
        """One cull per pool: the mask shard decoded through the table as fetched is the oracle's visible set."""
        import torch
        from garden_amd.multi import expand_mask_rows, mask_words
        for pid, meshes in self.pools.items():
            k = meshes.shape[0]
            table = self.seen[pid][1]
            self.vis.cull(pid, [VIEW])
            shard = torch.full((1 + mask_words(k),), -1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()  # (the fill runs on torch's stream; the library's stream is non-blocking)
            self.vis.copy_mask_device(0, shard.data_ptr(), mask_words(k))
            self.vis.wait()
            exp = self.oracle.prepare_meshes(meshes.copy(), self.sc.transforms, self.sc.entity_to_transform, VIEW)
            slots, counts = expand_mask_rows(shard.view(1, -1), k, entry_tables=[table], index_bases=[0])
            assert counts.tolist() == [exp["draw_count"]], pid
            assert np.array_equal(slots, np.sort(exp["visible_idx"]).astype(np.int64)), pid


def live_codes(sc):
    c = rs.codes(sc.transforms, sc.entity_to_transform)
    return c, c[sc.transforms["entity"] != 0]


def no_live_entry_ties_with_the_free_slots(sc, c):
    """(A paired pool then shows the transforms' order after a re-order on the device too.)"""
    return not np.any(c[sc.transforms["entity"] != 0] == rs.FREE_CODE)


# ---- a. the host build is the twin ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "hier", "shuffled"])
def test_a_mirror_built_on_the_host_lies_in_morton_order_of_its_roots(gpu, oracle, kind):
    if kind == "flat":
        sc = scene.flat_scene(1200)
    elif kind == "hier":
        sc = scene.hierarchy_scene(5000, depth=4, fanout=5)
    else:
        sc = scene.shuffled_scene(scene.flat_scene(5000), fraction=1.0, drop_transforms=0.05)
    m = Mirror(gpu, oracle)
    m.build(sc)
    table = m.seen[0][1]
    if kind == "shuffled":  # the general mesh path: by the entry of the transform; meshes without one last, in slot order
        assert not rs.paired(sc.meshes["entity"], sc.transforms, sc.entity_to_transform)
        bare = np.flatnonzero(rs.slots_of(sc.meshes["entity"], sc.entity_to_transform, sc.count) == GV_NONE)
        assert bare.size > 200 and np.array_equal(table[-bare.size:], bare)
    else:  # paired: the transforms' own order — ascending codes
        assert rs.paired(sc.meshes["entity"], sc.transforms, sc.entity_to_transform)
        c, live = live_codes(sc)
        assert np.all(np.diff(c[table].astype(np.int64)) >= 0) and no_live_entry_ties_with_the_free_slots(sc, c)


# ---- b. the device re-order is the twin, at the size edges ---------------------------------------------------------------------

GROWTH = [(895, 1_024),        # the smallest pool the rule re-orders: (n1 - n0) * 8 > n1 and n1 >= 1024
          (3_580, 4_096),      # the sort's tile edge (kSortTileKeys) ...
          (3_580, 4_097),      # ... and one key past it
          (61_000, 70_000),    # past kRankOnlyMaxSlots
          (470_000, 540_000)]  # past the 2048 x 256 threads of reorder_roots_kernel's capped grid: grid-stride loop, block partials


@pytest.mark.parametrize("hier", [False, True])
@pytest.mark.parametrize("n0,n1", GROWTH)
def test_a_mirror_reordered_on_the_device_lies_as_the_rule_says(gpu, oracle, n0, n1, hier):
    assert (n1 - n0) * 8 > n1 >= 1024
    full = scene.hierarchy_scene(n1, depth=4, fanout=5) if hier else scene.flat_scene(n1)
    m = Mirror(gpu, oracle)
    m.build(cut(full, n0), parity=False)
    m.step(cut(full, n1), reorders=1)
    assert not np.array_equal(m.seen[0][1][n0:], np.arange(n0, n1))  # (the new slots went to their places)


@pytest.mark.parametrize("hier", [False, True])
def test_a_tail_of_exactly_one_eighth_is_appended_as_it_is(gpu, oracle, hier):
    full = scene.hierarchy_scene(1_024, depth=4, fanout=5) if hier else scene.flat_scene(1_024)
    m = Mirror(gpu, oracle)
    m.build(cut(full, 896))
    t0 = m.seen[0][1]
    m.step(cut(full, 1_024), reorders=0)
    assert np.array_equal(m.seen[0][1], np.concatenate([t0, np.arange(896, 1_024, dtype=np.uint32)]))


# ---- c. ties and stability -----------------------------------------------------------------------------------------------------

def family_order_holds(sc, table):
    """In the order `table` every live entry's parent precedes it and every tree is one run of entries."""
    n = sc.transforms.shape[0]
    at = np.empty(n, np.int64)
    at[table] = np.arange(n)
    live = sc.transforms["entity"] != 0
    up = rs.slots_of(sc.transforms["parent"], sc.entity_to_transform, n)
    kids = np.flatnonzero(live & (up != GV_NONE))
    assert np.all(at[up[kids]] < at[kids])
    root = rs.roots(sc.transforms, sc.entity_to_transform)
    lying = root[table][live[table]]
    assert 1 + np.count_nonzero(lying[1:] != lying[:-1]) == np.unique(lying).size
    return kids.size, np.unique(lying).size


@pytest.mark.parametrize("kind", ["lattice", "hier"])
def test_equal_codes_keep_the_order_they_lay_in(gpu, oracle, kind):
    """Many entries per code: only a STABLE sort gives the rule's table, keeps a tree together and its ancestors in front
    (gv_mirror.cpp: 'stable: trees stay contiguous, ancestors stay in front of their descendants')."""
    n0, n1 = 5_000, 5_800
    if kind == "lattice":  # roots snapped to a 4 x 4 x 4 lattice: at most 64 codes
        full = scene.flat_scene(n1)
        side = 100.0 * n1 ** (1.0 / 3.0)
        cell = np.random.Generator(np.random.PCG64(64)).integers(0, 4, (n1, 3))
        full.transforms["position"][:, :3] = ((cell - 1.5) * (side / 4.0)).astype(np.float32)
    else:  # one code per tree
        full = scene.hierarchy_scene(n1, depth=4, fanout=5)
    m = Mirror(gpu, oracle)
    for step, sc in enumerate((cut(full, n0), cut(full, n1))):
        if step == 0:
            m.build(sc)
        else:
            m.step(sc, reorders=1)
        c, live = live_codes(sc)
        kids, trees = family_order_holds(sc, m.seen[0][1])
        if kind == "lattice":  # (the lattice's far corner is cell 1023 three times: those entries tie with the free slots as well)
            assert np.unique(live).size <= 64
        else:
            # the pool pairs with its transforms and no live entry ties with the free slots: the table is the transforms' order
            assert rs.paired(sc.meshes["entity"], sc.transforms, sc.entity_to_transform) and no_live_entry_ties_with_the_free_slots(sc, c)
            own = rs.roots(sc.transforms, sc.entity_to_transform) == np.arange(sc.count)
            root_codes = c[own & (sc.transforms["entity"] != 0)]
            assert np.unique(root_codes).size == root_codes.size == trees  # (no two trees in one cell: a tree is one run of equal codes)
            assert kids > sc.count // 2 and np.unique(live).size == trees


# ---- d. codes come from current positions --------------------------------------------------------------------------------------

def test_codes_come_from_the_positions_as_they_are_at_the_reorder(gpu, oracle):
    n0, n1 = 5_000, 5_800
    full = scene.hierarchy_scene(n1, depth=2, fanout=3)  # 1450 roots, their children behind them
    rng = np.random.Generator(np.random.PCG64(41))
    live = np.flatnonzero(full.transforms["entity"][:n0] != 0)
    is_root = rs.roots(full.transforms, full.entity_to_transform)[live] == live
    roots_, kids = live[is_root], live[~is_root]
    m = Mirror(gpu, oracle)
    sc = cut(full, n0)
    m.build(sc)

    def move(tr, slots, by):
        tr["position"][slots, :3] += by
        for s in slots:
            gpu.mark_dirty(GV_DIRTY_TRANSFORM, int(s), 1)

    # a move without growth: nothing is re-ordered, the table and the epoch stay
    few = np.concatenate([rng.choice(roots_, 20, replace=False), rng.choice(kids, 20, replace=False)])
    move(sc.transforms, few, rng.normal(0, 300, (few.size, 3)).astype(np.float32))
    full.transforms[:n0] = sc.transforms
    epoch, table = m.seen[0]
    m.step(reorders=0, what="move without growth")
    assert m.seen[0][0] == epoch and np.array_equal(m.seen[0][1], table)

    # moves and growth in one sync: the codes are those of the new positions, inside the new box
    stale = rs.expected_table(m.xt, n1, rs.codes(full.transforms, full.entity_to_transform))
    movers = rng.choice(roots_, 40, replace=False)
    by = rng.normal(0, 400, (40, 3)).astype(np.float32)
    x = full.transforms["position"][roots_, 0]
    by[0] = (x.min() - 500.0 - full.transforms["position"][movers[0], 0], 0, 0)  # two roots stretch the box along x:
    by[1] = (x.max() + 500.0 - full.transforms["position"][movers[1], 0], 0, 0)  # every cell on that axis changes
    some_kids = rng.choice(kids, 30, replace=False)  # (children move inside their tree: their code must stay their root's)
    before = rs.codes(full.transforms, full.entity_to_transform)
    sc = cut(full, n1)
    gpu.bind_transforms(sc.transforms, sc.entity_to_transform)  # (the marks below are read from the pool as it is bound at the sync)
    move(sc.transforms, movers, by)
    move(sc.transforms, some_kids, rng.normal(0, 30, (30, 3)).astype(np.float32))
    after = rs.codes(sc.transforms, sc.entity_to_transform)
    still = np.setdiff1d(roots_, movers)
    assert np.count_nonzero(before[still] != after[still]) > still.size // 2  # the box moved under the roots that did not
    m.step(sc, reorders=1, what="moves and growth")
    assert not np.array_equal(m.seen[0][1], stale)  # (the positions of the build would have given another table)


# ---- e. degenerate inputs ------------------------------------------------------------------------------------------------------

E0, E1 = 1_100, 1_300


def test_roots_on_one_plane_have_no_extent_on_that_axis(gpu, oracle):
    full = scene.flat_scene(E1)
    full.transforms["position"][:, 0] = np.float32(12.5)
    assert not rs.cells(full.transforms, full.entity_to_transform)[0][:, 0].any()
    m = Mirror(gpu, oracle)
    m.build(cut(full, E0))
    m.step(cut(full, E1), reorders=1)


def test_non_finite_coordinates_stay_out_of_the_box_and_fall_into_cell_0(gpu, oracle):
    """(Table and counters only: what such an entity's visibility is, is another test's matter.)"""
    full = scene.flat_scene(E1)
    live = np.flatnonzero(full.transforms["entity"] != 0)
    odd = np.concatenate([live[live < E0][10:400:65], live[live >= E0][5:200:40]])  # in the part built on the host and in the tail
    for k, s in enumerate(odd):
        full.transforms["position"][s, k % 3] = (np.inf, -np.inf, np.nan)[(k // 3) % 3]
    q, _ = rs.cells(full.transforms, full.entity_to_transform)
    for k, s in enumerate(odd):
        assert q[s, k % 3] == 0
    fine = np.setdiff1d(live, odd)
    assert q[fine].max(axis=0).tolist() == [1023] * 3 and q[fine].min(axis=0).tolist() == [0] * 3  # (a box of finite corners)
    m = Mirror(gpu, oracle)
    m.build(cut(full, E0), parity=False)
    m.step(cut(full, E1), reorders=1, sync="table", parity=False)


@pytest.mark.parametrize("where", ["built", "appended"])
def test_one_live_root_among_free_slots(gpu, oracle, where):
    full = scene.flat_scene(E1, defects=False)
    seen = oracle.prepare_meshes(full.meshes.copy(), full.transforms, full.entity_to_transform, VIEW)["visible_idx"]
    one = int(seen[seen < E0][0] if where == "built" else seen[seen >= E0][0])  # (a visible one: the parity check sees a bit)
    gone = np.arange(E1) != one
    full.entity_to_transform[full.transforms["entity"][gone]] = GV_NONE
    full.transforms["entity"][gone] = 0
    full.meshes["entity"][gone] = 0
    m = Mirror(gpu, oracle)
    m.build(cut(full, E0))
    m.step(cut(full, E1), reorders=1)
    assert m.seen[0][1][0] == one and np.array_equal(m.seen[0][1][1:], np.delete(np.arange(E1), one))


def test_a_live_root_at_the_maximum_corner_ties_with_the_free_slots(gpu, oracle):
    """Cell 1023 on all three axes: code 0x3FFFFFFF, the code of the free slots. The transforms' sort leaves such an entry among
    the free slots where it lay; a pool built on the host takes that order as it is, a pool re-ordered on the device sorts by the
    entry of the transform, which puts the live mesh in front of the meshes of free slots — the twin states both."""
    full = scene.flat_scene(E1)
    live = full.transforms["entity"] != 0
    free = np.flatnonzero(~live)
    assert free[0] < 400 and np.any((free > 500) & (free < E0)) and np.any(free >= E0)
    corner = full.transforms["position"][live, :3].max(axis=0)
    old = int(np.flatnonzero(live[:E0])[450])    # free slots on both sides of it in the part built on the host
    new = int(np.flatnonzero(live)[-3])          # ... and one more in the tail
    assert free[0] < old < free[free < E0][-1] and new >= E0
    full.transforms["position"][[old, new], :3] = corner
    m = Mirror(gpu, oracle)
    for step, sc in enumerate((cut(full, E0), cut(full, E1))):
        c = rs.codes(sc.transforms, sc.entity_to_transform)
        assert c[old] == rs.FREE_CODE and (step == 0 or c[new] == rs.FREE_CODE)
        if step == 0:
            m.build(sc)
            tail = m.seen[0][1][-(np.count_nonzero(sc.transforms["entity"] == 0) + 1):]
            assert old in tail and tail[0] != old and tail[-1] != old and np.all(np.diff(tail.astype(np.int64)) > 0)  # slot order decided
        else:
            m.step(sc, reorders=1)


def test_a_chain_ends_at_a_child_whose_parent_slot_is_free(gpu, oracle):
    full = scene.hierarchy_scene(E1, depth=3, fanout=3)
    tr = full.transforms
    parents = np.unique(rs.slots_of(tr["parent"], full.entity_to_transform, E1))
    parents = parents[parents != GV_NONE]
    # roots and inner nodes (the last ones with children in the tail); their children keep the link
    gone = np.concatenate([parents[3:60:7], parents[parents >= 120][:40:5], parents[parents >= 340][:40:5]])
    orphans = np.flatnonzero(np.isin(rs.slots_of(tr["parent"], full.entity_to_transform, E1), gone))
    full.entity_to_transform[tr["entity"][gone]] = GV_NONE
    tr["entity"][gone] = 0
    full.meshes["entity"][gone] = 0
    root = rs.roots(tr, full.entity_to_transform)
    assert orphans.size > 20 and np.all(tr["parent"][orphans] != 0) and np.array_equal(root[orphans], orphans)
    assert np.any(orphans < E0) and np.any(orphans >= E0)
    m = Mirror(gpu, oracle)
    m.build(cut(full, E0))
    m.step(cut(full, E1), reorders=1)


def test_parents_beyond_the_pool_are_no_parents(gpu, oracle):
    """The entity map still names slots beyond the bound pool (the library must take them for no slot; the oracle is given a map
    without them). Parents that never arrive leave their children roots; parents that arrive with the growth are reported like
    any other change of a link (GV_DIRTY_HIERARCHY), and the children then sort with their parent's tree."""
    full = scene.flat_scene(1_500)
    tr = full.transforms
    live = np.flatnonzero(tr["entity"] != 0)
    kids = live[live < E0]
    late, never = kids[20:60:2], kids[100:140:2]
    tr["parent"][late] = tr["entity"][live[(live >= E0) & (live < E1)][:late.size]]
    tr["parent"][never] = tr["entity"][live[live >= E1 + 50][:never.size]]
    tr["position"][np.concatenate([late, never]), :3] *= np.float32(0.01)  # (local positions: near their parents)
    m = Mirror(gpu, oracle)
    sc = cut(full, E0)
    assert np.array_equal(rs.roots(sc.transforms, full.entity_to_transform)[late], late)
    m.build(sc, lib_e2t=full.entity_to_transform)
    sc = cut(full, E1)
    root = rs.roots(sc.transforms, full.entity_to_transform)
    assert np.all(root[late] >= E0) and np.array_equal(root[never], never)
    gpu.bind_transforms(sc.transforms, full.entity_to_transform)
    for s in late:
        gpu.mark_dirty(GV_DIRTY_HIERARCHY, int(s), 1)
    m.step(sc, reorders=1, lib_e2t=full.entity_to_transform)
    at = np.empty(E1, np.int64)
    at[m.seen[0][1]] = np.arange(E1)
    # trees of two, no two in one cell; the sort is stable: the child lay in front of the parent that arrived after it
    assert np.all(at[root[late]] == at[late] + 1)


# ---- f. a mesh pool re-ordered alone -------------------------------------------------------------------------------------------

def test_a_mesh_pool_whose_own_tail_is_due_is_sorted_by_its_transforms_entries(gpu, oracle):
    full = scene.hierarchy_scene(7_000, depth=4, fanout=5)
    x0, x1, k0, k1 = 6_000, 7_000, 4_000, 4_600
    sc = cut(full, x0, k0)
    third = full.meshes[:x0:3].copy()  # another mesh system over the same transforms
    m = Mirror(gpu, oracle)
    m.build(sc, pools={0: sc.meshes, 1: third})
    # pool 0 grows past 1/8 of itself, the transforms stay: that pool alone, by the entries its transforms have now
    epoch1 = m.seen[1][0]
    grown = full.meshes[:k1].copy()
    m.step(pools={0: grown, 1: third}, reorders=0, alone=(0,), what="pool 0 alone")
    assert m.seen[1][0] == epoch1
    t0 = m.seen[0][1]
    assert not np.array_equal(t0[k0:], np.arange(k0, k1))
    keys = rs.mesh_keys(grown["entity"], sc.entity_to_transform, m.xt)[t0]
    assert np.all(np.diff(keys.astype(np.int64)) >= 0)
    # the transforms grow past 1/8: both pools follow them, each from the order it lay in
    m.step(cut(full, x1, k1), pools={0: grown, 1: third}, reorders=1, what="both pools follow")
    for pid, meshes in m.pools.items():
        keys = rs.mesh_keys(meshes["entity"], m.e2t, m.xt)[m.seen[pid][1]]
        assert np.all(np.diff(keys.astype(np.int64)) >= 0)


# ---- g. device and host agree where there are no ties --------------------------------------------------------------------------

def test_without_ties_the_device_and_the_host_give_the_same_mirror(gpu_bounds, oracle):
    """No two live slots share a code and none has the free slots' code: the order does not depend on how the entries lay, so a
    rebuild on the host after the re-order on the device leaves the table as it is (the epoch moves: the mirror was rebuilt). The
    two mirrors are then the same bytes, and the same view examines the same blocks through their boxes. Boxes are derived when a
    pool is at rest — after a change, the cull that follows a quiet one (gv_context.cpp may_rebuild_at) — so each side culls
    three times and the third is counted."""
    gpu = gpu_bounds
    n0, n1 = 5_000, 5_800
    for seed in range(scene.SEED + 700, scene.SEED + 732):  # (perturbed until the twin shows no tie: ~1 % of the seeds have one)
        full = scene.flat_scene(n1, seed=seed)
        c, live = live_codes(full)
        if np.unique(live).size == live.size and not np.any(live == rs.FREE_CODE):
            break
    else:
        raise AssertionError("no tie-free scene among 32 seeds")
    m = Mirror(gpu, oracle)
    m.build(cut(full, n0), parity=False)
    sc = cut(full, n1)

    def examined():
        m.check()
        gpu.cull(0, [VIEW])
        gpu.stats_reset()
        gpu.cull(0, [VIEW])
        gpu.wait()
        st = gpu.stats()
        assert st["bounds_blocks_total"] == (n1 + 255) // 256
        return st["bounds_blocks_examined"], st["bounds_blocks_total"]

    m.step(sc, reorders=1, sync="table", parity=False)
    device_table = m.seen[0][1]
    on_device = examined()
    m.build(sc, parity=False)  # (asserts the twin's table and that the epoch moved)
    assert m.seen[0][1].tobytes() == device_table.tobytes()
    assert examined() == on_device
