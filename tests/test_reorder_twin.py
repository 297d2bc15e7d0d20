"""Known answers, worked out by hand, for the plain twin of the mirror's ordering rule (tests/reorder_support.py). The GPU
tests (tests/test_gpu_mirror_order.py) take the twin's tables as the truth; these pin the twin itself. No GPU."""
import numpy as np

from garden_amd.pools import TRANSFORM_DTYPE
from reorder_support import FREE_CODE, GV_NONE, built_tables, cells, codes, expected_table, mesh_keys, paired, roots, spread10


def world(positions, parents=None, free=()):
    """Slot i holds entity i + 1 at positions[i]; parents[i]: a parent SLOT or None; free: slots without an entity."""
    n = len(positions)
    tr = np.zeros(n, dtype=TRANSFORM_DTYPE)
    tr["entity"] = np.arange(1, n + 1)
    tr["position"][:, :3] = np.asarray(positions, dtype=np.float32)
    for i, p in enumerate(parents or []):
        if p is not None:
            tr["parent"][i] = p + 1
    e2t = np.full(n + 1, GV_NONE, dtype=np.uint32)
    e2t[1:] = np.arange(n)
    for s in free:
        e2t[tr["entity"][s]] = GV_NONE
        tr["entity"][s] = 0
    return tr, e2t


def test_spread10_puts_bit_k_at_bit_3k():
    assert spread10(0) == 0
    assert spread10(1) == 1
    assert spread10(0x3FF) == 0x09249249
    assert spread10(0x2AA) == 0x08208208  # bits 1 3 5 7 9 -> bits 3 9 15 21 27
    assert spread10(np.array([1, 2, 512], np.uint32)).tolist() == [1, 8, 1 << 27]


BELOW_512 = np.nextafter(np.float32(512), np.float32(0))  # 511.99997: one float below the edge of cell 512
SCENE = dict(
    # x: box [0, 1024] (f * 1024 = x exactly); y: every root at 7 (zero extent); z: box [0, 1024], one +inf left out of it
    positions=[(0, 7, 0), (1024, 7, 1024), (BELOW_512, 7, 512), (512, 7, np.inf), (5000, -5000, 5000), (np.nan, 7, 256),
               (9999, -5, 9999), (-9999, 70, -9999)],
    parents=[None, None, None, None, None, None, 2, 6],  # slot 6 under slot 2, slot 7 under slot 6: a chain of three
    free=(4,))


def test_cells_at_the_box_edges_on_a_flat_axis_and_for_non_finite_coordinates():
    tr, e2t = world(**SCENE)
    q, root = cells(tr, e2t)
    assert root.tolist() == [0, 1, 2, 3, 4, 5, 2, 2]
    assert q[0].tolist() == [0, 0, 0]          # at lo
    assert q[1].tolist() == [1023, 0, 1023]    # at hi: 1024 clamps to 1023
    assert q[2].tolist() == [511, 0, 512]      # one float below the edge / on the edge
    assert q[3].tolist() == [512, 0, 0]        # +inf: outside the box, cell 0
    assert q[5].tolist() == [0, 0, 256]        # NaN: cell 0
    assert q[6].tolist() == q[7].tolist() == q[2].tolist()  # (the children's own positions widen no box)


def test_codes_interleave_x_y_z_and_a_chain_shares_its_roots_code():
    tr, e2t = world(**SCENE)
    c = codes(tr, e2t)
    assert c.dtype == np.uint32
    assert c.tolist() == [0, 0x2DB6DB6D, 0x21249249, 0x08000000, FREE_CODE, 0x04000000, 0x21249249, 0x21249249]
    assert expected_table(np.zeros(0, np.uint32), 8, c).tolist() == [0, 5, 3, 2, 6, 7, 1, 4]
    # y alone: bit k of the cell lands on bit 3k + 1
    tr, e2t = world([(0, 0, 0), (0, 1024, 0), (0, 3, 0)])
    assert codes(tr, e2t).tolist() == [0, 0x12492492, 0b010010]


def test_a_live_root_at_the_maximum_corner_ties_with_the_free_slots():
    tr, e2t = world([(9, 9, 9), (1, 1, 1), (0, 0, 0), (4, 4, 4)], free=(0, 3))
    c = codes(tr, e2t)
    assert c.tolist() == [FREE_CODE, 0x3FFFFFFF, 0, FREE_CODE]
    assert expected_table(np.zeros(0, np.uint32), 4, c).tolist() == [2, 0, 1, 3]  # slot order decides among the three


def test_chains_end_at_free_parents_and_at_parents_beyond_the_cut():
    tr, e2t = world([(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3)], parents=[None, None, 1, 2], free=(1,))
    assert roots(tr, e2t).tolist() == [0, 1, 2, 2]  # slot 2's parent is gone: the chain ends at slot 2
    assert roots(tr[:2].copy(), e2t).tolist() == [0, 1]
    tr, e2t = world([(0, 0, 0), (1, 1, 1), (2, 2, 2)], parents=[2, 0, None])
    assert roots(tr, e2t).tolist() == [2, 2, 2]
    assert roots(tr[:2].copy(), e2t).tolist() == [0, 0]  # slot 0's parent lies beyond the cut


def test_one_live_root_and_an_empty_world_have_no_extent():
    tr, e2t = world([(5, 6, 7), (1, 2, 3), (9, 9, 9)], free=(0, 2))
    assert codes(tr, e2t).tolist() == [FREE_CODE, 0, FREE_CODE]
    tr, e2t = world([(5, 6, 7), (1, 2, 3)], free=(0, 1))
    assert codes(tr, e2t).tolist() == [FREE_CODE, FREE_CODE]


def test_expected_table_sorts_the_mirror_as_it_lies_with_the_new_slots_at_its_tail():
    assert expected_table([2, 0, 1], 5, [5, 1, 5, 0, 1]).tolist() == [3, 1, 4, 2, 0]
    assert expected_table([2, 0, 1], 3, [0, 0, 0]).tolist() == [2, 0, 1]  # all equal: stays as it lies
    assert expected_table([], 3, [0, 0, 0]).tolist() == [0, 1, 2]


def test_mesh_keys_are_the_entries_of_the_transforms():
    e2t = np.array([GV_NONE, 0, 1, 2], np.uint32)
    keys = mesh_keys(np.array([2, 0, 1, 9, 3], np.uint32), e2t, [2, 0, 1])  # slot 0 -> entry 1, slot 1 -> entry 2, slot 2 -> entry 0
    assert keys.tolist() == [2, FREE_CODE, 1, FREE_CODE, 0]
    assert expected_table([], 5, keys).tolist() == [4, 2, 0, 1, 3]
    assert mesh_keys(np.array([3], np.uint32), e2t, [1, 0]).tolist() == [FREE_CODE]  # a transform slot beyond the table


def test_a_paired_pool_takes_its_transforms_table():
    tr, e2t = world([(9, 9, 9), (1, 1, 1), (0, 0, 0), (4, 4, 4)], free=(0, 3))
    ents = tr["entity"].copy()
    assert paired(ents, tr, e2t)
    xt, mt = built_tables(tr, e2t, ents)
    assert xt.tolist() == mt.tolist() == [2, 0, 1, 3]
    swapped = ents[[0, 2, 1, 3]].copy()  # meshes 1 and 2 belong to each other's transforms: the general rule
    assert not paired(swapped, tr, e2t)
    xt, mt = built_tables(tr, e2t, swapped)
    assert xt.tolist() == [2, 0, 1, 3] and mt.tolist() == [1, 2, 0, 3]
