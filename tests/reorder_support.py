"""A plain twin of the mirror's ordering rule (gv_mirror.cpp build_transform_order / build_mesh_order on the host,
gv_reorder.hip + the radix sort on bare keys on the device): numpy, float32 throughout, no tolerance anywhere. The library is
built with correctly rounded float division and without contraction, so the same few IEEE single-precision operations give
the same bits on both sides and the expected entry -> slot table can be stated exactly.

Known answers worked out by hand: tests/test_reorder_twin.py."""
import numpy as np

GV_NONE = 0xFFFFFFFF
FREE_CODE = 0x3FFFFFFF  # free transform slots, and meshes without a transform: last


def spread10(v):
    """10 bits -> every third bit."""
    v = np.asarray(v, dtype=np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def slots_of(entities, entity_to_transform, n):
    """Transform slot of every entity id (GV_NONE: id 0 / GV_NONE / beyond the map, no slot, or a slot >= n)."""
    entities = np.asarray(entities, dtype=np.uint32)
    e2t = np.asarray(entity_to_transform, dtype=np.uint32)
    out = np.full(entities.shape[0], GV_NONE, dtype=np.uint32)
    known = (entities != 0) & (entities < e2t.shape[0])
    out[known] = e2t[entities[known]]
    out[out >= n] = GV_NONE
    return out


def roots(transforms, entity_to_transform):
    """Root ancestor (a slot) of every transform slot: follow `parent` until it names no slot below n."""
    n = transforms.shape[0]
    up = slots_of(transforms["parent"], entity_to_transform, n)
    root = np.arange(n, dtype=np.uint32)
    for _ in range(n + 1):
        step = up[root]
        more = step != GV_NONE
        if not more.any():
            return root
        root[more] = step[more]
    raise ValueError("the hierarchy has a cycle")


def cells(transforms, entity_to_transform):
    """(q[n, 3], root[n]): the 10-bit cell per axis of every slot's root position inside the box of the live roots."""
    n = transforms.shape[0]
    root = roots(transforms, entity_to_transform)
    pos = np.ascontiguousarray(transforms["position"][:, :3], dtype=np.float32)
    own = (root == np.arange(n)) & (transforms["entity"] != 0)
    q = np.zeros((n, 3), dtype=np.uint32)
    with np.errstate(all="ignore"):
        for k in range(3):
            boxed = pos[own, k]
            boxed = boxed[np.isfinite(boxed)]
            lo = boxed.min() if boxed.size else np.float32(np.inf)
            hi = boxed.max() if boxed.size else np.float32(-np.inf)
            ext = np.float32(hi - lo)
            p = pos[root, k]
            if ext > 0:
                f = np.where(np.isfinite(p), (p - lo) / ext, np.float32(0)).astype(np.float32)
            else:
                f = np.zeros(n, dtype=np.float32)
            q[:, k] = np.fmin(np.float32(1023), np.fmax(np.float32(0), f * np.float32(1024))).astype(np.uint32)  # (fminf / fmaxf)
    return q, root


def codes(transforms, entity_to_transform):
    """One uint32 per transform slot: the 30-bit Morton code of its root's cell; free slots get FREE_CODE."""
    q, _ = cells(transforms, entity_to_transform)
    c = spread10(q[:, 0]) | (spread10(q[:, 1]) << np.uint32(1)) | (spread10(q[:, 2]) << np.uint32(2))
    c[transforms["entity"] == 0] = FREE_CODE
    return c.astype(np.uint32)


def expected_table(previous_table, n1, key):
    """The entry -> slot table after a stable sort by `key` (per slot) of the mirror as it lies: the previous order with the
    slots appended since at its tail, in slot order. (A build from nothing: an empty previous table.)"""
    previous_table = np.asarray(previous_table, dtype=np.uint32)
    lies = np.concatenate([previous_table, np.arange(previous_table.shape[0], n1, dtype=np.uint32)])
    return lies[np.argsort(np.asarray(key)[lies], kind="stable")]


def mesh_keys(mesh_entities, entity_to_transform, transform_table):
    """A mesh sorts by the mirror entry of its transform (the inverse of the transform order); without one, last."""
    table = np.asarray(transform_table, dtype=np.uint32)
    entry_of = np.empty(table.shape[0], dtype=np.uint32)
    entry_of[table] = np.arange(table.shape[0], dtype=np.uint32)
    slot = slots_of(mesh_entities, entity_to_transform, table.shape[0])
    key = np.full(slot.shape[0], FREE_CODE, dtype=np.uint32)
    key[slot != GV_NONE] = entry_of[slot[slot != GV_NONE]]
    return key


def paired(mesh_entities, transforms, entity_to_transform):
    """Mesh slot i <-> transform slot i, or no transform and a free transform slot: a build gives such a pool its transforms'
    table as it is."""
    n = transforms.shape[0]
    if mesh_entities.shape[0] != n:
        return False
    slot = slots_of(mesh_entities, entity_to_transform, n)
    return bool(np.all((slot == np.arange(n)) | ((slot == GV_NONE) & (transforms["entity"] == 0))))


def built_mesh_table(transform_table, mesh_entities, transforms, entity_to_transform):
    """The table of a mesh pool built from nothing over transforms that lie in `transform_table`."""
    if paired(mesh_entities, transforms, entity_to_transform):
        return np.array(transform_table, dtype=np.uint32)
    return expected_table(np.zeros(0, np.uint32), mesh_entities.shape[0], mesh_keys(mesh_entities, entity_to_transform, transform_table))


def built_tables(transforms, entity_to_transform, mesh_entities):
    """(transform table, mesh table) of a mirror built from nothing."""
    xt = expected_table(np.zeros(0, np.uint32), transforms.shape[0], codes(transforms, entity_to_transform))
    return xt, built_mesh_table(xt, mesh_entities, transforms, entity_to_transform)
