"""Test helpers of the world-matrix chain (calc_model -> mul_affine / mfma_chain_step -> model_rows; the five kernel forms of
garden_amd/csrc/gv_sweep.hip and the cull, emit and sphere-stream kernels that reuse the chain): world builders that put numeric
extremes, deep chains and chosen lane patterns in front of it, and the comparator of its bit contract. TEST INFRASTRUCTURE ONLY.

tests/test_sweep_census.py proves on the CPU, with the oracle alone, that these worlds hold what they are meant to hold (and not
so many NaN rows that the comparator's NaN clause could hide a failure); tests/test_gpu_sweep_forms.py runs them on the GPU.
Builders are pure numpy and deterministic from their arguments. They return scene.Scene; edge_world and sphere_world add the
attribute `planted` (bool per transform slot: the slot itself carries an extreme)."""
import numpy as np

from garden_amd import scene
from garden_amd.pools import GV_NONE, MESH_DTYPE, TRANSFORM_DTYPE

F32 = np.float32
EDGE_SPREAD = 60.0  # sigma of the positions of an edge world
# (transform count, seed) of the edge worlds the GPU tests use; the census pools its floors over exactly these
EDGE_WORLDS = [(257, 0), (257, 1), (1000, 0), (1000, 1), (4099, 0), (4099, 1)]
DEEP_LENGTH = 300
DEEP_SCALES = [0.6, 1.6, 1.0]
SPHERE_N = 70_001  # flat, exactly paired, above kHotMinSlots: culled from the sphere stream
# tile edges of the sweep forms: 64 slots per wave, 192 / 768 float4 per stage, 256 slots per workgroup
TILE_COUNTS = [1, 2, 63, 64, 65, 191, 192, 193, 255, 256, 257, 511, 512, 513, 769]
TILE_MESH_ENDS = [(513, 200), (300, 257), (257, 65), (769, 1)]  # the mesh pool ends in an earlier wave / workgroup: sweep-only lanes
TILE_UNPAIRED = (257, 300)

# the planted classes: (name, share of the slots). COMMON ones underflow, lose a sign or a rank; RARE ones overflow or are not
# finite, and poison every descendant (0 * inf in the columns of the product)
COMMON, RARE = 0.03, 0.004
CLASSES = [("scale_1e-20", COMMON), ("position_3e-41", COMMON), ("scale_1e-45", COMMON), ("position_minus_zero", COMMON),
           ("scale_zero", COMMON), ("scale_negated", COMMON), ("quat_1e-10", COMMON), ("quat_zero", COMMON),
           ("scale_3e19", RARE), ("position_-3e38", RARE), ("position_inf", RARE), ("quat_nan", RARE)]


def same_floats(got, exp):
    """The bit contract of world matrices and records: elementwise `bits equal OR both NaN`. Returns the flat
    indices that break it (empty: the arrays agree). The NaN clause is not a tolerance: an invalid operation (0 * inf, inf - inf)
    yields 0xFFC00000 on x86 and a positive quiet NaN on the GPU, so the bits of a NaN born inside the chain cannot be compared;
    finite values, subnormals, +-0 and +-inf are compared bit for bit."""
    got, exp = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(exp, dtype=np.float32)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    ok = (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))
    return np.flatnonzero(~ok)


def plant(tr, slot, cls, rng):
    """writes the extreme of class `cls` (an index into CLASSES) into transform slot `slot`"""
    name = CLASSES[cls][0]
    axis = int(rng.integers(0, 3))
    if name == "scale_1e-20":
        tr["scale"][slot, :3] = F32(1e-20)
    elif name == "position_3e-41":
        tr["position"][slot, axis] = F32(3e-41)
    elif name == "scale_1e-45":
        tr["scale"][slot, axis] = F32(1e-45)
    elif name == "position_minus_zero":
        tr["position"][slot, :3] = F32(-0.0)
    elif name == "scale_zero":
        tr["scale"][slot, :3] = F32(0.0)
    elif name == "scale_negated":
        tr["scale"][slot, axis] = -tr["scale"][slot, axis]
    elif name == "quat_1e-10":
        tr["rotation"][slot] = tr["rotation"][slot] * F32(1e-10)
    elif name == "quat_zero":
        tr["rotation"][slot] = F32(0.0)
    elif name == "scale_3e19":
        tr["scale"][slot, axis] = F32(3e19)
    elif name == "position_-3e38":
        tr["position"][slot, axis] = F32(-3e38)
    elif name == "position_inf":
        tr["position"][slot, axis] = F32(np.inf)
    elif name == "quat_nan":
        tr["rotation"][slot, int(rng.integers(0, 4))] = F32(np.nan)
    else:
        raise AssertionError(name)


def plant_classes(tr, rng, share=1.0):
    """every slot draws at most one class, class k with probability share * CLASSES[k][1]; returns the class per slot (-1: none)"""
    n = tr.shape[0]
    u = rng.random(n)
    cls = np.full(n, -1, np.int32)
    lo = 0.0
    for k, (_name, p) in enumerate(CLASSES):
        cls[(u >= lo) & (u < lo + share * p)] = k
        lo += share * p
    for s in np.flatnonzero(cls >= 0):
        plant(tr, int(s), int(cls[s]), rng)
    return cls


def _unit_quats(rng, n):
    q = rng.normal(0, 1, (n, 4)).astype(np.float32)
    q /= np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-6).astype(np.float32)
    return q


def _entity_map(tr, capacity):
    e2t = np.full(capacity, GV_NONE, np.uint32)
    live = tr["entity"] != 0
    e2t[tr["entity"][live]] = np.nonzero(live)[0].astype(np.uint32)
    return e2t


def _boxes(rng, meshes, tiny=0.0, huge=0.0, nan=0.0):
    """boxes as tests/test_gpu_fuzz.py draws them, `tiny` of them with the extent 1e-42 (subnormal), `huge` with 3e18 and `nan` with
    one NaN coordinate (the sphere pre-test must leave such a box to the exact test, which cannot reject it)"""
    n = meshes.shape[0]
    h = np.exp(rng.normal(-0.5, 0.8, (n, 3))).astype(np.float32)
    c = rng.normal(0, 0.5, (n, 3)).astype(np.float32)
    u = rng.random(n)
    small, big = u < tiny, (u >= tiny) & (u < tiny + huge)
    c[small | big] = 0
    h[small] = F32(1e-42)
    h[big] = F32(3e18)
    meshes["aabbMin"][:, :3] = c - h
    meshes["aabbMax"][:, :3] = c + h
    meshes["aabbMax"][(u >= tiny + huge) & (u < tiny + huge + nan), 0] = F32(np.nan)
    meshes["isEnabled"] = 1
    meshes["isVisible"] = 7


def edge_world(n, seed):
    """A forest of `n` transforms with planted extremes and an exactly paired mesh pool. Base values as tests/test_gpu_fuzz.py's
    random_world; 85 % of the slots take a parent from the 8 slots below them (a chain ends at one of the other 15 %, after ~7
    links on average, so a non-finite slot poisons a subtree and not the pool), 10 % have modelWithAncestors = 0."""
    rng = np.random.Generator(np.random.PCG64(0xED6E + 1000 * n + seed))
    tr = np.zeros(n, TRANSFORM_DTYPE)
    tr["entity"] = rng.permutation(np.arange(1, n + 1, dtype=np.uint32))
    tr["position"][:, :3] = rng.normal(0, EDGE_SPREAD, (n, 3)).astype(np.float32)
    tr["scale"][:, :3] = np.exp(rng.normal(0, 0.6, (n, 3))).astype(np.float32)
    tr["rotation"] = _unit_quats(rng, n)
    tr["rotation"][rng.random(n) < 0.1] = (0, 0, 0, 1)
    tr["selfActive"] = (rng.random(n) > 0.04).astype(np.uint8)
    tr["ancestorsActive"] = (rng.random(n) > 0.03).astype(np.uint8)
    tr["modelWithAncestors"] = (rng.random(n) > 0.1).astype(np.uint8)
    chained = rng.random(n) < 0.85
    below = rng.integers(1, 9, n)
    for s in range(1, n):
        if chained[s]:
            tr["parent"][s] = tr["entity"][max(0, s - int(below[s]))]
    cls = plant_classes(tr, rng)
    free = (rng.random(n) < 0.02) & (cls < 0)
    tr["entity"][free] = 0  # (a child of a freed slot keeps the id: it no longer resolves, the chain ends there)
    meshes = np.zeros(n, MESH_DTYPE)
    meshes["entity"] = tr["entity"]
    _boxes(rng, meshes, tiny=0.03, huge=0.01, nan=0.005)
    sc = scene.Scene(meshes, tr, _entity_map(tr, n + 1))
    sc.planted = cls >= 0
    return sc


def deep_world(length, scale):
    """One chain: a root and length - 1 descendants, each the child of the slot before it; random unit quaternions, positions
    N(0, 3), the uniform scale `scale` in every link (the product walks smoothly down through the subnormal range, or up to
    overflow). Meshes are paired."""
    rng = np.random.Generator(np.random.PCG64(0xDEE9 + length))
    tr = np.zeros(length, TRANSFORM_DTYPE)
    tr["entity"] = np.arange(1, length + 1, dtype=np.uint32)
    tr["parent"][1:] = tr["entity"][:-1]
    tr["position"][:, :3] = rng.normal(0, 3, (length, 3)).astype(np.float32)
    tr["scale"][:, :3] = F32(scale)
    tr["rotation"] = _unit_quats(rng, length)
    tr["selfActive"] = tr["ancestorsActive"] = tr["modelWithAncestors"] = 1
    meshes = np.zeros(length, MESH_DTYPE)
    meshes["entity"] = tr["entity"]
    _boxes(rng, meshes)
    return scene.Scene(meshes, tr, _entity_map(tr, length + 1))


def tile_depth(slot):
    """the chain depth tile_world gives slot `slot` before its exceptions"""
    if slot < 64:
        return 0                      # wave 0: roots only
    if slot < 128:
        return int(slot == 127)       # wave 1: one chained entry, in lane 63
    if slot < 192:
        return int(slot == 128)       # wave 2: one chained entry, in lane 0
    return slot % 8                   # later waves: depths 0 .. 7, lane by lane


def tile_world(nt, nm, seed):
    """Benign numbers, placed for lanes (meant for the slot-order context, where mirror entry = pool slot = lane): see tile_depth.
    A slot of depth d hangs below a slot of depth d - 1: the slot before it, or — every fifth — one at a HIGHER slot in another
    workgroup. Exceptions: one dangling parent id (past the entity map), one parent id whose slot was freed, a few free slots,
    a few slots with modelWithAncestors = 0. The mesh pool's first min(nm, nt) entities are the transform pool's (exactly paired
    when nm <= nt); entries past nt repeat entities of other slots."""
    rng = np.random.Generator(np.random.PCG64(0x711E + 4096 * nt + nm + 7 * seed))
    tr = np.zeros(nt, TRANSFORM_DTYPE)
    tr["entity"] = rng.permutation(np.arange(1, nt + 1, dtype=np.uint32))
    tr["position"][:, :3] = rng.normal(0, 30.0, (nt, 3)).astype(np.float32)
    tr["scale"][:, :3] = rng.uniform(0.5, 2.0, (nt, 3)).astype(np.float32)
    tr["rotation"] = _unit_quats(rng, nt)
    tr["selfActive"] = tr["ancestorsActive"] = tr["modelWithAncestors"] = 1
    tr["position"][0, :3] = (1.0, 2.0, 3.0)  # inside tile_view(): the pools of one and two slots show something too
    for s in range(nt):
        d = tile_depth(s)
        if d == 0:
            continue
        p = s - 1 if s >= 192 else s % 64  # waves 1 and 2 hang below a root of wave 0
        far = s - 1 + 8 * 40               # same depth as s - 1, 320 slots up: another workgroup
        if s >= 192 and s % 5 == 0 and far < nt:
            p = far
        assert tile_depth(p) == d - 1
        tr["parent"][s] = tr["entity"][p]
    if nt > 203:
        tr["parent"][203] = nt + 7  # dangling: an id past the entity map
    for s in (5, 200, 300, 522):    # free slots; 200 and 300 are parents (of 201 and 301): those chains end at an id without a slot
        if s < nt:
            tr["entity"][s] = 0
    for s in (197, 261, 518):
        if s < nt:
            tr["modelWithAncestors"][s] = 0
    meshes = np.zeros(nm, MESH_DTYPE)
    k = min(nm, nt)
    meshes["entity"][:k] = tr["entity"][:k]
    if nm > nt:
        meshes["entity"][nt:] = tr["entity"][(np.arange(nt, nm) * 7) % nt]
    _boxes(rng, meshes)
    return scene.Scene(meshes, tr, _entity_map(tr, nt + 1))


def sphere_world():
    """scene.flat_scene(SPHERE_N) with the classes of edge_world in 2 % of the slots (no parents), boxes of extent 1e-42 and 3e18,
    boxes with a NaN coordinate and positions +-3e38: what the sphere stream stores of them is a subnormal radius, one that overflows from finite inputs, a
    reach whose magnitude overflows"""
    sc = scene.flat_scene(SPHERE_N)
    rng = np.random.Generator(np.random.PCG64(0x5F3E))
    cls = plant_classes(sc.transforms, rng, share=0.02 / sum(p for _n, p in CLASSES))
    u = rng.random(SPHERE_N)
    small, big = u < 0.005, (u >= 0.005) & (u < 0.01)
    for mask, h in ((small, F32(1e-42)), (big, F32(3e18))):
        sc.meshes["aabbMin"][mask, :3] = -h
        sc.meshes["aabbMax"][mask, :3] = h
    far = np.flatnonzero((u >= 0.01) & (u < 0.015))
    sc.transforms["position"][far, far % 3] = np.where(far % 2 == 0, F32(3e38), F32(-3e38))
    sc.meshes["aabbMin"][(u >= 0.015) & (u < 0.018), 1] = F32(np.nan)
    sc.planted = (cls >= 0) | (u < 0.018)
    return sc


def replant(sc, slots, rng, first_class=0):
    """fresh extremes, one class after the other, into `slots` (a benign TRS first, so that classes do not pile up)"""
    tr = sc.transforms
    for k, s in enumerate(slots):
        s = int(s)
        tr["position"][s, :3] = rng.normal(0, 20.0, 3).astype(np.float32)
        tr["scale"][s, :3] = rng.uniform(0.5, 2.0, 3).astype(np.float32)
        tr["rotation"][s] = _unit_quats(rng, 1)[0]
        plant(tr, s, (first_class + k) % len(CLASSES), rng)


def interior_slots(sc):
    """slots that are the parent of at least one other slot"""
    e2t = np.asarray(sc.entity_to_transform)
    par = sc.transforms["parent"]
    ok = (par != 0) & (par < e2t.shape[0])
    slots = e2t[par[ok]]
    return np.unique(slots[slots != GV_NONE])


def planted_closure(sc):
    """bool per transform slot: the slot or one of the ancestors its model is built from is planted"""
    tr, e2t = sc.transforms, np.asarray(sc.entity_to_transform)
    out = sc.planted.copy()
    for s in range(tr.shape[0]):
        if out[s] or not tr["modelWithAncestors"][s]:
            continue
        p = int(tr["parent"][s])
        while p and p < e2t.shape[0] and e2t[p] != GV_NONE:
            ps = int(e2t[p])
            if sc.planted[ps]:
                out[s] = True
                break
            p = int(tr["parent"][ps])
    return out


def row_census(world):
    """per-row classes of an [n, 12] world-matrix array: dict of bool arrays"""
    bits = world.view(np.uint32)
    mag = bits & np.uint32(0x7FFFFFFF)
    return dict(nan=np.isnan(world).any(axis=1), finite=np.isfinite(world).all(axis=1), inf=np.isinf(world).any(axis=1),
                subnormal=((mag != 0) & (mag < np.uint32(0x00800000))).any(axis=1),
                minus_zero=(bits == np.uint32(0x80000000)).any(axis=1),
                zero3x3=(mag[:, :9] == 0).all(axis=1))


# ---- the views the GPU tests cull with (the census checks that each sees something, planted entries among it) ----
def perspective_view(seed=0, **kw):
    return dict(scene.main_camera_view(seed=scene.SEED + seed), **kw)


def cascade_view(size, seed=0, **kw):
    """an orthographic cascade `size` across around the origin"""
    return dict(scene.cascade_view(seed=scene.SEED + seed, size=float(size), depth=float(4 * size), index=1), **kw)


def edge_views():
    """(name, view) of the two view kinds an edge world is culled with, and the batched three"""
    persp, ortho = perspective_view(), cascade_view(4 * EDGE_SPREAD)
    return [("perspective", persp), ("cascade", ortho)]


def edge_batch():
    persp = perspective_view(1)
    return [persp, cascade_view(4 * EDGE_SPREAD, 1), dict(cascade_view(8 * EDGE_SPREAD, 2), shadow_pass=2)]


def deep_view(scale):
    """the single view a deep world is culled with: an orthographic main pass wide enough for where its chain wanders"""
    size = {0.6: 40.0, 1.6: 4000.0, 1.0: 400.0}[scale]
    return dict(cascade_view(size), shadow_pass=-1)


def tile_view():
    """an orthographic main pass 60 across around the origin: about half of a tile world's roots are inside"""
    return dict(cascade_view(60.0, 3), shadow_pass=-1)


def sphere_views():
    side = 100.0 * SPHERE_N ** (1.0 / 3.0)
    return [("perspective", perspective_view(5)), ("cascade", cascade_view(0.4 * side, 5))]


def deep_planted(sc, scale):
    """slots of a deep world whose world matrix has left the normal range (none for scale 1)"""
    links = np.arange(sc.transforms.shape[0])
    if scale == 1.0:
        return np.zeros(links.shape[0], bool)
    return links > np.log(1.1754944e-38 if scale < 1 else 3.4028235e38) / np.log(scale)
