"""Test helpers of the pyramid slots (gv_hiz_select / gv_hiz_drop, GvView::use_hiz = 1 + k) and of the batched pass that holds every
view against its own pyramid (cull_multi_hiz_kernel, garden_amd/csrc/gv_cull.hip): the depth images, the view sets and the table of
GPU cases (CASES) that tests/test_pyramid_slots_abi.py checks on the oracle alone and tests/test_gpu_pyramid_slots.py runs on the
device. TEST INFRASTRUCTURE ONLY.

A case binds one scene to one context, builds one pyramid per slot its view sets name — pyramid k from image k of the case, every
image of another size and with other occluders — and culls every view set twice: with one shared camera position (the batched
form: ONE cull launch) and with a camera position per view (one launch per view, each against its own pyramid)."""
import collections
import functools

import numpy as np

import cull_paths_support as cp
from garden_amd import scene
from garden_amd.lib import GV_MAX_PYRAMIDS

# Image sizes, by what the pyramid of each is (tests/hiz_paths_support.py): level 1 virtual and nested; odd levels, not nested under
# the reference rule, level 1 stored; level 1 virtual with 7 mips; a sliver; one level
IMAGE_SIZES = ((256, 256), (250, 130), (64, 64), (37, 5), (1, 1))

# A view set: per view the use_hiz byte, whether it wants records, and its kind — "main" a perspective main pass (writes isVisible),
# "spot" a perspective shadow pass, "cascade" an orthographic shadow pass
ViewSet = collections.namedtuple("ViewSet", "name use_hiz emit kinds")


def view_set(name, use_hiz, emit=None, kinds=None):
    n = len(use_hiz)
    return ViewSet(name, tuple(use_hiz), tuple(emit or (1,) * n), tuple(kinds or ("main",) * n))


VIEW_SETS = {s.name: s for s in (
    view_set("1-2", (1, 2)),
    view_set("0-2-3-4", (0, 2, 3, 4)),
    view_set("2-2-3", (2, 2, 3)),                       # two views share one pyramid
    view_set("3-0-1", (3, 0, 1)),
    view_set("eight", tuple(range(1, 9)), kinds=("main",) * 6 + ("cascade", "main")),  # eight views over eight pyramids
    view_set("emit-mix", (2, 3, 0, 1), emit=(1, 0, 1, 0)),
    view_set("main-and-shadows", (1, 2, 7, 4), kinds=("main", "spot", "cascade", "spot")),  # (pyramid 6 is a cascade's in every set)
    view_set("view0-plain", (0, 0, 5)),                 # only the last view queries
    view_set("only-view0", (3, 0, 0)),                  # only view 0 queries, and not pyramid 0
)}

Case = collections.namedtuple("Case", "name fixture kind n MAP depth sets first_size")


def case(name, fixture, kind, n, sets, first_size=0):
    MAP = {"flat": "exact", "hier": "exact", "spec": "speculate", "gen": "general"}[kind]
    return Case(name, fixture, kind, n, MAP, 3 if kind == "hier" else 0, tuple(sets), first_size)


# Pool sizes: lane, wave and workgroup edges (1, 64, 65, 257), an emit chunk plus one (4097), many workgroups (20 011), block
# bounds by flag (70 007 on gpu_bounds) and by size with the two non-exact mappings (262 147 / 262 149 on the slot-order context,
# where a shuffled pool's mapping is what cull_paths_support.mirror_mapping says). "rg16f": a context of this module's own with
# GV_CONFIG_HIZ_RG16F | GV_CONFIG_KEEP_SLOT_ORDER.
CASES = [
    case("one-entity", "gpu", "flat", 1, ("1-2", "3-0-1")),
    case("one-wave-64", "gpu", "flat", 64, ("2-2-3", "0-2-3-4"), first_size=1),
    case("wave-plus-one-65", "gpu_slot_order", "flat", 65, ("3-0-1", "2-2-3"), first_size=2),
    case("workgroup-plus-one-257", "gpu_slot_order", "spec", 257, ("0-2-3-4", "1-2", "only-view0"), first_size=3),
    case("chunk-plus-one-4097", "gpu_slot_order", "gen", 4097, ("eight", "view0-plain", "2-2-3"), first_size=4),
    case("many-workgroups-20011", "gpu", "flat", 20_011, ("1-2", "0-2-3-4", "main-and-shadows", "emit-mix", "eight")),
    case("speculate-20011", "gpu_slot_order", "spec", 20_011, ("2-2-3", "3-0-1", "view0-plain"), first_size=1),
    case("hierarchy-20011", "gpu", "hier", 20_011, ("emit-mix", "only-view0", "view0-plain")),
    case("bounds-70007", "gpu_bounds", "flat", 70_007, ("3-0-1", "0-2-3-4", "emit-mix")),
    case("auto-bounds-speculate-262147", "gpu_slot_order", "spec", 262_147, ("1-2", "view0-plain"), first_size=1),
    case("auto-bounds-general-262149", "gpu_slot_order", "gen", 262_149, ("only-view0", "0-2-3-4")),
    case("rg16f-20011", "rg16f", "flat", 20_011, ("1-2", "0-2-3-4", "main-and-shadows", "2-2-3")),
    case("rg16f-general-4097", "rg16f", "gen", 4097, ("3-0-1", "eight"), first_size=1),
]

FIXTURE_FLAGS = dict(cp.FIXTURE_FLAGS, rg16f=cp.Flags(False, False, True))


def pyramid_of(use_hiz):
    """GvView::use_hiz -> the pyramid it names (include/garden_vis.h)"""
    return use_hiz - 1 if 1 <= use_hiz <= GV_MAX_PYRAMIDS else 0


def pyramids_of(c):
    return sorted({pyramid_of(u) for s in c.sets for u in VIEW_SETS[s].use_hiz if u})


def image_size(c, pyramid):
    return IMAGE_SIZES[(c.first_size + pyramid) % len(IMAGE_SIZES)]


def pyramid_kind(c, pyramid):
    """"cascade" when an orthographic view of the case names the pyramid (its image then holds linear depths), else "perspective" """
    for s in c.sets:
        vs = VIEW_SETS[s]
        if any(u and pyramid_of(u) == pyramid and k == "cascade" for u, k in zip(vs.use_hiz, vs.kinds)):
            return "cascade"
    return "perspective"


@functools.lru_cache(maxsize=None)
def entity_distances(c):
    """(lower quartile, upper quartile) of the distance from the origin of what a main camera there has in its frustum — where the
    entities of the case's scene are, read off the oracle's own records (distanceSq) over three views"""
    from oracle import oracle_py
    sc = build_scene(c)
    d = [np.sqrt(oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, scene.main_camera_view(seed=scene.SEED + 5 + k),
                                          threads=4)["distance_sq"].astype(np.float64)) for k in range(3)]
    d = np.concatenate(d)
    d = d[np.isfinite(d) & (d > 0)]
    if d.size < 8:
        return 0.25 * cp.scene_side(c.n), 0.5 * cp.scene_side(c.n)
    return float(np.quantile(d, 0.25)), float(np.quantile(d, 0.75))


@functools.lru_cache(maxsize=None)
def depth_image(c, pyramid):
    """Image `pyramid` of a case: blocks of occluders AMONG the entities. Perspective (reversed Z, infinite far plane: depth = near /
    distance, near = 0.01 as scene.main_camera_view): distances log-uniform between the quartiles of the distances of the entities in
    view (an image of one block: spread evenly over the slots between the quartiles, so that no two slots hold the same).
    Cascade (scene.cascade_view: linear, the entities between 1/4 and 3/4): uniform in [0.35, 0.65]."""
    w, h = image_size(c, pyramid)
    rng = np.random.Generator(np.random.PCG64((scene.SEED ^ 0x51075) + 977 * pyramid + 31 * w + h))
    block = max(1, min(w, h) // 6)
    bw, bh = (w + block - 1) // block, (h + block - 1) // block
    if pyramid_kind(c, pyramid) == "cascade":
        d = rng.uniform(0.35, 0.65, size=(bh, bw)).astype(np.float32)
    else:
        near, far = entity_distances(c)
        dist = np.exp(rng.uniform(np.log(near), np.log(far), size=(bh, bw)))
        if bw * bh == 1:
            dist[:] = near + (far - near) * (pyramid + 1.0) / (GV_MAX_PYRAMIDS + 1.0)
        d = (np.float32(0.01) / dist.astype(np.float32)).astype(np.float32)
    d = np.ascontiguousarray(np.repeat(np.repeat(d, block, axis=0), block, axis=1)[:h, :w])
    d.setflags(write=False)
    return d


def make_views(c, set_name, shared=True):
    """the scene.make_view dicts of a view set. shared: every view at the main camera's position (the batched form); otherwise view i
    stands at a position of its own"""
    vs = VIEW_SETS[set_name]
    side = cp.scene_side(c.n)
    salt = sum(map(ord, set_name))
    out = []
    for i, (use_hiz, emit, kind) in enumerate(zip(vs.use_hiz, vs.emit, vs.kinds)):
        position = (0.0, 0.0, 0.0) if shared else (0.02 * side * i, -0.01 * side * i, 0.015 * side * i)
        if kind == "cascade":
            v = scene.cascade_view(seed=scene.SEED + 31 * salt, size=0.5 * side, depth=2.0 * side, index=i - 1)
            v["camera_position"][:3] = position
        else:
            v = scene.main_camera_view(seed=scene.SEED + 17 * salt + i, camera_position=position)
            if kind == "spot":
                v["shadow_pass"] = i - 1
        v["use_hiz"] = use_hiz
        v["emit_records"] = emit
        out.append(v)
    return out


def build_scene(c):
    return cp.build_scene(c.kind, c.n, c.n)


def oracle_pyramid(oracle, c, pyramid, rg16f=False):
    return oracle.Hiz(depth_image(c, pyramid), rg16f=rg16f)


def kernel_cell(c, set_name):
    """(MAP, BOUNDS, view 0 queries) of the cull_multi_hiz_kernel launch a view set of the case takes"""
    flags = FIXTURE_FLAGS[c.fixture]
    bounds = flags.block_bounds or (not flags.linear_scan and c.n > cp.AUTO_BOUNDS_MIN)
    return c.MAP, bool(bounds), bool(VIEW_SETS[set_name].use_hiz[0])


def takes_new_form(set_name):
    """gv_cull's own statement: 2 .. kMaxBatchViews views (every set here shares the camera or none does), some view names a
    pyramid other than 0"""
    vs = VIEW_SETS[set_name]
    return 2 <= len(vs.use_hiz) <= cp.MAX_BATCH_VIEWS and any(u and pyramid_of(u) != 0 for u in vs.use_hiz)


def compare_view(vis, oracle, meshes, transforms, e2t, view, index, hz, what, pool_id=None):
    """one view's results against the oracle's over the pyramid `hz` (None: no query), bit for bit; returns the oracle's result"""
    main_pass = view["shadow_pass"] < 0
    meshes["isVisible"] = 7  # poison: a main pass overwrites every slot, a shadow pass none
    got = vis.fetch(index, write_back=True, occupancy=meshes.shape[0], pool_id=pool_id)
    got_vis = meshes["isVisible"].copy()
    expected = meshes.copy()
    expected["isVisible"] = 7
    exp = oracle.prepare_meshes(expected, transforms, e2t, view, hiz=hz if view["use_hiz"] else None, threads=4)
    exp_vis = expected["isVisible"]
    assert got["draw_count"] == exp["draw_count"], (what, got["draw_count"], exp["draw_count"])
    if main_pass:
        assert np.array_equal(got_vis, exp_vis), what
        assert got["is_visible"] is not None and np.array_equal(got["is_visible"], exp_vis), what
    else:
        assert np.all(got_vis == 7) and np.all(exp_vis == 7), what
    if view["emit_records"]:
        o = np.argsort(exp["visible_idx"], kind="stable")  # (the oracle's workers deliver in ranges: by slot, as fetch() orders)
        assert np.array_equal(got["visible_idx"], exp["visible_idx"][o]), what
        assert np.array_equal(got["baked_model"].view(np.uint32), exp["baked_model"][o].view(np.uint32)), what
        assert np.array_equal(got["distance_sq"].view(np.uint32), exp["distance_sq"][o].view(np.uint32)), what
    return exp
