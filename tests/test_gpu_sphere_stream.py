"""The sphere stream of a flat, exactly paired pool (MeshMirror::hot: position + sphere radius per entry, read by the cull for
every entry; the TRS / AABB streams only for the lanes that need corners) must stay current after every sync.

Every step edits the pools through dirty marks only and compares visible_idx, bakedModel and isVisible with the CPU oracle,
with and without Hi-Z. Entities moved from outside the frustum to inside it are what a stale entry would miss."""
import numpy as np
import pytest

from garden_amd import scene

pytestmark = pytest.mark.gpu

GV_DIRTY_TRANSFORM, GV_DIRTY_HIERARCHY, GV_DIRTY_MESH = 0, 1, 2
N = 200_000  # above the pool size from which a sphere stream is kept


def exact(gpu, oracle, sc, view, hz=None):
    gpu.cull(0, [view])
    got = gpu.fetch(0, write_back=False, occupancy=sc.count)
    m2 = sc.meshes.copy()
    exp = oracle.prepare_meshes(m2, sc.transforms, sc.entity_to_transform, view, hiz=hz)
    assert np.array_equal(got["visible_idx"], np.sort(exp["visible_idx"]))
    o = np.argsort(exp["visible_idx"], kind="stable")
    assert np.array_equal(got["baked_model"].view(np.uint32), exp["baked_model"][o].view(np.uint32))
    assert np.array_equal(got["is_visible"], m2["isVisible"])
    return exp


def both(gpu, oracle, sc, view, hz):
    """The frustum-only and the Hi-Z form of the view; returns the frustum-only visible set."""
    exact(gpu, oracle, sc, dict(view, use_hiz=1), hz)
    return exact(gpu, oracle, sc, dict(view, use_hiz=0))["visible_idx"]


@pytest.fixture(scope="module")
def pyramid():
    depth = scene.synthetic_depth(1024, 512)
    depth[:, :400] = np.maximum(depth[:, :400], np.float32(0.3))
    return depth


@pytest.mark.parametrize("ctx_name", ["gpu_linear", "gpu", "gpu_slot_order"])
def test_sphere_stream_follows_every_kind_of_edit(request, oracle, pyramid, ctx_name):
    gpu = request.getfixturevalue(ctx_name)
    sc = scene.flat_scene(N)
    view = scene.main_camera_view()
    gpu.hiz_build(pyramid)
    hz = oracle.Hiz(pyramid)
    gpu.bind_transforms(sc.transforms, sc.entity_to_transform)
    gpu.bind_pool(0, sc.meshes)
    gpu.hierarchy_rebuild()
    vis = both(gpu, oracle, sc, view, hz)
    vis = both(gpu, oracle, sc, view, hz)  # a quiet frame
    assert 0 < vis.size < N // 2
    rng = np.random.Generator(np.random.PCG64(23))
    hidden = np.setdiff1d(np.arange(N), vis)

    def mark_xf(slots):
        for s in slots:
            gpu.mark_dirty(GV_DIRTY_TRANSFORM, int(s), 1)

    def mark_mesh(slots):
        for s in slots:
            gpu.mark_dirty(GV_DIRTY_MESH, int(s), 1, pool_id=0)

    # across the frustum planes, both ways: outside -> onto a visible entity's place, inside -> onto a hidden one's
    inward = rng.choice(hidden, 300, replace=False)
    outward = rng.choice(vis, 300, replace=False)
    sc.transforms["position"][inward, :3] = sc.transforms["position"][rng.choice(vis, 300), :3]
    sc.transforms["position"][outward, :3] = sc.transforms["position"][rng.choice(hidden, 300), :3]
    mark_xf(np.concatenate([inward, outward]))
    now = both(gpu, oracle, sc, view, hz)
    assert np.isin(inward, now).sum() > 100  # the stale-entry case really happened
    # AABB-only edits: boxes that grow across a plane, shrink, and become empty / zero-size
    boxes = rng.choice(N, 400, replace=False)
    sc.meshes["aabbMax"][boxes[:200], :3] *= np.float32(60.0)
    sc.meshes["aabbMin"][boxes[200:300], :3] = sc.meshes["aabbMax"][boxes[200:300], :3]
    sc.meshes["aabbMax"][boxes[300:], :3] = sc.meshes["aabbMin"][boxes[300:], :3] + np.float32(1e-3)
    mark_mesh(boxes)
    both(gpu, oracle, sc, view, hz)
    # mesh disable / enable, transform deactivation / reactivation
    toggled = rng.choice(now, 200, replace=False)
    sc.meshes["isEnabled"][toggled[:100]] ^= 1
    sc.transforms["selfActive"][toggled[100:]] ^= 1
    mark_mesh(toggled[:100])
    mark_xf(toggled[100:])
    both(gpu, oracle, sc, view, hz)
    sc.meshes["isEnabled"][toggled[:100]] ^= 1
    sc.transforms["selfActive"][toggled[100:]] ^= 1
    mark_mesh(toggled[:100])
    mark_xf(toggled[100:])
    both(gpu, oracle, sc, view, hz)
    # freed and refilled slots (the mesh's entity goes away and comes back)
    freed = rng.choice(now, 150, replace=False)
    ent = sc.meshes["entity"][freed].copy()
    sc.meshes["entity"][freed] = 0
    mark_mesh(freed)
    both(gpu, oracle, sc, view, hz)
    sc.meshes["entity"][freed] = ent
    mark_mesh(freed)
    both(gpu, oracle, sc, view, hz)
    # non-finite and zero-size inputs; then back to finite values
    odd = rng.choice(now, 60, replace=False)
    saved_pos, saved_scale = sc.transforms["position"][odd].copy(), sc.transforms["scale"][odd].copy()
    sc.transforms["position"][odd[0:15], 0] = np.nan
    sc.transforms["position"][odd[15:30], 1] = np.inf
    sc.transforms["scale"][odd[30:45], 2] = -np.inf
    sc.transforms["scale"][odd[45:], :3] = np.float32(0.0)
    sc.meshes["aabbMin"][odd[:10], 0] = np.nan
    mark_xf(odd)
    mark_mesh(odd[:10])
    both(gpu, oracle, sc, view, hz)
    sc.transforms["position"][odd], sc.transforms["scale"][odd] = saved_pos, saved_scale
    sc.meshes["aabbMin"][odd[:10], 0] = sc.meshes["aabbMax"][odd[:10], 0] - np.float32(1.0)
    mark_xf(odd)
    mark_mesh(odd[:10])
    both(gpu, oracle, sc, view, hz)
    # a large range (device-side gather) and a pool rewritten every frame, then at rest again
    lo = 10_000
    sc.transforms["position"][lo:lo + 5_000, :3] += rng.normal(0, 40, (5_000, 3)).astype(np.float32)
    gpu.mark_dirty(GV_DIRTY_TRANSFORM, lo, 5_000)
    both(gpu, oracle, sc, view, hz)
    for frame in range(4):
        sc.transforms["position"][:, :3] += rng.normal(0, 5, (N, 3)).astype(np.float32)
        gpu.mark_dirty(GV_DIRTY_TRANSFORM, 0, N)
        exact(gpu, oracle, sc, dict(view, use_hiz=frame % 2), hz if frame % 2 else None)
    for frame in range(3):
        both(gpu, oracle, sc, view, hz)


def test_sphere_stream_through_growth_churn_and_reorder(gpu_linear, oracle, pyramid):
    """Occupancy growth in batches until the unsorted tail forces a re-order of the mirror; moves after it."""
    gpu = gpu_linear
    full = scene.flat_scene(260_000)
    view = scene.main_camera_view()
    gpu.hiz_build(pyramid)
    hz = oracle.Hiz(pyramid)

    def cut(k):
        e2t = full.entity_to_transform.copy()
        e2t[e2t >= k] = 0xFFFFFFFF
        return scene.Scene(full.meshes[:k].copy(), full.transforms[:k].copy(), e2t)

    before = gpu.stats()["mirror_reorders"]
    sc = cut(150_000)
    gpu.bind_transforms(sc.transforms, sc.entity_to_transform)
    gpu.bind_pool(0, sc.meshes)
    gpu.hierarchy_rebuild()
    both(gpu, oracle, sc, view, hz)
    for k in (160_000, 175_000, 200_000, 230_000, 260_000):
        sc = cut(k)
        gpu.bind_transforms(sc.transforms, sc.entity_to_transform)
        gpu.bind_pool(0, sc.meshes)
        both(gpu, oracle, sc, view, hz)
    assert gpu.stats()["mirror_reorders"] > before
    rng = np.random.Generator(np.random.PCG64(5))
    vis = both(gpu, oracle, sc, view, hz)
    hidden = np.setdiff1d(np.arange(sc.count), vis)
    inward = rng.choice(hidden, 200, replace=False)
    sc.transforms["position"][inward, :3] = sc.transforms["position"][rng.choice(vis, 200), :3]
    for s in inward:
        gpu.mark_dirty(GV_DIRTY_TRANSFORM, int(s), 1)
    both(gpu, oracle, sc, view, hz)


def test_sphere_stream_with_column_binds(gpu_linear, oracle):
    gpu = gpu_linear
    sc = scene.flat_scene(N)
    t, m = sc.transforms, sc.meshes
    xf = dict(entity=t["entity"].copy(), parent=t["parent"].copy(), position=np.ascontiguousarray(t["position"][:, :3]),
              scale=np.ascontiguousarray(t["scale"][:, :3]), rotation=t["rotation"].copy(),
              self_active=t["selfActive"].copy(), ancestors_active=t["ancestorsActive"].copy(),
              model_with_ancestors=t["modelWithAncestors"].copy())
    mesh = dict(entity=m["entity"].copy(), is_enabled=m["isEnabled"].copy(),
                aabb_min=np.ascontiguousarray(m["aabbMin"][:, :3]), aabb_max=np.ascontiguousarray(m["aabbMax"][:, :3]),
                is_visible=np.full(N, 7, np.uint8))
    view = scene.main_camera_view()
    gpu.bind_transform_columns(xf, sc.entity_to_transform)
    gpu.bind_pool_columns(0, mesh)
    gpu.hierarchy_rebuild()
    vis = exact(gpu, oracle, sc, view)["visible_idx"]
    exact(gpu, oracle, sc, view)
    rng = np.random.Generator(np.random.PCG64(8))
    hidden = np.setdiff1d(np.arange(N), vis)
    inward = np.sort(rng.choice(hidden, 100, replace=False))
    xf["position"][inward] = xf["position"][rng.choice(vis, 100)]
    t["position"][inward, :3] = xf["position"][inward]
    xf["self_active"][vis[:50]] ^= 1
    t["selfActive"][vis[:50]] = xf["self_active"][vis[:50]]
    for s in np.concatenate([inward, vis[:50]]):
        gpu.mark_dirty(GV_DIRTY_TRANSFORM, int(s), 1)
    mesh["aabb_max"][vis[50:80]] *= np.float32(30.0)
    m["aabbMax"][vis[50:80], :3] = mesh["aabb_max"][vis[50:80]]
    for s in vis[50:80]:
        gpu.mark_dirty(GV_DIRTY_MESH, int(s), 1, pool_id=0)
    exact(gpu, oracle, sc, view)
