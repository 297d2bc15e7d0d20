"""gv_pick on the device: the editor's click selection (mesh-selector.cpp:67-122) over the mirror, checked bit for bit against the C
twin of DESIGN.md §4 item 8 (tests/pick_twin.h) fed with the oracle's candidates and camera-relative models, against an
independent float64 evaluation, and through its rules, the mirror's changes and the cull results it must leave alone."""
import numpy as np
import pytest

import pick_support as ps
from garden_amd import scene
from garden_amd.lib import GV_E_ARG, GV_E_STATE, GpuVisibility, GvError

pytestmark = pytest.mark.gpu

GV_DIRTY_TRANSFORM, GV_DIRTY_MESH = 0, 2
CAM = (10.5, -3.25, 7.0)
RAYS = 64


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return ps.build_twin(tmp_path_factory.mktemp("twin"))


def defective(sc, seed):
    """a few non-finite and singular transforms on top of the scene's own defects"""
    rng = np.random.Generator(np.random.PCG64(seed))
    k = rng.choice(sc.count, 64, replace=False)
    sc.transforms["rotation"][k[:16], 1] = np.nan
    sc.transforms["position"][k[16:32], 0] = np.inf
    sc.transforms["scale"][k[32:48], 2] = 0.0
    return sc


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()


def check_against_twin(vis, twin, pools, rays, pool_ids=(0,), camera_position=CAM, exclude=None, min_hits=None):
    got = ps.gpu_pick(vis, rays, pool_ids=pool_ids, camera_position=camera_position, exclude=exclude)
    exp = ps.decode(ps.twin_keys(twin, pools, rays, exclude=exclude), pool_ids)
    assert ps.as_bits(got) == ps.as_bits(exp)
    hits = sum(h is not None for h in got)
    assert hits >= (min_hits if min_hits is not None else len(rays) // 2), hits
    return got


@pytest.fixture(scope="module")
def flat2m():
    sc = defective(scene.flat_scene(2_000_000), 11)
    return sc, ps.candidates(sc, CAM)


@pytest.mark.parametrize("keep_slot_order", [False, True], ids=["spatial", "slot_order"])
def test_flat_2m_bit_exact(twin, flat2m, keep_slot_order):
    sc, pool = flat2m
    rays = ps.aimed_rays(pool, RAYS, 1)
    with GpuVisibility(device=0, keep_slot_order=keep_slot_order) as vis:
        bind(vis, sc)
        check_against_twin(vis, twin, [pool], rays)


def test_hierarchy_1m_bit_exact(twin):
    sc = defective(scene.hierarchy_scene(1_000_000), 12)
    pool = ps.candidates(sc, CAM)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        check_against_twin(vis, twin, [pool], ps.aimed_rays(pool, RAYS, 2, reach=(10.0, 200.0)))


def test_general_mapping_bit_exact(twin):
    sc = scene.shuffled_scene(scene.flat_scene(300_000), drop_transforms=0.02)
    pool = ps.candidates(sc, CAM)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        check_against_twin(vis, twin, [pool], ps.aimed_rays(pool, RAYS, 3))


def test_column_binds_bit_exact(twin):
    sc = defective(scene.flat_scene(300_000), 13)
    t, m = sc.transforms, sc.meshes
    xf = dict(entity=t["entity"].copy(), parent=t["parent"].copy(), position=np.ascontiguousarray(t["position"][:, :3]),
              scale=np.ascontiguousarray(t["scale"][:, :3]), rotation=t["rotation"].copy(),
              self_active=t["selfActive"].copy(), ancestors_active=t["ancestorsActive"].copy(),
              model_with_ancestors=t["modelWithAncestors"].copy())
    mesh = dict(entity=m["entity"].copy(), is_enabled=m["isEnabled"].copy(),
                aabb_min=np.ascontiguousarray(m["aabbMin"][:, :3]), aabb_max=np.ascontiguousarray(m["aabbMax"][:, :3]),
                is_visible=np.zeros(sc.count, np.uint8))
    pool = ps.candidates(sc, CAM)
    with GpuVisibility(device=0) as vis:
        vis.bind_transform_columns(xf, sc.entity_to_transform)
        vis.bind_pool_columns(0, mesh)
        vis.hierarchy_rebuild()
        check_against_twin(vis, twin, [pool], ps.aimed_rays(pool, RAYS, 4))


def test_ties_between_pools_and_slots(twin):
    """The same pivot in two pools (the same entities) and in two slots of one pool: the listed order, then the slot, decides."""
    sc = scene.flat_scene(20_000, defects=False)
    t = sc.transforms
    rng = np.random.Generator(np.random.PCG64(6))
    a = rng.choice(sc.count, 40, replace=False)
    twins_of, copies = a[:20], a[20:]
    for src, dst in zip(twins_of, copies):  # same TRS in another slot: the same model bits, the same key but the slot
        for f in ("position", "scale", "rotation"):
            t[f][dst] = t[f][src]
    second = sc.meshes.copy()
    pool = ps.candidates(sc, CAM)
    rays = ps.aimed_rays(pool, RAYS, 7, stray=0.0)
    p = {int(s): i for i, s in enumerate(pool.slots)}
    for k, s in enumerate(copies[:RAYS // 2]):
        rays[k, :3] = pool.models[p[int(s)], 9:12] + np.float32(30.0)
        rays[k, 3:] = -30.0
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, 3)
        vis.bind_pool(5, second)
        got = check_against_twin(vis, twin, [pool, pool], rays, pool_ids=(5, 3))
        assert all(h is None or h[0] == 5 for h in got)
        tied = [h[1] for h in got[:len(copies)] if h is not None]
        assert any(s in set(twins_of.tolist()) | set(copies.tolist()) for s in tied)
        got = check_against_twin(vis, twin, [pool, pool], rays, pool_ids=(3, 5), exclude=[None, 17])
        assert all(h is None or h[0] == 3 for h in got)


def test_float64_evaluation_agrees_where_the_winner_is_clear(twin):
    sc = scene.flat_scene(250_000)
    pool = ps.candidates(sc, CAM)
    rays = ps.aimed_rays(pool, RAYS, 8)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        got = ps.gpu_pick(vis, rays, camera_position=CAM)
    ambiguous = float64_check(pool, rays, got)
    print(f"float64 check: {ambiguous} of {len(rays)} rays ambiguous")
    assert ambiguous <= len(rays) // 10


def float64_check(pool, rays, got):
    """asserts `got` where the float64 evaluation is unambiguous; returns the number of ambiguous rays"""
    m = pool.models.astype(np.float64)
    A = np.stack([m[:, 0:3], m[:, 3:6], m[:, 6:9]], axis=2)  # A[k][r][c]: column c = m[3c : 3c + 3]
    t = m[:, 9:12]
    inv = np.linalg.inv(A)
    lo, hi = pool.boxes[:, :3].astype(np.float64), pool.boxes[:, 3:].astype(np.float64)
    eps = 1e-5
    ambiguous = 0
    for r, ray in enumerate(rays.astype(np.float64)):
        u = ray[:3] - t
        o = np.einsum("krc,kc->kr", inv, u)
        d = np.einsum("krc,c->kr", inv, ray[3:])
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (lo - o) / d, (hi - o) / d
        moving = d != 0
        near = np.where(moving, np.minimum(t1, t2), -np.inf).max(axis=1)
        far = np.where(moving, np.maximum(t1, t2), np.inf).min(axis=1)
        dist = (u * u).sum(axis=1)
        # clear verdicts keep a relative margin eps on every comparison; the rest is borderline and could go either way in fp32
        tol = eps * (1.0 + np.where(np.isfinite(near), np.abs(near), 0.0))
        m = eps * (np.abs(o) + 1.0)
        inside = np.where(moving, True, (lo + m < o) & (o < hi - m)).all(axis=1)
        outside = np.where(moving, False, (o < lo - m) | (o > hi + m)).any(axis=1)
        hit = inside & (near >= tol) & (near <= far - tol)
        miss = outside | (near < -tol) | (near > far + tol)
        close = ~hit & ~miss
        if not hit.any():
            clear = not close.any()
            ambiguous += not clear
            if clear:
                assert got[r] is None, (r, got[r])
            continue
        order = np.argsort(dist[hit], kind="stable")
        win = np.nonzero(hit)[0][order[0]]
        best = dist[win]
        runner = dist[hit][order[1]] if hit.sum() > 1 else np.inf
        borderline = close & (dist <= best * (1 + eps))
        if runner <= best * (1 + eps) or borderline.any():
            ambiguous += 1
            continue
        assert got[r] is not None and got[r][1] == int(pool.slots[win]), (r, got[r], int(pool.slots[win]))
        assert abs(got[r][2] - best) <= 1e-5 * best + 1e-6
    return ambiguous


def small_world():
    """Hand-placed entities on the +z axis of the camera, identity rotations, unit scale."""
    sc = scene.flat_scene(64, defects=False)
    t, m = sc.transforms, sc.meshes
    t["rotation"] = (0, 0, 0, 1)
    t["scale"][:, :3] = 1.0
    m["aabbMin"][:, :3] = -0.5
    m["aabbMax"][:, :3] = 0.5
    t["position"][:, :3] = np.stack([np.arange(64) * 10.0 + 1000.0, np.zeros(64), np.zeros(64)], axis=1)  # out of the way
    return sc


def test_filters_exclusion_and_the_nearer_pivot(twin):
    sc = small_world()
    t, m, e2t = sc.transforms, sc.meshes, sc.entity_to_transform
    for s, d in ((1, 10), (2, 12), (3, 14), (4, 16), (5, 18), (6, 20), (7, 40)):
        t["position"][s, :3] = (0.0, 0.0, d)
    m["isEnabled"][1] = 0        # disabled
    m["entity"][2] = 0           # free slot
    t["selfActive"][3] = 0       # inactive
    e2t[m["entity"][4]] = 0xFFFFFFFF  # no transform
    t["entity"][4] = 0
    # slot 5: a child of slot 8, whose ancestors are inactive
    t["parent"][5] = t["entity"][8]
    t["position"][5, :3] = (-1000.0 - 80.0, 0.0, 18.0)
    t["ancestorsActive"][5] = 0
    # slot 7: a large box reaching towards the camera (entered at t = 5) around a far pivot (40); slot 6 (pivot 20) is entered later
    m["aabbMin"][7, :3] = (-2.0, -2.0, -35.0)
    m["aabbMax"][7, :3] = (2.0, 2.0, 35.0)
    pool = ps.candidates(sc, (0, 0, 0))
    assert set(pool.slots.tolist()).isdisjoint({1, 2, 3, 4, 5})
    ray = np.array([[0, 0, 0, 0, 0, 1]], np.float32)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        assert vis.pick(ray, camera_position=(0, 0, 0)) == [(0, 6, 400.0)]  # the nearer pivot, not the first box along the ray
        assert vis.pick(ray, camera_position=(0, 0, 0), exclude=[6]) == [(0, 7, 1600.0)]
        assert vis.pick(ray, camera_position=(0, 0, 0), exclude=[7]) == [(0, 6, 400.0)]
        # the camera moves: models are camera-relative, so is the ray
        assert vis.pick(ray, camera_position=(0, 0, -5)) == [(0, 6, 625.0)]
        # a ray that starts inside slot 7's box does not pick it
        assert vis.pick(np.array([[0, 0, 30, 0, 0, 1]], np.float32), camera_position=(0, 0, 0)) == [None]
        # eight rays in one call == eight single calls
        rays = ps.aimed_rays(pool, 8, 9, reach=(3.0, 60.0), stray=0.0)
        rays[0] = ray[0]
        many = vis.pick(rays, camera_position=(0, 0, 0))
        assert many == [vis.pick(rays[k:k + 1], camera_position=(0, 0, 0))[0] for k in range(8)]
        assert ps.as_bits(many) == ps.as_bits(ps.decode(ps.twin_keys(twin, [pool], rays), [0]))


def test_pick_follows_moves_growth_and_reorder(twin):
    full = scene.flat_scene(260_000)

    def cut(k):
        e2t = full.entity_to_transform.copy()
        e2t[e2t >= k] = 0xFFFFFFFF
        return scene.Scene(full.meshes[:k].copy(), full.transforms[:k].copy(), e2t)

    with GpuVisibility(device=0, linear_scan=True) as vis:
        sc = cut(150_000)
        bind(vis, sc)
        pool = ps.candidates(sc, CAM)
        rays = ps.aimed_rays(pool, 16, 10, stray=0.0)
        got = check_against_twin(vis, twin, [pool], rays)
        # move every entity hit so far out of the way, through dirty marks
        moved = sorted({h[1] for h in got if h is not None})
        sc.transforms["position"][moved, :3] += np.float32(5000.0)
        for s in moved:
            vis.mark_dirty(GV_DIRTY_TRANSFORM, int(s), 1)
        pool = ps.candidates(sc, CAM)
        after = check_against_twin(vis, twin, [pool], rays, min_hits=0)
        assert not ({h[1] for h in after if h is not None} & set(moved))
        # box edits through dirty marks
        sc.meshes["aabbMax"][moved, :3] *= np.float32(0.0)
        sc.meshes["aabbMin"][moved, :3] *= np.float32(0.0)
        for s in moved:
            vis.mark_dirty(GV_DIRTY_MESH, int(s), 1, pool_id=0)
        check_against_twin(vis, twin, [ps.candidates(sc, CAM)], rays, min_hits=0)
        before = vis.stats()["mirror_reorders"]
        for k in (160_000, 175_000, 200_000, 230_000, 260_000):
            sc = cut(k)
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            pool = ps.candidates(sc, CAM)
            check_against_twin(vis, twin, [pool], ps.aimed_rays(pool, 16, k), min_hits=4)
        assert vis.stats()["mirror_reorders"] > before


def test_cull_results_untouched_and_error_codes(twin):
    sc = scene.flat_scene(300_000)
    view = scene.main_camera_view(camera_position=CAM)
    pool = ps.candidates(sc, CAM)
    rays = ps.aimed_rays(pool, 8, 11)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [view])
        first = vis.fetch(0, write_back=False, occupancy=sc.count)
        first = {k: (None if v is None else np.array(v, copy=True)) for k, v in first.items()}
        got = vis.pick(rays, camera_position=CAM)
        assert ps.as_bits(got) == ps.as_bits(ps.decode(ps.twin_keys(twin, [pool], rays), [0]))
        again = vis.fetch(0, write_back=False, occupancy=sc.count)
        assert first.keys() == again.keys()
        for k in first:
            assert (first[k] is None) == (again[k] is None), k
            if first[k] is not None:
                assert np.asarray(first[k]).tobytes() == np.asarray(again[k]).tobytes(), k
        assert first["draw_count"] > 0

        def code(**kw):
            args = dict(rays=rays[:1], pool_ids=(0,), camera_position=CAM)
            args.update(kw)
            with pytest.raises(GvError) as e:
                vis.pick(**args)
            return e.value.code

        assert code(pool_ids=(0, 1)) == GV_E_ARG  # pool 1 is not bound
        assert code(rays=np.zeros((0, 6), np.float32)) == GV_E_ARG
        assert code(rays=np.zeros((9, 6), np.float32)) == GV_E_ARG
        assert code(pool_ids=tuple([0] * 17)) == GV_E_ARG
        vis.cull_batch_begin()
        assert code() == GV_E_STATE
        vis.cull_batch_end()
        assert vis.pick(rays[:1], camera_position=CAM) == got[:1]
    with GpuVisibility(device=0) as vis:
        vis.bind_pool(0, sc.meshes)
        with pytest.raises(GvError) as e:
            vis.pick(rays[:1])
        assert e.value.code == GV_E_STATE  # no transforms bound


def test_index_map_slots_holes_and_ranks(twin):
    """With an index map, hits and excluded slots live in the mapped slot space and holes (GV_NONE) are never picked; a pool split
    over several contexts, each with its share's map, gives the single context's answer as the host minimum of their keys."""
    sc = scene.flat_scene(200_000)
    n = sc.count
    rng = np.random.Generator(np.random.PCG64(21))
    world = (rng.permutation(n) + 1000).astype(np.uint32)  # a permuted slot space
    world[rng.random(n) < 0.1] = ps.NONE                   # holes of a share
    pool = ps.candidates(sc, CAM)
    mapped = ps.Pool(world[pool.slots], pool.models, pool.boxes)
    rays = ps.aimed_rays(pool, 32, 22, stray=0.0)
    holes = pool.slots[world[pool.slots] == ps.NONE][:8]  # rays straight at hole entities: never picked
    p = {int(s): i for i, s in enumerate(pool.slots)}
    for k, s in enumerate(holes):
        rays[k, :3] = pool.models[p[int(s)], 9:12] + np.float32(4.0)
        rays[k, 3:] = -4.0
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.set_index_map(0, world)
        got = check_against_twin(vis, twin, [mapped], rays)
        assert all(h is None or (h[1] != ps.NONE and h[1] >= 1000) for h in got)
        assert not {h[1] for h in got if h is not None} & set(world[holes].tolist())
        for k, h in [(k, h) for k, h in enumerate(got) if h is not None][:6]:  # exclusion in the mapped space
            again = check_against_twin(vis, twin, [mapped], rays[k:k + 1], exclude=[h[1]], min_hits=0)
            assert again[0] is None or again[0][1] != h[1]
        wide = world.copy()
        wide[7] = 1 << 28
        vis.set_index_map(0, wide)
        with pytest.raises(GvError) as e:
            vis.pick(rays[:1], camera_position=CAM)
        assert e.value.code == GV_E_ARG
        vis.update_index_map(0, 7, world[7:8])  # the table is whole again
        assert vis.pick(rays[:8], camera_position=CAM) == got[:8]
        vis.set_index_map(0, world[:n - 1])
        with pytest.raises(GvError) as e:
            vis.pick(rays[:1], camera_position=CAM)
        assert e.value.code == GV_E_STATE
        with pytest.raises(ValueError):
            vis.pick(rays[:1], pool_ids=(0,), exclude=[1, 2])

    # three shares of the pool on three contexts (all transforms on each): the host minimum of the ranks' keys
    owner = rng.integers(0, 3, n)
    ranks = []
    try:
        for r in range(3):
            slots = np.nonzero(owner == r)[0]
            ctx = GpuVisibility(device=0)
            ranks.append(ctx)
            ctx.bind_transforms(sc.transforms, sc.entity_to_transform)
            ctx.bind_pool(0, sc.meshes[slots].copy())
            ctx.hierarchy_rebuild()
            ctx.set_index_map(0, world[slots])
        for ex in (None, [got[0][1] if got[0] else None]):
            merged = []
            for k in range(0, len(rays), 8):
                per_rank = [c.pick(rays[k:k + 8], camera_position=CAM, exclude=ex) for c in ranks]
                for hits in zip(*per_rank):
                    found = [h for h in hits if h is not None]
                    merged.append(min(found, key=lambda h: (int(np.float32(h[2]).view(np.uint32)), h[1])) if found else None)
            assert ps.as_bits(merged) == ps.as_bits(ps.decode(ps.twin_keys(twin, [mapped], rays, exclude=ex), [0]))
    finally:
        for c in ranks:
            c.close()


@pytest.fixture(scope="module")
def pick_select(tmp_path_factory):
    """tests/cpp/pick_select.cpp, built with the flags of the headless_tick rule of tests/cpp/Makefile"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cpp, lib = os.path.join(root, "tests", "cpp"), os.path.join(root, "garden_amd", "lib")
    exe = str(tmp_path_factory.mktemp("pick_select") / "pick_select")
    subprocess.run(["make", "-s", "-C", cpp, "build/gv_oracle.o"], check=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-invalid-offsetof", "-fno-strict-aliasing", "-march=haswell",
                    "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(cpp, "pick_select.cpp"),
                    os.path.join(cpp, "build", "gv_oracle.o"), "-o", exe, "-L" + lib, "-lgarden_vis", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-lpthread"], check=True)
    return exe


def test_mesh_selector_shim_matches_the_loop_on_one_and_four_ranks(pick_select):
    """GpuMeshSelector::select against a CPU restatement of mesh-selector.cpp:78-122, without and with a selection, on one
    context and on four (ranks mode, one device): the same entities every time."""
    import json
    import subprocess
    out = {}
    for ranks in (1, 4):
        p = subprocess.run([pick_select, "--entities", "30000", "--ranks", str(ranks), "--cursors", "300"], capture_output=True,
                           text=True, timeout=300)
        line = json.loads(p.stdout.strip().splitlines()[-1])
        assert p.returncode == 0 and line["ok"], (p.stdout[-2000:], p.stderr[-2000:])
        assert line["hits"] >= 60 and line["reselected"] >= 30, line
        out[ranks] = line
    assert out[1]["checksum"] == out[4]["checksum"] and out[1]["hits"] == out[4]["hits"], out
