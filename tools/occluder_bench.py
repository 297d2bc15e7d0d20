"""gv_pool_draw_occluders timing, the method of tools/view_delta_bench.py: cfg3's world (flat, the main camera, frustum only) in which
--occluders slots are walls (two axes scaled to 1 - 6 % of the world's side) with an occluder box at 0.9 of their AABB; everybody
else has none. Per case and image size, per frame: one gv_cull, waited for, then

    draw      gv_occluder_begin + ONE gv_pool_draw_occluders: microseconds of calls + wait (time.perf_counter), median over --frames
              frames after --warmup; and the library's own event brackets around the call's three launches (gv_profile_kernels, kind
              "hiz"), summed per call — in a pass of its own, because a bracket costs stream time
    build     gv_hiz_build_from_occluders of the same image, likewise: the yardstick beside it
    host      the alternative an engine has today: fetch the view's records and run the scalar twin over them on 16 threads (one
              image each, folded by np.maximum), every word asserted equal to the device's image
    traffic   from the twin: the pixels the drawn occluders cover with multiplicity, and those that would raise the stored word if
              the records were taken one after the other (what gets past the plain-load filter in that order: a model, the device's
              order differs), against the distinct pixels written

    python tools/occluder_bench.py [--cases 1000000:1024 10000000:16384] [--sizes 512x256 2048x1024] [--out FILE]

Prints one JSON line per case, size and pass."""
import argparse
import concurrent.futures
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
THREADS = 16


def stats(us):
    us = np.array(us)
    return dict(us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)))


def world(scene, n, occluders):
    sc = scene.flat_scene(n)
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ (0x0CCB + n)))
    walls = rng.permutation(n)[:occluders]
    side = 100.0 * n ** (1.0 / 3.0)
    sc.transforms["scale"][walls, 0] = rng.uniform(0.01, 0.06, occluders).astype(np.float32) * np.float32(side)
    sc.transforms["scale"][walls, 1] = rng.uniform(0.01, 0.06, occluders).astype(np.float32) * np.float32(side)
    lo = np.zeros((n, 4), np.float32)
    hi = np.zeros((n, 4), np.float32)
    lo[walls, :3] = 0.9 * sc.meshes["aabbMin"][walls, :3]
    hi[walls, :3] = 0.9 * sc.meshes["aabbMax"][walls, :3]
    return sc, lo, hi


def host_image(osup, twin, fetched, boxes, view_proj, width, height):
    n = int(fetched["draw_count"])
    slots = fetched["visible_idx"][:n].astype(np.int64)
    models = np.ascontiguousarray(fetched["baked_model"][:n], np.float32)
    held = np.ascontiguousarray(boxes[slots])
    parts = [(k * n // THREADS, (k + 1) * n // THREADS) for k in range(THREADS)]
    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        images = list(pool.map(lambda ab: osup.twin_draw(twin, models[ab[0]:ab[1]], held[ab[0]:ab[1]], view_proj, width, height)[0], parts))
    return np.maximum.reduce(images)


def run(a):
    import occluders_support as osup
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    twin = osup.build_twin(tempfile.mkdtemp(prefix="occluder_twin_"))
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    view = scene.main_camera_view()
    for case in a.cases:
        n, occluders = (int(x) for x in case.split(":"))
        sc, lo, hi = world(scene, n, occluders)
        boxes = osup.boxes_by_slot(lo, hi)
        with GpuVisibility(device=0) as vis:
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            vis.hierarchy_rebuild()
            vis.bind_occluders(0, lo, hi)
            for size in a.sizes:
                width, height = (int(x) for x in size.split("x"))
                for profiled in (False, True):
                    vis.profile_kernels(["hiz"] if profiled else [])
                    draw, build, draw_kernels, build_kernels, host = [], [], [], [], []
                    for k in range(a.warmup + a.frames):
                        vis.cull(0, [view])
                        vis.wait()
                        vis.stats_reset()
                        s = time.perf_counter()
                        vis.occluder_begin(width, height)
                        vis.draw_occluders(0, 0, a.min_pixels)
                        vis.wait()
                        t = time.perf_counter() - s
                        st = vis.stats()
                        vis.stats_reset()
                        s = time.perf_counter()
                        vis.hiz_build_from_occluders()
                        vis.wait()
                        tb = time.perf_counter() - s
                        if k < a.warmup:
                            continue
                        draw.append(t * 1e6)
                        build.append(tb * 1e6)
                        if profiled:
                            draw_kernels.append(st["device_ms"]["hiz"] * 1e3)  # every launch is bracketed: the sum of the three
                            build_kernels.append(vis.stats()["device_ms"]["hiz"] * 1e3)
                    line = dict(n=n, occluders=occluders, width=width, height=height, min_pixels=a.min_pixels, profiled=profiled, frames=a.frames)
                    if profiled:
                        line["draw_three_launches_kernels_us"] = stats(draw_kernels)
                        line["hiz_build_kernels_us"] = stats(build_kernels)
                    else:
                        line["begin_draw_wall"] = stats(draw)
                        line["hiz_build_wall"] = stats(build)
                        image, counts = vis.occluder_depth()
                        fetched = None
                        for _ in range(3):
                            s = time.perf_counter()
                            fetched = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
                            got = host_image(osup, twin, fetched, boxes, view["view_proj"], width, height)
                            host.append((time.perf_counter() - s) * 1e6)
                        assert osup.words(got).tolist() == osup.words(image).tolist()
                        m = int(fetched["draw_count"])
                        _, covered, raised = osup.twin_traffic(twin, fetched["baked_model"][:m], boxes[fetched["visible_idx"][:m].astype(np.int64)],
                                                               view["view_proj"], width, height, a.min_pixels)
                        line.update(records=m, counts=counts, host_fetch_and_twin_16_threads=stats(host), covered_pixels=covered,
                                    raised_in_record_order=raised, distinct_pixels_written=int(np.count_nonzero(image)))
                    report(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["1000000:1024", "10000000:16384"], help="entities:occluders")
    ap.add_argument("--sizes", nargs="+", default=["512x256", "2048x1024"])
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-pixels", type=int, default=1, dest="min_pixels")
    ap.add_argument("--out", default=None)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
