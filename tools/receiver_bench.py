"""gv_pool_draw_receivers timing, the method of tools/occluder_bench.py: cfg3's world (flat, the main camera, frustum only) and the
three orthographic cascades of scene.cascade_view, which share the main camera's position. Per case and mask size, per frame: one
gv_cull of the main view and the three cascades (frustum only, ONE batched pass: the parent's frame), waited for, then per cascade

    draw      gv_receiver_begin + ONE gv_pool_draw_receivers of the main view's records with the cascade's matrix: microseconds of
              calls + wait (time.perf_counter), median over --frames frames after --warmup; and the library's own event brackets
              around the call's three launches (gv_profile_kernels, kind "hiz"), summed per call — in a pass of its own, because a
              bracket costs stream time
    build     gv_hiz_build_from_receivers of the same mask, likewise
    cull      gv_cull of the cascade alone with use_hiz = 1, likewise; casters kept beside the frustum-only cull's count
    frame     the three masked cascades (draw + build + cull each) beside the one batched three-cascade frustum-only pass
    host      (--check) the alternative: fetch the records and run the scalar twin over them on 16 threads (one mask each, folded by
              np.minimum on the words), every word asserted equal to the device's mask

    python tools/receiver_bench.py [--cases 1000000 10000000] [--sizes 512x512 2048x2048] [--check] [--out FILE]

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
CASCADES = 3


def stats(us):
    us = np.array(us)
    return dict(us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)))


def host_mask(rs, twin, fetched, boxes, light, width, height):
    slots, models = rs.records(fetched)
    held = np.ascontiguousarray(boxes[slots])
    n = len(slots)
    parts = [(k * n // THREADS, (k + 1) * n // THREADS) for k in range(THREADS)]
    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        masks = list(pool.map(lambda ab: rs.twin_draw(twin, models[ab[0]:ab[1]], held[ab[0]:ab[1]], light, width, height)[0], parts))
    return np.minimum.reduce([rs.words(m) for m in masks])


def timed(vis, fn):
    s = time.perf_counter()
    fn()
    vis.wait()
    return (time.perf_counter() - s) * 1e6


def run(a):
    import receivers_support as rs
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    twin = rs.build_twin(tempfile.mkdtemp(prefix="receiver_twin_"))
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    main = scene.main_camera_view()
    plain = [scene.cascade_view(index=k) for k in range(CASCADES)]
    masked = [dict(v, use_hiz=1) for v in plain]
    for n in a.cases:
        sc = scene.flat_scene(n)
        boxes = rs.aabbs_by_slot(sc.meshes)
        with GpuVisibility(device=0) as vis:
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            vis.hierarchy_rebuild()
            for size in a.sizes:
                width, height = (int(x) for x in size.split("x"))
                for profiled in (False, True):
                    vis.profile_kernels(["hiz"] if profiled else [])
                    batched, frame = [], []
                    draw, build, cull, draw_kernels = ([[] for _ in range(CASCADES)] for _ in range(4))
                    kept_plain, kept_masked, counts = [0] * CASCADES, [0] * CASCADES, [None] * CASCADES
                    for k in range(a.warmup + a.frames):
                        t_batched = timed(vis, lambda: vis.cull(0, [main] + plain))
                        if k == a.warmup:
                            kept_plain = [vis.result_count(1 + c) for c in range(CASCADES)]
                        t_frame = 0.0
                        for c in range(CASCADES):
                            light = plain[c]["view_proj"]
                            vis.cull(0, [main])
                            vis.wait()
                            vis.stats_reset()
                            t_draw = timed(vis, lambda: (vis.receiver_begin(width, height), vis.draw_receivers(0, 0, light)))
                            kernels = vis.stats()["device_ms"]["hiz"] * 1e3
                            if k == a.warmup and not profiled:
                                mask, counts[c] = vis.receiver_mask()
                                if a.check:
                                    fetched = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
                                    s = time.perf_counter()
                                    want = host_mask(rs, twin, fetched, boxes, light, width, height)
                                    report(dict(n=n, width=width, height=height, cascade=c, host_twin_16_threads_us=(time.perf_counter() - s) * 1e6,
                                                equal=bool((want == rs.words(mask)).all()), texels_without_receiver=int(np.isinf(mask).sum())))
                                    assert (want == rs.words(mask)).all()
                            t_build = timed(vis, vis.hiz_build_from_receivers)
                            t_cull = timed(vis, lambda: vis.cull(0, [masked[c]]))
                            if k == a.warmup:
                                kept_masked[c] = vis.result_count(0)
                            if k >= a.warmup:
                                draw[c].append(t_draw), build[c].append(t_build), cull[c].append(t_cull), draw_kernels[c].append(kernels)
                            t_frame += t_draw + t_build + t_cull
                        if k >= a.warmup:
                            batched.append(t_batched), frame.append(t_frame)
                    line = dict(n=n, width=width, height=height, profiled=profiled, frames=a.frames)
                    if profiled:
                        line["draw_three_launches_kernels_us"] = [stats(x) for x in draw_kernels]
                    else:
                        line.update(begin_draw_wall=[stats(x) for x in draw], hiz_build_wall=[stats(x) for x in build],
                                    masked_cull_wall=[stats(x) for x in cull], three_masked_cascades_wall=stats(frame),
                                    main_and_three_cascades_batched_wall=stats(batched), counts=counts,
                                    casters_kept_frustum_only=kept_plain, casters_kept_masked=kept_masked)
                    report(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", type=int, default=[1_000_000, 10_000_000], help="entities")
    ap.add_argument("--sizes", nargs="+", default=["512x512", "2048x2048"])
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="every mask against the twin on 16 host threads")
    ap.add_argument("--out", default=None)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
