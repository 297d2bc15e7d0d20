"""gv_pool_view_delta timing, the method of tools/view_bounds_bench.py: cfg3's world (flat, main camera with Hi-Z against a 4096 x 4096
walls image); the camera turns about the world's y axis by --step radians per frame. Per size, per source (records: the emitted view;
bytes: the count-only view of the same camera) and per frame: one gv_cull, waited for, then ONE gv_pool_view_delta:

    wall      microseconds of call + wait (time.perf_counter), median over --frames frames after --warmup
    kernels   the library's own event brackets around the call's launches (gv_profile_kernels, kind "emit": one mark launch, count,
              place), summed per call — in a pass of its own, because a bracket costs stream time
    sparse    the channel's baseline is the previous frame's set;  dense: GV_DELTA_RESTART, appeared = all of C (a first call)

and beside them, in the same run and for the same frames: the host alternative an engine has today (two fetches and np.setdiff1d both
ways, every word asserted equal to the device's answer) and the yardstick, the parent's gv_pool_emit_instances over the same view.

    python tools/view_delta_bench.py --n 1000000 10000000 --frames 20 [--out FILE]

Prints one JSON line per size, source and phase."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def turned_view(scene, angle, emit_records):
    """the main camera of scene.main_camera_view turned by `angle` about y"""
    rng = np.random.Generator(np.random.PCG64(scene.SEED ^ 0xC0FFEE))
    q = scene._unit_quats(rng, 1)[0].astype(np.float64)
    h = 0.5 * angle
    r = np.array([0.0, math.sin(h), 0.0, math.cos(h)])  # xyzw
    x1, y1, z1, w1 = q
    x2, y2, z2, w2 = r
    turned = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                       w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2]).astype(np.float32)
    proj = scene.persp_inf_rev_z(math.radians(90.0), 16.0 / 9.0, 0.01)
    return scene.make_view(scene.mul_cm(proj, scene.view_from_quat(turned)), use_hiz=1, emit_records=emit_records)


def stats(us):
    us = np.array(us)
    return dict(us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)))


def run(a):
    import instances_support as isup
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    depth = scene.synthetic_depth(4096, 4096)
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for n in a.n:
        sc = scene.flat_scene(n)
        for source in ("records", "bytes"):
            emit = 1 if source == "records" else 0
            with GpuVisibility(device=0) as vis:
                vis.bind_transforms(sc.transforms, sc.entity_to_transform)
                vis.bind_pool(0, sc.meshes)
                vis.hierarchy_rebuild()
                vis.hiz_build(depth)
                vis.set_instance_layout(0, dtype=isup.BARE)
                frames = a.warmup + a.frames
                for profiled in (False, True):
                    vis.profile_kernels(["emit"] if profiled else [])
                    wall = {"sparse": [], "dense": []}
                    kernels = {"sparse": [], "dense": []}
                    host, emission, sizes = [], [], []
                    previous = None
                    for k in range(frames):
                        vis.cull(0, [turned_view(scene, a.step * k, emit)])
                        vis.wait()
                        for phase, channel, restart in (("sparse", 0, False), ("dense", 1, True)):
                            vis.stats_reset()
                            s = time.perf_counter()
                            vis.view_delta_issue(0, [0], channel, restart)
                            vis.wait()
                            t = time.perf_counter() - s
                            if k >= a.warmup:
                                wall[phase].append(t * 1e6)
                                if profiled:
                                    st = vis.stats()
                                    bracketed = vis.profile_samples()["emit"]  # the call's three launches
                                    kernels[phase].append(st["device_ms"]["emit"] * 1e3 * st["launches"]["emit"] / max(bracketed, 1))
                        if profiled:
                            continue
                        got = vis.view_delta_fetch(0, 0)
                        if k >= a.warmup:
                            sizes.append((len(got["appeared"]), len(got["vanished"]), got["visible_count"]))
                        # the host alternative: this frame's set and last frame's fetched, two set differences
                        s = time.perf_counter()
                        fetched = [vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0) for _ in range(2)]
                        now = fetched[1]["visible_idx"] if emit else np.flatnonzero(fetched[1]["is_visible"]).astype(np.uint32)
                        if previous is not None:
                            appeared, vanished = np.setdiff1d(now, previous), np.setdiff1d(previous, now)
                        t = time.perf_counter() - s
                        if previous is not None:
                            assert appeared.tolist() == got["appeared"].tolist() and vanished.tolist() == got["vanished"].tolist()
                            if k >= a.warmup:
                                host.append(t * 1e6)
                        previous = now
                        if emit:  # the yardstick: the instance emission of the same view
                            s = time.perf_counter()
                            vis.emit_instances(0, [0])
                            vis.wait()
                            if k >= a.warmup:
                                emission.append((time.perf_counter() - s) * 1e6)
                    for phase in ("sparse", "dense"):
                        line = dict(n=n, source=source, phase=phase, profiled=profiled, step=a.step, frames=a.frames)
                        if profiled:
                            line["kernels_us_per_call"] = stats(kernels[phase])
                        else:
                            line["wall"] = stats(wall[phase])
                            if phase == "sparse":
                                line["appeared_vanished_visible_mean"] = [float(x) for x in np.mean(np.array(sizes), axis=0)]
                                line["host_two_fetches_and_setdiff"] = stats(host)
                                if emission:
                                    line["emit_instances_wall"] = stats(emission)
                        report(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--step", type=float, default=0.01, help="radians the camera turns per frame")
    ap.add_argument("--out", default=None)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
