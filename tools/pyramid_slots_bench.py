"""Masked shadow cascades, one at a time against ONE pyramid or in one batched cull against a pyramid each (gv_hiz_select): timing, the
method of tools/receiver_bench.py. cfg3's world (flat), the main camera and the three orthographic cascades of scene.cascade_view,
which share the main camera's position; masks of 1024 x 1024 drawn from the main view's records. Per frame, in ONE run:

    (a) one_at_a_time   per cascade: mask, pyramid (the selected one), then gv_cull of [main, c0, c1, c2] with that cascade's use_hiz = 1 —
                        what GpuShadowReceivers::cull issues: three culls, a launch per view each. Timed: the three culls.
    (b) batched         three masks into pyramids 1..3, then ONE gv_cull of [main, c0, c1, c2] with use_hiz = [0, 2, 3, 4]
                        (cull_multi_hiz_kernel). Timed: that cull.
    (c) frustum_only    ONE gv_cull of [main, c0, c1, c2], no query: the batched pass the masks are an addition to
    (d) hiz_view0       ONE gv_cull with use_hiz = [1, 0, 0, 0] against a depth pyramid in slot 0: cull_multi_kernel<true, ...>,
                        the existing kernel next to which the new one is read

Wall clock: microseconds of call + wait (time.perf_counter), median over --frames frames after --warmup. Stream time: the library's
own event brackets (gv_profile_kernels) around the cull, scan and emit launches of the timed calls, summed per frame — in a pass of
its own, because a bracket costs stream time. Every case runs in a child process under its own time limit.

    python tools/pyramid_slots_bench.py [--cases 1000000 10000000] [--size 1024] [--out FILE]

Prints one JSON line per case and pass."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASCADES = 3
KINDS = ("cull", "scan", "emit")


def stats(us):
    us = np.array(us)
    return dict(us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)))


def child(a):
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    n, size = a.child, a.size
    main = scene.main_camera_view()
    plain = [scene.cascade_view(index=k) for k in range(CASCADES)]
    depth = scene.noise_depth(1920, 1080)
    sc = scene.flat_scene(n)
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        vis.bind_pool(0, sc.meshes)
        vis.hierarchy_rebuild()

        def timed(views):
            vis.stats_reset()
            s = time.perf_counter()
            vis.cull(0, views)
            vis.wait()
            wall = (time.perf_counter() - s) * 1e6
            ms = vis.stats()["device_ms"]
            return wall, {k: ms[k] * 1e3 for k in KINDS}

        def mask(c):
            vis.receiver_begin(size, size)
            vis.draw_receivers(0, 0, plain[c]["view_proj"])
            vis.hiz_build_from_receivers()

        for profiled in (False, True):
            vis.profile_kernels(list(KINDS) if profiled else [])
            wall = {k: [] for k in "abcd"}
            stream = {k: {kind: [] for kind in KINDS} for k in "abcd"}
            kept = {}
            for frame in range(a.warmup + a.frames):
                got = {}
                # (b): three masks into three slots, one cull
                vis.cull(0, [main])
                for c in range(CASCADES):
                    vis.hiz_select(1 + c)
                    mask(c)
                vis.hiz_select(0)
                vis.wait()  # (the masks and their pyramids are not part of the timed cull)
                got["b"] = timed([main] + [dict(plain[c], use_hiz=2 + c) for c in range(CASCADES)])
                kept["batched"] = [vis.result_count(1 + c) for c in range(CASCADES)]
                # (a): one pyramid, one cascade at a time, every view named again
                w, s = 0.0, dict.fromkeys(KINDS, 0.0)
                kept["one_at_a_time"] = []
                for c in range(CASCADES):
                    mask(c)
                    vis.wait()
                    w1, s1 = timed([main] + [dict(plain[k], use_hiz=int(k == c)) for k in range(CASCADES)])
                    kept["one_at_a_time"].append(vis.result_count(1 + c))
                    w += w1
                    s = {k: s[k] + s1[k] for k in KINDS}
                got["a"] = (w, s)
                # (c), (d)
                got["c"] = timed([main] + plain)
                kept["frustum_only"] = [vis.result_count(1 + c) for c in range(CASCADES)]
                vis.hiz_build(depth)
                got["d"] = timed([dict(main, use_hiz=1)] + plain)
                assert kept["batched"] == kept["one_at_a_time"], kept
                if frame >= a.warmup:
                    for k in "abcd":
                        wall[k].append(got[k][0])
                        for kind in KINDS:
                            stream[k][kind].append(got[k][1][kind])
            names = dict(a="one_at_a_time", b="batched", c="frustum_only", d="hiz_view0")
            line = dict(n=n, mask=size, profiled=profiled, frames=a.frames, casters_kept=kept)
            for k, name in names.items():
                if profiled:
                    line[name + "_stream_us"] = {kind: stats(stream[k][kind]) for kind in KINDS}
                    line[name + "_stream_us"]["sum_of_medians"] = float(sum(np.median(stream[k][kind]) for kind in KINDS))
                else:
                    line[name + "_wall"] = stats(wall[k])
            print(json.dumps(line), flush=True)
            for k in range(1, 4):
                vis.hiz_drop(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", type=int, default=[1_000_000, 10_000_000], help="entities")
    ap.add_argument("--size", type=int, default=1024, help="side of the masks")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    for n in a.cases:  # a child process per case, each under its own time limit; nothing more is started behind a failure
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--size", str(a.size), "--frames", str(a.frames),
                              "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=a.limit)
        sys.stdout.write(run.stdout)
        sys.stdout.flush()
        if run.returncode != 0:
            sys.stderr.write(run.stderr[-4000:])
            return run.returncode
        if a.out:
            with open(a.out, "a") as f:
                f.write(run.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
