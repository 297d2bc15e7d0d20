"""gv_pool_keep_models / gv_pool_emit_previous timing, the method of tools/receiver_bench.py: cfg3's world (flat, the main camera,
frustum only), two alternating cameras a small step apart so that most of a frame's draws were drawn the frame before. Per case, per
frame: one gv_cull of the main view, waited for, then each of

    instances_64    gv_pool_emit_instances, stride 64 (mvp alone): the parent's call, the baseline of the same run on the same box
    instances_128   ... stride 128 (mvp at 0): the buffer the pair below shares
    previous_64     gv_pool_emit_previous, stride 64 into the library's buffer (the whole-line path)
    previous_128    gv_pool_emit_previous, stride 128, prev_mvp at 64 beside mvp in the pool's own instance buffer ({mvp, prevMvp})
    keep            gv_pool_keep_models

as microseconds of call + wait (time.perf_counter), median over --frames frames after --warmup; and, in a pass of its own because a
bracket costs stream time, the library's event brackets around the call's launch (gv_profile_kernels, kind "emit": the keep and the
previous emission have one, the instance emission's launch has none); and --burst calls of one kind back to back with one wait.

    host            the alternative without the library's history: fetch this frame's records, join them by slot with last frame's
                    fetched records (numpy), multiply (float32 matmul, not the rule's fma nesting: a timing, not a check)

    python tools/previous_bench.py [--cases 1000000 10000000] [--out FILE]

Prints one JSON line per case and pass."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(us):
    us = np.array(us)
    return dict(us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)))


def host_join(vis, n, view, kept_view, last):
    """(seconds, kept draws) of the host path over this frame's records and last frame's fetched ones"""
    s = time.perf_counter()
    now = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
    slots, models = now["visible_idx"], now["baked_model"].reshape(-1, 12)
    row_of = np.full(n, -1, np.int64)
    row_of[last["visible_idx"]] = np.arange(len(last["visible_idx"]))
    rows = row_of[slots]
    kept = rows >= 0
    d = (view["camera_position"][:3] - kept_view["camera_position"][:3]).astype(np.float32)
    previous = models.copy()
    previous[:, 9:12] += d
    previous[kept] = last["baked_model"].reshape(-1, 12)[rows[kept]]
    full = np.zeros((len(slots), 4, 4), np.float32)  # [k][column][row]
    full[:, :, :3] = previous.reshape(-1, 4, 3)
    full[:, 3, 3] = 1.0
    pvp = kept_view["view_proj"].reshape(4, 4)       # [column][row]
    out = np.einsum("cr,kjc->kjr", pvp, full).astype(np.float32)
    return time.perf_counter() - s, int(kept.sum()), now, out


def run(a):
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    cameras = [scene.main_camera_view(), scene.main_camera_view(camera_position=(2.5, -1.25, 3.0))]
    names = ("instances_64", "instances_128", "previous_64", "previous_128", "keep")
    for n in a.cases:
        sc = scene.flat_scene(n)
        with GpuVisibility(device=0) as vis:
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            vis.hierarchy_rebuild()
            for profiled in (False, True):
                vis.profile_kernels(["emit"] if profiled else [])
                wall, kernel = {k: [] for k in names}, {k: [] for k in names}
                counts = None

                def timed(name, fn, keep):
                    vis.wait()
                    vis.stats_reset()
                    s = time.perf_counter()
                    fn()
                    vis.wait()
                    us = (time.perf_counter() - s) * 1e6
                    if keep:
                        wall[name].append(us)
                        kernel[name].append(vis.stats()["device_ms"]["emit"] * 1e3)

                for k in range(a.warmup + a.frames):
                    keep = k >= a.warmup
                    vis.cull(0, [cameras[k % 2]])
                    vis.wait()
                    vis.set_instance_layout(0, stride=64, mvp=0)
                    timed("instances_64", lambda: vis.emit_instances(0, [0]), keep)
                    timed("previous_64", lambda: vis.emit_previous(0, 0), keep)
                    vis.set_instance_layout(0, stride=128, mvp=0)
                    timed("instances_128", lambda: vis.emit_instances(0, [0]), keep)
                    target, _ = vis.instances_device(0)
                    _, stride, capacity = vis.instances_info(0)
                    timed("previous_128", lambda: vis.emit_previous(0, 0, stride=128, prev_mvp=64, device=(target, capacity * stride)), keep)
                    if k == a.warmup:
                        counts = vis.previous(0, counts_only=True)[1].tolist()
                    timed("keep", lambda: vis.keep_models(0, 0), keep)
                line = dict(n=n, profiled=profiled, frames=a.frames, counts_n_kept_written_epoch=counts)
                for name in names:
                    line[name] = stats(kernel[name] if profiled else wall[name])
                line["what"] = "kernel_us (event brackets)" if profiled else "wall_us (call + wait)"
                base = line["instances_64"]["us_median"]
                if base > 0:  # (the instance emission's launch has no event bracket: the profiled pass has nothing to divide by)
                    line["ratio_to_instances_64"] = {name: round(line[name]["us_median"] / base, 3) for name in names}
                report(line)
            # back to back: --burst calls of one kind issued without a wait between them, then one wait — the launch latency of the
            # single call overlaps the call in front of it, so the figure per call is the stream time (memset included)
            vis.profile_kernels([])
            vis.cull(0, [cameras[0]])
            vis.set_instance_layout(0, stride=64, mvp=0)
            calls = dict(instances_64=lambda: vis.emit_instances(0, [0]), previous_64=lambda: vis.emit_previous(0, 0),
                         previous_80_flag=lambda: vis.emit_previous(0, 0, stride=80, has_history=64), keep=lambda: vis.keep_models(0, 0, add=True))
            burst = {}
            for name, fn in calls.items():
                per_call = []
                for _ in range(a.warmup + a.frames):
                    vis.wait()
                    s = time.perf_counter()
                    for _ in range(a.burst):
                        fn()
                    vis.wait()
                    per_call.append((time.perf_counter() - s) * 1e6 / a.burst)
                burst[name] = stats(per_call[a.warmup:])
            report(dict(n=n, what="us per call, %d calls back to back then one wait" % a.burst, **burst,
                        ratio_to_instances_64={k: round(v["us_median"] / burst["instances_64"]["us_median"], 3) for k, v in burst.items()}))
            # the host path: two frames' records fetched and joined by slot
            vis.profile_kernels([])
            host = []
            vis.cull(0, [cameras[0]])
            last = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
            kept = 0
            for k in range(1, 1 + a.host_frames):
                vis.cull(0, [cameras[k % 2]])
                vis.wait()
                seconds, kept, last, _ = host_join(vis, n, cameras[k % 2], cameras[(k + 1) % 2], last)
                host.append(seconds * 1e6)
            report(dict(n=n, host_fetch_join_multiply=stats(host), host_frames=a.host_frames, kept=kept))
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", type=int, default=[1_000_000, 10_000_000], help="entities")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--burst", type=int, default=32)
    ap.add_argument("--out", default=None)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
