"""gv_pool_emit_draw_instances timing, the method of tools/instances_bench.py: cfg2 scene (flat, frustum-only main camera), wall-clock
microseconds per call (emission + wait, after warm-up), for the bare 64-byte layout and the sprite struct (stride 96, 32 bytes of
payload). Three phases per size and layout, over the SAME records of one cull:

    one_launch   gv_pool_emit_instances (instance_kernel, one launch) with a ready column of ones
    count1       gv_pool_emit_draw_instances (draw_counts_kernel + draw_instances_kernel) with the same column: the same bytes
    mean4        gv_pool_emit_draw_instances with counts uniform in 1 .. 7 (mean 4)

    python tools/draw_instances_bench.py --n 1000000 10000000 --calls 200 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), then --trace on the kernel trace it wrote — the phases
launch in a fixed order with a fixed number of calls, so the rows of each kernel are cut into phases by position:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/draw_instances_bench.py --n 1000000 10000000 --calls 100
    python tools/draw_instances_bench.py --n 1000000 10000000 --calls 100 --trace DIR

Prints one JSON line per size, layout and phase."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAYOUTS = ["bare64", "sprite96"]
PHASES = ["one_launch", "count1", "mean4"]


def run(a):
    import instances_support as isup
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    view = scene.main_camera_view()
    sprite = isup.layout_dtype(96, mvp=0)
    lines = []
    for n in a.n:
        sc = scene.flat_scene(n)
        rng = np.random.Generator(np.random.PCG64(n))
        ones = np.ones(n, np.uint32)
        mixed = rng.integers(1, 8, n, dtype=np.uint32)  # never 0: the candidates, hence the records, stay those of the cull
        payload = [rng.integers(0, 1 << 32, (n, 4), dtype=np.uint32) for _ in range(2)]
        with GpuVisibility(device=0) as vis:
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            vis.bind_ready(0, ones)
            vis.hierarchy_rebuild()
            vis.cull(0, [view])
            vis.wait()
            records = vis.result_count(0)
            for name in LAYOUTS:
                dtype = isup.BARE if name == "bare64" else sprite
                if name == "sprite96":
                    vis.bind_payload(0, payload)
                vis.set_instance_layout(0, dtype=dtype)
                if name == "sprite96":
                    vis.set_payload_layout(0, [64, 80])
                for phase in PHASES:
                    vis.bind_ready(0, mixed if phase == "mean4" else ones)  # (a rebind resets the count mirror: the first call uploads it)
                    emit = vis.emit_instances if phase == "one_launch" else vis.emit_draw_instances
                    samples = []
                    for k in range(a.warmup + a.calls):
                        s = time.perf_counter()
                        emit(0, [0])
                        vis.wait()
                        if k >= a.warmup:
                            samples.append(time.perf_counter() - s)
                    starts = np.zeros(2, np.uint32)  # (the starts alone: the instances stay on the device)
                    vis._check(vis.lib.gv_pool_instances_fetch(vis.ctx, 0, None, 0, starts.ctypes.data_as(C.POINTER(C.c_uint32)), 2))
                    us = np.array(samples) * 1e6
                    line = dict(n=n, layout=name, phase=phase, stride=dtype.itemsize, records=records, instances=int(starts[1]), calls=a.calls,
                                us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)))
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                if name == "sprite96":
                    vis.bind_payload(0, None)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def summarise(a):
    """the kernel rows of a rocprofv3 --kernel-trace csv of the same command line, cut into the phases by position"""
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = {"instance_kernel": [], "draw_counts_kernel": [], "draw_instances_kernel": []}
    with open(files[0]) as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in trace:
        for key in sorted(rows, key=len, reverse=True):
            if key in r["Kernel_Name"] and (key != "instance_kernel" or "draw_" not in r["Kernel_Name"]):
                rows[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                break
    per = a.warmup + a.calls
    cells = len(a.n) * len(LAYOUTS)
    assert len(rows["instance_kernel"]) == cells * per, (len(rows["instance_kernel"]), cells * per)
    assert len(rows["draw_counts_kernel"]) == len(rows["draw_instances_kernel"]) == 2 * cells * per
    cell = 0
    for n in a.n:
        for name in LAYOUTS:
            for phase in PHASES:
                line = dict(n=n, layout=name, phase=phase, calls=a.calls)
                if phase == "one_launch":
                    kernels = {"instance_kernel": rows["instance_kernel"][cell * per:(cell + 1) * per]}
                else:
                    at = (2 * cell + (phase == "mean4")) * per
                    kernels = {k: rows[k][at:at + per] for k in ("draw_counts_kernel", "draw_instances_kernel")}
                total = 0.0
                for k, us in kernels.items():
                    us = np.array(us[a.warmup:])
                    line[k + "_us"] = dict(avg=float(us.mean()), min=float(us.min()), max=float(us.max()))
                    total += float(us.mean())
                line["kernels_us_avg"] = total
                print(json.dumps(line), flush=True)
            cell += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace --output-format csv run of the same --n / --calls / --warmup")
    a = ap.parse_args()
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
