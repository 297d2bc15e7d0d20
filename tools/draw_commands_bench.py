"""gv_pool_emit_draw_commands timing, the method of tools/draw_instances_bench.py: cfg2 scene (flat, frustum-only main camera), the
20-byte indexed command layout, wall-clock microseconds per call (emission + wait, after warm-up) behind ONE gv_pool_emit_instances
of one cull. Per size, three id assignments x two modes:

    one          every slot has geometry 0 (an id column of zeros)
    runs64       64 geometries dealt in runs of 64 draws along the draw order (the mirror's Morton order: a cell's entities
                 share a geometry)
    random4096   random ids of 4 096 geometries: no runs to speak of

    per_draw     flags 0: command_kernel, one launch
    runs         GV_COMMANDS_MERGE_RUNS: command_heads_kernel + command_runs_kernel + command_kernel

and beside each assignment the host alternative an engine has today, timed in the same run: fetch the records (visible_idx in draw
order), then one pass on the CPU that writes the same per-draw structs (numpy, vectorised: `host_us`).

    python tools/draw_commands_bench.py --n 1000000 10000000 --calls 200 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), then --trace on the kernel trace it wrote — the phases
launch in a fixed order with a fixed number of calls, so the rows of each kernel are cut into phases by position:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/draw_commands_bench.py --n 1000000 10000000 --calls 100 --no-host
    python tools/draw_commands_bench.py --n 1000000 10000000 --calls 100 --trace DIR

Prints one JSON line per size, assignment and mode."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ASSIGNMENTS = ["one", "runs64", "random4096"]
MODES = ["per_draw", "runs"]
KERNELS = ["command_heads_kernel", "command_runs_kernel", "command_kernel"]


def run(a):
    import commands_support as csup
    import instances_support as isup
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    view = scene.main_camera_view()
    dtype = csup.INDEXED
    lines = []
    for n in a.n:
        sc = scene.flat_scene(n)
        rng = np.random.Generator(np.random.PCG64(n))
        table = csup.geometry_table([(36 * (g % 97 + 1), 36 * g, g % 13) for g in range(4096)])
        with GpuVisibility(device=0) as vis:
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            vis.hierarchy_rebuild()
            vis.cull(0, [view])
            vis.wait()
            order = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)["visible_idx"].copy()
            draws = len(order)
            vis.set_instance_layout(0, dtype=isup.BARE)
            vis.emit_instances(0, [0])
            vis.set_command_layout(0, dtype=dtype)
            for assignment in ASSIGNMENTS:
                ids = np.zeros(n, np.uint32)
                if assignment == "runs64":
                    ids[order] = (np.arange(draws) // 64) % 64
                elif assignment == "random4096":
                    ids[:] = rng.integers(0, 4096, n, dtype=np.uint32)
                vis.bind_geometry(0, ids, table)  # (a rebind resets the id mirror: the first call uploads it)
                host_us = None
                if not a.no_host:  # what an engine does today: records to the host, one pass that writes the structs
                    samples = []
                    for _ in range(3):
                        s = time.perf_counter()
                        slots = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)["visible_idx"]
                        g = table[ids[slots]]
                        out = np.zeros(len(slots), dtype)
                        out["count"], out["first"], out["vertex_offset"] = g["count"], g["first"], g["vertex_offset"]
                        out["instance_count"] = 1
                        out["first_instance"] = np.arange(len(slots), dtype=np.uint32)
                        samples.append(time.perf_counter() - s)
                    host_us = float(np.median(samples) * 1e6)
                for mode in MODES:
                    samples = []
                    for k in range(a.warmup + a.calls):
                        s = time.perf_counter()
                        vis.emit_draw_commands(0, merge_runs=mode == "runs")
                        vis.wait()
                        if k >= a.warmup:
                            samples.append(time.perf_counter() - s)
                    got, counts = vis.draw_commands(0, dtype=dtype)
                    if not a.no_host and mode == "per_draw":
                        assert got.tobytes() == out.tobytes()  # the two ways write the same bytes
                    us = np.array(samples) * 1e6
                    line = dict(n=n, assignment=assignment, mode=mode, stride=dtype.itemsize, draws=draws, commands=int(counts[0]), calls=a.calls,
                                us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)),
                                host_us=host_us)
                    print(json.dumps(line), flush=True)
                    lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def summarise(a):
    """the kernel rows of a rocprofv3 --kernel-trace csv of the same command line, cut into the phases by position"""
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = {k: [] for k in KERNELS}
    with open(files[0]) as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in trace:
        for key in KERNELS:  # (command_kernel last: the other names do not contain it, nor it them)
            if key in r["Kernel_Name"]:
                rows[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                break
    per = a.warmup + a.calls
    cells = len(a.n) * len(ASSIGNMENTS)
    assert len(rows["command_kernel"]) == 2 * cells * per, (len(rows["command_kernel"]), 2 * cells * per)
    assert len(rows["command_heads_kernel"]) == len(rows["command_runs_kernel"]) == cells * per
    cell = 0
    for n in a.n:
        for assignment in ASSIGNMENTS:
            for mode in MODES:
                line = dict(n=n, assignment=assignment, mode=mode, calls=a.calls)
                at = (2 * cell + (mode == "runs")) * per
                kernels = {"command_kernel": rows["command_kernel"][at:at + per]}
                if mode == "runs":
                    for k in KERNELS[:2]:
                        kernels[k] = rows[k][cell * per:(cell + 1) * per]
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
    ap.add_argument("--no-host", action="store_true", help="skip the host alternative (the run under rocprofv3)")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace --output-format csv run of the same --n / --calls / --warmup")
    a = ap.parse_args()
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
