"""gv_pool_select_lods timing, the method of tools/draw_commands_bench.py: cfg2 scene (flat, frustum-only main camera), wall-clock
microseconds per call (call + wait, after warm-up) behind ONE gv_pool_emit_instances of one cull. Per size:

    select       gv_pool_select_lods over 1 024 base geometries of four levels each (4 096 geometry table entries), a size per slot,
                 thresholds at the world's own quartiles of distance / size — and beside it the host alternative an engine has today,
                 timed in the same run: fetch the records, then one vectorised numpy pass that computes the same g_k (the fused
                 multiply-adds restated in float64), equality asserted (`host_us`).

    commands     gv_pool_emit_draw_commands behind the selection against the SAME emission from the id mirror (the selected ids
                 scattered into a per-slot column and bound, the selection dropped), bytes asserted equal; per-draw and run mode;
                 ids "one" (one geometry of one level: every g_k is 0) and "random4096" (the four-level table above).

    python tools/lod_select_bench.py --n 1000000 10000000 --calls 200 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), then --trace on the kernel trace it wrote — the phases
launch in a fixed order with a fixed number of calls, so the rows of each kernel are cut into phases by position:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/lod_select_bench.py --n 1000000 10000000 --calls 100 --no-host
    python tools/lod_select_bench.py --n 1000000 10000000 --calls 100 --trace DIR

Prints one JSON line per size and phase."""
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

ASSIGNMENTS = ["one", "random4096"]
MODES = ["per_draw", "runs"]
SOURCES = ["selection", "id_mirror"]
KERNELS = ["lod_kernel", "command_heads_kernel", "command_runs_kernel", "command_kernel"]
LEVELS, BASES = 4, 1024


def host_select(slots, models, ids, sizes, scale, levels, switch_at):
    """the rule of DESIGN.md §4 item 11 over fetched records, vectorised (every base geometry has the same `levels` thresholds)"""
    t = models.reshape(-1, 12)[:, 9:12].astype(np.float64)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    d2 = f32(t[:, 2] * t[:, 2] + f32(t[:, 1] * t[:, 1] + f32(t[:, 0] * t[:, 0])))  # fmaf(tz, tz, fmaf(ty, ty, tx * tx))
    x = (d2.astype(np.float32) * np.float32(scale))
    r = sizes[slots]
    level = np.zeros(len(slots), np.uint32)
    for i in range(levels - 1):
        y = r * np.float32(switch_at[i])
        level += x > y * y
    return ids[slots] + level


def timed(calls, warmup, fn, wait):
    samples = []
    for k in range(warmup + calls):
        s = time.perf_counter()
        fn()
        wait()
        if k >= warmup:
            samples.append(time.perf_counter() - s)
    us = np.array(samples) * 1e6
    return dict(us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)))


def run(a):
    import commands_support as csup
    import instances_support as isup
    import lod_support as lsup
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    view = scene.main_camera_view()
    dtype = csup.INDEXED
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for n in a.n:
        sc = scene.flat_scene(n)
        rng = np.random.Generator(np.random.PCG64(n))
        table = csup.geometry_table([(36 * (g % 97 + 1), 36 * g, g % 13) for g in range(LEVELS * BASES)])
        sizes = rng.uniform(0.5, 4.0, n).astype(np.float32)
        switch_at = lsup.quantile_thresholds(sc.transforms["position"], sizes, LEVELS)
        random_ids = (rng.integers(0, BASES, n) * LEVELS).astype(np.uint32)
        four = lsup.lod_table([(LEVELS, switch_at) if g % LEVELS == 0 else (1, []) for g in range(LEVELS * BASES)])
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
            # ---- select ----
            vis.bind_geometry(0, random_ids, table)
            vis.bind_lod(0, sizes, four)
            line = dict(n=n, phase="select", draws=draws, levels=LEVELS, calls=a.calls)
            line.update(timed(a.calls, a.warmup, lambda: vis.select_lods(0, [1.0]), vis.wait))
            got, counts = vis.lods(0)
            line["level_counts"] = counts[0].tolist()
            if not a.no_host:  # what an engine does today: records to the host, one pass that picks the levels
                samples = []
                for _ in range(3):
                    s = time.perf_counter()
                    f = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
                    g = host_select(f["visible_idx"], f["baked_model"], random_ids, sizes, 1.0, LEVELS, switch_at)
                    samples.append(time.perf_counter() - s)
                assert g.tolist() == got[0].tolist()  # the two ways select the same ids
                line["host_us"] = float(np.median(samples) * 1e6)
            report(line)
            # ---- commands behind the selection against the same emission from the id mirror ----
            for assignment in ASSIGNMENTS:
                base_ids = np.zeros(n, np.uint32) if assignment == "one" else random_ids
                lod = lsup.lod_table([(1, [])]) if assignment == "one" else four
                for mode in MODES:
                    vis.bind_geometry(0, base_ids, table)
                    vis.bind_lod(0, sizes, lod)
                    vis.select_lods(0, [1.0])
                    selected = vis.lods(0)[0][0]
                    effective = np.zeros(n, np.uint32)
                    effective[order] = selected  # the same ids, per slot
                    produced = {}
                    for source in SOURCES:
                        if source == "id_mirror":
                            vis.bind_geometry(0, effective, table)
                            vis.select_lods(0, None)
                        line = dict(n=n, phase="commands", assignment=assignment, mode=mode, source=source, stride=dtype.itemsize, draws=draws,
                                    calls=a.calls)
                        line.update(timed(a.calls, a.warmup, lambda: vis.emit_draw_commands(0, merge_runs=mode == "runs"), vis.wait))
                        bytes_, command_counts = vis.draw_commands(0)
                        produced[source] = bytes_.tobytes()
                        line["commands"] = int(command_counts[0])
                        report(line)
                    assert produced["selection"] == produced["id_mirror"]  # the two sources write the same bytes
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
    cells = len(ASSIGNMENTS) * len(MODES)  # per size; each cell: one selection, then `per` emissions per source
    assert len(rows["lod_kernel"]) == len(a.n) * (per + cells), (len(rows["lod_kernel"]), len(a.n) * (per + cells))
    assert len(rows["command_kernel"]) == len(a.n) * cells * len(SOURCES) * per
    assert len(rows["command_heads_kernel"]) == len(rows["command_runs_kernel"]) == len(a.n) * len(ASSIGNMENTS) * len(SOURCES) * per

    def stats(us):
        us = np.array(us[a.warmup:])
        return dict(avg=float(us.mean()), min=float(us.min()), max=float(us.max()))

    for i, n in enumerate(a.n):
        at = i * (per + cells)
        print(json.dumps(dict(n=n, phase="select", calls=a.calls, lod_kernel_us=stats(rows["lod_kernel"][at:at + per]))), flush=True)
        for j, assignment in enumerate(ASSIGNMENTS):
            for m, mode in enumerate(MODES):
                for s, source in enumerate(SOURCES):
                    line = dict(n=n, phase="commands", assignment=assignment, mode=mode, source=source, calls=a.calls)
                    at = (((i * len(ASSIGNMENTS) + j) * len(MODES) + m) * len(SOURCES) + s) * per
                    kernels = {"command_kernel": rows["command_kernel"][at:at + per]}
                    if mode == "runs":
                        at = ((i * len(ASSIGNMENTS) + j) * len(SOURCES) + s) * per
                        for k in KERNELS[1:3]:
                            kernels[k] = rows[k][at:at + per]
                    total = 0.0
                    for k, us in kernels.items():
                        line[k + "_us"] = stats(us)
                        total += line[k + "_us"]["avg"]
                    line["kernels_us_avg"] = total
                    print(json.dumps(line), flush=True)


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
