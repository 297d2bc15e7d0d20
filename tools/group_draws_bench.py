"""gv_pool_group_draws timing, the method of tools/lod_select_bench.py: cfg2 scene (flat, frustum-only main camera), wall-clock
microseconds per call (call + wait, after warm-up). A grouping changes the order it reads, so every timed call has a cull of its own
in front of it (cull + wait, untimed): each call groups the records as the cull emitted them. Per size:

    sort         gv_pool_sort of the same list in the same run, likewise behind a cull of its own: the parent's code, the yardstick.

    group        gv_pool_group_draws over a geometry table of 4 096 entries (two 8-bit digits), ids "one" (one geometry), "runs64" (64
                 geometries in runs of 64 slots) and "random4096"; without the flag and with GV_GROUP_BY_LOD (then the ids are base ids
                 at stride 4 of four levels each, a size per slot, thresholds at the world's own quartiles of distance / size).

    commands     gv_pool_emit_draw_commands in run mode behind ONE emission of the grouped view and behind one of the ungrouped view
                 (the parent's situation), with the command counts.

    host         what an engine does today (not with --no-host): fetch the records, np.argsort(kind="stable") of the keys, gather,
                 upload the three arrays again (torch, pinned-less host tensors to the device) — equality with the grouped fetch
                 asserted.

    python tools/group_draws_bench.py --n 1000000 --calls 100 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), ONE size per run, then --trace on the kernel trace it wrote —
the phases launch in a fixed order with a fixed number of calls, so the rows of each kernel are cut into phases by position:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/group_draws_bench.py --n 1000000 --calls 100 --no-host
    python tools/group_draws_bench.py --n 1000000 --calls 100 --trace DIR

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

ASSIGNMENTS = ["one", "runs64", "random4096"]
FLAGS = [False, True]
SOURCES = ["grouped", "ungrouped"]
LEVELS, BASES = 4, 1024
DIGITS = 2  # of K = 4 096


def timed(calls, warmup, before, fn, wait):
    samples = []
    for k in range(warmup + calls):
        if before:
            before()
            wait()
        s = time.perf_counter()
        fn()
        wait()
        if k >= warmup:
            samples.append(time.perf_counter() - s)
    us = np.array(samples) * 1e6
    return dict(us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)))


def ids_of(assignment, n, rng, by_lod):
    if assignment == "one":
        ids = np.zeros(n, np.uint32)
    elif assignment == "runs64":
        ids = ((np.arange(n) // 64) % 64).astype(np.uint32)
    else:
        ids = rng.integers(0, LEVELS * BASES, n).astype(np.uint32)
    return (ids // LEVELS) * LEVELS if by_lod else ids  # with levels: base ids at stride 4


def run(a):
    import commands_support as csup
    import group_support as gsup
    import instances_support as isup
    import lod_support as lsup
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    view = scene.main_camera_view()
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
        four = lsup.lod_table([(LEVELS, switch_at) if g % LEVELS == 0 else (1, []) for g in range(LEVELS * BASES)])
        twin = None
        with GpuVisibility(device=0) as vis:
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            vis.hierarchy_rebuild()
            cull = lambda: vis.cull(0, [view])
            cull()
            vis.wait()
            draws = int(vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)["draw_count"])
            vis.set_instance_layout(0, dtype=isup.BARE)
            vis.set_command_layout(0, dtype=csup.INDEXED)
            # ---- the yardstick: gv_pool_sort of the same list ----
            line = dict(n=n, phase="sort", draws=draws, calls=a.calls)
            line.update(timed(a.calls, a.warmup, cull, lambda: vis.sort(0, pool_id=0), vis.wait))
            report(line)
            for assignment in ASSIGNMENTS:
                for by_lod in FLAGS:
                    ids = ids_of(assignment, n, rng, by_lod)
                    vis.bind_geometry(0, ids, table)
                    vis.bind_lod(0, sizes, four)
                    group = lambda: vis.group_draws(0, pool_id=0, by_lod=by_lod, view_scale=1.0)
                    cull(), group(), vis.wait()  # (uploads the columns)
                    line = dict(n=n, phase="group", assignment=assignment, by_lod=by_lod, draws=draws, calls=a.calls)
                    line.update(timed(a.calls, a.warmup, cull, group, vis.wait))
                    report(line)
                    # ---- run-mode commands behind the grouped view, then behind the ungrouped one ----
                    for source in SOURCES:
                        if source == "ungrouped":
                            cull()
                        vis.emit_instances(0, [0])
                        if by_lod:
                            vis.select_lods(0, [1.0])
                        line = dict(n=n, phase="commands", assignment=assignment, by_lod=by_lod, source=source, draws=draws, calls=a.calls)
                        line.update(timed(a.calls, a.warmup, None, lambda: vis.emit_draw_commands(0, merge_runs=True), vis.wait))
                        _, command_counts = vis.draw_commands(0)
                        line["commands"] = int(command_counts[0])
                        report(line)
                    if a.no_host:
                        continue
                    # ---- the host alternative ----
                    import torch
                    if by_lod and twin is None:
                        import tempfile
                        twin = lsup.build_twin(tempfile.mkdtemp())
                    samples = []
                    for _ in range(3):
                        cull()
                        vis.wait()
                        s = time.perf_counter()
                        f = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
                        fetched = time.perf_counter()
                        lod = (twin, f["baked_model"], sizes, 1.0, four) if by_lod else None
                        kappa = gsup.keys(f["visible_idx"], ids, len(table), lod)
                        order = np.argsort(kappa, kind="stable")
                        host = gsup.expected_results(f, order)
                        ordered = time.perf_counter()
                        up = [torch.from_numpy(np.ascontiguousarray(host[k])).to("cuda:0") for k in ("visible_idx", "baked_model", "distance_sq")]
                        torch.cuda.synchronize()
                        samples.append((fetched - s, ordered - fetched, time.perf_counter() - ordered))
                        del up
                    group()
                    gsup.same_records(vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0), host, draws)  # the two ways agree
                    fetch_s, order_s, upload_s = np.median(np.array(samples), axis=0)
                    report(dict(n=n, phase="host", assignment=assignment, by_lod=by_lod, draws=draws, fetch_us=float(fetch_s * 1e6),
                                order_us=float(order_s * 1e6), upload_us=float(upload_s * 1e6), host_us=float((fetch_s + order_s + upload_s) * 1e6)))
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def summarise(a):
    """the kernel rows of a rocprofv3 --kernel-trace csv of the same command line (one size, --no-host), cut into phases by position"""
    assert len(a.n) == 1
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    names = ["group_key_kernel", "group_rank_kernel", "group_scatter_kernel", "command_heads_kernel", "command_runs_kernel", "command_kernel"]
    rows = {k: [] for k in names + ["sort_"]}
    with open(files[0]) as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in trace:
        for key in rows:  # (command_kernel behind the names that do not contain it)
            if key in r["Kernel_Name"]:
                rows[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                break
    per = a.warmup + a.calls
    cells = len(ASSIGNMENTS) * len(FLAGS)
    # every sort_ kernel of the run belongs to the sort phase (warm-up included: its calls are not told apart by position, the number
    # of launches per call depends on the previous frame's count)
    print(json.dumps(dict(n=a.n[0], phase="sort", calls=per, launches_per_call=len(rows["sort_"]) / per,
                          kernels_us_avg=float(np.sum(rows["sort_"]) / per))), flush=True)
    assert len(rows["group_key_kernel"]) == cells * (per + 1), len(rows["group_key_kernel"])
    assert len(rows["group_rank_kernel"]) == cells * (per + 1) * (DIGITS - 1) and len(rows["group_scatter_kernel"]) == cells * (per + 1) * DIGITS
    assert len(rows["command_kernel"]) == len(rows["command_heads_kernel"]) == len(rows["command_runs_kernel"]) == cells * len(SOURCES) * per

    def avg(us, width=1):  # `width` launches per call
        us = np.array(us).reshape(-1, width).sum(axis=1)
        return float(us.mean())

    cell = 0
    for assignment in ASSIGNMENTS:
        for by_lod in FLAGS:
            at = cell * (per + 1) + 1 + a.warmup  # (one untimed call in front of every cell's loop)
            key = avg(rows["group_key_kernel"][at:at + a.calls])
            rank = avg(rows["group_rank_kernel"][at * (DIGITS - 1):(at + a.calls) * (DIGITS - 1)], DIGITS - 1)
            scatter = avg(rows["group_scatter_kernel"][at * DIGITS:(at + a.calls) * DIGITS], DIGITS)
            print(json.dumps(dict(n=a.n[0], phase="group", assignment=assignment, by_lod=by_lod, calls=a.calls, key_us=key, rank_us=rank,
                                  scatter_us=scatter, kernels_us_avg=key + rank + scatter)), flush=True)
            for s, source in enumerate(SOURCES):
                at = (cell * len(SOURCES) + s) * per + a.warmup
                parts = {k: avg(rows[k][at:at + a.calls]) for k in names[3:]}
                print(json.dumps(dict(n=a.n[0], phase="commands", assignment=assignment, by_lod=by_lod, source=source, calls=a.calls,
                                      kernels_us_avg=sum(parts.values()), **{k + "_us": v for k, v in parts.items()})), flush=True)
            cell += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the host alternative (the run under rocprofv3)")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace --output-format csv run of the same --n (one size) / --calls / --warmup")
    a = ap.parse_args()
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
