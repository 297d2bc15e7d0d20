"""gv_pool_cull_clusters timing, the method of tools/draw_commands_bench.py: cfg2 scene (flat, the main camera), the 20-byte indexed
command layout, behind ONE gv_pool_emit_instances of one cull of the main view. Every slot draws one geometry of 8 (2^3) or 64 (4^3)
clusters, a regular sub-grid of the box [-1, 1]^3; the cull runs frustum only, and against a 1024^2 pyramid (synthetic depth) the
view names. Per size, cluster count and mode one JSON line:

    us_median      wall-clock microseconds per call (the call + the wait, after warm-up)
    per_draw_us    the per-draw command emission (gv_pool_emit_draw_commands) in the same run
    host_us        the host alternative: fetch the records, run the twin (tests/cluster_twin.h, the oracle's tests) on 16 threads over
                   the draws, upload the commands; its bytes are asserted equal to the device's
    tested / kept  clusters tested and commands written; bytes_per_candidate: what the five launches move per candidate by count
                   (cluster 32 B + model 48 B shared by the draw's clusters + prefix words + a bit + the command for survivors)

    python tools/cluster_cull_bench.py --n 1000000 10000000 --calls 100 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), then --trace on the kernel trace it wrote — the launches come
in a fixed order with a fixed number of calls, so the rows of each kernel are cut into the cells by position:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cluster_cull_bench.py --n 1000000 --calls 100 --no-host
    python tools/cluster_cull_bench.py --n 1000000 --calls 100 --trace DIR"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLUSTERS = [8, 64]
MODES = ["frustum", "hiz"]
KERNELS = ["cluster_count_kernel", "cluster_scan_kernel<0", "cluster_test_kernel", "cluster_scan_kernel<1", "cluster_write_kernel"]  # as the trace names them
THREADS = 16


def grid_clusters(count):
    from garden_amd.lib import CLUSTER_DTYPE
    cells = round(count ** (1.0 / 3.0))
    assert cells ** 3 == count
    out = np.zeros(count, CLUSTER_DTYPE)
    for j in range(count):
        at = np.array([j % cells, j // cells % cells, j // (cells * cells)], np.float32)
        out[j]["box_min"] = -1.0 + 2.0 * at / cells
        out[j]["box_max"] = -1.0 + 2.0 * (at + 1) / cells
        out[j]["first"], out[j]["count"] = 3 * 128 * j, 3 * 128
    return out


def host_alternative(ksup, fetched, table, ranges, clusters, view_proj, hiz, dtype):
    """records on the host -> the twin over THREADS slices of the draws -> the command structs"""
    n = int(fetched["draw_count"])
    models = np.ascontiguousarray(fetched["baked_model"], np.float32).reshape(-1, 12)[:n]
    g = np.zeros(n, np.uint32)
    first = np.arange(n + 1, dtype=np.uint32)
    edges = np.linspace(0, n, THREADS + 1).astype(np.int64)

    def part(k):
        lo, hi = int(edges[k]), int(edges[k + 1])
        return ksup.view_commands(models[lo:hi], g[lo:hi], first[lo:hi + 1], view_proj, hiz, table, ranges, clusters)

    with ThreadPoolExecutor(THREADS) as pool:
        parts = list(pool.map(part, range(THREADS)))
    commands = np.concatenate([p[0] for p in parts])
    out = np.zeros(len(commands), dtype)
    for name in dtype.names:
        out[name] = commands[name]
    return out, sum(p[1] for p in parts)


def run(a):
    import torch

    import clusters_support as ksup
    import commands_support as csup
    import instances_support as isup
    from garden_amd import scene
    from garden_amd.lib import CLUSTER_RANGE_DTYPE, GpuVisibility
    from oracle import oracle_py

    dtype = csup.INDEXED  # (no draw field: a slice of the host alternative numbers its draws from 0)
    depth = scene.synthetic_depth(1024, 1024)
    lines = []
    for n in a.n:
        sc = scene.flat_scene(n)
        table = csup.geometry_table([(3 * 128 * 64, 0, 0)])
        for mode in MODES:
            view = scene.main_camera_view(use_hiz=1 if mode == "hiz" else 0)
            with GpuVisibility(device=0) as vis:
                vis.bind_transforms(sc.transforms, sc.entity_to_transform)
                vis.bind_pool(0, sc.meshes)
                vis.hierarchy_rebuild()
                if mode == "hiz":
                    vis.hiz_build(depth)
                vis.cull(0, [view])
                vis.wait()
                vis.set_instance_layout(0, dtype=isup.BARE)
                vis.emit_instances(0, [0])
                vis.set_command_layout(0, dtype=dtype)
                vis.bind_geometry(0, None, table)
                samples = []
                for k in range(a.warmup + a.calls):
                    s = time.perf_counter()
                    vis.emit_draw_commands(0)
                    vis.wait()
                    if k >= a.warmup:
                        samples.append(time.perf_counter() - s)
                per_draw_us = float(np.median(samples) * 1e6)
                for count in CLUSTERS:
                    clusters = grid_clusters(count)
                    ranges = np.zeros(1, CLUSTER_RANGE_DTYPE)
                    ranges[0] = (0, count)
                    vis.bind_clusters(0, ranges, clusters)
                    # the target is the caller's, sized from a first call that holds nothing (the counts are always the true ones)
                    probe = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    vis.cull_clusters(0, device=(probe.data_ptr(), 64))
                    _, counts, tested = vis.cluster_commands(0)
                    kept = int(counts[0])
                    dev = torch.zeros((kept + 1, dtype.itemsize), dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    target = (dev.data_ptr(), dev.numel())
                    samples = []
                    for k in range(a.warmup + a.calls):
                        s = time.perf_counter()
                        vis.cull_clusters(0, device=target)
                        vis.wait()
                        if k >= a.warmup:
                            samples.append(time.perf_counter() - s)
                    us = np.array(samples) * 1e6
                    host_us = None
                    if not a.no_host:
                        hiz = oracle_py.Hiz(depth) if mode == "hiz" else None
                        s = time.perf_counter()
                        fetched = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
                        exp, host_tested = host_alternative(ksup, fetched, table, ranges, clusters, view["view_proj"], hiz, dtype)
                        up = torch.from_numpy(exp.view(np.uint8).reshape(-1, dtype.itemsize)).to("cuda:0")
                        torch.cuda.synchronize()
                        host_us = float((time.perf_counter() - s) * 1e6)
                        got, _, _ = vis.cluster_commands(0, dtype=dtype)
                        assert host_tested == int(tested[0]) and got[:kept].tobytes() == exp.tobytes()  # the two ways write the same bytes
                        del up
                    draws = int(tested[0]) // count
                    moved = int(tested[0]) * (32 + 4 + 4) + draws * (48 + 12 + 8 + 12) + int(tested[0]) // 4 + kept * (dtype.itemsize + 32 + 48)
                    line = dict(n=n, clusters=count, mode=mode, stride=dtype.itemsize, draws=draws, tested=int(tested[0]), kept=kept, calls=a.calls,
                                us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)),
                                per_draw_us=per_draw_us, host_us=host_us, bytes_per_candidate=moved / max(int(tested[0]), 1))
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del dev
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def summarise(a):
    """the kernel rows of a rocprofv3 --kernel-trace csv of the same command line (with --no-host), cut into the cells by position:
    per cell one probing call, then warmup + calls"""
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = {k: [] for k in KERNELS}
    with open(files[0]) as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in trace:
        for key in KERNELS:
            if key in r["Kernel_Name"].replace(" ", ""):
                rows[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                break
    per = 1 + a.warmup + a.calls
    cell = 0
    for n in a.n:
        for mode in MODES:
            for count in CLUSTERS:
                line = dict(n=n, clusters=count, mode=mode, calls=a.calls)
                total = 0.0
                for k in KERNELS:
                    assert len(rows[k]) == per * len(a.n) * len(MODES) * len(CLUSTERS), (k, len(rows[k]))
                    us = np.array(rows[k][cell * per + 1 + a.warmup:(cell + 1) * per])
                    line[k + "_us"] = dict(avg=float(us.mean()), min=float(us.min()), max=float(us.max()))
                    total += float(us.mean())
                line["kernels_us_avg"] = total
                print(json.dumps(line), flush=True)
                cell += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the host alternative (the run under rocprofv3)")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace --output-format csv run of the same --n / --calls / --warmup")
    a = ap.parse_args()
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
