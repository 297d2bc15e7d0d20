"""gv_pool_cull_cluster_cones timing beside gv_pool_cull_clusters in the same run, the method of tools/cluster_cull_bench.py: cfg2 scene
(flat, the main camera), the 20-byte indexed command layout, behind ONE gv_pool_emit_instances of one cull of the main view. Every
slot draws one geometry of 8 (2^3) or 64 (4^3) clusters, a regular sub-grid of the box [-1, 1]^3, each with an OUTWARD cone: the axis
from the model's origin through the cell's centre, the apex half a cell diagonal inside it, cutoff 0.5. The cull runs frustum only,
and against a 1024^2 pyramid (synthetic depth) the view names. Per size, cluster count and mode one JSON line:

    plain_us       gv_pool_cull_clusters: wall-clock microseconds per call (the call + the wait), the median of --calls after --warmup
    zero_us        gv_pool_cull_cluster_cones with an all-zero eye: the cone rejects nothing and the commands are the plain form's, so
                   the difference to plain_us is the price of the 32 extra bytes per cluster and the arithmetic
    cone_us        ... with the camera's point eye (0, 0, 0, 1): what the rejection costs or saves
    plain_kept / cone_kept   the commands each writes; tested: clusters tested (the same for all three)
    host_us        the host alternative of the cone call (sizes up to --host-max-n): fetch the records, run the twin
                   (tests/cluster_cone_twin.h over the oracle's tests) on 16 threads over the draws, upload the commands; its bytes are
                   asserted equal to the device's

    python tools/cluster_cones_bench.py --n 1000000 10000000 --calls 100 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), then --trace on the kernel trace it wrote — the launches come
in a fixed order with a fixed number of calls, so the rows of each kernel are cut into the cells by position:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cluster_cones_bench.py --n 1000000 --calls 100 --no-host
    python tools/cluster_cones_bench.py --n 1000000 --calls 100 --trace DIR"""
import argparse
import csv
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
VARIANTS = ["plain", "zero", "cone"]  # the order of the timed loops of a cell
SHARED = ["cluster_count_kernel", "cluster_scan_kernel<0", "cluster_scan_kernel<1", "cluster_write_kernel"]  # launched by every variant
TESTS = {"plain": "cluster_test_kernel", "zero": "cluster_cone_test_kernel", "cone": "cluster_cone_test_kernel"}  # as the trace names them
THREADS = 16
CAMERA_EYE = (0.0, 0.0, 0.0, 1.0)
CUTOFF = 0.5


def grid_clusters(count):
    """(clusters, cones): the 2^3 / 4^3 cells of the box [-1, 1]^3 and their outward cones"""
    from garden_amd.lib import CLUSTER_CONE_DTYPE, CLUSTER_DTYPE
    cells = round(count ** (1.0 / 3.0))
    assert cells ** 3 == count
    out = np.zeros(count, CLUSTER_DTYPE)
    cones = np.zeros(count, CLUSTER_CONE_DTYPE)
    for j in range(count):
        at = np.array([j % cells, j // cells % cells, j // (cells * cells)], np.float32)
        out[j]["box_min"] = -1.0 + 2.0 * at / cells
        out[j]["box_max"] = -1.0 + 2.0 * (at + 1) / cells
        out[j]["first"], out[j]["count"] = 3 * 128 * j, 3 * 128
        centre = np.float32(0.5) * (out[j]["box_min"] + out[j]["box_max"])
        axis = centre / np.float32(np.linalg.norm(centre))  # (an even grid: no cell is centred on the origin)
        cones[j]["axis"] = axis
        cones[j]["apex"] = centre - axis * np.float32(0.5 * np.linalg.norm(out[j]["box_max"] - out[j]["box_min"]))
        cones[j]["cutoff"] = CUTOFF
    return out, cones


def host_alternative(nsup, fetched, tables, view_proj, eye, hiz, dtype):
    """records on the host -> the twin over THREADS slices of the draws -> the command structs"""
    n = int(fetched["draw_count"])
    models = np.ascontiguousarray(fetched["baked_model"], np.float32).reshape(-1, 12)[:n]
    g = np.zeros(n, np.uint32)
    first = np.arange(n + 1, dtype=np.uint32)
    edges = np.linspace(0, n, THREADS + 1).astype(np.int64)

    def part(k):
        lo, hi = int(edges[k]), int(edges[k + 1])
        return nsup.view_commands(models[lo:hi], g[lo:hi], first[lo:hi + 1], view_proj, eye, hiz, tables=tables)

    with ThreadPoolExecutor(THREADS) as pool:
        parts = list(pool.map(part, range(THREADS)))
    commands = np.concatenate([p[0] for p in parts])
    out = np.zeros(len(commands), dtype)
    for name in dtype.names:
        out[name] = commands[name]
    return out, sum(p[1] for p in parts), sum(p[2]["cone_rejected"] for p in parts), sum(p[2]["cone_only"] for p in parts)


def run(a):
    import torch

    import cluster_cones_support as nsup
    import commands_support as csup
    import instances_support as isup
    from garden_amd import scene
    from garden_amd.lib import CLUSTER_RANGE_DTYPE, GpuVisibility
    from oracle import oracle_py

    dtype = csup.INDEXED  # (no draw field: a slice of the host alternative numbers its draws from 0)
    depth = scene.synthetic_depth(1024, 1024)
    eyes = {"zero": np.zeros((1, 4), np.float32), "cone": np.array([CAMERA_EYE], np.float32)}
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
                for count in CLUSTERS:
                    clusters, cones = grid_clusters(count)
                    ranges = np.zeros(1, CLUSTER_RANGE_DTYPE)
                    ranges[0] = (0, count)
                    vis.bind_clusters(0, ranges, clusters)
                    vis.bind_cluster_cones(0, cones)
                    # the target is the caller's, sized from first calls that hold nothing (the counts are always the true ones)
                    probe = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    vis.cull_clusters(0, device=(probe.data_ptr(), 64))
                    _, counts, tested = vis.cluster_commands(0)
                    plain_kept = int(counts[0])
                    vis.cull_clusters(0, device=(probe.data_ptr(), 64), eyes=eyes["cone"])
                    _, counts, cone_tested = vis.cluster_commands(0)
                    cone_kept = int(counts[0])
                    assert int(cone_tested[0]) == int(tested[0])
                    dev = torch.zeros((plain_kept + 1, dtype.itemsize), dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    target = (dev.data_ptr(), dev.numel())
                    us = {}
                    for variant in VARIANTS:
                        samples = []
                        for k in range(a.warmup + a.calls):
                            s = time.perf_counter()
                            vis.cull_clusters(0, device=target, eyes=eyes.get(variant))
                            vis.wait()
                            if k >= a.warmup:
                                samples.append(time.perf_counter() - s)
                        us[variant] = np.array(samples) * 1e6
                        if variant == "plain":
                            plain_bytes = dev.cpu().numpy().tobytes()
                        elif variant == "zero":
                            assert dev.cpu().numpy().tobytes() == plain_bytes  # an all-zero eye: the plain form's bytes
                    host_us = rejected = cone_only = None
                    if not a.no_host and n <= a.host_max_n:
                        hiz = oracle_py.Hiz(depth) if mode == "hiz" else None
                        s = time.perf_counter()
                        fetched = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
                        exp, host_tested, rejected, cone_only = host_alternative(nsup, fetched, (table, ranges, clusters, cones), view["view_proj"],
                                                                                 eyes["cone"][0], hiz, dtype)
                        up = torch.from_numpy(exp.view(np.uint8).reshape(-1, dtype.itemsize)).to("cuda:0")
                        torch.cuda.synchronize()
                        host_us = float((time.perf_counter() - s) * 1e6)
                        got, _, _ = vis.cluster_commands(0, dtype=dtype)
                        assert host_tested == int(tested[0]) and len(exp) == cone_kept
                        assert got[:cone_kept].tobytes() == exp.tobytes()  # the two ways write the same bytes
                        del up
                    line = dict(n=n, clusters=count, mode=mode, stride=dtype.itemsize, draws=int(tested[0]) // count, tested=int(tested[0]),
                                plain_kept=plain_kept, cone_kept=cone_kept, calls=a.calls, host_us=host_us, cone_rejected=rejected, cone_only=cone_only)
                    for variant in VARIANTS:
                        line[variant + "_us"] = float(np.median(us[variant]))
                        line[variant + "_us_p10"] = float(np.percentile(us[variant], 10))
                        line[variant + "_us_p90"] = float(np.percentile(us[variant], 90))
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del dev
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def summarise(a):
    """the kernel rows of a rocprofv3 --kernel-trace csv of the same command line (with --no-host), cut into the cells by position:
    per cell two probing calls (plain, cone), then warmup + calls of every variant"""
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    names = SHARED + ["cluster_test_kernel", "cluster_cone_test_kernel"]
    rows = {k: [] for k in names}
    with open(files[0]) as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in trace:
        name = r["Kernel_Name"].replace(" ", "")
        for key in ("cluster_cone_test_kernel", "cluster_test_kernel") + tuple(SHARED):  # (the cone kernel's name holds neither other test's)
            if key in name:
                rows[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                break
    loop = a.warmup + a.calls
    cells = len(a.n) * len(MODES) * len(CLUSTERS)
    for k in SHARED:
        assert len(rows[k]) == cells * (2 + 3 * loop), (k, len(rows[k]))
    assert len(rows["cluster_test_kernel"]) == cells * (1 + loop) and len(rows["cluster_cone_test_kernel"]) == cells * (1 + 2 * loop)
    cell = 0
    for n in a.n:
        for mode in MODES:
            for count in CLUSTERS:
                line = dict(n=n, clusters=count, mode=mode, calls=a.calls)
                for v, variant in enumerate(VARIANTS):
                    total, per = 0.0, {}
                    for k in SHARED:
                        first = cell * (2 + 3 * loop) + 2 + v * loop + a.warmup
                        us = np.array(rows[k][first:first + a.calls])
                        per[k] = float(us.mean())
                        total += per[k]
                    if variant == "plain":
                        first = cell * (1 + loop) + 1 + a.warmup
                        us = np.array(rows["cluster_test_kernel"][first:first + a.calls])
                    else:
                        first = cell * (1 + 2 * loop) + 1 + (v - 1) * loop + a.warmup
                        us = np.array(rows["cluster_cone_test_kernel"][first:first + a.calls])
                    per[TESTS[variant]] = float(us.mean())
                    total += per[TESTS[variant]]
                    line[variant] = dict(kernels_us_avg=total, **{k + "_us": x for k, x in per.items()})
                print(json.dumps(line), flush=True)
                cell += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the host alternative (the run under rocprofv3)")
    ap.add_argument("--host-max-n", type=int, default=10_000_000, help="the host alternative runs for sizes up to this one")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace --output-format csv run of the same --n / --calls / --warmup")
    a = ap.parse_args()
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
