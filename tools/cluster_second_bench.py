"""gv_pool_cull_clusters_second_phase timing, the method of tools/cluster_cull_bench.py: cfg2 scene (flat, the main camera), the
20-byte indexed command layout, behind ONE gv_pool_emit_instances of one cull of the main view against a 1024^2 pyramid (synthetic
depth). Every slot draws one geometry of 8 (2^3) or 64 (4^3) clusters. The cluster cull K1 runs against that pyramid; the pyramid is
rebuilt from a SECOND synthetic depth image (another seed) and the second phase is timed against it. Per size and cluster count one
JSON line:

    us_median      wall-clock microseconds per second-phase call (the call + the wait, after warm-up)
    first_us       a full gv_pool_cull_clusters against the new pyramid in the same run (what the second phase avoids re-testing)
    parent_us      the only way to the same commands without the second phase: a full gv_pool_cull_clusters against the new
                   pyramid, both fetches (its commands and K1's) and a set difference on the host; its bytes are asserted equal to
                   the device's
    tested / first_kept / pending / kept   clusters K1 tested and kept, pending clusters re-tested, second-phase commands

    python tools/cluster_second_bench.py --n 1000000 10000000 --calls 100 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), then --trace on the kernel trace it wrote — the launches come
in a fixed order with a fixed number of calls, so the rows of each kernel are cut into the cells by position:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cluster_second_bench.py --n 1000000 --calls 100 --no-host
    python tools/cluster_second_bench.py --n 1000000 --calls 100 --trace DIR"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLUSTERS = [8, 64]
KERNELS = ["cluster_second_count_kernel", "cluster_second_scan_kernel<0", "cluster_second_test_kernel", "cluster_second_scan_kernel<1",
           "cluster_second_write_kernel"]  # as the trace names them


def timed(vis, call, warmup, calls):
    samples = []
    for k in range(warmup + calls):
        s = time.perf_counter()
        call()
        vis.wait()
        if k >= warmup:
            samples.append(time.perf_counter() - s)
    return np.array(samples) * 1e6


def run(a):
    import torch

    import commands_support as csup
    import instances_support as isup
    from cluster_cull_bench import grid_clusters
    from garden_amd import scene
    from garden_amd.lib import CLUSTER_RANGE_DTYPE, GpuVisibility

    dtype = csup.INDEXED
    old, new = scene.synthetic_depth(1024, 1024), scene.synthetic_depth(1024, 1024, seed=scene.SEED + 1)
    lines = []
    for n in a.n:
        sc = scene.flat_scene(n)
        table = csup.geometry_table([(3 * 128 * 64, 0, 0)])
        view = scene.main_camera_view(use_hiz=1)
        with GpuVisibility(device=0) as vis:
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            vis.hierarchy_rebuild()
            vis.hiz_build(old)
            vis.cull(0, [view])
            vis.wait()
            vis.set_instance_layout(0, dtype=isup.BARE)
            vis.emit_instances(0, [0])
            vis.set_command_layout(0, dtype=dtype)
            vis.bind_geometry(0, None, table)
            for count in CLUSTERS:
                ranges = np.zeros(1, CLUSTER_RANGE_DTYPE)
                ranges[0] = (0, count)
                vis.bind_clusters(0, ranges, grid_clusters(count))
                # the targets are the caller's, sized from a first call that holds nothing (the counts are always the true ones)
                def own_target(cull, counts_of):
                    probe = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    cull((probe.data_ptr(), 64))
                    dev = torch.zeros((int(counts_of()[0]) + 1, dtype.itemsize), dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    return dev, (dev.data_ptr(), dev.numel())

                first_counts = lambda: vis.cluster_commands(0)[1]
                vis.hiz_build(new)
                full_dev, full_target = own_target(lambda t: vis.cull_clusters(0, device=t), first_counts)
                first_us = timed(vis, lambda: vis.cull_clusters(0, device=full_target), a.warmup, a.calls)  # a full cluster cull against the new pyramid
                parent_us = None
                if not a.no_host:
                    s = time.perf_counter()
                    vis.cull_clusters(0, device=full_target)
                    full, _, _ = vis.cluster_commands(0, dtype=dtype)
                    full = full.copy()
                    parent_us = (time.perf_counter() - s) * 1e6  # (the fetch of K1 and the difference are added below)
                vis.hiz_build(old)
                k1_dev, k1_target = own_target(lambda t: vis.cull_clusters(0, device=t), first_counts)
                vis.cull_clusters(0, device=k1_target)  # K1, against the old pyramid
                s = time.perf_counter()
                k1, k1_counts, tested = vis.cluster_commands(0, dtype=dtype)
                fetch_us = (time.perf_counter() - s) * 1e6
                vis.hiz_build(new)
                dev, target = own_target(lambda t: vis.cull_clusters_second_phase(0, target=t), lambda: vis.cluster_second_commands(0)[1])
                us = timed(vis, lambda: vis.cull_clusters_second_phase(0, target=target), a.warmup, a.calls)
                got, counts, pending = vis.cluster_second_commands(0, dtype=dtype)
                if not a.no_host:
                    s = time.perf_counter()
                    key = lambda c: (c["first_instance"].astype(np.uint64) << np.uint64(32)) | c["first"].astype(np.uint64)  # (draw, cluster)
                    late = full[~np.isin(key(full), key(k1))]  # what the new pyramid keeps and K1 did not, in the order of the commands
                    parent_us += fetch_us + (time.perf_counter() - s) * 1e6
                    assert late.tobytes() == got.tobytes()  # the two ways write the same bytes
                line = dict(n=n, clusters=count, stride=dtype.itemsize, tested=int(tested[0]), first_kept=int(k1_counts[0]), pending=int(pending[0]),
                            kept=int(counts[0]), calls=a.calls, us_median=float(np.median(us)), us_p10=float(np.percentile(us, 10)),
                            us_p90=float(np.percentile(us, 90)), first_us=float(np.median(first_us)), parent_us=parent_us)
                print(json.dumps(line), flush=True)
                lines.append(line)
                del full_dev, k1_dev, dev
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
        for count in CLUSTERS:
            line = dict(n=n, clusters=count, calls=a.calls)
            total = 0.0
            for k in KERNELS:
                assert len(rows[k]) == per * len(a.n) * len(CLUSTERS), (k, len(rows[k]))
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
    ap.add_argument("--no-host", action="store_true", help="skip the parent's path (the run under rocprofv3)")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace --output-format csv run of the same --n / --calls / --warmup")
    a = ap.parse_args()
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
