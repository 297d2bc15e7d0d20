"""gv_pool_cull_cluster_runs against gv_pool_cull_clusters, the method and the eight rows of tools/cluster_cull_bench.py: cfg2 scene
(flat, the main camera), the 20-byte indexed command layout, behind ONE gv_pool_emit_instances of one cull of the main view. Every
slot draws one geometry of 8 (2^3) or 64 (4^3) clusters, a regular sub-grid of the box [-1, 1]^3 whose index ranges lie back to back
(first[j + 1] == first[j] + count[j]); frustum only, and against a 1024^2 pyramid (synthetic depth) the view names. The two forms
ALTERNATE in the same process, call by call, each into a caller-owned target sized for what it writes. Per size, cluster count and
mode one JSON line:

    plain_us / runs_us     wall-clock microseconds per call (the call + the wait), median of --calls after --warmup
    plain_commands / runs_commands, tested, survivors per run
    bytes                  what each launch of the run form moves, computed from the shapes (D draws, T candidates, S survivors, H
                           heads, stride 20): see launch_bytes()

    python tools/cluster_runs_bench.py --n 1000000 10000000 --calls 100 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), then --trace on the kernel trace it wrote — the launches come
in a fixed order with a fixed number of calls, so the rows of each kernel are cut into the cells by position (a kernel both forms
launch alternates plain, runs):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cluster_runs_bench.py --n 1000000 --calls 100
    python tools/cluster_runs_bench.py --n 1000000 --calls 100 --trace DIR"""
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

from cluster_cull_bench import CLUSTERS, MODES, grid_clusters  # noqa: E402  (the same geometry: its index ranges are back to back)

SHARED = ["cluster_count_kernel", "cluster_scan_kernel<0", "cluster_scan_kernel<1"]  # launched by both forms, as the trace names them
PLAIN = ["cluster_test_kernel", "cluster_write_kernel"]
RUNS = ["cluster_run_test_kernel", "cluster_run_heads_kernel", "cluster_run_write_kernel"]


def launch_bytes(draws, tested, survivors, heads, stride):
    """bytes each of the run form's six launches moves, by count: a draw's record (idx 4, id 4, starts 8) and its two scratch words;
    a candidate's cluster (32) and its share of the draw's model (48 per draw) and a survive and a link bit; per tile of 256 the head
    count and prefix words; a head's two clusters, model, search words and command"""
    tiles = (tested + 255) // 256
    return dict(count=draws * (16 + 8), scan_candidates=(draws // 256 + 1) * 16 + tiles * 4,
                test=tested * 32 + draws * 48 + tested // 4, heads=tested // 4 + tested // 8 + tiles * 4, scan_heads=tiles * 8,
                write=tested // 8 + heads * (64 + 48 + 24 + stride),
                plain_write=tested // 8 + survivors * (32 + 48 + 24 + stride))


def run(a):
    import torch

    import commands_support as csup
    import instances_support as isup
    from garden_amd import scene
    from garden_amd.lib import CLUSTER_RANGE_DTYPE, GpuVisibility

    dtype = csup.INDEXED
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
                for count in CLUSTERS:
                    clusters = grid_clusters(count)
                    assert all(int(clusters[j]["first"]) + int(clusters[j]["count"]) == int(clusters[j + 1]["first"]) for j in range(count - 1))
                    ranges = np.zeros(1, CLUSTER_RANGE_DTYPE)
                    ranges[0] = (0, count)
                    vis.bind_clusters(0, ranges, clusters)
                    # the targets are the caller's, sized from a first call that holds nothing (the counts are always the true ones)
                    probe = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    vis.cull_clusters(0, device=(probe.data_ptr(), 64))
                    _, counts, tested = vis.cluster_commands(0)
                    kept = int(counts[0])
                    vis.cull_clusters(0, device=(probe.data_ptr(), 64), runs=True)
                    _, counts, run_tested = vis.cluster_commands(0)
                    heads = int(counts[0])
                    assert int(run_tested[0]) == int(tested[0])
                    plain_dev = torch.zeros((kept + 1, dtype.itemsize), dtype=torch.uint8, device="cuda:0")
                    runs_dev = torch.zeros((heads + 1, dtype.itemsize), dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    samples = {False: [], True: []}
                    for k in range(a.warmup + a.calls):
                        for runs, dev in ((False, plain_dev), (True, runs_dev)):
                            s = time.perf_counter()
                            vis.cull_clusters(0, device=(dev.data_ptr(), dev.numel()), runs=runs)
                            vis.wait()
                            if k >= a.warmup:
                                samples[runs].append(time.perf_counter() - s)
                    plain_us, runs_us = np.array(samples[False]) * 1e6, np.array(samples[True]) * 1e6
                    # the run commands draw exactly the indices the plain commands draw
                    got_plain = plain_dev.cpu().numpy()[:kept].reshape(-1).view(dtype)
                    got_runs = runs_dev.cpu().numpy()[:heads].reshape(-1).view(dtype)
                    assert int(got_plain["count"].sum(dtype=np.uint64)) == int(got_runs["count"].sum(dtype=np.uint64))
                    draws = int(tested[0]) // count
                    line = dict(n=n, clusters=count, mode=mode, stride=dtype.itemsize, draws=draws, tested=int(tested[0]), calls=a.calls,
                                plain_commands=kept, runs_commands=heads, survivors_per_run=kept / max(heads, 1),
                                plain_us=float(np.median(plain_us)), plain_p10=float(np.percentile(plain_us, 10)),
                                plain_p90=float(np.percentile(plain_us, 90)), runs_us=float(np.median(runs_us)),
                                runs_p10=float(np.percentile(runs_us, 10)), runs_p90=float(np.percentile(runs_us, 90)),
                                bytes=launch_bytes(draws, int(tested[0]), kept, heads, dtype.itemsize))
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del plain_dev, runs_dev
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def summarise(a):
    """the kernel rows of a rocprofv3 --kernel-trace csv of the same command line, cut into the cells by position: per cell one
    probing call of each form, then warmup + calls of each, alternating"""
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = {k: [] for k in SHARED + PLAIN + RUNS}
    with open(files[0]) as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in trace:
        for key in rows:
            if key in r["Kernel_Name"].replace(" ", ""):
                rows[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                break
    per = 1 + a.warmup + a.calls
    cells = len(a.n) * len(MODES) * len(CLUSTERS)
    cell = 0
    for n in a.n:
        for mode in MODES:
            for count in CLUSTERS:
                line = dict(n=n, clusters=count, mode=mode, calls=a.calls)
                totals = {"plain": 0.0, "runs": 0.0}
                for k in SHARED:  # plain, runs, plain, runs, ...
                    assert len(rows[k]) == 2 * per * cells, (k, len(rows[k]))
                    mine = np.array(rows[k][2 * cell * per:2 * (cell + 1) * per]).reshape(per, 2)[1 + a.warmup:]
                    for form, column in (("plain", 0), ("runs", 1)):
                        line[f"{form}:{k}_us"] = float(mine[:, column].mean())
                        totals[form] += float(mine[:, column].mean())
                for form, names in (("plain", PLAIN), ("runs", RUNS)):
                    for k in names:
                        assert len(rows[k]) == per * cells, (k, len(rows[k]))
                        us = np.array(rows[k][cell * per + 1 + a.warmup:(cell + 1) * per])
                        line[f"{form}:{k}_us"] = float(us.mean())
                        totals[form] += float(us.mean())
                line["plain_kernels_us"], line["runs_kernels_us"] = totals["plain"], totals["runs"]
                print(json.dumps(line), flush=True)
                cell += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace --output-format csv run of the same --n / --calls / --warmup")
    a = ap.parse_args()
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
