"""gv_pool_cull_cluster_lods timing beside gv_pool_cull_clusters in the same run, the method of tools/cluster_cones_bench.py: cfg2
scene (flat, the main camera), the 20-byte indexed command layout, behind ONE gv_pool_emit_instances of one cull of the main view.
Every slot draws one geometry: the binary cluster DAG over the 8 (2^3) or 64 (4^3) cells of the box [-1, 1]^3 — 15 or 127 clusters,
leaves first, self error 0 at the leaves and doubling per level from --error, nested spheres with a 3 % margin, the root's
parent_error +inf. The cull runs frustum only, and against a 1024^2 pyramid (synthetic depth) the view names. Per size, leaf count
and mode one JSON line:

    leaves_us      (a) gv_pool_cull_clusters over the LEAVES ALONE (a table of 8 / 64 clusters): what a user has today
    off_us         (b) gv_pool_cull_cluster_lods over the DAG with scale == 0: every cluster LOD-kept; its bytes are asserted equal to
                   gv_pool_cull_clusters' over the DAG
    lod_us         (c) ... with the camera's LOD view (point eye (0, 0, 0, 1), --scale, near_distance --near)
    runs_us        (d) (c) with GV_CLUSTERS_RUNS
    second_leaves_us / second_lod_us   (e) gv_pool_cull_clusters_second_phase behind (a) and behind (c) (mode hiz only), with the
                   pending clusters each tested
    tested / kept / commands of each; wall-clock microseconds per call (the call + the wait), the median of --calls after --warmup

    python tools/cluster_lods_bench.py --n 1000000 10000000 --calls 100 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), then --trace on the kernel trace it wrote — the launches come
in a fixed order with a fixed number of calls, so the rows of each test kernel are cut into the cells by position:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cluster_lods_bench.py --n 1000000 --calls 100
    python tools/cluster_lods_bench.py --n 1000000 --calls 100 --trace DIR"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEAVES = [8, 64]
MODES = ["frustum", "hiz"]
MARGIN = np.float32(1.03)


def dag(leaves, error):
    """(clusters, lods) of the binary DAG over `leaves` cells of [-1, 1]^3 in bit-interleaved order: 2 * leaves - 1 clusters, the
    levels one behind the other, every cluster's indices behind its predecessor's"""
    from garden_amd.lib import CLUSTER_DTYPE, CLUSTER_LOD_DTYPE
    levels = leaves.bit_length()
    bits = [sum(1 for b in range(levels - 1) if b % 3 == axis) for axis in range(3)]
    cell = (2.0 / np.array([1 << b for b in bits])).astype(np.float32)
    clusters = np.zeros(2 * leaves - 1, CLUSTER_DTYPE)
    lods = np.zeros(2 * leaves - 1, CLUSTER_LOD_DTYPE)
    boxes, spheres, index = {}, {}, {}
    j = at = 0
    for level in range(levels):
        for i in range(leaves >> level):
            if level == 0:
                ix = np.array([sum(((i >> b) & 1) << (b // 3) for b in range(levels - 1) if b % 3 == axis) for axis in range(3)], np.float32)
                lo, hi = (-1.0 + cell * ix).astype(np.float32), (-1.0 + cell * (ix + 1)).astype(np.float32)
                centre = np.float32(0.5) * (lo + hi)
                radius = np.float32(0.5) * np.float32(np.linalg.norm(hi - lo)) * MARGIN
            else:
                (lo0, hi0), (lo1, hi1) = boxes[level - 1, 2 * i], boxes[level - 1, 2 * i + 1]
                lo, hi = np.minimum(lo0, lo1), np.maximum(hi0, hi1)
                centre = np.float32(0.5) * (lo + hi)
                radius = max(np.float32(np.linalg.norm(centre - spheres[level - 1, 2 * i + s][0])) + spheres[level - 1, 2 * i + s][1]
                             for s in (0, 1)) * MARGIN
            boxes[level, i], spheres[level, i], index[level, i] = (lo, hi), (centre, np.float32(radius)), j
            clusters[j]["box_min"], clusters[j]["box_max"] = lo, hi
            clusters[j]["first"], clusters[j]["count"] = at, 3 * 128
            at += 3 * 128
            j += 1
    err = lambda level: np.float32(0.0 if level == 0 else error * 2.0 ** (level - 1))
    for (level, i), j in index.items():
        lods[j]["self_center"], lods[j]["self_radius"] = spheres[level, i]
        lods[j]["self_error"] = err(level)
        top = level == levels - 1
        lods[j]["parent_center"], lods[j]["parent_radius"] = spheres[level, i] if top else spheres[level + 1, i >> 1]
        lods[j]["parent_error"] = np.inf if top else err(level + 1)
    return clusters, lods


def timed(a, call, wait):
    samples = []
    for k in range(a.warmup + a.calls):
        s = time.perf_counter()
        call()
        wait()
        if k >= a.warmup:
            samples.append(time.perf_counter() - s)
    us = np.array(samples) * 1e6
    return float(np.median(us)), float(np.percentile(us, 10)), float(np.percentile(us, 90))


def run(a):
    import torch

    import commands_support as csup
    import instances_support as isup
    from garden_amd import scene
    from garden_amd.lib import CLUSTER_LOD_VIEW_DTYPE, CLUSTER_RANGE_DTYPE, GpuVisibility

    dtype = csup.INDEXED
    depth = scene.synthetic_depth(1024, 1024)
    off, camera = np.zeros(1, CLUSTER_LOD_VIEW_DTYPE), np.zeros(1, CLUSTER_LOD_VIEW_DTYPE)
    off[0]["eye"], off[0]["near_distance"] = (0, 0, 0, 1), 1.0
    camera[0]["eye"], camera[0]["scale"], camera[0]["near_distance"] = (0, 0, 0, 1), a.scale, a.near
    lines = []
    for n in a.n:
        sc = scene.flat_scene(n)
        table = csup.geometry_table([(3 * 128 * 127, 0, 0)])
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
                for leaves in LEAVES:
                    clusters, lods = dag(leaves, a.error)
                    ranges = np.zeros(1, CLUSTER_RANGE_DTYPE)
                    probe = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    small = (probe.data_ptr(), 64)
                    line = dict(n=n, leaves=leaves, dag=len(clusters), mode=mode, stride=dtype.itemsize, calls=a.calls, scale=a.scale, near=a.near,
                                error=a.error)

                    def counts_of():
                        _, counts, tested = vis.cluster_commands(0)
                        return int(counts[0]), int(tested[0])

                    # (a) the leaves alone
                    ranges[0] = (0, leaves)
                    vis.bind_clusters(0, ranges, clusters[:leaves])
                    vis.cull_clusters(0, device=small)
                    line["leaves_commands"], line["leaves_tested"] = counts_of()
                    dev = torch.zeros((line["leaves_commands"] + 1, dtype.itemsize), dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    target = (dev.data_ptr(), dev.numel())
                    dev2 = torch.zeros_like(dev)  # the second phase's commands: buffers of their own
                    torch.cuda.synchronize()
                    behind = (dev2.data_ptr(), dev2.numel())
                    line["leaves_us"], line["leaves_us_p10"], line["leaves_us_p90"] = timed(a, lambda: vis.cull_clusters(0, device=target), vis.wait)
                    if mode == "hiz":
                        vis.cull_clusters_second_phase(0, target=behind)
                        _, _, pending = vis.cluster_second_commands(0)
                        line["second_leaves_pending"] = int(pending[0])
                        line["second_leaves_us"], _, _ = timed(a, lambda: vis.cull_clusters_second_phase(0, target=behind), vis.wait)
                    del dev, dev2
                    # the DAG
                    ranges[0] = (0, len(clusters))
                    vis.bind_clusters(0, ranges, clusters)
                    vis.bind_cluster_lods(0, lods)
                    vis.cull_clusters(0, device=small)
                    line["dag_commands"], line["dag_tested"] = counts_of()
                    dev = torch.zeros((line["dag_commands"] + 1, dtype.itemsize), dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    target = (dev.data_ptr(), dev.numel())
                    dev2 = torch.zeros_like(dev)  # the second phase's commands: buffers of their own
                    torch.cuda.synchronize()
                    behind = (dev2.data_ptr(), dev2.numel())
                    vis.cull_clusters(0, device=target)
                    vis.wait()
                    plain_bytes = dev.cpu().numpy().tobytes()
                    dev.zero_()
                    torch.cuda.synchronize()
                    # (b) scale 0
                    line["off_us"], line["off_us_p10"], line["off_us_p90"] = timed(a, lambda: vis.cull_clusters(0, device=target, lods=off), vis.wait)
                    assert dev.cpu().numpy().tobytes() == plain_bytes  # scale 0: the plain form's bytes over the DAG
                    # (c) the camera's LOD view
                    vis.cull_clusters(0, device=small, lods=camera)
                    line["lod_commands"], line["lod_tested"] = counts_of()
                    line["lod_us"], line["lod_us_p10"], line["lod_us_p90"] = timed(a, lambda: vis.cull_clusters(0, device=target, lods=camera), vis.wait)
                    if mode == "hiz":
                        vis.cull_clusters_second_phase(0, target=behind)
                        _, _, pending = vis.cluster_second_commands(0)
                        line["second_lod_pending"] = int(pending[0])
                        line["second_lod_us"], _, _ = timed(a, lambda: vis.cull_clusters_second_phase(0, target=behind), vis.wait)
                    # (d) ... with runs
                    vis.cull_clusters(0, device=small, lods=camera, runs=True)
                    line["runs_commands"], _ = counts_of()
                    line["runs_us"], line["runs_us_p10"], line["runs_us_p90"] = timed(a, lambda: vis.cull_clusters(0, device=target, lods=camera, runs=True),
                                                                                      vis.wait)
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del dev, dev2
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


# per cell and test kernel: (untimed calls in front of each timed loop, timed loops) in launch order
TRACED = {
    "cluster_test_kernel": [1, "leaves", 2],                 # the probe, (a); then the probe and the reference over the DAG
    "cluster_lod_test_kernel": [0, "off", 1, "lod"],         # (b); the probe, (c)
    "cluster_lod_run_test_kernel": [1, "runs"],              # the probe, (d)
    "cluster_second_test_kernel": [1, "second_leaves"],      # mode hiz only
    "cluster_lod_second_test_kernel": [1, "second_lod"],     # mode hiz only
}


def summarise(a):
    """the test-kernel rows of a rocprofv3 --kernel-trace csv of the same command line, cut into the cells by position; every other
    cluster kernel as its mean over the whole run"""
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    with open(files[0]) as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    rows, others = {k: [] for k in TRACED}, {}
    for r in trace:
        name = r["Kernel_Name"].replace(" ", "")
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        for key in TRACED:
            if re.search(r"(^|::)" + key + r"(\(|$)", name):  # (the whole name: cluster_test_kernel is no part of another's)
                rows[key].append(us)
                break
        else:
            other = re.search(r"cluster_\w+(<\d+>)?", name)
            if other:
                others.setdefault(other.group(0), []).append(us)
    at = {k: 0 for k in TRACED}
    loop = a.warmup + a.calls
    for n in a.n:
        for mode in MODES:
            for leaves in LEAVES:
                line = dict(n=n, leaves=leaves, mode=mode, calls=a.calls)
                for key, plan in TRACED.items():
                    if "second" in key and mode != "hiz":
                        continue
                    for step in plan:
                        if isinstance(step, int):
                            at[key] += step
                        else:
                            us = np.array(rows[key][at[key] + a.warmup:at[key] + loop])
                            assert len(us) == a.calls, (key, step, len(us))
                            line[step + "_test_us"] = float(us.mean())
                            at[key] += loop
                print(json.dumps(line), flush=True)
    for key in TRACED:
        assert at[key] == len(rows[key]), (key, at[key], len(rows[key]))
    print(json.dumps({name: dict(launches=len(us), mean_us=float(np.mean(us))) for name, us in sorted(others.items())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scale", type=float, default=540.0, help="k of the camera's LOD view: (1080 / 2) / tan(45 deg) / 1 pixel")
    ap.add_argument("--near", type=float, default=0.1)
    ap.add_argument("--error", type=float, default=0.01, help="the self error of level 1, in model units; it doubles per level")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace --output-format csv run of the same --n / --calls / --warmup")
    a = ap.parse_args()
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
