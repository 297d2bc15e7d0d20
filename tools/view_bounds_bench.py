"""gv_pool_view_bounds timing, the method of tools/lod_select_bench.py: cfg3's world (flat, main camera with Hi-Z against a 4096 x 4096
walls image) plus three shadow cascades, wall-clock microseconds per call (call + wait, after warm-up) behind ONE gv_cull. Per size
and per item count (1: the main view; 4: the main view and the three cascades, each in its own rotation basis):

    bounds       gv_pool_view_bounds — and beside it the host alternative an engine has today, timed in the same run: fetch the
                 records, then one vectorised numpy pass over eight corners per record (the fused multiply-adds restated through
                 float64) and a min / max, equality of every word asserted (`host_us`).
    instances    the yardstick: the parent's gv_pool_emit_instances over the same views (the bare 64-byte layout), which reads the
                 same 52 bytes per record and writes 64 more.

    python tools/view_bounds_bench.py --n 1000000 10000000 --calls 100 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), then --trace on the kernel trace it wrote — the phases
launch in a fixed order with a fixed number of calls, so the rows of each kernel are cut into phases by position:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/view_bounds_bench.py --n 1000000 10000000 --calls 100 --no-host
    python tools/view_bounds_bench.py --n 1000000 10000000 --calls 100 --trace DIR

Prints one JSON line per size, item count and phase."""
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

ITEMS = [1, 4]
KERNELS = ["bounds_fold_kernel", "bounds_finish_kernel", "instance_kernel"]
RECORD_READ_BYTES = 4 + 48 + 4 + 16 + 8  # idx, bakedModel, inv, box a, box b


def f32(x):
    return x.astype(np.float32).astype(np.float64)


def affine(m, x, y, z):
    """rows 0..2 of an affine 3x4 (12 values per row of m, float4x3 order) applied to points: fma(c0, x, fma(c1, y, fma(c2, z, c3)))
    per row, every fma rounded to fp32 once (the products are exact in float64)"""
    return [f32(m[..., r] * x + f32(m[..., 3 + r] * y + f32(m[..., 6 + r] * z + m[..., 9 + r]))) for r in range(3)]


def host_bounds(slots, models, boxes, basis):
    """the rule of DESIGN.md §4 item 14 over fetched records, vectorised; returns (lo[3], hi[3], nan_records) as float32 / int"""
    m = models.reshape(-1, 12).astype(np.float64)
    box = boxes[slots].astype(np.float64)
    b = np.asarray(basis, np.float64).reshape(12)
    lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    nan = np.zeros(len(m), bool)
    for c in range(8):
        x, y, z = box[:, 3 if c & 1 else 0], box[:, 4 if c & 2 else 1], box[:, 5 if c & 4 else 2]
        q = affine(b, *affine(m, x, y, z))
        for r in range(3):
            v = q[r].astype(np.float32)
            nan |= np.isnan(v)
            if len(v):
                lo[r], hi[r] = min(lo[r], np.nanmin(v)), max(hi[r], np.nanmax(v))
    return lo, hi, int(nan.sum())


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
    import bounds_support as bs
    import instances_support as isup
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    views = [scene.main_camera_view(use_hiz=1)] + [scene.cascade_view(index=k) for k in range(3)]
    bases = [bs.rotation_basis(k, (10.0 * k, -5.0, 2.5)) for k in range(4)]
    depth = scene.synthetic_depth(4096, 4096)
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for n in a.n:
        sc = scene.flat_scene(n)
        boxes = bs.aabbs_by_slot(sc.meshes)
        with GpuVisibility(device=0) as vis:
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            vis.hierarchy_rebuild()
            vis.hiz_build(depth)
            vis.cull(0, views)
            vis.wait()
            vis.set_instance_layout(0, dtype=isup.BARE)
            for items in ITEMS:
                listed = list(range(items))
                draws = [int(vis.fetch(v, write_back=False, occupancy=n, order="raw", pool_id=0)["draw_count"]) for v in listed]
                line = dict(n=n, phase="bounds", items=items, draws=draws, calls=a.calls)
                line.update(timed(a.calls, a.warmup, lambda: vis.view_bounds_issue(0, listed, bases[:items]), vis.wait))
                got = vis.view_bounds_fetch(0)
                line["lo"], line["hi"] = got["lo"].tolist(), got["hi"].tolist()
                if not a.no_host:  # what an engine does today: records to the host, eight corners each, min / max
                    samples, split = [], []
                    for _ in range(3):
                        s = time.perf_counter()
                        fetched = [vis.fetch(v, write_back=False, occupancy=n, order="raw", pool_id=0) for v in listed]
                        mid = time.perf_counter()
                        host = [host_bounds(f["visible_idx"], f["baked_model"], boxes, bases[i]) for i, f in enumerate(fetched)]
                        samples.append(time.perf_counter() - s)
                        split.append(mid - s)
                    for i, (lo, hi, nan) in enumerate(host):  # the two ways give the same words
                        assert lo.view(np.uint32).tolist() == got[i]["lo"].view(np.uint32).tolist(), (i, lo, got[i]["lo"])
                        assert hi.view(np.uint32).tolist() == got[i]["hi"].view(np.uint32).tolist(), (i, hi, got[i]["hi"])
                        assert nan == int(got[i]["nan_records"]) and draws[i] == int(got[i]["draw_count"])
                    line["host_us"], line["host_fetch_us"] = float(np.median(samples) * 1e6), float(np.median(split) * 1e6)
                report(line)
                if not a.no_yardstick:
                    line = dict(n=n, phase="instances", items=items, draws=draws, calls=a.calls)
                    line.update(timed(a.calls, a.warmup, lambda: vis.emit_instances(0, listed), vis.wait))
                    report(line)
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
        for key in KERNELS:
            if key in r["Kernel_Name"] and "draw_instances" not in r["Kernel_Name"]:
                rows[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                break
    per = a.warmup + a.calls
    cells = len(a.n) * len(ITEMS)
    assert len(rows["bounds_fold_kernel"]) == len(rows["bounds_finish_kernel"]) == cells * per, len(rows["bounds_fold_kernel"])
    assert a.no_yardstick or len(rows["instance_kernel"]) == cells * per, len(rows["instance_kernel"])

    def stats(us):
        us = np.array(us[a.warmup:])
        return dict(avg=float(us.mean()), min=float(us.min()), max=float(us.max()))

    for i, n in enumerate(a.n):
        for j, items in enumerate(ITEMS):
            at = (i * len(ITEMS) + j) * per
            line = dict(n=n, items=items, calls=a.calls)
            for k in KERNELS[:2] if a.no_yardstick else KERNELS:
                line[k + "_us"] = stats(rows[k][at:at + per])
            line["bounds_us_avg"] = line["bounds_fold_kernel_us"]["avg"] + line["bounds_finish_kernel_us"]["avg"]
            if a.draws:  # achieved bytes per second of the fold: what the rule needs per record over the kernel's time
                draws = a.draws[i * len(ITEMS) + j]
                line["fold_read_bytes"] = draws * RECORD_READ_BYTES
                line["fold_gb_per_s"] = draws * RECORD_READ_BYTES / line["bounds_fold_kernel_us"]["avg"] / 1e3
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the host alternative (the run under rocprofv3)")
    ap.add_argument("--no-yardstick", action="store_true", help="skip the instance emission (runs that compare builds of the bounds kernels)")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace --output-format csv run of the same --n / --calls / --warmup")
    ap.add_argument("--draws", type=int, nargs="*", default=None, help="with --trace: the summed draws per (size, item count) cell, for bytes per second")
    a = ap.parse_args()
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
