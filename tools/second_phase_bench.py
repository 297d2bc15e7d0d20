"""gv_pool_cull_second_phase timing, the method of tools/group_draws_bench.py: cfg3's world (flat, main camera with Hi-Z, a 4096^2
depth image), wall-clock microseconds per call (call + wait, after warm-up). Phase 1 is culled once against the walls image A; the
pyramid is then rebuilt from B and stays, so every timed call does the same work. B is tried three ways: "same" (B = A: nothing is
new), "shifted" (the walls image rolled by --shift texels) and "noise" (scene.noise_depth). Per size and B:

    full         gv_cull of the same view against B into a context of its own (cull + emit kernels): the parent's code, the
                 yardstick — the first half of what an engine must do today.

    second       gv_pool_cull_second_phase(0 -> 1) against B.

    host         the whole host alternative (not with --no-host): the second cull, two fetches, np.setdiff1d, gather — equality with
                 the second view's fetch asserted.

    python tools/second_phase_bench.py --n 1000000 --calls 100 [--out FILE]

Kernel time: a run of its own under rocprofv3 (the program after `--`), ONE size per run, then --trace on the kernel trace it wrote —
the phases launch in a fixed order with a fixed number of calls, so the rows of each kernel are cut into phases by position:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/second_phase_bench.py --n 1000000 --calls 100 --no-host
    python tools/second_phase_bench.py --n 1000000 --calls 100 --trace DIR

Prints one JSON line per size, B and phase."""
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

IMAGES = ["same", "shifted", "noise"]


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


def image_b(which, a_image, shift):
    from garden_amd import scene
    if which == "same":
        return a_image
    if which == "shifted":
        return np.ascontiguousarray(np.roll(a_image, shift, axis=1))
    return scene.noise_depth(a_image.shape[1], a_image.shape[0])


def run(a):
    import second_phase_support as sp
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    view = scene.main_camera_view(use_hiz=1)
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for n in a.n:
        sc = scene.flat_scene(n)
        a_image = scene.synthetic_depth(a.size, a.size)
        for which in IMAGES:
            b_image = image_b(which, a_image, a.shift)
            with GpuVisibility(device=0) as vis, GpuVisibility(device=0) as other:
                for ctx, image in ((vis, a_image), (other, b_image)):
                    ctx.bind_transforms(sc.transforms, sc.entity_to_transform)
                    ctx.bind_pool(0, sc.meshes)
                    ctx.hiz_build(image)
                vis.cull(0, [view])
                vis.wait()
                vis.hiz_build(b_image)
                full = lambda: other.cull(0, [view])
                second = lambda: vis.cull_second_phase(0, 1, view, pool_id=0)
                line = dict(n=n, b=which, phase="full", calls=a.calls)
                line.update(timed(a.calls, a.warmup, full, other.wait))
                report(line)
                line = dict(n=n, b=which, phase="second", calls=a.calls)
                line.update(timed(a.calls, a.warmup, second, vis.wait))
                first = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
                got = vis.fetch(1, write_back=False, occupancy=n, order="raw", pool_id=0)
                line.update(first_draws=int(first["draw_count"]), new_draws=int(got["draw_count"]))
                report(line)
                if a.no_host:
                    continue
                samples = []
                for _ in range(3):
                    s = time.perf_counter()
                    other.cull(0, [view])
                    r = other.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
                    f = vis.fetch(0, write_back=False, occupancy=n, order="raw", pool_id=0)
                    fetched = time.perf_counter()
                    fresh = np.setdiff1d(r["visible_idx"], f["visible_idx"], assume_unique=True)
                    keep = np.isin(r["visible_idx"], fresh)
                    host = dict(visible_idx=r["visible_idx"][keep], baked_model=r["baked_model"][keep], distance_sq=r["distance_sq"][keep],
                                draw_count=int(keep.sum()))
                    samples.append((fetched - s, time.perf_counter() - fetched))
                sp.same_records(got, host)  # the two ways agree, order included
                fetch_s, diff_s = np.median(np.array(samples), axis=0)
                report(dict(n=n, b=which, phase="host", cull_and_fetches_us=float(fetch_s * 1e6), difference_us=float(diff_s * 1e6),
                            host_us=float((fetch_s + diff_s) * 1e6)))
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def summarise(a):
    """the kernel rows of a rocprofv3 --kernel-trace csv of the same command line (one size, --no-host), cut into phases by position:
    per image the yardstick's cull and emit kernels come first, then the call's"""
    assert len(a.n) == 1
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    with open(files[0]) as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    per = a.warmup + a.calls
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    mine = [r for r in trace if "second_" in r["Kernel_Name"]]
    assert len([r for r in mine if "second_cull_kernel" in r["Kernel_Name"]]) == len(IMAGES) * per
    at = 0
    for which in IMAGES:
        # the image's section: from its first kernel behind the previous section to its last second_union_kernel
        unions = [i for i, r in enumerate(trace) if "second_union_kernel" in r["Kernel_Name"]]
        end = unions[(IMAGES.index(which) + 1) * per - 1] + 1
        section = trace[at:end]
        at = end
        first_second = next(i for i, r in enumerate(section) if "second_seen_kernel" in r["Kernel_Name"])
        # the yardstick: every kernel (the pyramid's aside) that ran at least once per timed gv_cull in front of the first call; of
        # each, the last `calls` x (launches per call) rows are the timed culls' (set-up and warm-up come before them)
        yard = {}
        for r in section[:first_second]:
            if "hiz" not in r["Kernel_Name"]:
                yard.setdefault(r["Kernel_Name"].split("(")[0], []).append(us(r))
        full = {name: float(np.sum(rows[-a.calls * (len(rows) // per):]) / a.calls) for name, rows in yard.items() if len(rows) >= per}
        call = section[first_second:]
        names = ["second_seen_kernel", "second_cull_kernel", "emit_kernel", "second_union_kernel"]
        parts = {}
        for name in names:
            rows = [us(r) for r in call if name in r["Kernel_Name"]]
            assert len(rows) == per, (name, len(rows))
            parts[name + "_us"] = float(np.mean(rows[a.warmup:]))
        line = dict(n=a.n[0], b=which, phase="second", calls=a.calls, kernels_us_avg=float(sum(parts.values())), **parts)
        print(json.dumps(line), flush=True)
        print(json.dumps(dict(n=a.n[0], b=which, phase="full", calls=a.calls, kernels_us_avg=float(sum(full.values())),
                              per_kernel_us={name[-48:]: v for name, v in full.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=4096, help="side of the square depth images")
    ap.add_argument("--shift", type=int, default=97, help="texels the walls image is rolled by for the shifted B")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the host alternative (the run under rocprofv3)")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace --output-format csv run of the same --n (one size) / --calls / --warmup")
    a = ap.parse_args()
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
