"""gv_pick timing: wall-clock microseconds per call (after warm-up) at a given scene size and ray count, beside the editor's loop as
the reference runs it — single-threaded, per entity — through the C twin of the picking arithmetic (tests/pick_twin.h) compiled
-O2 -march=haswell. The CPU figure covers the inverse and the ray tests of the filter chain's candidates only (their models are
taken from the oracle beforehand): the reference also pays calcModel and a component lookup per entity, so it is a lower bound.

    python tools/pick_bench.py --n 10000000 --rays 1 8 --calls 300 [--hierarchy] [--no-cpu] [--out FILE]

Prints one JSON line per ray count. Kernel time: run under rocprofv3 --kernel-trace --stats (pick_kernel rows)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--hierarchy", action="store_true", help="4-deep hierarchy (cfg4 shape) instead of the flat cfg3 scene")
    ap.add_argument("--rays", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import pick_support as ps
    from garden_amd import scene
    from garden_amd.lib import GpuVisibility

    cam = (10.5, -3.25, 7.0)
    t0 = time.perf_counter()
    sc = scene.hierarchy_scene(a.n, depth=4, fanout=10) if a.hierarchy else scene.flat_scene(a.n)
    pool = ps.candidates(sc, cam, threads=16) if not a.no_cpu else None
    print(f"# scene {a.n} ({'hierarchy' if a.hierarchy else 'flat'}) in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    if pool is None:
        sub = ps.candidates(scene.flat_scene(100_000), cam)
        rays_all = ps.aimed_rays(sub, 8, 1, reach=(50.0, 2000.0))
    else:
        rays_all = ps.aimed_rays(pool, 8, 1, reach=(50.0, 2000.0))
    bytes_per_entity = 69 if a.hierarchy else 65
    twin = None if a.no_cpu else ps.build_twin(tempfile.mkdtemp(), march="haswell")
    lines = []
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        vis.bind_pool(0, sc.meshes)
        vis.hierarchy_rebuild()
        for r in a.rays:
            rays = rays_all[:r]
            for _ in range(a.warmup):
                got = vis.pick(rays, camera_position=cam)
            samples = []
            for _ in range(a.calls):
                s = time.perf_counter()
                vis.pick(rays, camera_position=cam)
                samples.append(time.perf_counter() - s)
            us = np.array(samples) * 1e6
            line = dict(n=a.n, hierarchy=bool(a.hierarchy), rays=r, calls=a.calls, us_median=float(np.median(us)),
                        us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)), bytes_per_entity=bytes_per_entity,
                        hits=sum(h is not None for h in got))
            line["tb_per_s_at_median"] = bytes_per_entity * a.n / (line["us_median"] * 1e-6) / 1e12
            if twin is not None:
                s = time.perf_counter()
                keys = ps.twin_keys(twin, [pool], rays)
                line["cpu_twin_ms"] = (time.perf_counter() - s) * 1e3
                line["twin_agrees"] = ps.as_bits(ps.decode(keys, [0])) == ps.as_bits(got)
            print(json.dumps(line))
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
