#!/usr/bin/env python3
"""Times gv_merge_sorted: `lists` pools of `size` entities each, culled by an enclosing orthographic view and sorted back to front,
merged `reps` times into one 64-byte SortedMesh array. Prints one JSON line with the wall time per merge (launch to stream drained)
and the bytes a merge must move: records x (4 + 48 + 4 read + stride written). For the kernel's own time run it under the
profiler, the program after `--`:

    rocprofv3 --kernel-trace --stats -d out -- python tools/merge_bench.py --lists 4 --size 30000
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from garden_amd import scene  # noqa: E402
from garden_amd.lib import GpuVisibility  # noqa: E402

SORTED_MESH = np.dtype(dict(names=["componentOffset", "bakedModel", "distanceSq", "bufferIndex"],
                            formats=[np.uint64, (np.float32, 12), np.float32, np.uint32], offsets=[0, 8, 56, 60], itemsize=64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=4)
    ap.add_argument("--size", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    sc = scene.flat_scene(a.lists * a.size, defects=False)
    half = 1.0e7
    view = scene.make_view(scene.ortho_rev_z(2 * half, 2 * half, -half, half))
    group = dict(group_id=0, items=[(k, 0, k, 64) for k in range(a.lists)], descending=True, dtype=SORTED_MESH)
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        for k in range(a.lists):
            vis.bind_pool(k, sc.meshes[k * a.size:(k + 1) * a.size].copy())
        vis.hierarchy_rebuild()
        for k in range(a.lists):
            vis.cull(k, [view])
            vis.sort(0, descending=True, pool_id=k)
        vis.wait()
        times = []
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            vis.merge_sorted([group])
            vis.wait()
            if r >= a.warmup:
                times.append(time.perf_counter() - t0)
        _, counts = vis.merged(0, SORTED_MESH)
    total = int(counts[-1])
    times = np.array(times) * 1e6
    print(json.dumps(dict(lists=a.lists, size=a.size, records=total, bytes_moved=total * (4 + 48 + 4 + SORTED_MESH.itemsize),
                          wall_us_median=float(np.median(times)), wall_us_p10=float(np.percentile(times, 10)),
                          wall_us_p90=float(np.percentile(times, 90)), reps=a.reps)))


if __name__ == "__main__":
    main()
