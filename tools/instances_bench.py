"""gv_pool_emit_instances timing on the cfg2 scene (flat, frustum-only main camera): wall-clock microseconds per call (emission +
wait, after warm-up) for the bare 64-byte layout, for one with all four fields and for the sprite struct (stride 96: mvp, colour, uvSize,
uvOffset) with the 32 bytes behind mvp bound as the pool's payload (gv_pool_bind_payload), achieved bytes/s from the byte model of
DESIGN.md §5.12, and beside it the same instances built by the host in the same run — the draw loop restated through the C twin
(tests/instance_twin.h, -O2 -march=haswell) on 1 thread and on the worker threads of gv_host_parallel_ranges, including the fetch
of the records it needs.

    python tools/instances_bench.py --n 1000000 10000000 --calls 200 [--layouts bare64 full128 sprite96] [--no-cpu] [--out FILE]

Prints one JSON line per size and layout. Kernel time: run under rocprofv3 --kernel-trace --stats (the program after `--`): the
instance_kernel rows, and the emit kernel's rows of the same run as the nearest existing stream of the same shape."""
import argparse
import ctypes as C
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
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--layouts", nargs="+", default=["bare64", "full128", "sprite96"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import instances_support as isup
    from garden_amd import lib, scene
    from garden_amd.lib import GpuVisibility

    twin = None if a.no_cpu else isup.build_twin(tempfile.mkdtemp(), march="haswell")
    view = scene.main_camera_view()
    # bytes per record: the model (48) and the fields read, the instance written; sprite96 reads idx (4), the model and one payload
    # row (pitch 32) and writes the whole 96-byte instance
    sprite = isup.layout_dtype(96, mvp=0)
    layouts = {"bare64": (isup.BARE, 48 + 64), "full128": (isup.FULL, 48 + 4 + 4 + 64 + 48 + 4 + 4), "sprite96": (sprite, 4 + 48 + 32 + 96)}
    layouts = {k: layouts[k] for k in a.layouts}
    lines = []
    for n in a.n:
        sc = scene.flat_scene(n)
        with GpuVisibility(device=0) as vis:
            vis.bind_transforms(sc.transforms, sc.entity_to_transform)
            vis.bind_pool(0, sc.meshes)
            vis.hierarchy_rebuild()
            for _ in range(3):  # (the emit kernel's rows of the trace: the stream the instance kernel is set against)
                vis.cull(0, [view])
                vis.wait()
            records = vis.result_count(0)
            payload = None
            for name, (dtype, bytes_per_record) in layouts.items():
                if name == "sprite96":  # colour (16 bytes) and uvSize | uvOffset (16 bytes) of every slot, any bits
                    rng = np.random.Generator(np.random.PCG64(n))
                    payload = [rng.integers(0, 1 << 32, (n, 4), dtype=np.uint32) for _ in range(2)]
                    vis.bind_payload(0, payload)
                    s = time.perf_counter()
                    vis.sync()
                    vis.wait()
                    first_upload_ms = (time.perf_counter() - s) * 1e3
                vis.set_instance_layout(0, dtype=dtype)
                if name == "sprite96":
                    vis.set_payload_layout(0, [64, 80])
                samples = []
                for k in range(a.warmup + a.calls):
                    s = time.perf_counter()
                    vis.emit_instances(0, [0])
                    vis.wait()
                    if k >= a.warmup:
                        samples.append(time.perf_counter() - s)
                us = np.array(samples) * 1e6
                line = dict(n=n, layout=name, stride=dtype.itemsize, records=records, calls=a.calls, us_median=float(np.median(us)),
                            us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)), bytes_per_record=bytes_per_record,
                            algorithmic_mb=records * bytes_per_record / 1e6)
                line["wall_gb_per_s_at_median"] = records * bytes_per_record / (line["us_median"] * 1e-6) / 1e9
                if name == "sprite96":
                    line["payload_first_upload_ms"] = first_upload_ms
                if twin is not None:
                    got, starts = vis.instances(0)
                    # the host builds the same array: fetch of the records + the restated draw loop
                    s = time.perf_counter()
                    f = vis.fetch(0, write_back=False, order="raw", pool_id=0)
                    line["host_fetch_ms"] = (time.perf_counter() - s) * 1e3
                    models = np.ascontiguousarray(f["baked_model"])
                    vp = np.ascontiguousarray(view["view_proj"], dtype=np.float32)
                    out = np.zeros(records, dtype)
                    mvps = np.empty((records, 16), np.float32)

                    def fill(lo, hi):
                        twin.twin_many(vp.ctypes.data, models[lo:hi].ctypes.data, hi - lo, mvps[lo:hi].ctypes.data)
                        out["mvp"][lo:hi] = mvps[lo:hi]
                        if "model" in dtype.names:
                            out["model"][lo:hi] = models[lo:hi]
                            out["slot"][lo:hi] = f["visible_idx"][lo:hi]
                            out["distanceSq"][lo:hi] = f["distance_sq"][lo:hi]
                        if name == "sprite96":  # sprite.cpp:127-129: the draw's own component, found through the record's slot
                            raw = out.view(np.uint8).reshape(records, -1)
                            raw[lo:hi, 64:80] = payload[0][f["visible_idx"][lo:hi]].view(np.uint8)
                            raw[lo:hi, 80:96] = payload[1][f["visible_idx"][lo:hi]].view(np.uint8)

                    s = time.perf_counter()
                    fill(0, records)
                    line["host_1_thread_ms"] = (time.perf_counter() - s) * 1e3
                    one = out.view(np.uint8).reshape(records, -1).copy()
                    out[:] = np.zeros(1, dtype)
                    callback = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32)(lambda user, lo, hi: fill(lo, hi))
                    s = time.perf_counter()
                    lib.load().gv_host_parallel_ranges(0, records, callback, None)
                    line["host_worker_threads_ms"] = (time.perf_counter() - s) * 1e3
                    line["host_agrees"] = bool(one.tobytes() == got.tobytes() == out.view(np.uint8).tobytes())
                print(json.dumps(line), flush=True)
                lines.append(line)
                if name == "sprite96":
                    vis.bind_payload(0, None)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
