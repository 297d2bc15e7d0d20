"""Test helpers of gv_pool_emit_instances: the C twin (tests/instance_twin.h) built into a shared library, instance layouts as
numpy structured dtypes, and the expected instance bytes of an emission from the fetched records. TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF

_TWIN_SRC = """#include "instance_twin.h"
void twin_mvp(const float* view_proj, const float* model, float* mvp) { instance_twin_mvp(view_proj, model, mvp); }
void twin_many(const float* view_proj, const float* models, uint32_t n, float* mvps) { instance_twin_many(view_proj, models, n, mvps); }
"""


def build_twin(directory, march=None):
    """gcc -O2 -ffp-contract=off (optionally -march=...) of the twin into `directory`; returns the ctypes library."""
    src = os.path.join(str(directory), "instance_twin.c")
    out = os.path.join(str(directory), "libinstance_twin%s.so" % ("_" + march if march else ""))
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    cmd = ["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out, "-lm"]
    if march:
        cmd.insert(3, "-march=" + march)
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    P = C.c_void_p
    lib.twin_mvp.argtypes = [P, P, P]
    lib.twin_mvp.restype = None
    lib.twin_many.argtypes = [P, P, C.c_uint32, P]
    lib.twin_many.restype = None
    return lib


def twin_mvp(twin, view_proj, model):
    vp = np.ascontiguousarray(view_proj, dtype=np.float32).reshape(16)
    m = np.ascontiguousarray(model, dtype=np.float32).reshape(12)
    out = np.empty(16, np.float32)
    twin.twin_mvp(vp.ctypes.data, m.ctypes.data, out.ctypes.data)
    return out


def twin_many(twin, view_proj, models):
    vp = np.ascontiguousarray(view_proj, dtype=np.float32).reshape(16)
    m = np.ascontiguousarray(models, dtype=np.float32).reshape(-1, 12)
    out = np.empty((len(m), 16), np.float32)
    twin.twin_many(vp.ctypes.data, m.ctypes.data, len(m), out.ctypes.data)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def layout_dtype(stride=64, mvp=0, model=None, slot=None, distance_sq=None):
    """The instance struct as a numpy structured dtype (fields at explicit offsets; the rest of the stride is the plugin's)."""
    names, formats, offsets = ["mvp"], [(np.float32, 16)], [mvp]
    for name, fmt, at in (("model", (np.float32, 12), model), ("slot", np.uint32, slot), ("distanceSq", np.float32, distance_sq)):
        if at is not None:
            names.append(name), formats.append(fmt), offsets.append(at)
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=stride))


BARE = layout_dtype()
FULL = layout_dtype(stride=128, mvp=0, model=64, slot=112, distance_sq=116)


def field_mask(dtype):
    """bool[stride]: the bytes of an instance that belong to the layout's fields"""
    mask = np.zeros(dtype.itemsize, bool)
    for name in dtype.names:
        sub, at = dtype.fields[name][0], dtype.fields[name][1]
        mask[at:at + sub.itemsize] = True
    return mask


def expected(twin, dtype, views, fetched, index_map=None, background=None):
    """The bytes an emission of `views` (the view dicts, in the order listed) must produce from the `fetched` results of the same
    views (GpuVisibility.fetch(order="raw")): a uint8 array [total, stride] over `background` (a uint8 pattern [>= total, stride],
    default zeros), and starts."""
    counts = [int(f["draw_count"]) for f in fetched]
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    total = int(starts[-1])
    rows = np.zeros(total, dtype)
    raw = rows.view(np.uint8).reshape(total, dtype.itemsize)
    if background is not None:
        raw[:] = background[:total]
    for v, f, at in zip(views, fetched, starts[:-1]):
        n = int(f["draw_count"])
        if not n:
            continue
        part = rows[at:at + n]
        part["mvp"] = twin_many(twin, v["view_proj"], f["baked_model"])
        if "model" in dtype.names:
            part["model"] = f["baked_model"]
        if "slot" in dtype.names:
            part["slot"] = f["visible_idx"] if index_map is None else np.asarray(index_map, np.uint32)[f["visible_idx"]]
        if "distanceSq" in dtype.names:
            part["distanceSq"] = f["distance_sq"]
    return raw, starts


def same_results(a, b):
    """two GpuVisibility.fetch dicts, byte for byte"""
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
