"""Test helpers of gv_pool_select_lods: the C twin (tests/lod_twin.h) built into a shared library, the expected selection of an
emission from the fetched records, the expected command bytes given per-DRAW geometry ids (the placement rule of DESIGN.md §4 item
10 restated over tests/commands_support.view_commands), and the flat world the GPU tests use. TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

import commands_support as csup

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_LEVELS = 8
LOD_DTYPE = np.dtype([("levels", np.uint32), ("switch_at", np.float32, (MAX_LEVELS - 1,))])

_TWIN_SRC = """#include "lod_twin.h"
uint32_t twin_level(const float* model, float size, float scale, uint32_t levels, const float* switch_at)
{
    return lod_twin_level(model, size, scale, levels, switch_at);
}
uint32_t twin_effective(uint32_t base, uint32_t level) { return lod_twin_effective(base, level); }
void twin_many(const float* models, const uint32_t* base, const float* size, uint32_t n, float scale, const uint32_t* table,
               uint32_t table_count, uint32_t* out, uint32_t* hist)
{
    lod_twin_many(models, base, size, n, scale, table, table_count, out, hist);
}
"""


def build_twin(directory):
    """gcc -O2 -ffp-contract=off of the twin into `directory`; returns the ctypes library."""
    src = os.path.join(str(directory), "lod_twin.c")
    out = os.path.join(str(directory), "liblod_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", HERE, src, "-o", out, "-lm"],
                   check=True)
    lib = C.CDLL(out)
    P, U32, F = C.c_void_p, C.c_uint32, C.c_float
    lib.twin_level.argtypes = [P, F, F, U32, P]
    lib.twin_level.restype = U32
    lib.twin_effective.argtypes = [U32, U32]
    lib.twin_effective.restype = U32
    lib.twin_many.argtypes = [P, P, P, U32, F, P, U32, P, P]
    lib.twin_many.restype = None
    return lib


def lod_table(rows):
    """rows of (levels, [switch_at ...]) as a LOD_DTYPE array (the words behind the thresholds given stay 0)"""
    table = np.zeros(len(rows), LOD_DTYPE)
    for k, (levels, switch_at) in enumerate(rows):
        table[k]["levels"] = levels
        table[k]["switch_at"][:len(switch_at)] = np.asarray(switch_at, np.float32)
    return table


def model_at(x, y, z):
    """a bakedModel (12 floats, float4x3 order) whose translation is (x, y, z)"""
    m = np.zeros(12, np.float32)
    m[0] = m[4] = m[8] = 1.0
    m[9:12] = (x, y, z)
    return m


def twin_level(twin, model, size, scale, levels, switch_at):
    m = np.ascontiguousarray(model, dtype=np.float32).reshape(12)
    sw = np.zeros(MAX_LEVELS - 1, np.float32)
    sw[:len(switch_at)] = np.asarray(switch_at, np.float32)
    return int(twin.twin_level(m.ctypes.data, np.float32(size), np.float32(scale), int(levels), sw.ctypes.data))


def twin_many(twin, models, base, size, scale, table):
    """(g[n], hist[8]) of n draws of one view: models [n, 12], base ids and sizes PER DRAW"""
    m = np.ascontiguousarray(models, dtype=np.float32).reshape(-1, 12)
    b = np.ascontiguousarray(base, dtype=np.uint32)
    r = np.ascontiguousarray(size, dtype=np.float32)
    t = np.ascontiguousarray(table)
    assert t.dtype == LOD_DTYPE and len(b) == len(m) == len(r)
    out, hist = np.zeros(len(m), np.uint32), np.zeros(MAX_LEVELS, np.uint32)
    twin.twin_many(m.ctypes.data, b.ctypes.data, r.ctypes.data, len(m), np.float32(scale), t.ctypes.data, len(t), out.ctypes.data,
                   hist.ctypes.data)
    return out, hist


def select_expected(twin, fetched, scales, ids, sizes, table):
    """What a selection behind an emission of the `fetched` views (GpuVisibility.fetch(order="raw"), in the emission's order) must
    give: (g per view, level_counts [views, 8]). ids / sizes: per POOL slot, or None (id 0 / size 1)."""
    per_view, counts = [], np.zeros((len(fetched), MAX_LEVELS), np.uint32)
    for v, f in enumerate(fetched):
        n = int(f["draw_count"])
        slots = f["visible_idx"][:n].astype(np.int64)
        base = np.zeros(n, np.uint32) if ids is None else np.asarray(ids)[slots].astype(np.uint32)
        size = np.ones(n, np.float32) if sizes is None else np.asarray(sizes, np.float32)[slots]
        g, counts[v] = twin_many(twin, np.asarray(f["baked_model"], np.float32).reshape(-1, 12)[:n], base, size, scales[v], table)
        per_view.append(g)
    return per_view, counts


def expected_commands(fetched, starts, bases, draw_ids, table, dtype, merge=False, region=0, capacity=None, pattern=None):
    """commands_support.expected with the geometry id of every DRAW given (draw_ids: one array per view) instead of one id per pool
    slot: each view's commands come from commands_support.view_commands over the draws themselves, the placement (packed /
    regions, capacity, padding) is restated here."""
    stride = dtype.itemsize
    per_view = []
    for v, f in enumerate(fetched):
        n = int(f["draw_count"])
        assert len(draw_ids[v]) == n
        if bases is None:
            first = [int(starts[v]) + k for k in range(n)] + [int(starts[v + 1])]
        else:
            first_instance, draw_starts = bases
            first = [int(first_instance[int(draw_starts[v]) + k]) for k in range(n)] + [int(starts[v + 1])]
        per_view.append(csup.view_commands(np.arange(n), first, draw_ids[v], table, merge))  # ("slot" k holds the id of draw k)
    counts = np.array([len(c) for c in per_view], np.uint32)
    placed, at = {}, 0
    for v, commands in enumerate(per_view):
        if region:
            for j in range(region):
                placed[v * region + j] = commands[j] if j < len(commands) else None
        else:
            for j, c in enumerate(commands):
                placed[at + j] = c
            at += len(commands)
    rows = len(pattern)
    room = rows if capacity is None else capacity
    out = pattern.copy()
    one = np.zeros(1, dtype)
    for position, c in placed.items():
        if position >= room:
            continue
        assert position < rows, "the pattern is too small for the test's own target"
        one[:] = 0
        if c is not None:
            for name in dtype.names:
                one[name] = c[name]
        out[position] = one.view(np.uint8).reshape(stride)
    return out, counts


def quantile_thresholds(positions, sizes, levels, camera=(0.0, 0.0, 0.0), scale=1.0):
    """switch_at[0 .. levels - 2]: the world's own quantiles of sqrt(d2 * scale) / size at j / levels, so that every level holds
    about n / levels draws by construction (non-finite ratios are left out)"""
    t = np.asarray(positions, np.float64)[:, :3] - np.asarray(camera, np.float64)
    with np.errstate(all="ignore"):
        ratio = np.sqrt((t * t).sum(axis=1) * scale) / np.asarray(sizes, np.float64)
    ratio = ratio[np.isfinite(ratio)]
    return [float(np.quantile(ratio, j / levels)) for j in range(1, levels)]
