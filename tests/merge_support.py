"""Test helpers of gv_merge_sorted: the C twin of its order (tests/merge_twin.h) and expected(): the per-pool records fetched
through the existing API, packed into the group's record layout and merged with the twin."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF

_TWIN_SRC = """#include "merge_twin.h"
uint32_t twin_key(uint32_t bits) { return merge_twin_key(bits); }
uint32_t twin_order(const uint32_t* const* keys, const uint32_t* counts, uint32_t lists, int descending, uint32_t* out_list, uint32_t* out_index)
{ return merge_twin_order(keys, counts, lists, descending, out_list, out_index); }
"""


def record_dtype(stride=64, component_offset=0, baked_model=8, distance_sq=56, buffer_index=60):
    """The record struct as a numpy structured dtype (the rest of the stride is padding, delivered as zeros)."""
    names, formats, offsets = ["componentOffset", "bakedModel", "distanceSq"], [np.uint64, (np.float32, 12), np.float32], \
        [component_offset, baked_model, distance_sq]
    if buffer_index is not None:
        names.append("bufferIndex"), formats.append(np.uint32), offsets.append(buffer_index)
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=stride))


SORTED_MESH = record_dtype()                                                                # the 64-byte SortedMesh
WIDE = record_dtype(stride=80, component_offset=64, baked_model=16, distance_sq=4, buffer_index=None)  # 80 bytes, no bufferIndex


def build_twin(directory):
    """gcc -std=c99 -pedantic of the twin into `directory`; returns the ctypes library."""
    src = os.path.join(str(directory), "merge_twin.c")
    out = os.path.join(str(directory), "libmerge_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-fPIC", "-shared", "-I", HERE, src, "-o", out],
                   check=True)
    lib = C.CDLL(out)
    lib.twin_key.argtypes = [C.c_uint32]
    lib.twin_key.restype = C.c_uint32
    lib.twin_order.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    lib.twin_order.restype = C.c_uint32
    return lib


def key_of(bits):
    """T on a uint32 array (numpy)"""
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def twin_order(twin, lists, descending):
    """lists: float32 (or uint32 bit pattern) arrays, each sorted in the direction. Returns (list, index) of every merged entry."""
    keys = [np.ascontiguousarray(np.asarray(k).view(np.uint32)) for k in lists]
    counts = np.array([len(k) for k in keys], np.uint32)
    total = int(counts.sum())
    ptrs = (C.c_void_p * max(len(keys), 1))(*[k.ctypes.data for k in keys])
    out_list, out_index = np.zeros(max(total, 1), np.uint32), np.zeros(max(total, 1), np.uint32)
    got = twin.twin_order(ptrs, counts.ctypes.data, len(keys), 1 if descending else 0, out_list.ctypes.data, out_index.ctypes.data)
    assert got == total
    return out_list[:total], out_index[:total]


def numpy_order(lists, descending):
    """The same order from numpy: a stable sort of the concatenation by T (descending: by ~T, which keeps ties in place)."""
    keys = [np.asarray(k).view(np.uint32) for k in lists]
    t = key_of(np.concatenate(keys)) if keys else np.zeros(0, np.uint32)
    order = np.argsort(~t if descending else t, kind="stable")
    which = np.concatenate([np.full(len(k), l, np.uint32) for l, k in enumerate(keys)]) if keys else np.zeros(0, np.uint32)
    index = np.concatenate([np.arange(len(k), dtype=np.uint32) for k in keys]) if keys else np.zeros(0, np.uint32)
    return which[order], index[order]


def pack(dtype, fetched, buffer_index, component_stride, slot_map=None):
    """One member's fetched records (GpuVisibility.fetch(order="raw")) in the group's layout, every other byte zero."""
    n = int(fetched["draw_count"])
    rows = np.zeros(n, dtype)
    if n:
        slots = fetched["visible_idx"].astype(np.uint64)
        if slot_map is not None:
            slots = np.asarray(slot_map, np.uint32)[fetched["visible_idx"]].astype(np.uint64)
        rows["componentOffset"] = slots * np.uint64(component_stride)
        rows["bakedModel"] = fetched["baked_model"]
        rows["distanceSq"] = fetched["distance_sq"]
        if "bufferIndex" in dtype.names:
            rows["bufferIndex"] = buffer_index
    return rows


def expected(twin, dtype, fetched, items, descending, slot_maps=None):
    """The merged array (uint8 [total * stride]) and counts[items + 1] a group must produce: `fetched` the members' results in item
    order, items = (pool_id, view_index, buffer_index, component_stride) each, slot_maps: {pool_id: index map} of the pools that
    deliver GV_RESULTS_MAP_RECORDS."""
    packed = [pack(dtype, f, it[2], it[3], (slot_maps or {}).get(it[0])) for f, it in zip(fetched, items)]
    which, index = twin_order(twin, [f["distance_sq"] for f in fetched], descending)
    starts = np.concatenate([[0], np.cumsum([len(p) for p in packed])]).astype(np.int64)
    # bytewise from here on: a structured copy would skip the padding
    everything = np.concatenate([p.view(np.uint8).reshape(len(p), dtype.itemsize) for p in packed])
    merged = everything[starts[which] + index]
    counts = np.array([len(p) for p in packed] + [len(everything)], np.uint32)
    return np.ascontiguousarray(merged).reshape(-1), counts
