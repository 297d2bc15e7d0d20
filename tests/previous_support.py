"""Test helpers of gv_pool_keep_models / gv_pool_forget_models / gv_pool_emit_previous: the C twin (tests/previous_twin.h) built into a
shared library with a numpy-backed history, the two frames every case of tests/second_phase_support.py's table runs (frame 1: the
table's own view against the case's depth image A; frame 2: the camera moved and turned, a marked 10 % of the transforms moved, the
same pyramid),
the census of those frames on the oracle, and the expected bytes of an emission, which come from the twin fed the FETCHED records.
TEST INFRASTRUCTURE ONLY."""
import collections
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

import second_phase_support as sp
from garden_amd import scene
from hiz_paths_support import header_constant

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
SEED = scene.SEED

# gv_previous_kernels.hpp
BLOCK, TILES, ROW_BYTES, STAMP_WORD = 256, 4, 64, 12
HEADER_NAMES = {"kPreviousBlock": BLOCK, "kPreviousEmitTiles": TILES, "kPreviousRowBytes": ROW_BYTES, "kPreviousStampWord": STAMP_WORD, "kMinPreviousStride": 64,
                "kMaxPreviousStride": 256}
# draw counts of the kernel edges: empty, one lane, a wave's and a tile's edges, one more than the TILES * BLOCK records of an emit workgroup
EDGE_DRAWS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
EDGE_SLOTS = 2048

# frame 2 of a case: the camera moves by CAMERA_STEP and turns by TURN (a fraction of a second unit quaternion added to the first); the
# transforms whose slot s has (s // MOVE_RUN) % 10 == MOVE_PHASE — 10 % of them, in runs that make few dirty ranges — move by MOVE_STEP
CAMERA_STEP = (2.5, -1.25, 3.0)
TURN = 0.01
MOVE_RUN, MOVE_PHASE = 4, 3
MOVE_STEP = (2.0, -1.5, 0.75)
CLASS_MIN = 64  # draws each class holds in a case that can hold them (class_floor)


def header_constants():
    return {name: header_constant("gv_previous_kernels.hpp", name) for name in HEADER_NAMES}


# ---- the twin --------------------------------------------------------------------------------------------------------------------

class _TwinHistory(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("slots", C.c_uint32), ("epoch", C.c_uint32), ("view_proj", C.c_float * 16),
                ("camera_position", C.c_float * 3)]


_TWIN_SRC = """#include "previous_twin.h"
void twin_keep(PreviousTwinHistory* h, const float* vp, const float* cam, const uint32_t* slots, const float* models, uint32_t n, int add)
{ previous_twin_keep(h, vp, cam, slots, models, n, add); }
void twin_forget(PreviousTwinHistory* h, uint32_t first, uint32_t count) { previous_twin_forget(h, first, count); }
uint32_t twin_many(const PreviousTwinHistory* h, const float* vp, const float* cam, const float* pvp, int cut, const uint32_t* slots,
                   const float* models, uint32_t n, float* out, uint32_t* has)
{ return previous_twin_many(h, vp, cam, pvp, cut, slots, models, n, out, has); }
void twin_mvp(const float* view_proj, const float* model, float* mvp) { instance_twin_mvp(view_proj, model, mvp); }
"""


@functools.lru_cache(maxsize=None)
def build_twin(directory):
    """gcc -O2 -ffp-contract=off of the twin into `directory`; returns the ctypes library"""
    src = os.path.join(str(directory), "previous_twin.c")
    out = os.path.join(str(directory), "libprevious_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", HERE, src,
                    "-o", out, "-lm"], check=True)
    lib = C.CDLL(out)
    P, U32 = C.c_void_p, C.c_uint32
    lib.twin_keep.argtypes = [P, P, P, P, P, U32, C.c_int]
    lib.twin_keep.restype = None
    lib.twin_forget.argtypes = [P, U32, U32]
    lib.twin_forget.restype = None
    lib.twin_many.argtypes = [P, P, P, P, C.c_int, P, P, U32, P, P]
    lib.twin_many.restype = U32
    lib.twin_mvp.argtypes = [P, P, P]
    lib.twin_mvp.restype = None
    return lib


def _f32(a, n):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)[:n].copy()


class History:
    """PoolState::Models as the twin keeps it: rows of 16 words per pool slot"""

    def __init__(self, twin):
        self.twin = twin
        self.rows = np.zeros((0, 16), np.uint32)
        self.h = _TwinHistory()

    @property
    def epoch(self):
        return int(self.h.epoch)

    @property
    def slots(self):
        return int(self.h.slots)

    def _sync(self):
        self.h.rows = self.rows.ctypes.data

    def _records(self, fetched):
        n = int(fetched["draw_count"])
        slots = np.ascontiguousarray(fetched["visible_idx"][:n], dtype=np.uint32)
        models = np.ascontiguousarray(fetched["baked_model"][:n], dtype=np.float32).reshape(n, 12)
        return n, slots, models

    def keep(self, view, fetched, occupancy, add=False):
        """gv_pool_keep_models of a view (the view dict) whose records were fetched in delivery order (order='raw')"""
        if occupancy > self.h.slots:  # the coverage grows: old rows survive, new rows are zero
            grown = np.zeros((occupancy, 16), np.uint32)
            grown[:self.h.slots] = self.rows[:self.h.slots]
            self.rows, self.h.slots = grown, occupancy
        self._sync()
        n, slots, models = self._records(fetched)
        vp, cam = _f32(view["view_proj"], 16), _f32(view["camera_position"], 3)
        self.twin.twin_keep(C.addressof(self.h), vp.ctypes.data, cam.ctypes.data, slots.ctypes.data, models.ctypes.data, n, 1 if add else 0)

    def forget(self, first=0, count=0):
        self._sync()
        self.twin.twin_forget(C.addressof(self.h), first, count)

    def expect(self, view, fetched, prev_view_proj=None, cut=False):
        """(prev_mvp [n, 16] float32, has_history [n] uint32, kept draws) of gv_pool_emit_previous over the fetched records"""
        self._sync()
        n, slots, models = self._records(fetched)
        vp, cam = _f32(view["view_proj"], 16), _f32(view["camera_position"], 3)
        pvp = None if prev_view_proj is None else _f32(prev_view_proj, 16)
        out, has = np.zeros((n, 16), np.float32), np.zeros(n, np.uint32)
        kept = self.twin.twin_many(C.addressof(self.h), vp.ctypes.data, cam.ctypes.data, None if pvp is None else pvp.ctypes.data, 1 if cut else 0,
                                   slots.ctypes.data, models.ctypes.data, n, out.ctypes.data, has.ctypes.data)
        return out, has, int(kept)


def layout_dtype(stride=64, prev_mvp=0, has_history=None):
    names, formats, offsets = ["prevMvp"], [(np.float32, 16)], [prev_mvp]
    if has_history is not None:
        names.append("hasHistory"), formats.append(np.uint32), offsets.append(has_history)
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=stride))


def same_words(got, exp, what=""):
    """two float arrays word for word; a NaN is compared as a class: NaN where NaN is expected, any payload"""
    g, e = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(exp, dtype=np.float32)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    nan = np.isnan(e)
    assert np.array_equal(np.isnan(g), nan), what
    bad = (g.view(np.uint32) != e.view(np.uint32)) & ~nan
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def same_items(items, dtype, exp_mvp, exp_has, what=""):
    """the fetched items [written, stride] uint8 against the twin's answer for the first `written` draws"""
    written = len(items)
    rows = np.ascontiguousarray(items).reshape(-1).view(dtype) if written else np.zeros(0, dtype)
    same_words(rows["prevMvp"], exp_mvp[:written], what)
    if "hasHistory" in dtype.names:
        assert rows["hasHistory"].tolist() == exp_has[:written].tolist(), what


# ---- the two frames of a case ------------------------------------------------------------------------------------------------------

def first_view():
    return sp.view()


def second_view(turn=TURN, step=CAMERA_STEP):
    """the camera of sp.view(), moved by `step` and turned: its quaternion plus `turn` times a second unit quaternion, normalised"""
    rng = np.random.Generator(np.random.PCG64(SEED ^ 0xC0FFEE))
    q = scene._unit_quats(rng, 1)[0]
    q = (q + np.float32(turn) * scene._unit_quats(rng, 1)[0]).astype(np.float32)
    q = (q / np.sqrt(np.sum(q * q, dtype=np.float32), dtype=np.float32)).astype(np.float32)
    proj = scene.persp_inf_rev_z(math.radians(90.0), 16.0 / 9.0, 0.01)
    return scene.make_view(scene.mul_cm(proj, scene.view_from_quat(q)), camera_position=step, use_hiz=1)


def moved_transforms(n, phase=MOVE_PHASE):
    """bool[n]: the transform slots that move between the frames"""
    return (np.arange(n) // MOVE_RUN) % 10 == phase


def moved_runs(n, phase=MOVE_PHASE):
    """(first, count) of every run of moved transform slots: the GV_DIRTY_TRANSFORM marks"""
    return [(first, min(MOVE_RUN, n - first)) for first in range(phase * MOVE_RUN, n, 10 * MOVE_RUN)]


def move(sc, phase=MOVE_PHASE, step=MOVE_STEP):
    """moves the marked transforms of `sc` in place; returns the marks"""
    n = len(sc.transforms)
    sc.transforms["position"][moved_transforms(n, phase), :3] += np.asarray(step, np.float32)
    return moved_runs(n, phase)


def mesh_moved(sc, phase=MOVE_PHASE):
    """bool per mesh slot: its own transform is one of the moved ones"""
    entity = sc.meshes["entity"].astype(np.int64)
    slot = np.where(entity < len(sc.entity_to_transform), sc.entity_to_transform[np.minimum(entity, len(sc.entity_to_transform) - 1)], NONE)
    moved = moved_transforms(len(sc.transforms), phase)
    return (slot != NONE) & moved[np.minimum(slot, len(moved) - 1)]


Census = collections.namedtuple("Census", "draws unmoved moved fresh")


@functools.lru_cache(maxsize=None)
def census(name):
    """the oracle's two frames of a case: the draws of frame 2, and of those the kept and unmoved, the kept and moved, the fresh"""
    c = sp.CASE_BY_NAME[name]
    a, _ = sp.depth_images(c)
    sc = sp.world(c)
    first = np.asarray(sp.oracle_cull(sc, first_view(), a, c.rg16f)["visible_idx"], np.uint32)
    move(sc)
    second = np.asarray(sp.oracle_cull(sc, second_view(), a, c.rg16f)["visible_idx"], np.uint32)
    kept = np.isin(second, first)
    moved = mesh_moved(sc)[second] if len(second) else np.zeros(0, bool)
    return Census(len(second), int((kept & ~moved).sum()), int((kept & moved).sum()), int((~kept).sum()))


def class_floor(c):
    """What each class must hold in case `c`. 64 draws wherever the case can hold them: the moved class is 10 % of the draws both frames
    share, and those are a part of the frustum's share of the pool, so a pool below 64 * 10 * 8 = 5120 slots cannot; there each class
    must still hold a draw — except where even that cannot be (the declared empty case of the table, and pools of fewer than 10 * MOVE_RUN
    slots per visible draw), where the case runs the kernels' small sizes and the classes are covered by the larger cases."""
    if c.empty or c.n < 256:
        return 0
    return CLASS_MIN if c.n >= 5120 else 1
