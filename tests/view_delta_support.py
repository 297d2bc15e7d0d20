"""Test helpers of gv_pool_view_delta: the sizes at which its kernels change path (compared with garden_amd/csrc/gv_delta_kernels.hpp
by tests/test_view_delta_abi.py), the worlds and cameras of the edge cases, and the expected answers, which are exact: the oracle's
sets of pool slots through np.setdiff1d. The case table of the occlusion cases is tests/second_phase_support.py's CASES, imported:
frame 1 culls against depth image A (the oracle's `first` there), frame 2 against B (`full`).
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import second_phase_support as sp
from garden_amd import scene
from hiz_paths_support import header_constant

SEED = scene.SEED
MIN_SHARE = sp.MIN_SHARE  # of the frustum survivors, for each of appeared / vanished / stayed

# gv_delta_kernels.hpp: a set's word, and what a wave / a workgroup of delta_count_kernel and delta_place_kernel spans
WORD, WAVE, GROUP, BLOCK = 64, 4096, 16384, 256
HEADER_NAMES = {"kDeltaWordSlots": WORD, "kDeltaWaveSlots": WAVE, "kDeltaGroupSlots": GROUP, "kDeltaBlock": BLOCK}
# one below, at and one above each; two workgroup spans + 1: a base crosses a workgroup (and BLOCK entries + 1: the mark launches' second workgroup)
EDGE_SIZES = (WORD - 1, WORD, WORD + 1, BLOCK + 1, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1)


def header_constants():
    return {name: header_constant("gv_delta_kernels.hpp", name) for name in HEADER_NAMES}


def edge_world(n):
    return scene.flat_scene(n, seed=SEED + n)


def cameras():
    """two frustum-only main cameras at the origin that look different ways (no pyramid)"""
    return scene.main_camera_view(seed=SEED), scene.main_camera_view(seed=SEED + 1)


def slots_of(sc, view, depth=None, rg16f=False):
    """the oracle's set of one cull: pool slots, ascending"""
    return np.asarray(sp.oracle_cull(sc, view, depth, rg16f)["visible_idx"], np.uint32)


@functools.lru_cache(maxsize=None)
def edge_sets(n):
    """(C1, C2) of the edge world of n slots under the two cameras; computed once, treat as read-only"""
    sc = edge_world(n)
    first, second = cameras()
    return slots_of(sc, first), slots_of(sc, second)


@functools.lru_cache(maxsize=None)
def enclosed_set(n):
    """C3 of the edge world: an orthographic view that holds the whole scene (the dense answer: nearly every slot appears)"""
    return slots_of(edge_world(n), enclosing())


def enclosing(half=1.0e7):
    return scene.make_view(scene.ortho_rev_z(2 * half, 2 * half, -half, half))


def delta(previous, current):
    """(appeared, vanished) of two sets of slots, ascending each"""
    return np.setdiff1d(current, previous).astype(np.uint32), np.setdiff1d(previous, current).astype(np.uint32)


def case_sets(name):
    """(C1, C2) of a case of sp.CASES: the oracle's first (against A) and full (against B)"""
    e = sp.expected(name)
    return np.asarray(e.first["visible_idx"], np.uint32), np.asarray(e.full["visible_idx"], np.uint32)


def bytes_of(slots, n):
    out = np.zeros(n, np.uint8)
    out[slots] = 1
    return out


def same_answer(got, previous, current, universe):
    appeared, vanished = delta(previous, current)
    assert got["appeared"].dtype == np.uint32 and got["vanished"].dtype == np.uint32
    assert got["appeared"].tolist() == appeared.tolist()
    assert got["vanished"].tolist() == vanished.tolist()
    assert (got["visible_count"], got["slots"]) == (len(current), universe)
