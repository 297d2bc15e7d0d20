"""gv_pool_emit_instances on the CPU tier: the header declares the four entry points and the library exports them, GvInstanceLayout
has the C layout in ctypes, and the C twin of the instance arithmetic (tests/instance_twin.h) passes
hand-derived cases, gives the same bits with and without hardware fma, and stays inside the rounding bound of its four operations
against float64."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import instances_support as isup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gv_pool_set_instance_layout", "gv_pool_emit_instances", "gv_pool_instances_device", "gv_pool_instances_info",
           "gv_pool_instances_fetch")


def test_header_declares_and_library_exports_the_entry_points():
    from garden_amd import lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in lib.EXPORTS, name
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        for name in SYMBOLS:
            assert hasattr(handle, name), name
        assert handle.gv_abi_version() == 4
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-pedantic"], ["g++", "-std=c++11", "-pedantic", "-x", "c++"]], ids=["c99", "cxx11"])
def test_instance_layout_struct_matches_the_header(tmp_path, compiler):
    from garden_amd import lib
    cls = lib.GvInstanceLayout
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "garden_vis.h"', "int main(void) {",
             '    printf("%zu", sizeof(GvInstanceLayout));']
    for field, _ in cls._fields_:
        lines.append(f'    printf(" %zu", offsetof(GvInstanceLayout, {field}));')
    lines += ['    printf("\\n");', "    return 0;", "}"]
    src = tmp_path / "instance_abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "instance_abi"
    subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, *offsets = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(cls) == 20
    assert [int(o) for o in offsets] == [getattr(cls, f).offset for f, _ in cls._fields_] == [0, 4, 8, 12, 16]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return isup.build_twin(tmp_path_factory.mktemp("twin"))


IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


def completed(model):
    """the 12 floats as the column-major 4x4 with the bottom row (0, 0, 0, 1)"""
    m = np.zeros((4, 4), np.float32)  # m[c][r]
    m[:, :3] = np.asarray(model, np.float32).reshape(4, 3)
    m[3][3] = 1.0
    return m.reshape(16)


def test_twin_identity_view_proj_keeps_the_model_bit_for_bit(twin):
    rng = np.random.Generator(np.random.PCG64(1))
    for model in rng.standard_normal((64, 12)).astype(np.float32) * np.float32(1000.0):
        assert isup.bits(isup.twin_mvp(twin, IDENTITY, model)).tolist() == isup.bits(completed(model)).tolist()


def test_twin_pure_scale(twin):
    # diag(2, 3, 0.5, 1): row i of every column times s_i — one rounding, the other three terms are +0
    vp = np.diag(np.array([2, 3, 0.5, 1], np.float32)).reshape(16)
    model = np.array([1.5, -2.25, 7, 0.1, 0.2, 0.3, -5, 11, 13, 100.5, -200.25, 0.7], np.float32)
    exp = completed(model).reshape(4, 4) * np.array([2, 3, 0.5, 1], np.float32)[None, :]  # [c][r] * s_r, in float32
    assert isup.bits(isup.twin_mvp(twin, vp, model)).tolist() == isup.bits(exp.reshape(16)).tolist()


def test_twin_orthographic_reversed_z_by_hand(twin):
    # calcOrthoProjRevZ(width 8, height 4, near 0, far 16): x' = x / 4, y' = -y / 2, z' = 1 - z / 16, w' = 1
    vp = np.zeros(16, np.float32)
    vp[0], vp[5], vp[10], vp[14], vp[15] = 0.25, -0.5, -0.0625, 1.0, 1.0
    model = np.array([2, 0, 0, 0, 4, 0, 0, 0, 8, 4, -2, 8], np.float32)  # scale (2, 4, 8) at (4, -2, 8)
    exp = np.array([0.5, 0, 0, 0,      # c0: (2, 0, 0, 0)
                    0, -2, 0, 0,       # c1: (0, 4, 0, 0)
                    0, 0, -0.5, 0,     # c2: (0, 0, 8, 0)
                    1, 1, 0.5, 1],     # c3: (4, -2, 8, 1): 4/4, 2/2, 1 - 8/16, 1
                   np.float32)
    got = isup.twin_mvp(twin, vp, model)
    assert isup.bits(got).tolist() == isup.bits(exp).tolist()  # every zero is +0: a chain that starts at +0 never leaves -0 behind a zero product


def test_twin_negative_zero_is_decided_by_the_fourth_term(twin):
    # element [0][0]: fma(a3, 0, fma(0, -1, fma(0, -1, fma(-1e-30, 1e-30, +0)))): the product underflows to -0 and the two -0 products
    # keep it; the LAST term a3 * 0 decides: +0 for a3 = 0 or positive (+0 + -0 = +0), -0 for a negative a3. Without the term: -0 always.
    model = np.array([1e-30, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)
    vp = np.zeros(16, np.float32)
    vp[0] = -1e-30
    assert int(isup.bits(isup.twin_mvp(twin, vp, model))[0]) == 0x00000000
    vp[12] = 5.0
    assert int(isup.bits(isup.twin_mvp(twin, vp, model))[0]) == 0x00000000
    vp[12] = -5.0
    assert int(isup.bits(isup.twin_mvp(twin, vp, model))[0]) == 0x80000000


def test_twin_non_finite_view_proj_reaches_every_column(twin):
    # a NaN (or infinite) translation entry of view_proj meets the bottom-row 0 of the model's columns 0..2: NaN * 0 and inf * 0 are NaN
    model = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.float32)
    clean = isup.twin_mvp(twin, IDENTITY, model)
    for bad in (np.nan, np.inf, -np.inf):
        vp = IDENTITY.copy()
        vp[12] = bad  # a.c3[0]: row 0 of the last column
        got = isup.twin_mvp(twin, vp, model)
        row0 = got.reshape(4, 4)[:, 0]
        assert np.isnan(row0[:3]).all(), (bad, row0)
        assert np.isnan(row0[3]) if np.isnan(bad) else row0[3] == bad  # column 3: fma(bad, 1, 10)
        rest = np.ones(16, bool)
        rest[[0, 4, 8, 12]] = False
        assert isup.bits(got)[rest].tolist() == isup.bits(clean)[rest].tolist()
    # a NaN in the model stays in its own column
    model[4] = np.nan
    got = isup.twin_mvp(twin, IDENTITY, model).reshape(4, 4)
    assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2, 3]]).any()


def random_pairs(n, seed):
    """n (view_proj, model) pairs: perspective and orthographic projections times a random rotation, TRS-like models"""
    from garden_amd import scene
    rng = np.random.Generator(np.random.PCG64(seed))
    vps = np.empty((n, 16), np.float32)
    quats = rng.standard_normal((n, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    for k in range(n):
        if k & 1:
            proj = scene.persp_inf_rev_z(math.radians(rng.uniform(30, 120)), rng.uniform(0.5, 2.5), 10.0 ** rng.uniform(-3, 0))
        else:
            proj = scene.ortho_rev_z(10.0 ** rng.uniform(0, 4), 10.0 ** rng.uniform(0, 4), -(10.0 ** rng.uniform(0, 4)), 10.0 ** rng.uniform(0, 4))
        vps[k] = scene.mul_cm(proj, scene.view_from_quat(quats[k].astype(np.float32)))
    models = rng.standard_normal((n, 12)).astype(np.float32)
    models[:, :9] *= (10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
    models[:, 9:] *= (10.0 ** rng.uniform(0, 4, (n, 1))).astype(np.float32)
    return vps, models


def test_twin_same_bits_with_and_without_hardware_fma(twin, tmp_path):
    haswell = isup.build_twin(tmp_path, march="haswell")
    vps, models = random_pairs(2000, 3)
    for vp, m in zip(vps, models):
        assert isup.bits(isup.twin_mvp(twin, vp, m)).tolist() == isup.bits(isup.twin_mvp(haswell, vp, m)).tolist()


def test_twin_against_float64_within_the_bound_of_four_rounded_operations(twin):
    """per element |err| <= gamma_4 * sum_k |a_k * b_k|, gamma_4 = 4u / (1 - 4u), u = 2^-24: the standard bound for four rounded
    operations (one per fma of the chain), not a tuned tolerance"""
    n = 100_000
    vps, models = random_pairs(n, 4)
    got = np.empty((n, 16), np.float32)
    for k in range(n):
        twin.twin_mvp(vps[k].ctypes.data, models[k].ctypes.data, got[k].ctypes.data)
    a = vps.astype(np.float64).reshape(n, 4, 4)  # a[n][k][i] = a.c_k[i]
    b = np.zeros((n, 4, 4), np.float64)          # b[n][j][k] = b.c_j[k]
    b[:, :, :3] = models.astype(np.float64).reshape(n, 4, 3)
    b[:, 3, 3] = 1.0
    ref = np.einsum("nki,njk->nji", a, b)
    mag = np.einsum("nki,njk->nji", np.abs(a), np.abs(b))
    u = 2.0 ** -24
    gamma4 = 4 * u / (1 - 4 * u)
    err = np.abs(got.astype(np.float64).reshape(n, 4, 4) - ref)
    worst = float((err / np.maximum(mag, np.finfo(np.float64).tiny)).max())
    print(f"worst |err| / sum|a_k b_k| = {worst:.3e}, gamma_4 = {gamma4:.3e}")
    assert (err <= gamma4 * mag).all()
