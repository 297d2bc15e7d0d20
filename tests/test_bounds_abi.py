"""gv_pool_view_bounds and its companions on the CPU tier: the header declares the three entry points with the signatures
garden_amd/lib.py binds, the library exports them, GvViewBounds is 32 bytes in C99 and in ctypes, the ABI version is still 4 (the
change is additive); the C twin of the rule the GPU tests compare against (tests/bounds_twin.h) gives the answers written out by
hand below; a census of the GPU case table (tests/bounds_support.py) on the oracle's records; and the csm_lite.hpp side of the shim
(csm::fit / casterBasis / tightenedDepth) in a small stand-alone C++ program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bounds_support as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32, F32 = C.c_void_p, C.c_uint32, C.c_float
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def signatures():
    from garden_amd import lib
    return {
        "gv_pool_view_bounds": ("GvCtx* ctx, uint32_t pool_id, const uint32_t* view_indices, const float* bases, uint32_t item_count",
                                [P, U32, C.POINTER(U32), C.POINTER(F32), U32]),
        "gv_pool_view_bounds_device": ("GvCtx* ctx, uint32_t pool_id, const void** bounds, uint32_t* item_count",
                                       [P, U32, C.POINTER(P), C.POINTER(U32)]),
        "gv_pool_view_bounds_fetch": ("GvCtx* ctx, uint32_t pool_id, GvViewBounds* bounds, uint32_t capacity",
                                      [P, U32, C.POINTER(lib.GvViewBounds), U32]),
    }


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)


def test_header_declares_the_entry_points_with_these_signatures():
    text = header()
    for name, (params, _) in signatures().items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert " ".join(m.group(1).split()) == params, name
    assert re.search(r"#define GV_MAX_BOUNDS_ITEMS 8u?\b", text)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    for name in signatures():
        assert name in lib.EXPORTS, name
    assert lib.GV_MAX_BOUNDS_ITEMS == 8 == bs.MAX_ITEMS
    assert C.sizeof(lib.GvViewBounds) == 32 and lib.BOUNDS_DTYPE.itemsize == 32 and lib.BOUNDS_DTYPE == bs.BOUNDS_DTYPE
    assert [(n, lib.BOUNDS_DTYPE.fields[n][1]) for n in lib.BOUNDS_DTYPE.names] == [("lo", 0), ("draw_count", 12), ("hi", 16), ("nan_records", 28)]
    assert [(n, getattr(lib.GvViewBounds, n).offset) for n, _ in lib.GvViewBounds._fields_] == \
        [("lo", 0), ("draw_count", 12), ("hi", 16), ("nan_records", 28)]
    for method in ("view_bounds", "view_bounds_device"):
        assert callable(getattr(lib.GpuVisibility, method)), method
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        assert handle.gv_abi_version() == 4
        for name, (_, argtypes) in signatures().items():
            fn = getattr(handle, name)
            assert list(fn.argtypes) == argtypes, name
            assert fn.restype in (C.c_int, C.c_int32), name


def test_header_compiles_as_c99_and_the_struct_is_32_bytes(tmp_path):
    src = tmp_path / "bounds_abi.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "garden_vis.h"\n'
                   "typedef char view_bounds_is_32_bytes[sizeof(GvViewBounds) == 32 ? 1 : -1];\n"
                   "typedef char hi_at_16[offsetof(GvViewBounds, hi) == 16 ? 1 : -1];\n"
                   "typedef char abi_is_4[GV_ABI_VERSION == 4u ? 1 : -1];\n"
                   "int main(void) {\n"
                   "    int (*issue)(GvCtx*, uint32_t, const uint32_t*, const float*, uint32_t) = gv_pool_view_bounds;\n"
                   "    int (*dev)(GvCtx*, uint32_t, const void**, uint32_t*) = gv_pool_view_bounds_device;\n"
                   "    int (*fetch)(GvCtx*, uint32_t, GvViewBounds*, uint32_t) = gv_pool_view_bounds_fetch;\n"
                   "    GvViewBounds b = {{0.0f, 0.0f, 0.0f}, 1u, {1.0f, 1.0f, 1.0f}, 0u};\n"
                   '    printf("%u %u %d\\n", (unsigned)GV_MAX_BOUNDS_ITEMS, b.draw_count + b.nan_records, issue && dev && fetch);\n'
                   "    return 0;\n}\n")
    obj = tmp_path / "bounds_abi.o"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(obj)], check=True)


# ---- the twin against answers written out by hand -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return bs.build_twin(tmp_path_factory.mktemp("bounds_twin"))


def model(translation=(0, 0, 0), diagonal=(1, 1, 1)):
    m = np.zeros(12, np.float32)
    m[0], m[4], m[8] = diagonal
    m[9:12] = translation
    return m


def bits(values):
    return np.asarray(values, np.float32).view(np.uint32).tolist()


def answer(twin, models, boxes, basis):
    e = bs.twin_bounds(twin, models, boxes, basis)
    return bits(e["lo"]), bits(e["hi"]), int(e["draw_count"]), int(e["nan_records"])


def test_twin_one_unit_box_under_the_identity(twin):
    assert answer(twin, [model()], [[0, 0, 0, 1, 1, 1]], bs.IDENTITY) == (bits([0, 0, 0]), bits([1, 1, 1]), 1, 0)


def test_twin_rotated_basis_with_an_exact_answer(twin):
    """a quarter turn about z and a translation: q = (10 - p.y, 20 + p.x, 30 + p.z); the box (1, 2, 3) .. (4, 6, 8) scaled by two
    and moved by (100, 0, 0): p in (102, 4, 6) .. (108, 12, 16)"""
    basis = np.array([0, 1, 0, -1, 0, 0, 0, 0, 1, 10, 20, 30], np.float32)
    got = answer(twin, [model((100, 0, 0), (2, 2, 2))], [[1, 2, 3, 4, 6, 8]], basis)
    assert got == (bits([-2, 122, 36]), bits([6, 128, 46]), 1, 0)


def test_twin_minus_zero_sorts_below_plus_zero(twin):
    """a record whose every term is -0 gives q = -0; one of +0 terms gives +0 (the -0 of the basis is absorbed): lo takes -0 and hi
    takes +0 whatever the order, and each alone answers itself"""
    basis = bs.IDENTITY.copy()
    basis[9:12] = -0.0
    minus, plus = (model((-0.0, -0.0, -0.0)), [-0.0] * 6), (model((0.0, 0.0, 0.0)), [0.0] * 6)
    mz, pz = bits([-0.0] * 3), bits([0.0] * 3)
    assert mz != pz
    for order in ((minus, plus), (plus, minus)):
        assert answer(twin, [r[0] for r in order], [r[1] for r in order], basis) == (mz, pz, 2, 0)
    assert answer(twin, [minus[0]], [minus[1]], basis) == (mz, mz, 1, 0)
    assert answer(twin, [plus[0]], [plus[1]], basis) == (pz, pz, 1, 0)
    assert twin.twin_key(np.float32(-0.0)) == 0x7FFFFFFF and twin.twin_key(np.float32(0.0)) == 0x80000000


def test_twin_nan_is_skipped_in_its_axis_only_and_infinities_take_part(twin):
    """two pivots with empty boxes, (inf, 5, 6) and (1, 2, 3), under rows (1, 0, 0), (0, 1, 0), (-1, 0, 1): the first record gives
    +inf in axis 0, 0 x inf = NaN in axis 1 (all eight corners: counted ONCE) and -inf in axis 2"""
    basis = np.array([1, 0, -1, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    got = answer(twin, [model((INF, 5, 6)), model((1, 2, 3))], [[0] * 6] * 2, basis)
    assert got == (bits([1, 2, -INF]), bits([INF, 2, 2]), 2, 1)
    # the NaN record alone: axis 1 has nothing taking part
    got = answer(twin, [model((INF, 5, 6))], [[0] * 6], basis)
    assert got == (bits([INF, INF, -INF]), bits([INF, -INF, -INF]), 1, 1)
    # a NaN in the basis' translation: that axis is empty, every record counts once
    basis = bs.IDENTITY.copy()
    basis[10] = NAN
    got = answer(twin, [model((1, 2, 3)), model((4, 5, 6))], [[0, 0, 0, 1, 1, 1]] * 2, basis)
    assert got == (bits([1, INF, 3]), bits([5, -INF, 7]), 2, 2)


def test_twin_no_records_is_the_empty_answer(twin):
    assert answer(twin, np.zeros((0, 12), np.float32), np.zeros((0, 6), np.float32), bs.rotation_basis(1)) == \
        (bits([INF] * 3), bits([-INF] * 3), 0, 0)


def test_twin_empty_box_of_a_non_candidate_is_its_pivot(twin):
    m = np.array([0.5, -2.0, 3.0, 1.5, 0.25, -4.0, 7.0, 8.0, -9.0, 7.0, 8.0, 9.0], np.float32)
    assert answer(twin, [m], [[0] * 6], bs.IDENTITY) == (bits([7, 8, 9]), bits([7, 8, 9]), 1, 0)
    meshes = np.zeros(3, dtype=[("entity", np.uint32), ("isEnabled", np.uint8), ("aabbMin", np.float32, (4,)), ("aabbMax", np.float32, (4,))])
    meshes["aabbMin"][:, :3], meshes["aabbMax"][:, :3] = -1.0, 2.0
    meshes["entity"], meshes["isEnabled"] = [1, 0, 3], [1, 1, 0]
    assert bs.aabbs_by_slot(meshes).tolist() == [[-1, -1, -1, 2, 2, 2], [0] * 6, [0] * 6]


# ---- the census of the GPU case table on the oracle ---------------------------------------------------------------------------------

def test_case_table_follows_the_kernel_header():
    assert bs.BLOCK == 256 and bs.R % bs.BLOCK == 0 and bs.R >= bs.BLOCK
    assert set(bs.EDGE_SIZES) == {1, 63, 64, 65, 255, 256, 257, bs.R - 1, bs.R, bs.R + 1, 2 * bs.R + 1, bs.BLOCK * bs.R + 1}
    assert bs.OUTLIER_WORLD == 2 * bs.R + 1 == bs.PLANTED_N
    assert set(bs.OUTLIER_POSITIONS) == {0, 63, 64, 255, 256, bs.R - 1, bs.R, 2 * bs.R} and max(bs.OUTLIER_POSITIONS) < bs.OUTLIER_WORLD
    # BLOCK rows give every lane of the finish kernel one row; one record more opens row BLOCK + 1, which lane 0 folds as its second
    assert (bs.FINISH_TWO_ROWS + bs.R - 1) // bs.R == bs.BLOCK + 1 and (bs.FINISH_TWO_ROWS - 1 + bs.R - 1) // bs.R == bs.BLOCK


@pytest.mark.parametrize("n", bs.EDGE_SIZES)
def test_edge_worlds_have_no_nan_and_several_records_attain_the_extremes(n, twin):
    records, boxes = bs.oracle_records("edge", n)
    assert int(records["draw_count"]) == n  # the enclosing view holds the whole world
    basis = bs.rotation_basis(n)
    e = bs.expected(twin, records, boxes, basis)
    assert int(e["nan_records"]) == 0 and int(e["draw_count"]) == n
    assert np.isfinite(e["lo"]).all() and np.isfinite(e["hi"]).all() and (e["lo"] < e["hi"]).all()
    q = bs.twin_coords(twin, records["baked_model"], boxes[records["visible_idx"]], basis)
    assert bits(q.min(axis=(0, 1))) == bits(e["lo"]) and bits(q.max(axis=(0, 1))) == bits(e["hi"])
    assert len(set(bs.attained_by(q))) >= min(4, n)  # (a world of one record has one)


def test_planted_world_has_some_nan_records_and_finite_values_on_both_sides(twin):
    records, boxes = bs.oracle_records("planted")
    n = int(records["draw_count"])
    assert n > 0.9 * bs.PLANTED_N
    basis = bs.rotation_basis(0)
    e = bs.expected(twin, records, boxes, basis)
    assert 0 < int(e["nan_records"]) < bs.NAN_CAP * n
    q = bs.twin_coords(twin, records["baked_model"], boxes[records["visible_idx"]], basis)
    assert int(e["nan_records"]) == int(np.isnan(q).any(axis=(1, 2)).sum())
    finite = np.isfinite(q)
    for r in range(3):
        assert ((q[..., r] < 0) & finite[..., r]).any() and ((q[..., r] > 0) & finite[..., r]).any(), r
    assert np.isinf(q).any()  # the infinities take part
    # under the identity the far pivots are the extremes, finite
    e = bs.expected(twin, records, boxes, bs.IDENTITY)
    assert np.isfinite(e["lo"]).all() and np.isfinite(e["hi"]).all() and np.abs(e["lo"]).max() > 1.0e19
    # the basis with planted extremes: +-inf on both sides of axis 0, finite axis 1, nothing in axis 2
    e = bs.expected(twin, records, boxes, bs.extreme_basis())
    assert bits(e["lo"]) == bits([-INF, e["lo"][1], INF]) and bits(e["hi"]) == bits([INF, e["hi"][1], -INF])
    assert int(e["nan_records"]) == n


# ---- the shim's csm side ------------------------------------------------------------------------------------------------------------

CSM_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include "garden_amd/csrc/host/csm_lite.hpp"
using namespace garden;
static int fail(const char* what, int a, int b) { printf("FAIL %s (%d, %d)\n", what, a, b); return 1; }
int main()
{
    const float fov = 1.2f, aspect = 16.0f / 9.0f, zCoeff = 10.0f;
    const f32x4 lights[3] = {f32x4(0.3f, -0.8f, 0.5f), f32x4(-0.6f, -0.6f, -0.5f), f32x4(0.0f, -1.0f, 0.0f)};
    const float slices[3][2] = {{0.01f, 8.0f}, {8.0f, 40.0f}, {40.0f, 300.0f}};
    for (int cam = 0; cam < 3; cam++)
        for (int l = 0; l < 3; l++)
            for (int s = 0; s < 3; s++) {
                f32x4x4 view;  // a camera turned about y (translation zeroed)
                const float a = 0.9f * (float)cam;
                view.m[0] = std::cos(a); view.m[2] = std::sin(a); view.m[8] = -std::sin(a); view.m[10] = std::cos(a);
                const csm::CascadeFit fit = csm::fit(view, lights[l], fov, aspect, slices[s][0], slices[s][1], zCoeff, 2048);
                const csm::Cascade plain = csm::calcLightViewProj(view, lights[l], fov, aspect, slices[s][0], slices[s][1], zCoeff, 2048);
                if (memcmp(&fit.cascade, &plain, sizeof(plain)) != 0)
                    return fail("fit().cascade differs from calcLightViewProj", cam, l);
                if (!(fit.lo.z <= fit.sliceLo.z && fit.sliceHi.z <= fit.hi.z && fit.lo.x == fit.sliceLo.x && fit.hi.y == fit.sliceHi.y))
                    return fail("the extended range does not hold the slice", cam, l);
                float basis[12];
                csm::casterBasis(fit, basis);
                // hand-made casters: points in the light view inside the extended range, brought back to the camera-relative world
                const csm::Mat4 back = csm::inverse(fit.stabilized);
                const double zs[4] = {fit.lo.z * 0.5 + fit.sliceLo.z * 0.5, fit.sliceLo.z, 0.5 * (fit.sliceLo.z + fit.sliceHi.z),
                                      fit.sliceHi.z * 0.25 + fit.hi.z * 0.75};
                for (int count = 1; count <= 4; count++) {  // the nearest caster alone, then farther ones as well
                    GvViewBounds b;
                    for (int r = 0; r < 3; r++) { b.lo[r] = INFINITY; b.hi[r] = -INFINITY; }
                    b.draw_count = (uint32_t)count; b.nan_records = 0;
                    float corners[4][3];
                    for (int k = 0; k < count; k++) {
                        const csm::Vec3 p = csm::transformPoint(back, {0.5 * (fit.lo.x + fit.hi.x), 0.5 * (fit.lo.y + fit.hi.y), zs[k]});
                        corners[k][0] = (float)p.x; corners[k][1] = (float)p.y; corners[k][2] = (float)p.z;
                        for (int r = 0; r < 3; r++) {  // the rule's projection
                            const float q = fmaf(basis[r], corners[k][0], fmaf(basis[3 + r], corners[k][1], fmaf(basis[6 + r], corners[k][2], basis[9 + r])));
                            b.lo[r] = std::fmin(b.lo[r], q); b.hi[r] = std::fmax(b.hi[r], q);
                        }
                    }
                    const csm::Cascade tight = csm::tightenedDepth(fit, b);
                    if (memcmp(&tight.cameraOffset, &plain.cameraOffset, sizeof(plain.cameraOffset)) != 0)
                        return fail("cameraOffset changed", cam, count);
                    for (int c = 0; c < 4; c++)  // x and y untouched: rows 0 and 1 of the projection
                        if (tight.viewProj.m[4 * c] != plain.viewProj.m[4 * c] || tight.viewProj.m[4 * c + 1] != plain.viewProj.m[4 * c + 1])
                            return fail("x / y changed", cam, count);
                    // depth of a point = row 2 of viewProj; reversed Z: 1 at the near end, 0 at the far end. The matrix is rounded to
                    // fp32 once (relative 2^-24 per entry, four entries) and the corner and the bound once each: 16 x 2^-24 x the
                    // largest term is the slack
                    for (int k = 0; k < count; k++) {
                        double d = tight.viewProj.m[14], big = std::fabs(d);
                        for (int c = 0; c < 3; c++) { d += (double)tight.viewProj.m[4 * c + 2] * corners[k][c]; big = std::fmax(big, std::fabs((double)tight.viewProj.m[4 * c + 2] * corners[k][c])); }
                        const double slack = 16.0 * big / 16777216.0;
                        if (!(d >= -slack && d <= 1.0 + slack))
                            return fail("a caster corner leaves the depth range", cam * 100 + l * 10 + s, count * 10 + k);
                    }
                    // never wider than the extended range: |d depth / d z| = 1 / (z1 - z0) grows
                    double before = 0, after = 0;
                    for (int c = 0; c < 3; c++) { before += (double)plain.viewProj.m[4 * c + 2] * plain.viewProj.m[4 * c + 2]; after += (double)tight.viewProj.m[4 * c + 2] * tight.viewProj.m[4 * c + 2]; }
                    if (!(after >= before * (1.0 - 1.0e-6)))
                        return fail("the tightened range is wider", cam, count);
                    if (count == 1 && !(after > before * 1.5))
                        return fail("one caster in front of the slice did not tighten the range", cam, l);
                }
                // empty, non-finite and inverted bounds: the cascade as it is
                GvViewBounds e;
                for (int r = 0; r < 3; r++) { e.lo[r] = INFINITY; e.hi[r] = -INFINITY; }
                e.draw_count = 0; e.nan_records = 0;
                GvViewBounds nan = e, inverted = e, infinite = e, beyond = e;
                nan.lo[2] = NAN; nan.hi[2] = 1.0f;
                inverted.lo[2] = 2.0f; inverted.hi[2] = 1.0f;
                infinite.lo[2] = -INFINITY; infinite.hi[2] = 1.0f;
                beyond.lo[2] = beyond.hi[2] = (float)(fit.hi.z * 2.0 + 1.0);  // casters beyond the far end: the range would be empty
                const GvViewBounds* all[5] = {&e, &nan, &inverted, &infinite, &beyond};
                for (int k = 0; k < 5; k++) {
                    const csm::Cascade same = csm::tightenedDepth(fit, *all[k]);
                    if (memcmp(&same, &plain, sizeof(plain)) != 0)
                        return fail("unusable bounds changed the cascade", cam, k);
                }
            }
    printf("csm fit ok\n");
    return 0;
}
"""


def test_csm_fit_is_calc_light_view_proj_and_tightened_depth_holds_the_casters(tmp_path):
    src, exe = tmp_path / "csm_fit.cpp", tmp_path / "csm_fit"
    src.write_text(CSM_PROGRAM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-I", ROOT, str(src), "-o", str(exe), "-lm"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "csm fit ok" in p.stdout, p.stdout + p.stderr
