"""gv_pool_bind_cluster_lods / gv_pool_cull_cluster_lods on the CPU tier. The header declares both entry points, GvClusterLod (48
bytes) and GvClusterLodView (32 bytes) with the stated layouts and signatures (a compile check against the header itself, C11 for
_Static_assert; the C99 twin checks the same sizes in tests/cluster_lods_support.py);
GV_ABI_VERSION is still 4 (the change is additive); the library exports the symbols; garden_amd/lib.py binds the same signatures, has
CLUSTER_LOD_DTYPE and CLUSTER_LOD_VIEW_DTYPE with the header's offsets, GpuVisibility.bind_cluster_lods and the `lods` keyword of
cull_clusters, default None; a NULL context gives GV_E_ARG."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t

COMPILE_CHECK = r"""
#include <stddef.h>
#include "garden_vis.h"
_Static_assert(GV_ABI_VERSION == 4u, "additions only");
_Static_assert(GV_CLUSTERS_FRUSTUM_ONLY == 1u && GV_CLUSTERS_RUNS == 2u, "two flag bits");
_Static_assert(sizeof(GvClusterLod) == 48 && offsetof(GvClusterLod, self_center) == 0 && offsetof(GvClusterLod, self_radius) == 12 &&
               offsetof(GvClusterLod, parent_center) == 16 && offsetof(GvClusterLod, parent_radius) == 28 &&
               offsetof(GvClusterLod, self_error) == 32 && offsetof(GvClusterLod, parent_error) == 36 && offsetof(GvClusterLod, reserved) == 40,
               "three 16-byte pieces");
_Static_assert(sizeof(GvClusterLodView) == 32 && offsetof(GvClusterLodView, eye) == 0 && offsetof(GvClusterLodView, scale) == 16 &&
               offsetof(GvClusterLodView, near_distance) == 20 && offsetof(GvClusterLodView, reserved) == 24, "eight floats");
int (*const bind_lods)(GvCtx*, uint32_t, const GvClusterLod*, uint32_t) = gv_pool_bind_cluster_lods;
int (*const cull_lods)(GvCtx*, uint32_t, uint32_t, const GvClusterLodView*, uint32_t, const GvClusterEye*, uint32_t, uint32_t, void*, size_t) =
    gv_pool_cull_cluster_lods;
"""


def test_header_declares_the_functions_and_the_structs_as_stated(tmp_path):
    src = tmp_path / "cluster_lods_abi.c"
    src.write_text(COMPILE_CHECK)
    build = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                            str(tmp_path / "cluster_lods_abi.o")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    assert "gv_pool_bind_cluster_lods" in lib.EXPORTS and "gv_pool_cull_cluster_lods" in lib.EXPORTS
    lod, view = lib.CLUSTER_LOD_DTYPE, lib.CLUSTER_LOD_VIEW_DTYPE
    assert lod.itemsize == 48 and lod.names == ("self_center", "self_radius", "parent_center", "parent_radius", "self_error", "parent_error", "reserved")
    assert [lod.fields[n][1] for n in lod.names] == [0, 12, 16, 28, 32, 36, 40]
    assert view.itemsize == 32 and view.names == ("eye", "scale", "near_distance", "reserved")
    assert [view.fields[n][1] for n in view.names] == [0, 16, 20, 24]
    parameters = inspect.signature(lib.GpuVisibility.cull_clusters).parameters
    assert parameters["lods"].default is None and parameters["eyes"].default is None and parameters["runs"].default is False
    assert list(inspect.signature(lib.GpuVisibility.bind_cluster_lods).parameters) == ["self", "pool_id", "lods"]
    handle = lib.load()
    assert handle.gv_abi_version() == 4
    assert list(handle.gv_pool_bind_cluster_lods.argtypes) == [P, U32, P, U32]
    assert list(handle.gv_pool_cull_cluster_lods.argtypes) == [P, U32, U32, P, U32, P, U32, U32, P, SZ]


def test_a_null_context_gives_gv_e_arg():
    from garden_amd import lib
    handle = lib.load()
    assert handle.gv_pool_bind_cluster_lods(None, 0, None, 0) == lib.GV_E_ARG
    assert handle.gv_pool_cull_cluster_lods(None, 0, 0, None, 0, None, 0, 0, None, 0) == lib.GV_E_ARG
