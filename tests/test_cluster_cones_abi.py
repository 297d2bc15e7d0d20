"""gv_pool_bind_cluster_cones / gv_pool_cull_cluster_cones on the CPU tier. The header declares both entry points, GvClusterCone (32
bytes, meshopt_Bounds' cone fields in place), GvClusterEye and GV_CLUSTERS_RUNS == 2 with the stated signatures (a compile check
against the header itself); GV_ABI_VERSION is still 4 (the change is additive); the library exports the symbols; garden_amd/lib.py
binds the same signatures, has CLUSTER_CONE_DTYPE, GpuVisibility.bind_cluster_cones and the `eyes` keyword of cull_clusters, default
None; a NULL context gives GV_E_ARG. And the host side through tests/cpp/cluster_cones_host_test.cpp: every row of both error lists,
refused calls changing nothing, the cones dropped by gv_pool_bind_clusters, the lifetime line, the launch counts and the upload
bytes — the CPU build runs every host source plus the four cluster sources under AddressSanitizer + UBSan against tests/cpp/hip_stub
(host_build.py) as a stand-alone child process; the driver defines the launch functions of the cluster launch headers as no-ops
itself."""
import ctypes as C
import inspect
import os
import re
import subprocess

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t

COMPILE_CHECK = r"""
#include <stddef.h>
#include "garden_vis.h"
_Static_assert(GV_ABI_VERSION == 4u, "additions only");
_Static_assert(GV_CLUSTERS_FRUSTUM_ONLY == 1u && GV_CLUSTERS_RUNS == 2u, "two flag bits");
_Static_assert(sizeof(GvClusterCone) == 32 && offsetof(GvClusterCone, apex) == 0 && offsetof(GvClusterCone, cutoff) == 12 &&
               offsetof(GvClusterCone, axis) == 16 && offsetof(GvClusterCone, reserved) == 28, "two 16-byte pieces");
_Static_assert(sizeof(GvClusterEye) == 16 && offsetof(GvClusterEye, eye) == 0, "four floats");
int (*const bind_cones)(GvCtx*, uint32_t, const GvClusterCone*, uint32_t) = gv_pool_bind_cluster_cones;
int (*const cull_cones)(GvCtx*, uint32_t, uint32_t, const GvClusterEye*, uint32_t, uint32_t, void*, size_t) = gv_pool_cull_cluster_cones;
"""

OK_LINES = ("bind: every row of the error list, the bytes are counted, a refused bind changes nothing, a bind ends the result: ok",
            "cull: every row of the error lists with and without runs, a refused call changes nothing: ok",
            "pyramid: a view that names a pyramid that is not built is refused without the frustum-only flag: ok",
            "dropped: gv_pool_bind_clusters, a new table or removal, drops the cones: ok",
            "lifetimes: the pool's one cluster result, ended where it ends and by a cone bind, replaced by any form; five and six launches; "
            "the second phase carries the kept eyes: ok",
            "cluster cones: ok")


def test_header_declares_the_functions_and_the_structs_as_stated(tmp_path):
    src = tmp_path / "cluster_cones_abi.c"
    src.write_text(COMPILE_CHECK)
    build = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                            str(tmp_path / "cluster_cones_abi.o")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    assert "gv_pool_bind_cluster_cones" in lib.EXPORTS and "gv_pool_cull_cluster_cones" in lib.EXPORTS
    assert lib.GV_CLUSTERS_RUNS == 2
    assert lib.CLUSTER_CONE_DTYPE.itemsize == 32 and lib.CLUSTER_CONE_DTYPE.names == ("apex", "cutoff", "axis", "reserved")
    assert [lib.CLUSTER_CONE_DTYPE.fields[n][1] for n in lib.CLUSTER_CONE_DTYPE.names] == [0, 12, 16, 28]
    parameters = inspect.signature(lib.GpuVisibility.cull_clusters).parameters
    assert parameters["eyes"].default is None and parameters["runs"].default is False
    assert list(inspect.signature(lib.GpuVisibility.bind_cluster_cones).parameters) == ["self", "pool_id", "cones"]
    handle = lib.load()
    assert handle.gv_abi_version() == 4
    assert list(handle.gv_pool_bind_cluster_cones.argtypes) == [P, U32, P, U32]
    assert list(handle.gv_pool_cull_cluster_cones.argtypes) == [P, U32, U32, P, U32, U32, P, SZ]


def test_a_null_context_gives_gv_e_arg():
    from garden_amd import lib
    handle = lib.load()
    assert handle.gv_pool_bind_cluster_cones(None, 0, None, 0) == lib.GV_E_ARG
    assert handle.gv_pool_cull_cluster_cones(None, 0, 0, None, 0, 0, None, 0) == lib.GV_E_ARG


def test_cluster_cones_host_side_under_address_and_ub_sanitizers(tmp_path):
    sources = host_build.ALL_HOST_SOURCES + ("gv_clusters.cpp", "gv_cluster_runs.cpp", "gv_clusters_second.cpp", "gv_cluster_cones.cpp")
    exe, _ = host_build.build_host_program(tmp_path, "cluster_cones_host_test.cpp", sources, host_build.ASAN_UBSAN, "cluster_cones_host_test",
                                           defines=("-DGV_HIP_STUB=1",))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = run.stdout + run.stderr
    assert run.returncode == 0, text[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, text[-4000:]
    # every call whose code the driver pins, over its five steps
    assert "error list: 62 rows as pinned" in run.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
