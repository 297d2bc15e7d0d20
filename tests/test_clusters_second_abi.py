"""gv_pool_cull_clusters_second_phase and its two readers on the CPU tier: the header declares the three entry points with the stated
signatures (a compile check against the header itself), GV_ABI_VERSION is still 4 (the change is additive), the library exports the
symbols, garden_amd/lib.py binds the same signatures, and a NULL context gives GV_E_ARG."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t

COMPILE_CHECK = r"""
#include <stddef.h>
#include "garden_vis.h"
_Static_assert(GV_ABI_VERSION == 4u, "additions only");
int (*const second_phase)(GvCtx*, uint32_t, uint32_t, uint32_t, void*, size_t) = gv_pool_cull_clusters_second_phase;
int (*const second_device)(GvCtx*, uint32_t, const void**, const void**) = gv_pool_cluster_second_commands_device;
int (*const second_fetch)(GvCtx*, uint32_t, void*, size_t, uint32_t*, uint32_t) = gv_pool_cluster_second_commands_fetch;
"""

SIGNATURES = {
    "gv_pool_cull_clusters_second_phase": [P, U32, U32, U32, P, SZ],
    "gv_pool_cluster_second_commands_device": [P, U32, C.POINTER(P), C.POINTER(P)],
    "gv_pool_cluster_second_commands_fetch": [P, U32, P, SZ, C.POINTER(U32), U32],
}


def test_header_declares_the_three_functions_as_stated(tmp_path):
    src = tmp_path / "clusters_second_abi.c"
    src.write_text(COMPILE_CHECK)
    build = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                            str(tmp_path / "clusters_second_abi.o")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    for name in SIGNATURES:
        assert name in lib.EXPORTS, name
    for method in ("cull_clusters_second_phase", "cluster_second_commands_device", "cluster_second_commands"):
        assert callable(getattr(lib.GpuVisibility, method)), method
    handle = lib.load()
    assert handle.gv_abi_version() == 4
    for name, argtypes in SIGNATURES.items():
        assert list(getattr(handle, name).argtypes) == argtypes, name


def test_a_null_context_gives_gv_e_arg():
    from garden_amd import lib
    handle = lib.load()
    a, b = C.c_void_p(), C.c_void_p()
    counts = (C.c_uint32 * 16)()
    assert handle.gv_pool_cull_clusters_second_phase(None, 0, 0, 0, None, 0) == lib.GV_E_ARG
    assert handle.gv_pool_cluster_second_commands_device(None, 0, C.byref(a), C.byref(b)) == lib.GV_E_ARG
    assert handle.gv_pool_cluster_second_commands_fetch(None, 0, None, 0, counts, 16) == lib.GV_E_ARG
