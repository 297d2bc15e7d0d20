"""gv_pool_cull_cluster_runs on the CPU tier: the header declares the entry point with the stated signature and
GV_CLUSTER_RUN_SPAN == 256 (a compile check against the header itself), GV_ABI_VERSION is still 4 (the change is additive), the
library exports the symbol, garden_amd/lib.py binds the same signature and GpuVisibility.cull_clusters has the `runs` keyword,
default off, and a NULL context gives GV_E_ARG."""
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
_Static_assert(GV_CLUSTER_RUN_SPAN == 256u, "the span the rule states");
int (*const cluster_runs)(GvCtx*, uint32_t, uint32_t, uint32_t, void*, size_t) = gv_pool_cull_cluster_runs;
int (*const clusters)(GvCtx*, uint32_t, uint32_t, uint32_t, void*, size_t) = gv_pool_cull_clusters;
"""


def test_header_declares_the_function_and_the_span_as_stated(tmp_path):
    src = tmp_path / "cluster_runs_abi.c"
    src.write_text(COMPILE_CHECK)
    build = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                            str(tmp_path / "cluster_runs_abi.o")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_library_exports_it_and_lib_py_binds_the_same_signature():
    from garden_amd import lib
    assert "gv_pool_cull_cluster_runs" in lib.EXPORTS
    assert lib.GV_CLUSTER_RUN_SPAN == 256
    runs = inspect.signature(lib.GpuVisibility.cull_clusters).parameters["runs"]
    assert runs.default is False
    handle = lib.load()
    assert handle.gv_abi_version() == 4
    assert list(handle.gv_pool_cull_cluster_runs.argtypes) == [P, U32, U32, U32, P, SZ]


def test_a_null_context_gives_gv_e_arg():
    from garden_amd import lib
    handle = lib.load()
    assert handle.gv_pool_cull_cluster_runs(None, 0, 0, 0, None, 0) == lib.GV_E_ARG
