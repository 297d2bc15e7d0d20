"""gv_pool_emit_draw_instances and its companions on the CPU tier: the header declares the four entry points with the signatures
garden_amd/lib.py binds, the library exports them, GV_MAX_DRAW_INSTANCES is there, and the ABI version is still 4 (the change is
additive)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t
# name -> (the parameter list of the header, whitespace squeezed; the argtypes lib.py must bind)
SIGNATURES = {
    "gv_pool_emit_draw_instances": (
        "GvCtx* ctx, uint32_t pool_id, const uint32_t* view_indices, uint32_t view_count, void* dst_device, size_t capacity_bytes",
        [P, U32, C.POINTER(U32), U32, P, SZ]),
    "gv_pool_set_instance_index_field": ("GvCtx* ctx, uint32_t pool_id, uint32_t offset", [P, U32, U32]),
    "gv_pool_draw_bases_device": ("GvCtx* ctx, uint32_t pool_id, const void** first_instance, const void** draw_starts",
                                  [P, U32, C.POINTER(P), C.POINTER(P)]),
    "gv_pool_draw_bases_fetch": (
        "GvCtx* ctx, uint32_t pool_id, uint32_t* first_instance, uint32_t capacity, uint32_t* draw_starts, uint32_t starts_capacity",
        [P, U32, C.POINTER(U32), U32, C.POINTER(U32), U32]),
}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)


def test_header_declares_the_entry_points_with_these_signatures():
    text = header()
    for name, (params, _) in SIGNATURES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert " ".join(m.group(1).split()) == params, name
    assert re.search(r"#define GV_MAX_DRAW_INSTANCES 65535u?\b", text)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    for name in SIGNATURES:
        assert name in lib.EXPORTS, name
    assert lib.GV_MAX_DRAW_INSTANCES == 65535
    for method in ("emit_draw_instances", "set_instance_index_field", "draw_bases_device", "draw_bases"):
        assert callable(getattr(lib.GpuVisibility, method)), method
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        assert handle.gv_abi_version() == 4
        for name, (_, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)
            assert list(fn.argtypes) == argtypes, name
            assert fn.restype in (C.c_int, C.c_int32), name


def test_header_compiles_as_c99_with_the_new_declarations(tmp_path):
    import subprocess
    src = tmp_path / "draw_abi.c"
    src.write_text('#include <stdio.h>\n#include "garden_vis.h"\n'
                   "int main(void) {\n"
                   "    int (*emit)(GvCtx*, uint32_t, const uint32_t*, uint32_t, void*, size_t) = gv_pool_emit_draw_instances;\n"
                   "    int (*field)(GvCtx*, uint32_t, uint32_t) = gv_pool_set_instance_index_field;\n"
                   "    int (*dev)(GvCtx*, uint32_t, const void**, const void**) = gv_pool_draw_bases_device;\n"
                   "    int (*fetch)(GvCtx*, uint32_t, uint32_t*, uint32_t, uint32_t*, uint32_t) = gv_pool_draw_bases_fetch;\n"
                   '    printf("%u %d\\n", (unsigned)GV_MAX_DRAW_INSTANCES, emit && field && dev && fetch);\n'
                   "    return 0;\n}\n")
    obj = tmp_path / "draw_abi.o"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(obj)], check=True)
