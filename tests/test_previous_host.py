"""gv_pool_keep_models / gv_pool_forget_models / gv_pool_emit_previous and their readers on the host side through
tests/cpp/previous_host_test.cpp: the code of every row of the header's error lists, one failing argument at a time, a refused call
changing neither the history nor the result, GV_KEEP_ADD's state, the result ending at the next cull and second phase while the
history survives them, emissions, sorts and re-binds, and the fetch's capacity check and field-by-field copy. The CPU build runs every
host source plus gv_previous.cpp under AddressSanitizer + UBSan against tests/cpp/hip_stub (host_build.py) as a stand-alone child
process; the driver defines the launch functions of gv_previous_kernels.hpp as no-ops itself."""
import subprocess

import host_build

OK_LINES = ("a refused call changes neither history nor result: ok",
            "keep add: refused into an empty history and for another matrix or camera, bit for bit: ok",
            "lifetimes: the result ended at a cull and at a second phase, the history at nothing but forget: ok",
            "fetch: a capacity too small writes nothing, fields copied and the bytes between them left: ok",
            "previous: ok")


def test_previous_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe, _ = host_build.build_host_program(tmp_path, "previous_host_test.cpp", host_build.ALL_HOST_SOURCES + ("gv_previous.cpp",),
                                           host_build.ASAN_UBSAN, "previous_host_test", defines=("-DGV_HIP_STUB=1",))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = run.stdout + run.stderr
    assert run.returncode == 0, text[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, text[-4000:]
    # 5 NULL contexts, 2 views of a pool never culled, 1 fetch without a result, the 29 refused calls on an empty and on a full state, 2 ended views
    assert "error list: 68 rows as pinned" in run.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
