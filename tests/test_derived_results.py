"""The results derived from a view's delivered records (instance data, draw bases, draw commands, LOD selection, view bounds, merged
arrays) through tests/cpp/derived_results_test.cpp: which call ends which result, the code every reader returns for a bad context,
pool, view, side column or target, every allocation of a whole sequence failing in turn, and a context that has used every buffer
being destroyed. The CPU build runs all fourteen host sources under AddressSanitizer + UBSan against tests/cpp/hip_stub
(host_build.py); the GPU build runs the same driver against libgarden_vis.so (tests/cpp/derived_results.mk)."""
import os
import subprocess

import pytest

import host_build

OK_LINES = ("lifetime matrix: 41 events x 7 results as pinned: ok",
            "empty pool: the early returns end what a cull, a second phase and a grouping end: ok",
            "reader prologues: 8 entry points x 9 cases, 64 codes as pinned: ok",
            "ownership: a context that used every buffer of every derived result was destroyed: ok",
            "derived results: ok")


def test_derived_results_under_address_and_ub_sanitizers(tmp_path):
    """Every host source of the library (host_build.ALL_HOST_SOURCES) as plain C++ against the stub runtime, with
    -fsanitize=address,undefined, driven through include/garden_vis.h: the tables of the driver hold, every reserve covers what the
    fetches copy, every allocation failing once is GV_E_OOM and the context completes the sequence afterwards, and the leak check at
    exit finds nothing a destroyed context left behind."""
    exe, launches = host_build.build_host_program(tmp_path, "derived_results_test.cpp", host_build.ALL_HOST_SOURCES, host_build.ASAN_UBSAN,
                                                  "derived_results_test", defines=("-DGV_HIP_STUB=1",))
    assert launches > 50
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = run.stdout + run.stderr
    assert run.returncode == 0, text[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, text[-4000:]
    assert "allocation failures in the derived results:" in run.stdout and "every context completed the sequence: ok" in run.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]


@pytest.mark.gpu
def test_derived_results_on_the_device():
    """The same driver against libgarden_vis.so, no sanitizer: the same tables with the real kernels behind every call"""
    exe = os.path.join(host_build.ROOT, "tests", "cpp", "build", "derived_results_test")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(host_build.ROOT, "tests", "cpp"), "-f", "derived_results.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, (run.stdout + run.stderr)[-4000:]
