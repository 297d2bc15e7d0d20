"""The occluder calls on the host side through tests/cpp/occluders_host_test.cpp: the code of every row of the header's error lists, a
refused call changing nothing, the two-image rule (a begin never hands out the image the current pyramid reads, whatever the sizes),
the box mirror's dirty bookkeeping through GvStats::upload_bytes, and every allocation of a frame failing in turn. The CPU build runs
every host source plus gv_occluders.cpp under AddressSanitizer + UBSan against tests/cpp/hip_stub (host_build.py) as a stand-alone
child process; the GPU build runs the same driver against libgarden_vis.so (tests/cpp/occluders_host.mk)."""
import json
import os
import subprocess

import pytest

import host_build

OK_LINES = ("a refused call changes nothing: ok",
            "kept away from the pyramid's image, before and after it moved: ok",
            "mirror marks: first draw, marks, overlaps, clamping, gv_sync, mesh marks, rebind and removal as pinned: ok",
            "occluders: ok")


def test_occluders_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe, _ = host_build.build_host_program(tmp_path, "occluders_host_test.cpp", host_build.ALL_HOST_SOURCES + ("gv_occluders.cpp",),
                                           host_build.ASAN_UBSAN, "occluders_host_test", defines=("-DGV_HIP_STUB=1",))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = run.stdout + run.stderr
    assert run.returncode == 0, text[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, text[-4000:]
    assert "error list: 49 rows as pinned" in run.stdout, text[-4000:]
    assert "allocation failures in the occluder frame:" in run.stdout and "every context completed the sequence: ok" in run.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]


@pytest.mark.gpu
def test_occluders_host_driver_on_the_device():
    """The same driver against libgarden_vis.so, no sanitizer: the same codes, images and upload bytes with the real kernels behind
    every call"""
    exe = os.path.join(host_build.ROOT, "tests", "cpp", "build", "occluders_host_test")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(host_build.ROOT, "tests", "cpp"), "-f", "occluders_host.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, (run.stdout + run.stderr)[-4000:]


@pytest.mark.gpu
def test_headless_frames_through_the_shim():
    """tests/cpp/occluders.cpp: GpuOccluders + GpuSecondPhase over five headless ticks against the host path fed the fetched image"""
    exe = os.path.join(host_build.ROOT, "tests", "cpp", "build", "occluders")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(host_build.ROOT, "tests", "cpp"), "-f", "occluders.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "occluders ok" in run.stdout, (run.stdout + run.stderr)[-4000:]
    result = json.loads(run.stdout.splitlines()[0])
    assert result["ok"] and result["occluders_drawn"] > 0 and result["culled_by_the_pyramid"] > 0 and result["new"] > 0
