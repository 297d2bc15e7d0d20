"""The pyramid slots on the host side through tests/cpp/pyramid_slots_host_test.cpp: the code of every row of the header's error
lists for gv_hiz_select / gv_hiz_drop and of the "pyramid not built" rows of gv_cull and gv_pool_cull_second_phase, a refused call
changing nothing, select / build / drop lifetimes, the image-taking rule (one pyramid: the two images of old in the turn of old;
several: never an image a built pyramid reads, the lowest free one otherwise) and every allocation of a frame with three pyramids
failing in turn. The CPU build runs every host source plus gv_occluders.cpp and gv_receivers.cpp under AddressSanitizer + UBSan
against tests/cpp/hip_stub (host_build.py) as a stand-alone child process — leaks included: every slot's buffers are the context's to
free —; the GPU build runs the same driver against libgarden_vis.so (tests/cpp/pyramid_slots_host.mk)."""
import os
import subprocess

import pytest

import host_build

OK_LINES = ("a refused call changes nothing: ok",
            "lifetimes: builds land in the selected slot, drops leave the others, views name their pyramids: ok",
            "every image a pyramid reads untouched; a drop frees the reference alone: ok",
            "pyramid slots: ok")


def test_pyramid_slots_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe, _ = host_build.build_host_program(tmp_path, "pyramid_slots_host_test.cpp",
                                           host_build.ALL_HOST_SOURCES + ("gv_occluders.cpp", "gv_receivers.cpp"),
                                           host_build.ASAN_UBSAN, "pyramid_slots_host_test", defines=("-DGV_HIP_STUB=1",))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = run.stdout + run.stderr
    assert run.returncode == 0, text[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, text[-4000:]
    assert "error list: 11 rows as pinned" in run.stdout, text[-4000:]
    assert "allocation failures in the frame of three pyramids:" in run.stdout and "every context completed the sequence: ok" in run.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]


@pytest.mark.gpu
def test_pyramid_slots_host_driver_on_the_device():
    """The same driver against libgarden_vis.so, no sanitizer: the same codes, lifetimes and images with the real kernels behind
    every call"""
    exe = os.path.join(host_build.ROOT, "tests", "cpp", "build", "pyramid_slots_host_test")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(host_build.ROOT, "tests", "cpp"), "-f", "pyramid_slots_host.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, (run.stdout + run.stderr)[-4000:]
