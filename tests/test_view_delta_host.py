"""gv_pool_view_delta on the host side through tests/cpp/view_delta_host_test.cpp: the code of every row of the header's error list,
a refused call changing nothing, the baseline and the answer surviving culls, a second phase, an emission, a sort and re-binds,
channels that do not disturb each other, the drop call, every allocation of a call sequence failing in turn, a context that used
every channel of two pools being destroyed, and the write-back loop on hand-made lists. The CPU build runs every host source plus
gv_delta.cpp under AddressSanitizer + UBSan against tests/cpp/hip_stub (host_build.py) as a stand-alone child process; the GPU build
runs the same driver against libgarden_vis.so (tests/cpp/view_delta_host.mk)."""
import os
import subprocess

import pytest

import host_build

OK_LINES = ("a refused call changes nothing: ok",
            "lifetimes: baseline and answer survived 6 events, a narrowed view, a restart and both re-binds: ok",
            "channels: independent of each other and of other pools, drop and empty pool: ok",
            "ownership: a context that used every channel of two pools was destroyed: ok",
            "view delta: ok")


def test_view_delta_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe, _ = host_build.build_host_program(tmp_path, "view_delta_host_test.cpp", host_build.ALL_HOST_SOURCES + ("gv_delta.cpp",),
                                           host_build.ASAN_UBSAN, "view_delta_host_test", defines=("-DGV_HIP_STUB=1",))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = run.stdout + run.stderr
    assert run.returncode == 0, text[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, text[-4000:]
    assert "error list: 34 rows as pinned" in run.stdout, text[-4000:]
    assert "allocation failures in the view delta:" in run.stdout and "every context completed the sequence: ok" in run.stdout, text[-4000:]
    assert "write-back: plain column, mapped target with holes, slots beyond the occupancy and unlisted bytes as pinned: ok" in run.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]


@pytest.mark.gpu
def test_view_delta_host_driver_on_the_device():
    """The same driver against libgarden_vis.so, no sanitizer: the same codes and lifetimes with the real kernels behind every call,
    and the invariants of every answer (ascending, disjoint, |C| + vanished - appeared = the baseline's |C|)"""
    exe = os.path.join(host_build.ROOT, "tests", "cpp", "build", "view_delta_host_test")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(host_build.ROOT, "tests", "cpp"), "-f", "view_delta_host.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, (run.stdout + run.stderr)[-4000:]
