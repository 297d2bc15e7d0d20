"""The receiver-mask calls on the host side through tests/cpp/receivers_host_test.cpp and the shim through tests/cpp/receivers.cpp: the code of every row of the header's error
lists, a refused call changing nothing, the two-image rule restated for the receiver pair (a begin never hands out the image the
current pyramid reads, before and after the pyramid moves, with an occluder image open alongside), and every allocation of a frame
failing in turn. The CPU build runs every host source plus gv_occluders.cpp and gv_receivers.cpp under AddressSanitizer + UBSan against
tests/cpp/hip_stub (host_build.py) as a stand-alone child process; the GPU build runs the same driver against libgarden_vis.so
(tests/cpp/receivers_host.mk)."""
import json
import os
import subprocess

import pytest

import host_build

OK_LINES = ("a refused call changes nothing: ok",
            "kept away from the pyramid's image, before and after it moved, an occluder image open alongside: ok",
            "receivers: ok")


def test_receivers_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe, _ = host_build.build_host_program(tmp_path, "receivers_host_test.cpp",
                                           host_build.ALL_HOST_SOURCES + ("gv_occluders.cpp", "gv_receivers.cpp"),
                                           host_build.ASAN_UBSAN, "receivers_host_test", defines=("-DGV_HIP_STUB=1",))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = run.stdout + run.stderr
    assert run.returncode == 0, text[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, text[-4000:]
    assert "error list: 39 rows as pinned" in run.stdout, text[-4000:]
    assert "allocation failures in the receiver frame:" in run.stdout and "every context completed the sequence: ok" in run.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]


@pytest.mark.gpu
def test_receivers_host_driver_on_the_device():
    """The same driver against libgarden_vis.so, no sanitizer: the same codes and images with the real kernels behind every call,
    every record of two draws counted in exactly one class"""
    exe = os.path.join(host_build.ROOT, "tests", "cpp", "build", "receivers_host_test")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(host_build.ROOT, "tests", "cpp"), "-f", "receivers_host.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, (run.stdout + run.stderr)[-4000:]


@pytest.mark.gpu
def test_masked_cascades_through_the_shim():
    """tests/cpp/receivers.cpp: GpuShadowReceivers over five headless ticks with the main pass and three cascades; every cascade's
    list against the host path's cull fed the fetched mask, record for record; casters were dropped"""
    exe = os.path.join(host_build.ROOT, "tests", "cpp", "build", "receivers")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(host_build.ROOT, "tests", "cpp"), "-f", "receivers.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "receivers ok" in run.stdout, (run.stdout + run.stderr)[-4000:]
    result = json.loads(run.stdout.splitlines()[0])
    assert result["ok"] and result["ticks"] == 5 and result["cascades"] == 3
    assert result["dropped"] > 0 and result["kept_masked"] > 0 and result["kept_frustum_only"] == result["kept_masked"] + result["dropped"]
    assert result["receivers_drawn"] > 0 and result["kept_because_the_main_pass_sees_them"] > 0 and result["texels_without_receiver"] > 0


def test_the_shim_header_compiles_against_csm_lite(tmp_path):
    """host/shadow_receivers.hpp is header-only: GpuShadowReceivers with begin, draw (a viewProj or a csm::Cascade), build, counts and
    the cascade's view for the masked cull, compiled with the warnings of the shim's drivers"""
    src = tmp_path / "shadow_receivers_tu.cpp"
    src.write_text('#include "shadow_receivers.hpp"\n'
                   "using R = garden::GpuShadowReceivers;\n"
                   "void (R::*const begin)(uint32_t, uint32_t) = &R::begin;\n"
                   "void (R::*const draw)(uint32_t, uint32_t, const garden::csm::Cascade&) = &R::draw;\n"
                   "void (R::*const build)() = &R::build;\n"
                   "const GvReceiverCounts& (R::*const counts)() = &R::counts;\n"
                   "void (R::*const cull)(uint32_t, int8_t) = &R::cull;\n"
                   "bool (R::*const supported)() const noexcept = &R::isSupported;\n"
                   "GvView view(const garden::csm::Cascade& c) { return R::cascadeView(c, garden::f32x4(1, 2, 3), 0); }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-invalid-offsetof", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                    "-I", "/opt/rocm/include", "-I", os.path.join(host_build.ROOT, "garden_amd", "csrc", "host"), str(src)], check=True)
