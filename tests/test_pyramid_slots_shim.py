"""The pyramid slots through the shim (host/shadow_receivers.hpp): tests/cpp/receivers_batched.cpp runs headless ticks with the main
pass and three cascades — three masks into three slots, ONE cull of all four views, the second phase of the main pass afterwards
against the untouched slot 0 — and holds every list to the one-at-a-time order; the header's new members compile with the warnings
of the shim's drivers."""
import json
import os
import subprocess

import pytest

import host_build


@pytest.mark.gpu
def test_batched_masked_cascades_through_the_shim():
    """five ticks, a moving camera and movers, a main pass that queries its depth pyramid (slot 0): cullCascades gives record for
    record the lists of GpuShadowReceivers::cull, the main pass's depth pyramid reads back the same before and after the masks,
    GpuSecondPhase after the cascades delivers the host path's R(B) minus S1 — and there are such records"""
    exe = os.path.join(host_build.ROOT, "tests", "cpp", "build", "receivers_batched")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(host_build.ROOT, "tests", "cpp"), "-f", "receivers_batched.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "receivers_batched ok" in run.stdout, (run.stdout + run.stderr)[-4000:]
    result = json.loads(run.stdout.splitlines()[0])
    assert result["ok"] and result["ticks"] == 5 and result["cascades"] == 3
    assert result["dropped"] > 0 and result["kept_masked"] > 0 and result["second_phase_new"] > 0 and result["occluded_in_first_phase"] > 0
    assert result["culls_issued"] == {"batched": 1, "one_at_a_time": 3}
    assert result["cull_launches"] == {"batched": 5, "one_at_a_time": 5 * 3 * 4}


def test_the_shim_headers_new_members_compile_against_csm_lite(tmp_path):
    """begin with a slot, the cascade's view against a slot, cullCascades and its lists, beside the members the one-at-a-time order
    keeps (tests/test_receivers_host.py pins those)"""
    src = tmp_path / "shadow_receivers_slots_tu.cpp"
    src.write_text('#include "shadow_receivers.hpp"\n'
                   "using R = garden::GpuShadowReceivers;\n"
                   "void (R::*const begin)(uint32_t, uint32_t) = &R::begin;\n"
                   "void (R::*const beginSlot)(uint32_t, uint32_t, uint32_t) = &R::begin;\n"
                   "void (R::*const build)() = &R::build;\n"
                   "void (R::*const cull)(uint32_t, int8_t) = &R::cull;\n"
                   "void (R::*const cullCascades)(uint32_t, const std::vector<int8_t>&, const std::vector<uint32_t>&) = &R::cullCascades;\n"
                   "const garden::UnsortedMesh* (R::*const meshes)(size_t) const = &R::meshes;\n"
                   "uint32_t (R::*const drawCount)(size_t) const = &R::drawCount;\n"
                   "const garden::UnsortedMesh* (R::*const meshesOne)() const noexcept = &R::meshes;\n"
                   "GvView view(const garden::csm::Cascade& c) { return R::cascadeView(c, garden::f32x4(1, 2, 3), 0, true, 2); }\n"
                   "static_assert(GV_MAX_PYRAMIDS == GV_MAX_VIEWS, \"one pyramid per view\");\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-invalid-offsetof", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                    "-I", "/opt/rocm/include", "-I", os.path.join(host_build.ROOT, "garden_amd", "csrc", "host"), str(src)], check=True)
