"""The CPU build of libgarden_vis's host side, shared by the tests that run it under a sanitizer: the host sources as plain C++
against tests/cpp/hip_stub (device memory = zeroed host memory, copies = memcpy, kernels = generated no-ops; the mirror re-order
and the exchange's kernels as plain loops), one stand-alone driver with a main() of its own, linked into a program that is run as
a child process. TEST-ONLY: the product library is built by garden_amd/csrc/Makefile and refuses to run without a gfx950 device."""
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "garden_amd", "csrc")
STUB = os.path.join(ROOT, "tests", "cpp", "hip_stub")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"  # (g++ 11 has no _Float16, which gv_context.cpp's RG16F read-back uses)

# what host_orchestration_test.cpp drives
ORCHESTRATION_SOURCES = ("gv_context.cpp", "gv_results.cpp", "gv_mirror.cpp", "gv_exchange.cpp", "gv_scene.cpp", "gv_workers.cpp")
# ... and the files behind the derived results and the pick: every host source of the library
ALL_HOST_SOURCES = ORCHESTRATION_SOURCES + ("gv_pick.cpp", "gv_instance.cpp", "gv_merge.cpp", "gv_commands.cpp", "gv_lod.cpp", "gv_group.cpp",
                                            "gv_second.cpp", "gv_bounds.cpp")
# (-fno-sanitize=function: RCCL's entry points are called through dlsym'ed pointers whose parameter structs are declared on
# each side of the C boundary — same layout, different C++ types)
ASAN_UBSAN = ("-fsanitize=address,undefined", "-fno-sanitize=function", "-fno-sanitize-recover=undefined")


def kernel_stubs(tmp_path, csrc=CSRC):
    """kernel_stubs.cpp, generated from the launch headers of `csrc`: its path and how many launch functions it defines"""
    gen = subprocess.run([sys.executable, os.path.join(STUB, "make_kernel_stubs.py"), csrc], capture_output=True, text=True)
    assert gen.returncode == 0, gen.stderr
    path = tmp_path / "kernel_stubs.cpp"
    path.write_text(gen.stdout)
    return str(path), gen.stdout.count("hipError_t launch_")


def flags_for(sanitize, csrc=CSRC):
    return ["-std=c++17", "-O1", "-g", *sanitize, "-I" + STUB, "-I" + csrc]


def build_host_program(tmp_path, driver, host_sources, sanitize, exe_name, csrc=CSRC, defines=()):
    """Compiles `driver` (a file of tests/cpp), the generated kernel stubs, the stub build's two CPU kernels and `host_sources` of
    `csrc` side by side with `sanitize` (whose first entry is the -fsanitize= flag the link needs too) and links them; returns the
    program's path and the number of launch functions that were stubbed."""
    stubs, launches = kernel_stubs(tmp_path, csrc)
    flags = flags_for(sanitize, csrc) + list(defines)
    sources = [stubs, os.path.join(STUB, "reorder_cpu.cpp"), os.path.join(STUB, "exchange_cpu.cpp"), os.path.join(ROOT, "tests", "cpp", driver)] + \
              [os.path.join(csrc, f) for f in host_sources]
    objects, builds = [], []
    for src in sources:  # compiled side by side
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        objects.append(obj)
        builds.append(subprocess.Popen([CLANG, *flags, "-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for b in builds:
        out, _ = b.communicate(timeout=900)
        assert b.returncode == 0, out[-3000:]
    exe = str(tmp_path / exe_name)
    link = subprocess.run([CLANG, sanitize[0], *objects, "-o", exe, "-lpthread", "-ldl"], capture_output=True, text=True)
    assert link.returncode == 0, link.stderr[-3000:]
    return exe, launches


def build_stub_transport(tmp_path, sanitize, name):
    """RCCL's entry points over shared memory (tests/cpp/rccl_stub), built against the same stub runtime and sanitizers; named to the
    library with GV_RCCL_LIBRARY"""
    transport = str(tmp_path / name)
    tb = subprocess.run([CLANG, *flags_for(sanitize), "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "rccl_stub", "rccl_stub.cpp"), "-o", transport,
                         "-lrt", "-lpthread"], capture_output=True, text=True)
    assert tb.returncode == 0, tb.stderr[-3000:]
    return transport
