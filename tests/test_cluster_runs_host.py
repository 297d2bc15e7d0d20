"""gv_pool_cull_cluster_runs on the host side through tests/cpp/cluster_runs_host_test.cpp: the code of every row of the two error
lists it shares with gv_pool_cull_clusters, one failing argument at a time, a refused call changing nothing, the lifetime line (ended
by a cull, a second phase, an instance emission, a rebind and a cluster cull of the other form; not by gv_pool_emit_draw_commands, a
sort of another pool or gv_hiz_build), the fetch's capacity checks and the two refusals that come from the host's bound. The CPU
build runs every host source plus gv_clusters.cpp, gv_cluster_runs.cpp and gv_clusters_second.cpp under AddressSanitizer + UBSan
against tests/cpp/hip_stub (host_build.py) as a stand-alone child process; the driver defines the launch functions of the three
cluster launch headers as no-ops itself."""
import subprocess

import host_build

OK_LINES = ("cull: every row of the error lists, a refused call changes nothing: ok",
            "pyramid: a view that names a pyramid that is not built is refused without the frustum-only flag: ok",
            "lifetimes: ended by a cull, a second phase, an instance emission, a rebind and a cluster cull of the other form; not by draw "
            "commands, another pool's sort or a pyramid build: ok",
            "fetch: an array too small gives GV_E_ARG and nothing is written: ok",
            "bounds: more than 2^32 - 1 candidates refused, a library-owned target beyond 2 GiB refused and a caller-owned one taken: ok",
            "cluster runs: ok")


def test_cluster_runs_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe, _ = host_build.build_host_program(tmp_path, "cluster_runs_host_test.cpp",
                                           host_build.ALL_HOST_SOURCES + ("gv_clusters.cpp", "gv_cluster_runs.cpp", "gv_clusters_second.cpp"),
                                           host_build.ASAN_UBSAN, "cluster_runs_host_test", defines=("-DGV_HIP_STUB=1",))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = run.stdout + run.stderr
    assert run.returncode == 0, text[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, text[-4000:]
    # every call whose code the driver pins, over its five steps
    assert "error list: 34 rows as pinned" in run.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
