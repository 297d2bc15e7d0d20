"""gv_pool_cull_clusters_second_phase and its readers on the host side through tests/cpp/clusters_second_host_test.cpp: the code of
every row of the header's two error lists, one failing argument at a time, a refused call changing nothing of either cluster result,
the refusal after a geometry or layout call since the cluster cull (whose message says to cull the clusters again), the lifetime line
(ended wherever the cluster cull ends and by a new one; not by gv_pool_emit_draw_commands, a sort of another pool or gv_hiz_build),
the fetch's capacity checks and the cluster cull's result still fetchable afterwards. The CPU build runs every host source plus
gv_clusters.cpp and gv_clusters_second.cpp under AddressSanitizer + UBSan against tests/cpp/hip_stub (host_build.py) as a
stand-alone child process; the driver defines the launch functions of the two cluster launch headers as no-ops itself."""
import subprocess

import host_build

OK_LINES = ("errors: every row of the two lists, a refused call changes nothing: ok",
            "rebinds: refused after a geometry or layout call since the cluster cull, lifted by a new one: ok",
            "lifetimes: ended wherever the cluster cull ends and by a new one; not by draw commands, another pool's sort or a pyramid build: ok",
            "fetch: an array too small gives GV_E_ARG and nothing is written; the cluster cull's result is still fetchable: ok",
            "bounds: a library-owned target beyond 2 GiB refused, a caller-owned one and regions taken: ok",
            "clusters second: ok")


def test_clusters_second_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe, _ = host_build.build_host_program(tmp_path, "clusters_second_host_test.cpp",
                                           host_build.ALL_HOST_SOURCES + ("gv_clusters.cpp", "gv_clusters_second.cpp"),
                                           host_build.ASAN_UBSAN, "clusters_second_host_test", defines=("-DGV_HIP_STUB=1",))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = run.stdout + run.stderr
    assert run.returncode == 0, text[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, text[-4000:]
    # every call whose code the driver pins, over its five steps
    assert "error list: 36 rows as pinned" in run.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
