"""The host side of gv_pool_bind_cluster_lods / gv_pool_cull_cluster_lods through tests/cpp/cluster_lods_host_test.cpp: every row of
both error lists under every flag combination, without and with eyes; the older forms refusing what they refuse; refused calls
changing nothing; the LOD table dropped by gv_pool_bind_clusters; the lifetime line, the launch counts and the upload bytes; the
kept views (and eyes) reaching the second phase's launch. The CPU build runs every host source plus the five cluster sources under
AddressSanitizer + UBSan against tests/cpp/hip_stub (host_build.py) as a stand-alone child process; the driver defines the launch
functions of the cluster launch headers as no-ops itself. Nothing is loaded into Python under a sanitizer."""
import subprocess

import host_build

OK_LINES = ("bind: every row of the error list, the bytes are counted, a refused bind changes nothing, a bind ends the result: ok",
            "cull: every row of the error lists under every flag combination, a refused call changes nothing: ok",
            "pyramid: a view that names a pyramid that is not built is refused without the frustum-only flag: ok",
            "dropped: gv_pool_bind_clusters, a new table or removal, drops the LOD table: ok",
            "lifetimes: the pool's one cluster result, ended where it ends and by a LOD bind, replaced by any form; five and six launches; "
            "the second phase carries the kept views and eyes: ok",
            "cluster lods: ok")


def test_cluster_lods_host_side_under_address_and_ub_sanitizers(tmp_path):
    sources = host_build.ALL_HOST_SOURCES + ("gv_clusters.cpp", "gv_cluster_runs.cpp", "gv_clusters_second.cpp", "gv_cluster_cones.cpp",
                                             "gv_cluster_lods.cpp")
    exe, _ = host_build.build_host_program(tmp_path, "cluster_lods_host_test.cpp", sources, host_build.ASAN_UBSAN, "cluster_lods_host_test",
                                           defines=("-DGV_HIP_STUB=1",))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    text = run.stdout + run.stderr
    assert run.returncode == 0, text[-4000:]
    for line in OK_LINES:
        assert line in run.stdout, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
