"""GpuClusterCommands::setClusterLods / setLodViews / lodScale (garden_amd/csrc/host/cluster_commands.hpp) on the device, through
tests/cpp/cluster_lods.cpp: five ticks of the shim with a moving camera, a main pass and one cascade that names the camera's eye with
half its scale, runs on odd ticks, cones and eyes from tick 3 on; every command of both passes equals a host path that fetches the
records, calls the oracle and applies the twins of the LOD rule and the cone rule."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_cluster_lods_shim_five_ticks_against_the_twin():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "build", "cluster_lods")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "tests", "cpp"), "-f", "cluster_lods.mk"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    result = json.loads(run.stdout.splitlines()[-1])
    print(result)
    assert result["ok"] and result["ticks"] == 5 and result["passes"] == 2
    assert result["tested"] > 2 * result["lod_kept"] and result["lod_kept"] > result["survivors"] > 0  # a cut, and the unchanged test had work on it
    assert result["main_kept"] > result["cascade_kept"] > 0  # half the scale: a coarser cut for the cascade
    assert result["cone_rejected"] > 0                       # the ticks with eyes rejected clusters of the cut
