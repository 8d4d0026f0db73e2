"""csrc/norm_pool_plan.h -- the host-side planning of vl_nnbnorm, vl_nnpool and their fusion -- needs neither HIP nor a GPU:
tests/norm_pool_plan_check.cpp includes nothing else.  It asserts, as literals, the derived quantities that
tests/test_gpu_norm_pool_edges.py and tests/pool_routing.py state beside their shapes (which kernel and which branch a case
reaches), and the invariants of every plan over a sweep of small geometries."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_norm_pool_plan_figures_and_invariants(tmp_path):
    exe = str(tmp_path / "norm_pool_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "norm_pool_plan_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    assert int(r.stdout.split()[0]) > 35000000      # the whole sweep ran
