"""csrc/conv_plan.h -- the host-side planning of vl_nnconv -- needs neither HIP nor a GPU: tests/conv_plan_check.cpp
includes nothing else, sweeps the dgrad class / tap-table planning against the definition of the convolution over a grid
of small geometries and runs the "can this kernel run it" predicates on the layers of the shipped networks."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_conv_plan_against_its_definition(tmp_path):
    exe = str(tmp_path / "conv_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "conv_plan_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    assert int(r.stdout.split()[0]) > 500000      # the whole grid ran

