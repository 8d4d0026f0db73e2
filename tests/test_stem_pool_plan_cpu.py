"""csrc/stem_pool_plan.h -- the work decomposition of the three fused stem kernels and the addresses of the backward kernel's
pooled loads -- needs neither HIP nor a GPU: tests/stem_pool_plan_check.cpp includes the plan headers and nothing else.  It
asserts, as literals, the figures that tests/test_gpu_stem_pool_edges.py states beside its shapes, and over every admitted
geometry of a sweep that every unit is walked exactly once, that the forward's segments tile the window columns, and that
every pooled load the backward kernel issues lies inside the pooled tensors and delivers each element to the lanes, and the
number of times, the kernel's design states.  A buffer load's scalar offset is not range-checked by the hardware and no GPU
test can see a stray read: this is the check that can."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("stem_pool_plan") / "stem_pool_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread",
                        os.path.join(ROOT, "tests", "stem_pool_plan_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_stem_pool_plan_figures_and_invariants(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    assert int(r.stdout.split()[0]) > 7000000000      # the whole sweep ran


def test_in_bounds_assertion_fails_on_the_arithmetic_before_the_plan(exe):
    """--parent: the lane and scalar offsets as the kernel formed them before this header -- both groups of 16 filters
    whatever K is, no lane masked, quads shifted back in the tensor's last window column only.  The same in-bounds
    assertion must find loads past the end of the pooled tensors (for K < 96, and at K = 96 with 15 window rows)."""
    r = subprocess.run([exe, "--parent"], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip())
    assert r.returncode == 1 and "FAILED in-bounds" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    first = r.stdout.split()
    assert int(first[2]) > 0 and int(first[4]) > int(first[2])      # "<n> of <m> loads ... end past the tensor"
