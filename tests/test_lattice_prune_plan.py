"""CPU: which steps the second pruning pass of dagnn.build_plan (_prune_reader_lattices) marks, and the lattice index
arithmetic of csrc/conv_plan.h.  Plan structure only, no operator runs.

In the plain ResNet-50 teacher the 3 x 3 layer in front of each pruned stage-end expansion has that expansion as its only
reader, and the expansion samples every other row of every other column: the 3 x 3 step carries out_lattice = (2, 2).  In
the SE teacher the expansion's squeeze reads every pixel, so nothing is marked there."""
import os
import shutil
import subprocess

import pytest

from mcncrossmodalemotions_amd import dagnn, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE = {"res2c_branch2b", "res3d_branch2b", "res4f_branch2b"}


def lattices(net, training=False):
    return {st.rec.name: tuple(st.out_lattice) for st in net._plan(training) if st.out_lattice is not None}


def run_strides(net, training=False):
    return {st.rec.name: tuple(st.run_stride) for st in net._plan(training) if st.run_stride is not None}


def teacher(name):
    net = zoo.ferPlusZoo(name, seed=100)
    zoo.strip_losses(net)
    net.mode = "test"
    return net


@pytest.fixture(scope="module")
def plain():
    return teacher("resnet50-ferplus")


def test_the_plain_teacher_marks_exactly_the_three_3x3_layers(plain):
    assert lattices(plain) == {n: (2, 2) for n in LATTICE}
    steps = {st.rec.name: st for st in plain._plan(False)}
    for n in LATTICE:
        assert type(steps[n]) is dagnn._ConvFoldStep and steps[n].run_stride is None and steps[n].sum_rec is None
        assert tuple(steps[n].rec.block.size[:2]) == (3, 3)


def test_the_se_teacher_marks_nothing():
    assert lattices(teacher("senet50-ferplus")) == {}


def test_run_strides_and_steps_are_what_they_are_without_the_pass(plain):
    on = run_strides(plain)
    names = [st.rec.name for st in plain._plan(False)]
    layers = [[q.name for q in st.recs] for st in plain._plan(False)]
    plain.latticePrune = False
    try:
        assert lattices(plain) == {}
        assert run_strides(plain) == on
        assert [st.rec.name for st in plain._plan(False)] == names
        assert [[q.name for q in st.recs] for st in plain._plan(False)] == layers
    finally:
        plain.latticePrune = True
    assert {k for k, v in on.items() if v != (1, 1)} == {n[:-1] + "c" for n in LATTICE}


def test_nothing_is_marked_outside_forward_only_test_mode(plain):
    assert lattices(plain, training=True) == {}
    for attr, off, on in (("mode", "normal", "test"), ("fuse", False, True), ("stridePrune", False, True),
                          ("latticePrune", False, True)):
        setattr(plain, attr, off)
        try:
            assert lattices(plain) == {}, attr
        finally:
            setattr(plain, attr, on)
    assert set(lattices(plain)) == LATTICE


def test_the_switch_is_read_from_the_environment(monkeypatch):
    monkeypatch.setenv("XM_LATTICE_PRUNE", "0")
    assert dagnn.DagNN().latticePrune is False
    monkeypatch.setenv("XM_LATTICE_PRUNE", "1")
    assert dagnn.DagNN().latticePrune is True
    monkeypatch.delenv("XM_LATTICE_PRUNE")
    assert dagnn.DagNN().latticePrune is True


def test_a_replica_keeps_the_switch(plain):
    plain.latticePrune = False
    try:
        assert plain.replica().latticePrune is False
    finally:
        plain.latticePrune = True


def test_a_precious_or_shared_3x3_output_keeps_its_extent(plain):
    var = [l for l in plain.layers if l.name == "res3d_branch2b"][0].outputs[0]
    # precious: the convolution no longer folds its bnorm at all, and nothing is marked on it
    plain.vars[var].precious = True
    try:
        assert set(lattices(plain)) == LATTICE - {"res3d_branch2b"}
    finally:
        plain.vars[var].precious = False
    assert set(lattices(plain)) == LATTICE
    # the variable the expansion reads (behind the folded bnorm and ReLU) precious, or read by a second layer
    out = {st.rec.name: st for st in plain._plan(False)}["res3d_branch2b"].outputs[0]
    plain.vars[out].precious = True
    try:
        assert set(lattices(plain)) == LATTICE - {"res3d_branch2b"}
        assert {k for k, v in run_strides(plain).items() if v != (1, 1)} == {n[:-1] + "c" for n in LATTICE}
    finally:
        plain.vars[out].precious = False
    net = teacher("resnet50-ferplus")
    out = {st.rec.name: st for st in net._plan(False)}["res2c_branch2b"].outputs[0]
    net.addLayer("side_pool", dagnn.Pooling([2, 2], (2, 2), (0, 0, 0, 0), "max"), out, "side_pool")
    assert set(lattices(net)) == LATTICE - {"res2c_branch2b"}


def test_the_narrow_resnet_of_the_gpu_test_is_marked_too():
    net = zoo.resnet50(False, 8, 0.125, (1, 1, 1, 1))
    zoo.strip_losses(net)
    net.mode = "test"
    assert lattices(net) == {"res%da_branch2b" % s: (2, 2) for s in (2, 3, 4)}
    se = zoo.resnet50(True, 8, 0.125, (1, 1, 1, 1))
    zoo.strip_losses(se)
    se.mode = "test"
    assert lattices(se) == {}


def test_library_validates_the_lattice_call_before_any_device_work():
    import ctypes as C
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    assert L.xm_version() >= 123
    assert "123 = + xm_nnconv_forward_lattice" in open(os.path.join(ROOT, "include", "xmodal.h")).read()
    p = C.c_void_p(64)

    def call(resid, flags, ly, lx):
        return L.xm_nnconv_forward_lattice(p, 8, 8, 16, 2, p, 3, 3, 16, 32, None, p, 1, 1, 1, 1, 1, 1, 1, 1, None, None, resid,
                                           flags, ly, lx, None)
    assert call(None, 0, 0, 2) == 1 and b"lattice steps" in L.xm_last_error()        # XM_EINVAL
    assert call(None, 0, 2, -1) == 1
    assert call(p, 0, 2, 2) == 5 and b"residual" in L.xm_last_error()                # XM_ENOTSUP
    assert call(None, 4, 2, 2) == 5 and b"ReLU" in L.xm_last_error()                 # XM_FUSE_SIGMOID


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_lattice_index_arithmetic_against_its_definition(tmp_path):
    exe = str(tmp_path / "lattice_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "lattice_plan_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # the whole grid ran: 9 lattices x sum over Ho <= 9, Wo <= 7, N <= 3 of (Ho Wo N + 1) cuts
    assert int(r.stdout.split()[0]) == 9 * sum(h * w * n + 1 for h in range(1, 10) for w in range(1, 8) for n in range(1, 4))
