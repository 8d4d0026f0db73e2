"""CPU: which steps the stage-boundary pruning pass of dagnn.build_plan touches (plan structure only, no operator runs).

A stage of the Caffe-style teachers ends in a 1 x 1 expansion whose output is read only by the two 1 x 1 / stride-2
convolutions that open the next stage; in forward-only test-mode plans that expansion runs with the readers' stride and the
readers with unit stride."""
import pytest

from mcncrossmodalemotions_amd import dagnn, zoo


def pruned(net, training=False):
    """({conv layer of a step that runs with a stride > 1 of its own}, {conv layer of a step forced to unit stride})"""
    big, unit = set(), set()
    for st in net._plan(training):
        if st.run_stride is None:
            continue
        (unit if tuple(st.run_stride) == (1, 1) else big).add(st.rec.name)
    return big, unit


EXPANSIONS = {"res2c_branch2c", "res3d_branch2c", "res4f_branch2c"}
READERS = {"res%da_branch%s" % (s, b) for s in (3, 4, 5) for b in ("1", "2a")}


@pytest.fixture(scope="module", params=["resnet50-ferplus", "senet50-ferplus"])
def teacher(request):
    net = zoo.ferPlusZoo(request.param, seed=100)
    zoo.strip_losses(net)
    net.mode = "test"
    return net


def test_teachers_prune_exactly_the_three_stage_ends(teacher):
    big, unit = pruned(teacher)
    assert big == EXPANSIONS and unit == READERS
    steps = {st.rec.name: st for st in teacher._plan(False)}
    for name in EXPANSIONS:
        assert tuple(steps[name].run_stride) == (2, 2)
        assert isinstance(steps[name], dagnn._ConvFoldStep)
    if any(isinstance(l.block, dagnn.Axpy) for l in teacher.layers):     # the SE teacher: the gated expansion
        assert all(isinstance(steps[n], dagnn._SEFoldStep) for n in EXPANSIONS)


def test_nothing_is_pruned_outside_forward_only_test_mode(teacher):
    assert pruned(teacher, training=True) == (set(), set())
    teacher.mode = "normal"
    try:
        assert pruned(teacher) == (set(), set())
    finally:
        teacher.mode = "test"
    teacher.fuse = False
    try:
        assert pruned(teacher) == (set(), set())
    finally:
        teacher.fuse = True
    teacher.stridePrune = False
    try:
        assert pruned(teacher) == (set(), set())
    finally:
        teacher.stridePrune = True
    assert pruned(teacher)[0] == EXPANSIONS


def test_the_switch_is_read_from_the_environment(monkeypatch):
    monkeypatch.setenv("XM_STRIDE_PRUNE", "0")
    assert dagnn.DagNN().stridePrune is False
    monkeypatch.setenv("XM_STRIDE_PRUNE", "1")
    assert dagnn.DagNN().stridePrune is True
    monkeypatch.delenv("XM_STRIDE_PRUNE")
    assert dagnn.DagNN().stridePrune is True


def test_a_precious_boundary_keeps_its_extent(teacher):
    teacher.vars["res3dx"].precious = True
    try:
        big, unit = pruned(teacher)
        assert big == EXPANSIONS - {"res3d_branch2c"}
        assert unit == READERS - {"res4a_branch1", "res4a_branch2a"}
    finally:
        teacher.vars["res3dx"].precious = False
    assert pruned(teacher) == (EXPANSIONS, READERS)


def small(se=False):
    net = zoo.resnet50(se, 8, 0.125, (1, 1, 1, 1))
    zoo.strip_losses(net)
    net.mode = "test"
    return net


@pytest.mark.parametrize("se", [False, True])
def test_a_reader_that_is_no_strided_1x1_keeps_the_boundary(se):
    net = small(se)
    assert pruned(net) == ({"res2a_branch2c", "res3a_branch2c", "res4a_branch2c"},
                           {"res%da_branch%s" % (s, b) for s in (3, 4, 5) for b in ("1", "2a")})
    # a third reader of res3ax: a pooling layer
    net.addLayer("side_pool", dagnn.Pooling([2, 2], (2, 2), (0, 0, 0, 0), "max"), "res3ax", "side_pool")
    big, unit = pruned(net)
    assert big == {"res2a_branch2c", "res4a_branch2c"}
    assert unit == {"res3a_branch1", "res3a_branch2a", "res5a_branch1", "res5a_branch2a"}


def test_readers_with_different_strides_keep_the_boundary():
    net = small()
    blk = [l for l in net.layers if l.name == "res4a_branch1"][0].block
    blk.stride = (1, 1)
    net._plan_key = None
    big, unit = pruned(net)
    assert "res3a_branch2c" not in big and not ({"res4a_branch1", "res4a_branch2a"} & unit)
    blk.stride = (2, 1)       # differs from res4a_branch2a's (2, 2)
    net._plan_key = None
    assert "res3a_branch2c" not in pruned(net)[0]
    # a 3 x 3 reader with the right stride is no 1 x 1 reader
    net2 = small()
    b2 = [l for l in net2.layers if l.name == "res3a_branch2a"][0].block
    b2.size = (3, 3) + tuple(b2.size[2:])
    b2.pad = (1, 1, 1, 1)
    assert "res2a_branch2c" not in pruned(net2)[0]


def test_library_rejects_an_inconsistent_residual_extent():
    """argument validation happens before any device work (the pointers are never followed)"""
    import ctypes as C
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    assert L.xm_version() >= 117
    p = C.c_void_p(64)

    def call(res_H, res_W, rsy, rsx):
        return L.xm_nnconv_forward_strided_residual(p, 8, 8, 16, 2, p, 1, 1, 16, 32, None, p, 2, 2, 0, 0, 0, 0, 1, 1, None,
                                                    None, None, p, res_H, res_W, rsy, rsx, 0, None)
    for bad in ((8, 8, 3, 3), (9, 8, 2, 2), (8, 10, 2, 2), (4, 4, 2, 2), (8, 8, 0, 2), (0, 8, 2, 2), (8, 8, 1, 1)):
        assert call(*bad) == 1, bad                                # XM_EINVAL
        assert b"residual" in L.xm_last_error(), (bad, L.xm_last_error())


def test_pinned_table_entries_are_in_the_shipped_table():
    """the tuning-table entries that were set by reduction structure, not by speed (tune_gfx950.pinned.txt says why), are
    still what the shipped table holds: a regenerated table that silently replaced one would change the teachers' bits"""
    import os
    here = os.path.dirname(os.path.abspath(dagnn.__file__))
    table = {tuple(l.split()[:9]): l.split()[9] for l in open(os.path.join(here, "tune_gfx950.txt")).read().splitlines()[1:]}
    pinned = [l.split("#")[0].split() for l in open(os.path.join(here, "tune_gfx950.pinned.txt")) if l.split("#")[0].strip()]
    assert len(pinned) == 20 and all(len(p) == 10 for p in pinned)
    wrong = [" ".join(p) for p in pinned if table.get(tuple(p[:9])) != p[9]]
    assert not wrong, wrong
