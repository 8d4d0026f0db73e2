"""GPU: a ResNet-50 teacher computes the same BITS with and without the lattice pass of dagnn.build_plan
(_prune_reader_lattices): the logits are bit-identical, and the outputs of the three 3 x 3 layers in front of the pruned
stage-end expansions agree bit for bit at the lattice pixels (the others are unspecified and nothing reads them).

zoo.resnet50 at an eighth of the width with one block per stage over 200 x 200 inputs (3 x 3 layers over 50 x 50, 25 x 25
and 13 x 13 maps with 8, 16 and 32 channels: odd extents, reductions that are no multiple of the stage depth; the last
stage is 7 x 7, the head's pooling window), and the full teacher at two faces.  The "off" arm runs first: with find mode on
it measures every full-extent layer, and the "on" arm then finds the configuration each layer runs with.  The halo-patch kernels are switched off for both arms (`conv_halo` 0), so
that every full-extent 3 x 3 layer is an implicit-GEMM launch and all three lattice calls have to compute the lattice only
-- the record of each call ("conv_last_lattice") is read right behind it.  Each network is compared once more with the
library's own selection, whatever it is: there a layer may stay at full extent, the bits may not differ."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def marked(net):
    return {st.rec.name: st.outputs[0] for st in net._plan(False) if st.out_lattice is not None}


def run(net, x, on, keep, monkeypatch, L):
    """({variable: value}, [conv_last_lattice of every out_lattice call])"""
    from mcncrossmodalemotions_amd import dagnn, vl
    ran = []
    real = vl.vl_nnconv

    def spy(*a, **kw):
        y = real(*a, **kw)
        if kw.get("out_lattice") is not None:
            ran.append(L.xm_debug_get(b"conv_last_lattice"))
        return y
    net.latticePrune = on
    with monkeypatch.context() as m:
        m.setattr(dagnn.vl, "vl_nnconv", spy)
        net.eval(["data", x])
    return {v: vl.to_numpy(net.vars[v].value) for v in keep}, ran


def compare(net, x, monkeypatch, L, names, must_run):
    net.latticePrune = True
    m = marked(net)
    assert sorted(m) == sorted(names)
    logits = net.layers[-1].outputs[0]
    keep = list(m.values()) + [logits]
    off, ran = run(net, x, False, keep, monkeypatch, L)
    assert ran == [] and marked(net) == {}
    on, ran = run(net, x, True, keep, monkeypatch, L)
    assert len(ran) == 3 and (not must_run or ran == [1, 1, 1]), ran
    assert float(np.abs(off[logits]).max()) > 0
    assert np.array_equal(bits(on[logits]), bits(off[logits])), "logits differ by %.3e" % float(np.abs(on[logits] - off[logits]).max())
    for name, v in m.items():
        a, b = on[v][::2, ::2], off[v][::2, ::2]
        assert a.shape == b.shape and float(np.abs(b).max()) > 0
        assert np.array_equal(bits(a), bits(b)), "%s: %d lattice values differ" % (name, int((bits(a) != bits(b)).sum()))
    return ran


def test_narrow_resnet(gpu, monkeypatch):
    from mcncrossmodalemotions_amd import _lib, vl, zoo
    L = _lib.load()
    net = zoo.synthetic_pretrained(zoo.resnet50(False, 8, 0.125, (1, 1, 1, 1)), 7)
    zoo.strip_losses(net)
    net.move("gpu")
    net.mode = "test"
    x = vl.from_numpy(np.random.default_rng(3).standard_normal((200, 200, 3, 3)).astype(np.float32))
    names = ["res%da_branch2b" % s for s in (2, 3, 4)]
    old = L.xm_debug_force_conv_halo(0)
    try:
        compare(net, x, monkeypatch, L, names, True)
    finally:
        L.xm_debug_force_conv_halo(old)
    ran = compare(net, x, monkeypatch, L, names, False)
    print("lattice calls that computed the lattice only, library's own selection:", ran)


def test_full_resnet50_at_two_faces(gpu, monkeypatch):
    from mcncrossmodalemotions_amd import _lib, vl, zoo
    L = _lib.load()
    net = zoo.ferPlusZoo("resnet50-ferplus", seed=100)
    zoo.strip_losses(net)
    net.move("gpu")
    net.mode = "test"
    x = vl.from_numpy(np.random.default_rng(4).standard_normal((224, 224, 3, 2)).astype(np.float32))
    old = L.xm_debug_force_conv_halo(0)
    try:
        compare(net, x, monkeypatch, L, ["res2c_branch2b", "res3d_branch2b", "res4f_branch2b"], True)
    finally:
        L.xm_debug_force_conv_halo(old)
    ran = compare(net, x, monkeypatch, L, ["res2c_branch2b", "res3d_branch2b", "res4f_branch2b"], False)
    print("lattice calls that computed the lattice only, library's own selection:", ran)
