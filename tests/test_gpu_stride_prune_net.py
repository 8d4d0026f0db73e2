"""GPU: the pruned and the unpruned plan of a small (SE-)ResNet compute the same thing.

zoo.resnet50 at a quarter of the width with one block per stage, cut behind res5ax; 64 x 64 inputs, three samples, test mode.
With one block per stage res2ax / res3ax / res4ax are the stage boundaries: each is read by the two 1 x 1 / stride-2
convolutions of the next stage only, so all three expansions are pruned.  Tolerance: the one the path-selector test uses for
outputs, 2e-4 of the tensor's largest magnitude (the two arms run other tile shapes, i.e. other summation orders)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 2e-4


def build(se):
    from mcncrossmodalemotions_amd import zoo
    net = zoo.synthetic_pretrained(zoo.resnet50(se, width_mult=0.25, blocks=(1, 1, 1, 1)), 7)
    for name in ("top1error", "loss", "classifier", "pool5"):
        net.removeLayer(name)
    net.move("gpu")
    net.mode = "test"
    net.vars["res5ax"].precious = True
    return net


def run(net, x, prune, keep=("res5ax",)):
    from mcncrossmodalemotions_amd import vl
    net.stridePrune = prune
    net.eval(["data", x])
    return {k: vl.to_numpy(net.vars[k].value) for k in keep}


def agree(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(np.abs(b).max())
    err = float(np.abs(a.astype(np.float64) - b).max())
    print("%s: largest difference %.2e of %.3g" % (what, err, scale))
    assert scale > 0 and err <= TOL * scale, "%s: %.3e > %.1e * %.3g" % (what, err, TOL, scale)


@pytest.mark.parametrize("se", [False, True], ids=["plain", "se"])
def test_pruned_and_unpruned_plans_agree(gpu, se):
    from mcncrossmodalemotions_amd import vl
    from oracle import oracle as O
    net = build(se)
    x = vl.from_numpy(O.F(np.random.default_rng(3).standard_normal((64, 64, 3, 3))))
    off = run(net, x, False)
    assert not any(st.run_stride is not None for st in net._plan(False))
    on = run(net, x, True)
    assert sorted(st.rec.name for st in net._plan(False) if st.run_stride not in (None, (1, 1))) == \
        ["res2a_branch2c", "res3a_branch2c", "res4a_branch2c"]
    assert off["res5ax"].shape == (2, 2, 512, 3)
    agree(on["res5ax"], off["res5ax"], "res5ax, pruned against unpruned")
    # a precious boundary keeps its full extent (16 x 16 behind the stem's two halvings), the other two stay pruned
    net.vars["res2ax"].precious = True
    got = run(net, x, True, keep=("res5ax", "res2ax"))
    assert sorted(st.rec.name for st in net._plan(False) if st.run_stride not in (None, (1, 1))) == \
        ["res3a_branch2c", "res4a_branch2c"]
    assert got["res2ax"].shape == (16, 16, 64, 3)
    agree(got["res5ax"], off["res5ax"], "res5ax with res2ax precious")
    full = run(net, x, False, keep=("res2ax",))
    agree(got["res2ax"], full["res2ax"], "res2ax itself")
