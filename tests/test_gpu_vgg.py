"""GPU: the VGG face teachers end to end -- the two zoo graphs against the CPU oracle (test-mode forward; one training eval of
the vgg-vd-face + insertBNLayers stand-in), the LRN variant of VGG-M, which the oracle cannot run, against the same vl.* calls
made by hand, and the consumers (FrozenTeacher, buildImdb, ferplus_baselines' training step) with a 7-class VGG teacher.
Narrow networks on three to five faces: every case takes a second or two."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_net
from test_gpu_imdb import framed_imdb
from test_gpu_ops import close

pytestmark = pytest.mark.gpu


def _faces(rng, size, n):
    return O.F(rng.standard_normal((size, size, 3, n)) * 40)


# ------------------------------------------------------------------------------------- test-mode forward against the oracle
@pytest.mark.parametrize("which", ["vgg-vd", "vgg-m-bn"])
def test_forward_matches_the_oracle(gpu, which):
    from mcncrossmodalemotions_amd import vl, zoo
    if which == "vgg-vd":
        net, size = zoo.vgg_vd_face(width_mult=1 / 16, image_size=64), 64
    else:
        net, size = zoo.vgg_m_face(bn=True, width_mult=1 / 8), 224
    zoo.synthetic_pretrained(net, 21)
    x = _faces(np.random.default_rng(3), size, 3)
    P0 = oracle_net.host_params(net)
    V = oracle_net.forward(net, {"input": x}, P0, mode="test")
    net.mode = "test"
    net.move("gpu")
    net.eval(["input", vl.from_numpy(x)])
    assert tuple(net.vars["prob"].value.shape) == (1, 1, 2622, 3)
    for v in ("fc8", "prob"):
        got, ref = vl.to_numpy(net.vars[v].value), V[v]
        print("%s %s: max err %.3e, max |ref| %.3g" % (which, v, np.abs(got - ref).max(), np.abs(ref).max()))
        close(got, ref, 1e-4, "%s %s" % (which, v))


# ------------------------------------------------------------- one training eval of vgg-vd-face + BN against the oracle
def test_vgg_vd_bn_training_eval_matches_the_oracle(gpu):
    """the method and the bounds of tests/test_gpu_nets.py::test_teacher_training_backward (objective 1e-4, parameter
    derivatives 5e-4), with the oracle's backward pass run on the HIP path's own forward values: an unfused HIP pass over
    the same batch and the same dropout masks leaves every variable, so each ReLU mask and each pooling route the oracle
    uses is the one the HIP arithmetic decided"""
    from mcncrossmodalemotions_amd import dagnn, vl, zoo
    rng = np.random.default_rng(8)
    net = zoo.ferPlusZoo("vgg-vd-face", seed=4, width_mult=1 / 16, image_size=64, useBnorm=1, dropoutRate=0.5)
    N = 3
    votes = rng.random((1, 1, 7, N)) + 0.05
    inputs = {"data": _faces(rng, 64, N), "label": O.F(votes / votes.sum(2, keepdims=True)),
              "hardlabel": O.F(votes.argmax(2).reshape(1, 1, 1, N) + 1)}
    P0 = oracle_net.host_params(net)
    net.pack_params()
    net.mode = "normal"
    dev = [v for k in inputs for v in (k, vl.from_numpy(inputs[k]))]
    drops = [l for l in net.layers if isinstance(l.block, dagnn.DropOut)]
    assert len(drops) == 2 and sum(isinstance(l.block, dagnn.BatchNorm) for l in net.layers) == 15

    net.fuse = False                                    # every variable is written: the HIP path's decisions
    net.eval(dev)
    hip = {k: vl.to_numpy(v.value) for k, v in net.vars.items() if v.value is not None}
    hip.update({l.name + ".mask": vl.to_numpy(l.block.mask) for l in drops})
    net.fuse = True
    for l in drops:
        l.block._offset = 0                             # the same masks again
    net.eval(dev, ["objective", 1])
    for l in drops:
        assert np.array_equal(vl.to_numpy(l.block.mask), hip[l.name + ".mask"])

    V = oracle_net.forward(net, dict(inputs, **{k: v for k, v in hip.items() if k.endswith(".mask")}), P0, mode="normal")
    close(hip["prediction"], V["prediction"], 1e-4, "prediction (unfused)")
    close(vl.to_numpy(net.vars["objective"].value).ravel()[0], V["objective"], 1e-4, "objective")
    close(vl.to_numpy(net.vars["classerror"].value).ravel()[0], V["classerror"], 0, "classerror")
    hip["objective"] = np.float32(hip["objective"].ravel()[0])
    _, DP = oracle_net.backward(net, hip, {"objective": np.float32(1)}, P0, mode="normal")
    assert set(DP) == set(net.params)
    worst = 0.0
    for name, ref in DP.items():
        got = vl.to_numpy(net.params[name].der).reshape(ref.shape, order="F")
        worst = max(worst, np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
        close(got, ref, 5e-4, "der " + name)
    print("vgg-vd-face + BN training eval: worst derivative error / max(1, max |ref|) = %.3e" % worst)


# ------------------------------------------------------------------------------------- VGG-M with its norm1 / norm2 layers
def _by_hand(net, x, dzdy=None):
    """the layers of a chain, one vl.* call each in layer order; with dzdy also the backward calls -> (values, derivatives)"""
    from mcncrossmodalemotions_amd import dagnn, vl
    training = dzdy is not None
    val, aux = {"input": x}, {}
    for l in net.layers:
        b, xin = l.block, val[l.inputs[0]]
        prm = [net.params[p].value for p in l.params]
        if isinstance(b, dagnn.Conv):
            y = vl.vl_nnconv(xin, prm[0], prm[1], stride=b.stride, pad=b.pad, dilate=b.dilate)
        elif isinstance(b, dagnn.ReLU):
            y = vl.vl_nnrelu(xin)
        elif isinstance(b, dagnn.LRN):
            y = vl.vl_nnnormalize(xin, b.param)
        elif isinstance(b, dagnn.Pooling):
            if training:
                y, aux[l.name] = vl.vl_nnpool(xin, b.poolSize, stride=b.stride, pad=b.pad, method="max", want_argmax=True)
            else:
                y = vl.vl_nnpool(xin, b.poolSize, stride=b.stride, pad=b.pad, method="max")
        else:
            assert isinstance(b, dagnn.SoftMax), l.name
            y = vl.vl_nnsoftmax(xin)
        val[l.outputs[0]] = y
    if not training:
        return val, None
    der, dz = {}, dzdy
    for l in reversed(net.layers):
        b, xin = l.block, val[l.inputs[0]]
        prm = [net.params[p].value for p in l.params]
        if isinstance(b, dagnn.Conv):
            first = l.inputs[0] == "input"
            dz, df, db = vl.vl_nnconv(xin, prm[0], prm[1], dz, stride=b.stride, pad=b.pad, dilate=b.dilate, no_der_data=first)
            der[l.params[0]], der[l.params[1]] = df, db
        elif isinstance(b, dagnn.ReLU):
            dz = vl.vl_nnrelu(xin, dz)
        elif isinstance(b, dagnn.LRN):
            dz = vl.vl_nnnormalize(xin, b.param, dz)
        elif isinstance(b, dagnn.Pooling):
            dz = vl.vl_nnpool(xin, b.poolSize, dz, stride=b.stride, pad=b.pad, method="max", argmax=aux[l.name])
        else:
            dz = vl.vl_nnsoftmax(xin, dz)
    return val, der


def _plan(net, training):
    from mcncrossmodalemotions_amd import dagnn
    return [(type(st).__name__, [q.name for q in st.recs]) for st in dagnn.build_plan(net, training)]


def test_vgg_m_with_lrn_is_its_layers_by_hand(gpu):
    import torch
    from mcncrossmodalemotions_amd import dagnn, vl, zoo
    net = zoo.vgg_m_face(bn=False, num_classes=9, width_mult=1 / 8)
    zoo.synthetic_pretrained(net, 6)
    net.move("gpu")
    rng = np.random.default_rng(2)
    x = vl.from_numpy(_faces(rng, 224, 3))
    dzdy = vl.from_numpy(O.F(rng.standard_normal((1, 1, 9, 3))))
    checked = ("norm1", "pool1", "norm2", "pool2", "fc8", "prob")

    def run(mode, fuse, der):
        net.mode, net.fuse = mode, fuse
        for v in checked:
            net.vars[v].precious = not fuse          # (a fused plan does not write what it swallows; these it keeps anyway)
        net.eval(["input", x], ["prob", dzdy] if der else None)
        vals = {v: net.vars[v].value.clone() for v in ("fc8", "prob")}
        if not fuse:
            vals.update({v: net.vars[v].value.clone() for v in checked})
        ders = {k: p.der.clone() for k, p in net.params.items()} if der else None
        return vals, ders

    # the LRN steps are generic steps, and around them the plans are those of the graph without the two layers
    bare = zoo.vgg_m_face(bn=False, num_classes=9, width_mult=1 / 8)
    bare.removeLayer(["norm1", "norm2"])
    bare.setLayerInputs("pool1", "relu1")
    bare.setLayerInputs("pool2", "relu2")
    for mode, training in (("test", False), ("normal", True), ("normal", False)):
        net.mode = bare.mode = mode
        plan = _plan(net, training)
        lrn = [s for s in plan if s[1][0] in ("norm1", "norm2")]
        assert lrn == [("_Step", ["norm1"]), ("_Step", ["norm2"])]
        assert [s for s in plan if s not in lrn] == _plan(bare, training), (mode, training)
    net.mode = "test"
    assert ("_ConvActStep", ["conv1", "relu1"]) in _plan(net, False) and ("_PoolStep", ["pool1"]) in _plan(net, False)

    for mode, der in (("test", False), ("normal", True)):
        run(mode, False, der)                                           # (first sight of the shapes: kernels are chosen)
        vals, ders = run(mode, False, der)
        hand, hder = _by_hand(net, x, dzdy if der else None)
        for v in checked:
            assert torch.equal(vals[v], hand[v]), (mode, v)
        if der:
            assert set(hder) == set(ders)
            for k in hder:
                assert torch.equal(ders[k], hder[k].reshape(ders[k].shape)), k
        fvals, fders = run(mode, True, der)
        for v in ("fc8", "prob"):
            close(vl.to_numpy(fvals[v]), vl.to_numpy(vals[v]), 1e-4, "fused %s %s" % (mode, v))
        if der:
            for k in ders:
                close(vl.to_numpy(fders[k]), vl.to_numpy(ders[k]), 1e-4, "fused der " + k)
    y1 = vl.to_numpy(hand["norm1"])
    assert np.isfinite(y1).all() and np.abs(y1).max() > 1


# ----------------------------------------------------------------------------------------------------------- the consumers
def _fer_teacher(seed=2):
    from mcncrossmodalemotions_amd import zoo
    return zoo.ferPlusZoo("vgg-vd-face-fer", seed=seed, width_mult=1 / 16, image_size=64)


def test_frozen_vgg_teacher_lanes(gpu):
    from mcncrossmodalemotions_amd import batch, vl, zoo
    faces = batch.getImageBatch(5, imageSize=(64, 64), averageImage=(129.1863, 104.7624, 93.5940), seed=3)
    outs = []
    for lanes in (1, 2):
        net = _fer_teacher()
        net.mode = "test"
        net.move("gpu")
        t = zoo.FrozenTeacher(net, lanes=lanes)
        assert t.output == "prediction" and len(t.nets) == lanes
        outs.append(vl.to_numpy(t.logits(faces)))
    assert outs[0].shape == (1, 1, 7, 5) and np.unique(outs[0].reshape(7, 5).T, axis=0).shape[0] == 5
    close(outs[1], outs[0], 1e-4, "two lanes")


def test_build_imdb_with_a_vgg_teacher(gpu):
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    imdb, frames = framed_imdb(2, 5, frameSize=(80, 72), min_seconds=1.0, max_seconds=2.0)
    net = _fer_teacher()
    built = fe.buildImdb(net, imdb, frames, batchSize=16)
    assert net.mode == "test" and len(built.wavLogits) == 2
    counts = [int((imdb.images["denseFramesWavIds"] == i).sum()) for i in imdb.images["id"]]
    for cell, n in zip(built.wavLogits, counts):
        assert cell.dtype == np.float32 and cell.shape == (n, 7) and n > 0 and np.isfinite(cell).all()
    dev, offs = built.device_logits(gpu)
    assert int(dev.shape[1]) == 7 and list(offs) == [0, counts[0], counts[0] + counts[1]]


def test_compute_visual_feats_with_a_vgg_teacher(gpu):
    from mcncrossmodalemotions_amd import batch, external
    tracks = [batch.getImageBatch(n, imageSize=(64, 64), seed=n) for n in (3, 4)]
    logits = external.compute_visual_feats(_fer_teacher(), tracks, batchSize=5)
    assert [l.shape for l in logits] == [(3, 7), (4, 7)] and all(np.isfinite(l).all() for l in logits)


def test_ferplus_baselines_trains_a_vgg_teacher(gpu, tmp_path):
    """the driver itself, as ferplus_baselines.m is written for a VGG teacher: one epoch, narrow, on synthetic FER+ images"""
    from mcncrossmodalemotions_amd import batch, dagnn
    from mcncrossmodalemotions_amd.ferplus_baselines import ferplus_baselines
    imdb = batch.SyntheticFerPlusImdb(num_images=16, seed=2)
    net, info = ferplus_baselines(modelName="vgg-vd-face", useBnorm=1, imdb=imdb, expRoot=str(tmp_path), widthMult=1 / 16,
                                  batchSize=4, learningRate=[0.01], numEpochs=1)
    assert sum(isinstance(l.block, dagnn.BatchNorm) for l in net.layers) == 15
    assert len(info["train"]) == 1 and np.isfinite(info["train"][0]["objective"]) and 0 <= info["train"][0]["classerror"] <= 1
    assert info["train"][0]["num"] == int((imdb.images["set"] == 1).sum()) > 0


def test_two_training_steps_of_ferplus_baselines_loop(gpu):
    """the loop body of ferplus_baselines (cnn_train_dag -> train_step on getBatchFerPlus batches) on the vgg-vd-face + BN
    stand-in: the steps run, every BatchNorm's moments move off their initial (0, 1), every parameter stays finite"""
    from mcncrossmodalemotions_amd import batch, dagnn, train, vl, zoo
    net = zoo.ferPlusZoo("vgg-vd-face", seed=9, width_mult=1 / 16, image_size=64, useBnorm=1, dropoutRate=0.5,
                         finetuneLR=0.1, numOutputs=8)
    imdb = batch.SyntheticFerPlusImdb(num_images=16, seed=4)
    idx = [int(i) for i in np.nonzero(imdb.images["set"] == 1)[0][:8]]
    opts = train.TrainOpts(learningRate=[0.01], batchSize=4)
    rng = np.random.default_rng(1)
    norm = net.meta["normalization"]
    before = None
    for step in range(2):
        inputs = batch.getBatchFerPlus(imdb, idx[4 * step:4 * step + 4], rng=rng, imageSize=tuple(norm["imageSize"][:2]),
                                       averageImage=norm["averageImage"])
        train.train_step(net, inputs, opts, 0, None, 4)
        if before is None:
            before = {k: vl.to_numpy(p.value).copy() for k, p in net.params.items()}
    bns = [l for l in net.layers if isinstance(l.block, dagnn.BatchNorm)]
    assert len(bns) == 15
    for l in bns:
        mom = vl.to_numpy(net.params[l.params[2]].value)
        assert not np.array_equal(mom[:, 0], np.zeros(mom.shape[0])) and not np.array_equal(mom[:, 1], np.ones(mom.shape[0]))
        assert not np.array_equal(mom, before[l.params[2]]), l.name
    for k, p in net.params.items():
        assert np.isfinite(vl.to_numpy(p.value)).all(), k
    assert np.isfinite(float(vl.to_numpy(net.vars["objective"].value).ravel()[0]))
