"""CPU: the host side of teacher training (teacher/ferplus_baselines.m, teacher/ferPlusZoo.m) -- computeAugs draws and
closed forms, the [5 4 2 1 8 7] reorder, buildExpDirName, the ferPlusZoo training graph, getBatchFerPlus's set check --
and the ABI of the sampler operators (declared, typed, exported)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ABI = ["xm_nnaffinegrid", "xm_nnaffinegrid_backward", "xm_nnbilinearsampler", "xm_nnbilinearsampler_backward",
           "xm_ferplus_batch"]


def _augs_restated(B, rng):
    """ferplus_baselines.m:224-268 written out again, draw by draw (MATLAB column-major order)."""
    minXY = rng.integers(1, 10, size=2 * B).reshape((B, 2), order="F")          # randi(9, B, 2)
    zoomSc = 0.96 + 0.08 * rng.random(B)
    thetas = rng.integers(1, 4, size=B * B)[:B]                                  # randi(3, B): B x B, first B used
    skews = rng.integers(1, 4, size=2 * B).reshape((B, 2), order="F")
    drop = rng.random(B) > 0.5
    out = np.zeros((3, 3, B))
    for i in range(B):
        z = zoomSc[i]
        zs = (z - 1) / z
        Z = np.array([[1, 0, zs - 2 * zs * minXY[i, 1]], [0, 1, zs - 2 * zs * minXY[i, 0]], [0, 0, 1]]) * z
        t = [-np.pi / 18, 0, np.pi / 18][thetas[i] - 1]
        R = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
        s1, s2 = [-0.1, 0, 0.1][skews[i, 0] - 1], [-0.1, 0, 0.1][skews[i, 1] - 1]
        S = np.array([[1, s1, 0], [s2, 1, 0], [0, 0, 1]])
        out[:, :, i] = np.eye(3) if drop[i] else Z @ R @ S
    return out, dict(minXY=minXY, zoomSc=zoomSc, thetas=thetas, skews=skews, drop=drop)


def test_compute_augs_draw_order_and_closed_forms():
    from mcncrossmodalemotions_amd import batch
    B = 7
    got = batch.computeAugs(B, np.random.default_rng(5))
    ref, _ = _augs_restated(B, np.random.default_rng(5))
    assert got.shape == (3, 3, B)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-15)
    # the B x B randi quirk: computeAugs consumes 2B + B + B*B + 2B + B numbers, so the NEXT draw of the stream is the
    # one after all of them (a B-element theta draw would leave the stream elsewhere)
    r1 = np.random.default_rng(9)
    batch.computeAugs(B, r1)
    r2 = np.random.default_rng(9)
    _augs_restated(B, r2)
    assert r1.random() == r2.random()
    r3 = np.random.default_rng(9)
    r3.integers(1, 10, 2 * B), r3.random(B), r3.integers(1, 4, B), r3.integers(1, 4, 2 * B), r3.random(B)
    r1b = np.random.default_rng(9)
    batch.computeAugs(B, r1b)
    assert r1b.random() != r3.random()


def test_compute_augs_ranges():
    from mcncrossmodalemotions_amd import batch
    B = 2000
    affs, d = batch.computeAugs(B, np.random.default_rng(1)), _augs_restated(B, np.random.default_rng(1))[1]
    assert set(np.unique(d["minXY"])) == set(range(1, 10))             # maxOffset = round(224 / 25) = 9
    assert d["zoomSc"].min() >= 0.96 and d["zoomSc"].max() <= 1.04
    ident = np.array([np.array_equal(affs[:, :, i], np.eye(3)) for i in range(B)])
    assert np.array_equal(ident, d["drop"])
    assert 0.45 < ident.mean() < 0.55                                   # "only apply data augmentation 50% of the time"
    kept = affs[:, :, ~ident]
    zoom = kept[2, 2]                                                   # last row of zoomOut(..) * R * S = [0 0 zoomSc]
    assert zoom.min() >= 0.96 and zoom.max() <= 1.04
    # rotation angle and skews recovered from the 2 x 2 block: M / zoom = R(t) [1 s1; s2 1]
    for i in range(0, kept.shape[2], 97):
        M = kept[:2, :2, i] / zoom[i]
        found = False
        for t in (-np.pi / 18, 0, np.pi / 18):
            R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
            S = R.T @ M
            if np.allclose(np.diag(S), 1, atol=1e-12) and all(
                    min(abs(S[a, b] - v) for v in (-0.1, 0, 0.1)) < 1e-12 for a, b in ((0, 1), (1, 0))):
                found = True
        assert found, M


def test_affine_reorder_maps_xy_matrices_onto_the_grid_convention():
    """tmp([5 4 2 1 8 7]) of a matrix acting on (x, y, 1) gives c1..c6 with grid Y = c1 y + c3 x + c5 and
    grid X = c2 y + c4 x + c6 -- exactly the transformed (y', x')."""
    from mcncrossmodalemotions_amd import batch
    np.testing.assert_array_equal(batch.affine_params(np.eye(3)), [1, 0, 0, 1, 0, 0])
    rng = np.random.default_rng(3)
    for aff in [batch.computeAugs(1, rng)[:, :, 0] for _ in range(20)] + [rng.standard_normal((3, 3))]:
        c = batch.affine_params(aff)
        for _ in range(5):
            x, y = rng.uniform(-1, 1, 2)
            xp, yp, _ = aff @ np.array([x, y, 1.0])
            assert abs((c[0] * y + c[2] * x + c[4]) - yp) < 1e-12
            assert abs((c[1] * y + c[3] * x + c[5]) - xp) < 1e-12


def test_build_exp_dir_name():
    from mcncrossmodalemotions_amd.ferplus_baselines import buildExpDirName
    r = "data/grimaces/fer2013+"
    assert buildExpDirName() == os.path.join(r, "senet50_ft-dag-distributions-CNTK-dropout-0.5-aug")
    assert buildExpDirName("resnet50_ft-dag", "softmaxlog", "clean", 0, False) == \
        os.path.join(r, "resnet50_ft-dag-softmaxlog")
    assert buildExpDirName("resnet50_ft-dag", "distributions", "full", 0.1, True, root="x") == \
        os.path.join("x", "resnet50_ft-dag-distributions-full-dropout-0.1-aug")


@pytest.mark.parametrize("dataType,numOutputs", [("CNTK", 8), ("clean", 8), ("full", 10)])
def test_num_classes(dataType, numOutputs):
    from mcncrossmodalemotions_amd import batch
    assert batch.ferplus_num_classes(dataType) == numOutputs
    with pytest.raises(ValueError):
        batch.ferplus_num_classes("other")


@pytest.mark.parametrize("modelName,dropped", [("senet50_ft-dag", ["res5a_fc1", "res5a_fc2"]),
                                               ("resnet50_ft-dag", ["res5a_branch2b", "res5a_branch2c"])])
@pytest.mark.parametrize("numOutputs", [8, 10])
def test_ferpluszoo_training_graph(modelName, dropped, numOutputs):
    from mcncrossmodalemotions_amd import dagnn, zoo
    net = zoo.ferPlusZoo(modelName, width_mult=0.125, blocks=(1, 1, 1, 1), useBnorm=True, finetuneLR=0.1,
                         dropoutRate=0.5, lossType="distributions", numOutputs=numOutputs)
    # dropout behind convLayers(end-2:end-1), between each and its consumer
    drops = [l for l in net.layers if isinstance(l.block, dagnn.DropOut)]
    assert [l.name for l in drops] == [d + "_drop" for d in dropped]
    for l, d in zip(drops, dropped):
        assert l.inputs == [d] and l.block.rate == 0.5
        assert [m.name for m in net.layers if (d + "_drop") in m.inputs]
        assert not [m.name for m in net.layers if d in m.inputs and m is not l]
    # learning rates: finetuneLR on every parameter of layers(1:end-2) -- the classifier keeps its own
    body = {p for l in net.layers if l.name not in ("classifier", "loss", "classerror") for p in l.params}
    assert body and all(net.params[p].learningRate == 0.1 for p in body)
    assert net.params["classifier_filter"].learningRate == 1.0 and net.params["classifier_bias"].learningRate == 2.0
    assert net.getLayer("classifier").block.size[3] == numOutputs
    # heads
    loss, err = net.getLayer("loss"), net.getLayer("classerror")
    assert isinstance(loss.block, dagnn.SoftmaxCELoss) and loss.block.temperature == 1 and not loss.block.logitTargets
    assert loss.inputs == ["prediction", "label"] and loss.outputs == ["objective"]
    assert isinstance(err.block, dagnn.Loss) and err.block.loss == "classerror"
    assert err.inputs == ["prediction", "hardlabel"] and err.outputs == ["classerror"]
    assert net.getInputs() == ["data", "label", "hardlabel"]
    assert net.meta["classes"]["name"][:2] == ["neutral", "happiness"]
    # softmaxlog: the batch has no 'hardlabel', classerror reads 'label'
    net2 = zoo.ferPlusZoo(modelName, width_mult=0.125, blocks=(1, 1, 1, 1), lossType="softmaxlog", numOutputs=8)
    assert net2.getLayer("loss").block.loss == "softmaxlog"
    assert net2.getLayer("classerror").inputs == ["prediction", "label"]
    assert not any(isinstance(l.block, dagnn.DropOut) for l in net2.layers)       # dropoutRate 0 (default)
    with pytest.raises(ValueError):
        zoo.ferPlusZoo(modelName, width_mult=0.125, blocks=(1, 1, 1, 1), lossType="huber")


def test_get_batch_ferplus_rejects_mixed_sets():
    from mcncrossmodalemotions_amd import batch
    imdb = batch.SyntheticFerPlusImdb(num_images=16, seed=2)
    s = imdb.images["set"]
    mixed = [int(np.nonzero(s == 1)[0][0]), int(np.nonzero(s == 2)[0][0])]
    with pytest.raises(AssertionError, match="mixed"):
        batch.getBatchFerPlus(imdb, mixed)


def test_synthetic_ferplus_imdb():
    from mcncrossmodalemotions_amd import batch
    imdb = batch.SyntheticFerPlusImdb(num_images=40, seed=1, val_fraction=0.25, test_fraction=0.1)
    im = imdb.images
    assert im["data"].shape == (48, 48, 1, 40) and im["data"].dtype == np.float32
    assert im["data"].min() >= 0 and im["data"].max() <= 255 and np.array_equal(im["data"], np.round(im["data"]))
    assert im["votes"].shape == (40, 10) and (im["votes"][:, :8].sum(1) > 0).all()
    assert np.array_equal(im["hardLabels"].ravel(), im["votes"][:, :8].argmax(1) + 1)
    assert sorted(set(im["set"])) == [1, 2, 3] and len(imdb.meta["classes"]) == 10


def test_sampler_operators_reject_host_tensors():
    import torch
    from mcncrossmodalemotions_amd import vl
    x = torch.zeros(4, 4, 1, 1)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        vl.vl_nnbilinearsampler(x, torch.zeros(2, 4, 4, 1))
    with pytest.raises(RuntimeError, match="not on the GPU"):
        vl.vl_nnaffinegrid(torch.zeros(1, 1, 6, 1), (4, 4))
    with pytest.raises(RuntimeError, match="not on the GPU"):
        vl.ferplus_batch(x, torch.zeros(1, 1, 6, 1), None, (0, 0, 0), (4, 4))


def test_sampler_abi_declared_typed_and_exported():
    from mcncrossmodalemotions_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    for name in NEW_ABI:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    L = _lib.load()
    for name in NEW_ABI:
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name]
    assert L.xm_version() >= 107
    # argument counts agree with the header's prototypes
    for name in NEW_ABI:
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
