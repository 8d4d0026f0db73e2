"""GPU: the FER+ teacher-training path (teacher/ferplus_baselines.m) -- the fused xm_ferplus_batch against the standalone
operators and an fp64 restatement, one senet50_ft-dag training step on a getBatchFerPlus batch against the oracle, and
ferplus_baselines end to end (train, checkpoint, resume, evaluate from the best checkpoint)."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_net
from test_gpu_sampler import close, grid_ref, sampler_ref

pytestmark = pytest.mark.gpu

AVG = (131.0912, 103.8827, 91.4953)


def _normalized_rgb(grey, flips):
    """the reference's host loop (:180-186): grey -> x3 minus averageImage -> fliplr"""
    rgb = np.repeat(grey.astype(np.float32), 3, axis=2) - np.asarray(AVG, np.float32).reshape(1, 1, 3, 1)
    for n in np.nonzero(flips)[0]:
        rgb[:, :, :, n] = rgb[:, ::-1, :, n]
    return rgb


def test_ferplus_batch_matches_composition_and_restatement(gpu):
    import torch
    from mcncrossmodalemotions_amd import batch, vl
    N = 128
    imdb = batch.SyntheticFerPlusImdb(num_images=N, seed=4)
    grey = imdb.images["data"]
    rng = np.random.default_rng(8)
    flips = (rng.random(N) > 0.5).astype(np.int32)
    augs = batch.computeAugs(N, rng)
    A = np.stack([batch.affine_params(augs[:, :, i]) for i in range(N)], 1).astype(np.float32)    # 6 x N
    assert flips.any() and not flips.all()
    assert sum(not np.array_equal(augs[:, :, i], np.eye(3)) for i in range(N)) > N // 4
    Ad = vl.from_numpy(A.reshape(1, 1, 6, N))
    fd = torch.from_numpy(flips).cuda()
    out = vl.to_numpy(vl.ferplus_batch(vl.from_numpy(grey), Ad, fd, AVG, (224, 224)))
    assert out.shape == (224, 224, 3, N)
    rgb = _normalized_rgb(grey, flips)
    comp = vl.to_numpy(vl.vl_nnbilinearsampler(vl.from_numpy(rgb), vl.vl_nnaffinegrid(Ad, [224, 224])))
    close(out, comp, 2e-6, "fused vs standalone operators")
    sub = slice(0, 128, 9)                                            # the fp64 restatement on every 9th sample
    ref = sampler_ref(rgb[:, :, :, sub].astype(np.float64), grid_ref(A[:, sub].astype(np.float64), 224, 224))
    close(out[:, :, :, sub], ref, 1e-5, "fused vs fp64 restatement")
    # identity transforms at 48 -> 48: exactly the normalised (and flipped) image
    I6 = np.tile(np.array([1, 0, 0, 1, 0, 0], np.float32), (N, 1)).T.reshape(1, 1, 6, N)
    same = vl.to_numpy(vl.ferplus_batch(vl.from_numpy(grey), vl.from_numpy(I6), fd, AVG, (48, 48)))
    assert np.array_equal(same, rgb)
    same0 = vl.to_numpy(vl.ferplus_batch(vl.from_numpy(grey), vl.from_numpy(I6), None, AVG, (48, 48)))
    assert np.array_equal(same0, _normalized_rgb(grey, np.zeros(N)))


def test_get_batch_ferplus(gpu):
    """draw order (flips, then computeAugs), identity transforms outside training, votes / hard labels"""
    from mcncrossmodalemotions_amd import batch, vl
    imdb = batch.SyntheticFerPlusImdb(num_images=32, seed=6, val_fraction=0.5)
    s = imdb.images["set"]
    tr, va = [int(i) for i in np.nonzero(s == 1)[0][:6]], [int(i) for i in np.nonzero(s == 2)[0][:6]]
    inp = batch.getBatchFerPlus(imdb, tr, rng=np.random.default_rng(3), imageSize=(64, 64))
    assert inp[::2] == ["data", "label", "hardlabel"]
    d = dict(zip(inp[::2], inp[1::2]))
    r = np.random.default_rng(3)
    flips = r.random(6) > 0.5
    augs = batch.computeAugs(6, r)
    A = np.stack([batch.affine_params(augs[:, :, i]) for i in range(6)], 1)
    ref = sampler_ref(_normalized_rgb(imdb.images["data"][:, :, :, tr], flips), grid_ref(A, 64, 64))
    close(vl.to_numpy(d["data"]), ref, 1e-5, "train batch")
    v = imdb.images["votes"][tr, :8]
    close(vl.to_numpy(d["label"]).reshape(8, 6), (v / v.sum(1, keepdims=True)).T, 1e-6, "votes")
    assert np.array_equal(vl.to_numpy(d["hardlabel"]).ravel(), imdb.images["hardLabels"].ravel()[tr])
    # validation: no flips, identity transforms (a plain resize), computeAugs still advances the stream
    rv = np.random.default_rng(5)
    inp = batch.getBatchFerPlus(imdb, va, rng=rv, imageSize=(48, 48), lossType="softmaxlog", dataType="full")
    assert inp[::2] == ["data", "label"]
    assert np.array_equal(vl.to_numpy(inp[1]), _normalized_rgb(imdb.images["data"][:, :, :, va], np.zeros(6)))
    r = np.random.default_rng(5)
    batch.computeAugs(6, r)
    assert rv.random() == r.random()


def test_senet_training_step_on_ferplus_batch_matches_oracle(gpu):
    """one train-mode step of the narrow senet50_ft-dag (finetuneLR, dropout behind the last SE projections, the
    SoftmaxCELoss / classerror heads) on a getBatchFerPlus batch: the data tensor and the dropout masks the HIP step
    drew are handed to the oracle, which reproduces the objective, every parameter derivative and the SGD update with
    the per-layer learning rates."""
    from mcncrossmodalemotions_amd import batch, dagnn, train, vl, zoo
    net = zoo.ferPlusZoo("senet50_ft-dag", seed=11, width_mult=0.125, blocks=(1, 1, 1, 1), finetuneLR=0.1,
                         dropoutRate=0.5, lossType="distributions", numOutputs=8)
    net.getLayer("pool5").block.poolSize = [2, 2]                      # 64 x 64 input (as the teacher step tests)
    imdb = batch.SyntheticFerPlusImdb(num_images=16, seed=12)
    idx = [int(i) for i in np.nonzero(imdb.images["set"] == 1)[0][:4]]
    inputs = batch.getBatchFerPlus(imdb, idx, rng=np.random.default_rng(2), imageSize=(64, 64),
                                   averageImage=net.meta["normalization"]["averageImage"])
    P0 = oracle_net.host_params(net)
    net.pack_params()
    net.mode = "normal"
    net.eval(inputs, ["objective", 1])
    d = {k: vl.to_numpy(v) for k, v in zip(inputs[::2], inputs[1::2])}
    drops = [l for l in net.layers if isinstance(l.block, dagnn.DropOut)]
    assert len(drops) == 2
    masks = {l.name + ".mask": vl.to_numpy(l.block.mask) for l in drops}
    V = oracle_net.forward(net, dict(d, **masks), P0, mode="normal")
    _, DP = oracle_net.backward(net, V, {"objective": np.float32(1)}, P0, mode="normal")
    close(vl.to_numpy(net.vars["objective"].value).ravel()[0], V["objective"], 1e-4, "objective")
    close(vl.to_numpy(net.vars["classerror"].value).ravel()[0], V["classerror"], 0, "classerror")
    for name, ref in DP.items():
        close(vl.to_numpy(net.params[name].der).reshape(ref.shape, order="F"), ref, 5e-4, "der " + name)
    N = 4
    train.accumulate_gradients(net, train.TrainOpts(batchSize=N), 0.01, N, 1)
    lrs = set()
    for name, p in net.params.items():
        lrs.add(p.learningRate)
        if p.trainMethod == "average":
            ref = O.average_update(P0[name], DP[name], p.learningRate, 1)
        else:
            ref, _ = O.sgd_update(P0[name], np.zeros_like(P0[name]), DP[name].reshape(P0[name].shape, order="F"),
                                  0.01 * p.learningRate, 0.9, 5e-4 * p.weightDecay, N)
        close(vl.to_numpy(p.value), ref, 1e-5, "sgd " + name)
    assert lrs == {0.1, 1.0, 2.0}


def test_ferplus_baselines_train_resume_evaluate(gpu, tmp_path):
    import torch
    from mcncrossmodalemotions_amd import batch, train
    from mcncrossmodalemotions_amd.ferplus_baselines import ferplus_baselines
    imdb = batch.SyntheticFerPlusImdb(num_images=24, seed=1)
    kw = dict(imdb=imdb, expRoot=str(tmp_path), widthMult=0.125, blocks=(1, 1, 1, 1), batchSize=8,
              learningRate=[0.01, 0.01, 0.001])
    net, info = ferplus_baselines(numEpochs=2, **kw)
    expDir = os.path.join(str(tmp_path), "senet50_ft-dag-distributions-CNTK-dropout-0.5-aug")
    assert sorted(os.listdir(expDir)) == ["net-epoch-1.pt", "net-epoch-2.pt"]
    assert len(info["train"]) == 2 and len(info["val"]) == 2
    for st in info["train"] + info["val"]:
        assert np.isfinite(st["objective"]) and 0 <= st["classerror"] <= 1
    assert info["train"][0]["num"] == int((imdb.images["set"] == 1).sum())
    # parameters moved, grouped by the per-layer learning rates (finetuneLR 0.1 on the body, the classifier's own)
    keys = {k for k, a, b in net._flat.segments if b > a}
    assert ("gradient", 0.1, 1.0) in keys and ("gradient", 1.0, 1.0) in keys and ("gradient", 2.0, 0.0) in keys
    ck1 = torch.load(os.path.join(expDir, "net-epoch-1.pt"), weights_only=True)
    for name, p in net.params.items():
        if p.trainMethod == "gradient":
            moved = not torch.equal(ck1["params"][name].cpu(), p.value.permute(*reversed(range(p.value.dim())))
                                    .contiguous().reshape(ck1["params"][name].shape).cpu())
            assert moved, name
    # continue: resumes from net-epoch-2 and runs epoch 3 only
    net3, info3 = ferplus_baselines(numEpochs=3, **kw)
    assert len(info3["train"]) == 3 and info3["train"][:2] == info["train"]
    assert sorted(os.listdir(expDir)) == ["net-epoch-1.pt", "net-epoch-2.pt", "net-epoch-3.pt"]
    # evaluate only, from the best checkpoint: reloads it, writes nothing
    stamp = {f: os.stat(os.path.join(expDir, f)).st_mtime_ns for f in os.listdir(expDir)}
    val_err = [info3["val"][e]["classerror"] for e in range(3)]
    best = int(np.argmin(val_err)) + 1
    neve, infoe = ferplus_baselines(numEpochs=3, evaluateOnly={"subset": "val", "fromCkpt": True}, **kw)
    assert {f: os.stat(os.path.join(expDir, f)).st_mtime_ns for f in os.listdir(expDir)} == stamp
    assert len(infoe["val"]) == 1 and infoe["train"][0]["num"] == 0
    ckb = torch.load(os.path.join(expDir, "net-epoch-%d.pt" % best), weights_only=True)
    for name, p in neve.params.items():
        got = p.value.permute(*reversed(range(p.value.dim()))).contiguous().reshape(ckb["params"][name].shape)
        assert torch.equal(got.cpu(), ckb["params"][name].cpu()), name
    assert imdb.images["set"].min() >= 1 and (imdb.images["set"] == 1).any()      # the caller's imdb is unchanged
    # a second identical evaluation gives the same validation statistics (nothing was updated)
    _, infoe2 = ferplus_baselines(numEpochs=3, evaluateOnly={"subset": "val", "fromCkpt": True}, **kw)
    assert infoe2["val"][0]["objective"] == pytest.approx(infoe["val"][0]["objective"], rel=1e-6)
    del train


@pytest.mark.parametrize("Ho,Wo", [(50, 37), (7, 9), (1, 5)])
def test_ferplus_batch_any_output_size(gpu, Ho, Wo):
    """output heights that are not a multiple of four (the one-pixel-per-thread kernel) against the standalone pair"""
    import torch
    from mcncrossmodalemotions_amd import batch, vl
    N = 6
    imdb = batch.SyntheticFerPlusImdb(num_images=N, seed=Ho)
    rng = np.random.default_rng(Wo)
    flips = (np.arange(N) % 2).astype(np.int32)
    augs = batch.computeAugs(N, rng)
    A = np.stack([batch.affine_params(augs[:, :, i]) for i in range(N)], 1).astype(np.float32)
    Ad = vl.from_numpy(A.reshape(1, 1, 6, N))
    out = vl.to_numpy(vl.ferplus_batch(vl.from_numpy(imdb.images["data"]), Ad, torch.from_numpy(flips).cuda(), AVG,
                                       (Ho, Wo)))
    rgb = _normalized_rgb(imdb.images["data"], flips)
    comp = vl.to_numpy(vl.vl_nnbilinearsampler(vl.from_numpy(rgb), vl.vl_nnaffinegrid(Ad, [Ho, Wo])))
    close(out, comp, 2e-6, "fused vs standalone %dx%d" % (Ho, Wo))
