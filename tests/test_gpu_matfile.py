"""Model files on the device: a loaded graph must reach the fused HIP plans and give their results exactly,
whatever the file calls its layers and in whatever order it lists them.

The nets are the narrow zoo ones (1/8 width, one block per stage) on 2 inputs of the full geometry -- 224 x 224 x 3 faces,
512 x 100 spectrograms --, the smallest at which the stem fusion, the SE tail fusion and the pool6 bucket engage."""
import glob
import os

import numpy as np
import pytest
import scipy.io as sio

import test_matfile_cpu as MC

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ numpy reference
def np_forward(P, x):
    """float64 evaluation of the hand-written graph of tests/test_matfile_cpu.py: conv 3x3 pad 1 -> test-mode bnorm from
    the stored moments (column 2 is sigma) -> relu -> max pool 2x2 / 2 -> full-size conv -> softmax -> softmaxlog loss"""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    Hh, Ww, _, Nn = x.shape
    K = P["c1f"].shape[3]
    xp = np.zeros((Hh + 2, Ww + 2) + x.shape[2:])
    xp[1:-1, 1:-1] = x
    x1 = np.zeros((Hh, Ww, K, Nn))
    for i in range(Hh):
        for j in range(Ww):
            for k in range(K):
                for n in range(Nn):
                    x1[i, j, k, n] = P["c1b"][k, 0] + np.sum(xp[i:i + 3, j:j + 3, :, n] * P["c1f"][:, :, :, k])
    mu, sigma = P["bn1x"][:, 0], P["bn1x"][:, 1]
    x2 = P["bn1m"][:, 0][None, None, :, None] * (x1 - mu[None, None, :, None]) / sigma[None, None, :, None] \
        + P["bn1b"][:, 0][None, None, :, None]
    x3 = np.maximum(x2, 0)
    x4 = np.zeros((Hh // 2, Ww // 2, K, Nn))
    for i in range(Hh // 2):
        for j in range(Ww // 2):
            x4[i, j] = x3[2 * i:2 * i + 2, 2 * j:2 * j + 2].max((0, 1))
    scores = np.zeros((1, 1, 1, Nn))
    for n in range(Nn):
        scores[0, 0, 0, n] = P["fcb"][0, 0] + np.sum(x4[:, :, :, n] * P["fcf"][:, :, :, 0])
    e = np.exp(scores - scores.max(2, keepdims=True))
    probs = e / e.sum(2, keepdims=True)
    # vl_nnloss 'softmaxlog' on probs with label 1: sum over the samples of log(sum_c exp(p_c)) - p_label
    objective = float(np.sum(np.log(np.exp(probs).sum(2)) - probs[:, :, 0, :]))
    return {"x4": x4, "scores": scores, "probs": probs, "objective": objective}


def test_handwritten_file_against_numpy(gpu, tmp_path):
    from mcncrossmodalemotions_amd import dagnn, vl
    spec, truth = MC.handwritten_spec(seed=3)
    net = dagnn.load_mat(MC.write_spec(tmp_path / "hand.mat", spec))
    rng = np.random.default_rng(4)
    x = rng.standard_normal((MC.H, MC.W, MC.C0, MC.N)).astype(np.float32)
    ref = np_forward(truth, x.astype(np.float64))
    net.move("gpu")
    net.mode = "test"
    for v in ("scores", "probs"):
        net.vars[v].precious = True            # x4 is precious in the file
    net.eval(["input", vl.from_numpy(np.asfortranarray(x)), "label", vl.from_numpy(np.ones((1, 1, 1, MC.N), np.float32))])
    assert "_ConvFoldStep" in MC.plan_classes(net, False)
    for v in ("x4", "scores", "probs"):
        got = vl.to_numpy(net.vars[v].value).astype(np.float64).reshape(ref[v].shape, order="F")
        err, scale = float(np.abs(got - ref[v]).max()), max(1.0, float(np.abs(ref[v]).max()))
        print("%s: max err %.3e, allowance %.3e" % (v, err, 1e-4 * scale))
        assert err <= 1e-4 * scale, v
    assert float(np.abs(ref["x4"]).max()) > 0.5 and float(np.abs(ref["scores"]).max()) > 0.1       # not a trivial case
    obj = float(vl.to_numpy(net.vars["objective"].value).ravel()[0])
    print("objective: %.3e (ref %.3e)" % (obj, ref["objective"]))
    assert abs(obj - ref["objective"]) <= 1e-4 * max(1.0, abs(ref["objective"]))


# ------------------------------------------------------------------------------------------------ same plan, same bits
def _student():
    from mcncrossmodalemotions_amd import zoo
    return zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=5)


def _teacher_ft():
    from mcncrossmodalemotions_amd import zoo
    return zoo.ferPlusZoo("senet50_ft-dag", seed=7, width_mult=0.125, blocks=(1, 1, 1, 1), dropoutRate=0.5)


def _inputs(which, rng):
    from mcncrossmodalemotions_amd import vl
    if which == "student":
        data = vl.from_numpy(np.asfortranarray(rng.standard_normal((512, 100, 1, 2)).astype(np.float32)))
        lgo = np.asfortranarray((rng.standard_normal((1, 1, 8, 2)) * 3).astype(np.float32))
        lab = np.asfortranarray((lgo.reshape(8, 2).argmax(0).reshape(1, 1, 1, 2) + 1).astype(np.float32))
        return {"data": data, "logitTarget": vl.from_numpy(lgo), "maxLabel": vl.from_numpy(lab)}
    faces = np.asfortranarray((rng.standard_normal((224, 224, 3, 2)) * 40).astype(np.float32))
    p = rng.uniform(0.05, 1, (1, 1, 7, 2))
    label = np.asfortranarray((p / p.sum(2, keepdims=True)).astype(np.float32))
    hard = np.asfortranarray((label.reshape(7, 2).argmax(0).reshape(1, 1, 1, 2) + 1).astype(np.float32))
    return {"data": vl.from_numpy(faces), "label": vl.from_numpy(label), "hardlabel": vl.from_numpy(hard)}


def _bits(t):
    from mcncrossmodalemotions_amd import vl
    return vl.to_numpy(t).view(np.uint32)


@pytest.mark.parametrize("which", ["student", "teacher"])
def test_renamed_shuffled_file_runs_the_same_plan(gpu, which, tmp_path):
    """save -> rename every layer, variable and parameter -> shuffle the layers -> load: the same step classes in the same
    order, bit-identical test-mode outputs and bit-identical parameter derivatives of one training eval.  Fails when
    loading defeats a fusion: the SE fold, the conv + bnorm (+ sum) (+ relu) fold, the stem, the fused SE tail backward."""
    from mcncrossmodalemotions_amd import dagnn
    net = _student() if which == "student" else _teacher_ft()
    s, vmap, pmap = MC.renamed_and_shuffled(net, seed=11)
    path = str(tmp_path / "renamed.mat")
    sio.savemat(path, s)
    back = dagnn.load_mat(path)
    assert set(back.params).isdisjoint(net.params) and "prediction" not in back.vars and back.getLayer("pool6") is None
    inputs = _inputs(which, np.random.default_rng(6))
    for n, m in ((net, None), (back, vmap)):
        n.pack_params()
        n.vars[(m or {}).get("prediction", "prediction")].precious = True
    drops = [l.block for l in net.layers if isinstance(l.block, dagnn.DropOut)]
    assert len(drops) == (2 if which == "teacher" else 0)
    assert [l.block.seed for l in back.layers if isinstance(l.block, dagnn.DropOut)] == [b.seed for b in drops]

    def run(n, m, training):
        name = (lambda v: m[v]) if m else (lambda v: v)
        n.mode = "normal" if training else "test"
        n.eval({name(k): t for k, t in inputs.items()}, {name("objective"): 1} if training else None)
        out = _bits(n.vars[name("prediction")].value).copy()
        ders = {k: _bits(p.der).copy() for k, p in n.params.items()} if training else None
        return out, ders

    for training in (False, True):      # first use of every shape: the library times its tile configurations here
        run(net, None, training)
    for b in drops:
        b._offset = 0                   # the mask stream starts over, as it does for the loaded net
    for training in (False, True):
        a_cls, b_cls = MC.plan_classes(net, training), MC.plan_classes(back, training)
        assert a_cls == b_cls
        out_a, der_a = run(net, None, training)
        out_b, der_b = run(back, vmap, training)
        assert np.array_equal(out_a, out_b), ("prediction", training)
        if training:
            assert sorted(der_b) == sorted(pmap[k] for k in der_a)
            for k, d in der_a.items():
                assert d.shape == der_b[pmap[k]].shape and np.array_equal(d, der_b[pmap[k]]), k
            assert sum(int(np.any(d)) for d in der_a.values()) > len(der_a) // 2        # derivatives did flow
    back.mode = "test"
    fused = set(MC.plan_classes(back, False)) | set(MC.plan_classes(back, True))
    assert fused >= ({"_ConvFoldStep", "_BnReluPoolStep", "_BnReluStep"} if which == "student" else
                     {"_SEFoldStep", "_ConvFoldStep", "_SEBnTrainStep", "_AddReluStep", "_BnReluPoolStep"})


# ------------------------------------------------------------------------------------------------ the teacher from a file
def _framed_imdb(num_tracks, seed):
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe
    syn = batch.SyntheticEmoVoxImdb(num_tracks=num_tracks, seed=seed, min_seconds=1.0, max_seconds=1.5)
    src = fe.src_imdb(syn)
    frames = batch.SyntheticDenseFrames(src, seed=seed, frameSize=(240, 230))
    return fe.addFramesToImdb(src, frames.lister, find=frames.find), frames


def test_frozen_teacher_from_a_model_file(gpu, tmp_path):
    from mcncrossmodalemotions_amd import dagnn, fetch_emovoxceleb_imdb as fe, vl, zoo
    build = lambda: zoo.ferPlusZoo("senet50-ferplus", seed=7, width_mult=0.125, blocks=(1, 1, 1, 1))
    dagnn.save_mat(build(), str(tmp_path / "senet50-ferplus.mat"))
    imdb, frames = _framed_imdb(4, 5)
    assert len(imdb.images["id"]) == 4
    want = fe.buildImdb(build(), imdb, frames, batchSize=16)            # the net the file was written from
    loaded = zoo.ferPlusZoo("senet50-ferplus", modelDir=str(tmp_path))
    teacher, size, avg = fe._as_teacher(loaded, 2)
    assert isinstance(teacher, zoo.FrozenTeacher) and size == (224, 224) and list(avg) == [131.0912, 103.8827, 91.4953]
    assert "_SEFoldStep" in MC.plan_classes(loaded, False)
    got = fe.buildImdb(teacher, imdb, frames, batchSize=16)
    assert len(got.wavLogits) == len(want.wavLogits) == 4
    for a, b in zip(got.wavLogits, want.wavLogits):
        assert a.shape == b.shape and a.shape[0] > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.std(np.concatenate(want.wavLogits, 0), 0).min() > 0
    # ... and through fetch_emovoxceleb_imdb, which builds the teacher itself
    fetched = fe.fetch_emovoxceleb_imdb("senet50-ferplus", imdbDir=str(tmp_path / "feats"), imdb=imdb, frames=frames,
                                        modelDir=str(tmp_path), verbose=False, batchSize=16)
    for a, b in zip(fetched.wavLogits, want.wavLogits):
        assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), b.view(np.uint32))
    with pytest.raises(FileNotFoundError, match="resnet50-ferplus.mat"):
        fe.fetch_emovoxceleb_imdb("resnet50-ferplus", imdbDir=str(tmp_path / "feats"), imdb=imdb, frames=frames,
                                  modelDir=str(tmp_path), verbose=False)


# ------------------------------------------------------------------------------------------------ the student from a file
def test_distillation_starts_from_the_file(gpu, tmp_path, monkeypatch):
    """run_distillation(modelDir, fromScratch=False): one mini-epoch of two batches from the saved student; every step's
    loss is that of the same run on the in-memory net the file was written from; a checkpoint is written as before"""
    from mcncrossmodalemotions_amd import batch as xbatch, dagnn, train, zoo
    from mcncrossmodalemotions_amd.run_distillation import run_distillation
    dagnn.save_mat(_student(), str(tmp_path / "emovoxceleb-student.mat"))
    losses = []
    inner = train.train_step

    def spy(net, *a, **kw):
        inner(net, *a, **kw)
        losses[-1].append(float(net.getLayer("loss").block.lastValue.reshape(-1)[0].item()))

    monkeypatch.setattr(train, "train_step", spy)

    def go(tag, **kw):
        imdb = xbatch.SyntheticEmoVoxImdb(num_tracks=16, seed=0, num_emotions=8, min_seconds=1.5, max_seconds=6.0,
                                          val_fraction=0.25)
        ntrain = sum(1 for s in imdb.set if s == 1)
        assert ntrain > 8
        losses.append([])
        return run_distillation(gpus=[0], numSeconds=1, batchSize=4, numEpochs=1, miniEpochRatio=8.5 / ntrain, miniVal=0.5,
                                imdb=imdb, widthMult=0.125, dataDir=str(tmp_path / tag), learningRate=[1e-3], cont=False,
                                fromScratch=False, **kw)

    go("first", modelDir=str(tmp_path))             # first use of every shape: the library times its tile configurations
    del losses[:]
    net, info = go("file", modelDir=str(tmp_path))
    assert info["train"][0]["num"] == 8 and len(losses[0]) == 2
    assert all(isinstance(p.value, __import__("torch").Tensor) for p in net.params.values())
    assert len(glob.glob(os.path.join(str(tmp_path / "file"), "*", "net-epoch-1.pt"))) == 1
    memory = _student()
    monkeypatch.setattr(zoo, "emoVoxZoo", lambda *a, **kw: memory)
    _, info2 = go("memory")
    assert len(losses[1]) == 2 and np.isfinite(losses[0]).all() and losses[0][0] > 0
    assert losses[0][0] == losses[1][0]                        # it started from the file's weights
    assert losses[0] == losses[1] and info["train"][0]["objective"] == info2["train"][0]["objective"]
    assert losses[0][0] != losses[0][1]
