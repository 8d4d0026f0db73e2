"""GPU end-to-end parity: whole graphs (student step, teachers) through the dagnn mirror over the
HIP C ABI vs the same graphs executed by the CPU oracle."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_net

pytestmark = pytest.mark.gpu


def close(a, b, tol, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, "%s: max err %.3e > %.1e * %.3g" % (what, err, tol, scale)


def _student_inputs(rng, W, N):
    spec = np.abs(rng.standard_normal((512, W, 1, N))).astype(np.float32)
    data = O.spec_rownorm(O.F(spec))
    lgo = O.F(rng.standard_normal((1, 1, 8, N)) * 3)
    lab = O.F(lgo.reshape(8, N).argmax(0).reshape(1, 1, 1, N) + 1)
    return data, lgo, lab


@pytest.mark.parametrize("fuse", [False, True])
def test_student_step_matches_oracle(gpu, fuse):
    """VGGVox student (1/8 width, full 512x100 geometry): forward, loss, every parameter
    derivative and the SGD update against the oracle (fp64-accumulate)."""
    from mcncrossmodalemotions_amd import vl, zoo, train
    rng = np.random.default_rng(21)
    N, W = 4, 100
    net = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=5)
    net.fuse = fuse
    P0 = oracle_net.host_params(net)
    data, lgo, lab = _student_inputs(rng, W, N)
    V = oracle_net.forward(net, {"data": data, "logitTarget": lgo, "maxLabel": lab}, P0, mode="normal")
    _, DP = oracle_net.backward(net, V, {"objective": np.float32(1)}, P0, mode="normal")
    net.pack_params()
    inputs = ["data", vl.from_numpy(data), "logitTarget", vl.from_numpy(lgo), "maxLabel", vl.from_numpy(lab)]
    net.vars["prediction"].precious = True
    net.mode = "normal"
    net.eval(inputs, ["objective", 1])
    close(vl.to_numpy(net.vars["prediction"].value), V["prediction"], 1e-4, "prediction")
    close(vl.to_numpy(net.vars["objective"].value).ravel()[0], V["objective"], 1e-5, "objective")
    close(vl.to_numpy(net.vars["classerror"].value).ravel()[0], V["classerror"], 0, "classerror")
    for name, ref in DP.items():
        got = vl.to_numpy(net.params[name].der)
        # gradients: relative to the largest entry of that parameter's gradient
        close(got.reshape(ref.shape, order="F"), ref, 2e-4, "der " + name)
    # SGD step (cnn_train_dag defaults): compare updated weights
    opts = train.TrainOpts(batchSize=N)
    train.accumulate_gradients(net, opts, 1e-4, N, 1)
    for name, p in net.params.items():
        if p.trainMethod == "average":
            ref = O.average_update(P0[name], DP[name], p.learningRate, 1)
        else:
            ref, _ = O.sgd_update(P0[name], np.zeros_like(P0[name]), DP[name].reshape(P0[name].shape, order="F"),
                                  1e-4 * p.learningRate, 0.9, 5e-4 * p.weightDecay, N)
        close(vl.to_numpy(p.value), ref, 1e-5, "sgd " + name)


def test_student_step_with_dropout(gpu):
    """emoVoxZoo(..., 'dropout', 0.5) (emoVoxZoo.m:18,116-135): training-mode dagnn.DropOut behind fc6 and fc7.  The
    masks the HIP step drew are the documented stream (seed = layer index + 1, offsets advancing per call), and with
    those masks as inputs the oracle reproduces prediction, loss and every parameter derivative; a second step draws
    different masks; test mode is the identity."""
    from mcncrossmodalemotions_amd import dagnn, vl, zoo
    rng = np.random.default_rng(23)
    N, W = 4, 100
    net = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=5, dropout=0.5)
    drops = [l for l in net.layers if isinstance(l.block, dagnn.DropOut)]
    assert [l.name for l in drops] == ["fc6_drop", "fc7_drop"]
    P0 = oracle_net.host_params(net)
    data, lgo, lab = _student_inputs(rng, W, N)
    net.pack_params()
    inputs = ["data", vl.from_numpy(data), "logitTarget", vl.from_numpy(lgo), "maxLabel", vl.from_numpy(lab)]
    net.vars["prediction"].precious = True
    net.mode = "normal"
    net.eval(inputs, ["objective", 1])
    masks = {}
    for l in drops:
        m = vl.to_numpy(l.block.mask)
        assert np.array_equal(m, O.dropout_mask(m.shape, 0.5, l.block.seed, 0)), l.name
        masks[l.name + ".mask"] = m
    ins = dict({"data": data, "logitTarget": lgo, "maxLabel": lab}, **masks)
    V = oracle_net.forward(net, ins, P0, mode="normal")
    _, DP = oracle_net.backward(net, V, {"objective": np.float32(1)}, P0, mode="normal")
    close(vl.to_numpy(net.vars["prediction"].value), V["prediction"], 1e-4, "prediction")
    close(vl.to_numpy(net.vars["objective"].value).ravel()[0], V["objective"], 1e-5, "objective")
    for name, ref in DP.items():
        close(vl.to_numpy(net.params[name].der).reshape(ref.shape, order="F"), ref, 2e-4, "der " + name)
    first = {l.name: vl.to_numpy(l.block.mask) for l in drops}
    net.eval(inputs, ["objective", 1])
    for l in drops:
        m = vl.to_numpy(l.block.mask)
        assert not np.array_equal(m, first[l.name])
        assert np.array_equal(m, O.dropout_mask(m.shape, 0.5, l.block.seed, (m.size + 3) // 4))
    net.mode = "test"
    net.eval(inputs)
    Vt = oracle_net.forward(net, {"data": data, "logitTarget": lgo, "maxLabel": lab}, P0, mode="test")
    close(vl.to_numpy(net.vars["prediction"].value), Vt["prediction"], 1e-4, "test-mode prediction")
    # round-4 advisor: the counter offsets are training state (a resumed run continues the mask sequence instead of
    # repeating it), and a data-parallel worker folds its rank into the seed (no two shards share masks)
    import os
    import tempfile
    from mcncrossmodalemotions_amd import train
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "net-epoch-1.pt")
        train.save_checkpoint(net, path, {}, 1)
        offs = {l.name: l.block._offset for l in drops}
        assert all(v == 2 * ((first[k].size + 3) // 4) for k, v in offs.items()), offs
        net2 = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=5, dropout=0.5)
        net2.pack_params()
        train.load_checkpoint(net2, path)
        assert {l.name: l.block._offset for l in net2.layers if isinstance(l.block, dagnn.DropOut)} == offs
    net.mode = "normal"
    net.workerRank = 1
    net.eval(inputs, ["objective", 1])
    for l in drops:
        m = vl.to_numpy(l.block.mask)
        assert not np.array_equal(m, O.dropout_mask(m.shape, 0.5, l.block.seed, offs[l.name])), l.name
        assert np.array_equal(m, O.dropout_mask(m.shape, 0.5, (l.block.seed + 0x9E3779B1) & 0x7FFFFFFF, offs[l.name]))


def test_pool6_buckets_on_device(gpu):
    """emoVoxZoo.m:258-259: every clip width bucket yields a 1 x 1 x C pool6 output."""
    from mcncrossmodalemotions_amd import vl, zoo
    rng = np.random.default_rng(2)
    for W in (100, 300, 700, 1000):
        net = zoo.emoVoxZoo(numSeconds=W / 100, width_mult=0.0625, scratch=0)
        net.move("gpu")
        net.mode = "test"
        net.vars["x_pool6"].precious = True
        net.eval(["data", vl.from_numpy(O.F(rng.standard_normal((512, W, 1, 1))))])
        assert tuple(net.vars["x_pool6"].value.shape[:2]) == (1, 1), W


@pytest.mark.parametrize("name", ["resnet50-ferplus", "senet50-ferplus"])
def test_teacher_forward_matches_oracle(gpu, name):
    """Frozen teacher in test mode (fetch_emovoxceleb_imdb.m:98-131), 1/8 width, one block per
    stage, 64x64 input; folded conv+bn+sum+relu plan vs unfused plan vs oracle."""
    from mcncrossmodalemotions_amd import vl, zoo
    rng = np.random.default_rng(33)
    net = zoo.ferPlusZoo(name, seed=7, width_mult=0.125, blocks=(2, 1, 1, 1))
    zoo.strip_losses(net)
    # 64x64 input -> pool5 sees 2x2: shrink the window like a smaller imageSize would
    net.getLayer("pool5").block.poolSize = [2, 2]
    net.mode = "test"
    x = O.F(rng.standard_normal((64, 64, 3, 3)) * 40)
    V = oracle_net.forward(net, {"data": x}, mode="test")
    net.move("gpu")
    net.vars["prediction"].precious = True
    outs = {}
    for fuse in (False, True):
        net.fuse = fuse
        net._plan_key = None
        net.eval(["data", vl.from_numpy(x)])
        outs[fuse] = vl.to_numpy(net.vars["prediction"].value)
        close(outs[fuse], V["prediction"], 1e-4, "%s logits fuse=%s" % (name, fuse))
    close(outs[True], outs[False], 1e-5, "fused vs unfused")


def test_frozen_teacher_lanes_match_single_stream(gpu):
    """zoo.FrozenTeacher (fetch_emovoxceleb_imdb.m:98-136): sample slices on two / three HIP streams
    give the logits of the one-stream evaluation and of the oracle (uneven split included)."""
    from mcncrossmodalemotions_amd import vl, zoo
    rng = np.random.default_rng(35)
    net = zoo.ferPlusZoo("senet50-ferplus", seed=8, width_mult=0.125, blocks=(1, 1, 1, 1))
    zoo.strip_losses(net)
    net.getLayer("pool5").block.poolSize = [2, 2]
    net.mode = "test"
    x = O.F(rng.standard_normal((64, 64, 3, 7)) * 40)
    V = oracle_net.forward(net, {"data": x}, mode="test")
    net.move("gpu")
    xd = vl.from_numpy(x)
    one = vl.to_numpy(zoo.FrozenTeacher(net, lanes=1).logits(xd))
    close(one, V["prediction"], 1e-4, "single lane vs oracle")
    for lanes in (2, 3):
        ft = zoo.FrozenTeacher(net, lanes=lanes)
        for _ in range(2):  # second call reuses plans / replicas
            got = vl.to_numpy(ft.logits(xd))
        assert got.shape == one.shape
        # (not bit-identical: the slices select other tile configurations / split-K factors, and the SE squeeze of a
        # small slice takes the skinny-FC kernel instead of the GEMM -- other summation orders, fp32 round-off level)
        close(got, one, 3e-5, "%d lanes vs single" % lanes)
        close(got, V["prediction"], 1e-4, "%d lanes vs oracle" % lanes)
    net.mode = "normal"
    with pytest.raises(ValueError):
        zoo.FrozenTeacher(net)


def test_teacher_training_backward(gpu):
    """config-5 precedent (ferplus_baselines.m:140): SE teacher fwd+bwd in train mode."""
    from mcncrossmodalemotions_amd import vl, zoo
    rng = np.random.default_rng(44)
    net = zoo.ferPlusZoo("senet50-ferplus", seed=9, width_mult=0.125, blocks=(1, 1, 1, 1))
    net.removeLayer("top1error")
    net.getLayer("pool5").block.poolSize = [2, 2]
    x = O.F(rng.standard_normal((64, 64, 3, 4)) * 40)
    lab = O.F(rng.integers(1, 9, (1, 1, 1, 4)))
    P0 = oracle_net.host_params(net)
    V = oracle_net.forward(net, {"data": x, "label": lab}, P0, mode="normal")
    _, DP = oracle_net.backward(net, V, {"objective": np.float32(1)}, P0, mode="normal")
    net.pack_params()
    net.mode = "normal"
    net.eval(["data", vl.from_numpy(x), "label", vl.from_numpy(lab)], ["objective", 1])
    close(vl.to_numpy(net.vars["objective"].value).ravel()[0], V["objective"], 1e-4, "objective")
    for name, ref in DP.items():
        got = vl.to_numpy(net.params[name].der)
        close(got.reshape(ref.shape, order="F"), ref, 5e-4, "der " + name)


def test_batch_provider(gpu):
    from mcncrossmodalemotions_amd import vl, batch
    imdb = batch.SyntheticEmoVoxImdb(num_tracks=16, seed=3)
    rng = np.random.default_rng(0)
    inputs = batch.getBatchEmoVoxCeleb(imdb, range(8), imageSize=(512, 300), rng=rng)
    d = dict(zip(inputs[::2], inputs[1::2]))
    assert tuple(d["data"].shape) == (512, 300, 1, 8)
    assert tuple(d["logitTarget"].shape) == (1, 1, 8, 8) and tuple(d["maxLabel"].shape) == (1, 1, 1, 8)
    data = vl.to_numpy(d["data"])
    # rows are zero-mean / unit (unbiased) std over time: getBatchEmoVoxCeleb.m:164-169
    assert np.abs(data.mean(1)).max() < 1e-4 and np.abs(data.std(1, ddof=1) - 1).max() < 1e-3
    # replay the host-side window arithmetic and check the aggregated targets against the oracle
    rng = np.random.default_rng(0)
    lg = vl.to_numpy(d["logitTarget"]).reshape(8, 8)
    for k in range(8):
        total = min(int(imdb.num_samples[k]), int(19.9 * 16000))
        aud = batch.aud_samples(300)
        wd = total - int(round(aud))
        wr = int(rng.integers(1, wd + 1)) if wd >= 1 else 1       # wr = randi(wd): 1-based (:109-114)
        s, e = O.time2idx(wr / 16000), O.time2idx((wr + aud - 1) / 16000)
        e = min(e, imdb.wavLogits[k].shape[0])
        ref = O.aggregate_logits(imdb.wavLogits[k], s, e, "max")
        rng.integers(0, 2 ** 31) if k == 7 else None
        assert np.abs(lg[:, k] - ref).max() < 1e-6
    # waveform path: crop -> runSpec -> row normalisation, against the oracle's float64 FFT
    rng = np.random.default_rng(1)
    inp2 = batch.getBatchEmoVoxCeleb(imdb, [2, 5], imageSize=(512, 100), rng=rng, use_wav=True)
    rng = np.random.default_rng(1)
    for k, ii in enumerate([2, 5]):
        L = int(round(batch.aud_samples(100)))
        wd = min(int(imdb.num_samples[ii]), int(19.9 * 16000)) - L
        wr = int(rng.integers(1, wd + 1)) if wd >= 1 else 1
        w = imdb.device_wav(ii, inp2[1].device)[wr - 1:wr - 1 + L].cpu().numpy()   # audioread(f, [wr wr+L-1])
        ref = O.spec_rownorm(O.run_spec(w))
        close(vl.to_numpy(inp2[1])[:, :, 0, k], ref[:, :, 0, 0], 1e-3, "wav front-end sample %d" % k)
    faces = batch.getImageBatch(4)
    f = vl.to_numpy(faces)
    assert f.shape == (224, 224, 3, 4)
    # the three channels differ only by the mean offset (fetch_emovoxceleb_imdb.m:176-193)
    assert np.abs((f[:, :, 0] - f[:, :, 1]) - (103.8827 - 131.0912)).max() < 1e-3


@pytest.mark.parametrize("transformation", ["IS", "IN", "ISN", "ISNv"])
def test_batch_provider_speed_and_noise_augmentation(gpu, transformation):
    """getBatchEmoVoxCeleb.m:102-135,217-245: 'S' reads a window of round(audSamp * speedR) samples, speedR = 0.95 +
    0.1 rand, and resamples it by round(fs / speedR) / fs; 'N' adds Nratio = rand * noisevol times a random stretch of a
    random noise file; 'v' (validation) switches both off.  The device path (xm_resample with the host-designed filter,
    xm_scale_axpy, runSpec, row normalisation) against the oracle's float64 composition on the replayed draws; the
    logit rows follow [wr, wr + audSamp) as upstream."""
    from mcncrossmodalemotions_amd import batch, vl
    imdb = batch.SyntheticEmoVoxImdb(num_tracks=6, seed=9, min_seconds=2.5, max_seconds=6.0)
    idx = [1, 4, 5]
    W = 100
    aud = batch.aud_samples(W)
    L = int(round(aud))
    rng = np.random.default_rng(77)
    inp = batch.getBatchEmoVoxCeleb(imdb, idx, imageSize=(512, W), rng=rng, use_wav=True, transformation=transformation)
    d = {inp[i]: inp[i + 1] for i in range(0, len(inp), 2)}
    im, lg = vl.to_numpy(d["data"]), vl.to_numpy(d["logitTarget"]).reshape(8, len(idx))
    chspeed, _, noisy = batch.findSettings(transformation)
    assert (chspeed, noisy) == ("S" in transformation and "v" not in transformation,
                                "N" in transformation and "v" not in transformation)
    rng = np.random.default_rng(77)
    fs = 16000
    for k, ii in enumerate(idx):
        total = min(int(imdb.num_samples[ii]), int(19.9 * fs))
        wav = imdb.device_wav(ii, d["data"].device).cpu().numpy().astype(np.float64)
        if chspeed:
            speedR = 0.95 + float(rng.random()) * 0.1
            audR = int(round(aud * speedR))
            wr = int(rng.integers(1, total - audR + 1))
            z = O.resample(wav[wr - 1:wr - 1 + audR], int(round(fs / speedR)), fs)
            assert abs(z.size - L) <= 1
            z = np.concatenate([z, np.zeros(max(0, L - z.size))])[:L]
            nlen = min(-(-audR * int(round(fs / speedR)) // fs), L)
        else:
            wd = total - L
            wr = int(rng.integers(1, wd + 1)) if wd >= 1 else 1
            z = wav[wr - 1:wr - 1 + L]
            z = np.concatenate([z, np.zeros(L - z.size)])
            nlen = L
        if noisy:
            nz = (-(-audR * int(round(fs / speedR)) // fs)) if chspeed else L
            nir, nwr, ratio = int(rng.integers(1, imdb.noisenum + 1)), int(rng.integers(1, imdb.noiselen - nz + 1)), \
                float(rng.random()) * imdb.noisevol
            y = imdb.device_noise(nir, d["data"].device).cpu().numpy().astype(np.float64)[nwr - 1:nwr - 1 + nlen]
            z[:nlen] = z[:nlen] + y * ratio
        ref = O.spec_rownorm(O.run_spec(z.astype(np.float32)))
        close(im[:, :, 0, k], ref[:, :, 0, 0], 2e-3, "%s sample %d" % (transformation, k))
        s_, e_ = O.time2idx(wr / fs), min(O.time2idx((wr + aud - 1) / fs), imdb.wavLogits[ii].shape[0])
        assert np.abs(lg[:, k] - O.aggregate_logits(imdb.wavLogits[ii], s_, e_, "max")).max() < 1e-6
    with pytest.raises(ValueError):
        batch.getBatchEmoVoxCeleb(imdb, idx, imageSize=(512, W), rng=rng, transformation="IS")   # needs the waveform


def test_resample_kernel_vs_oracle(gpu):
    import torch
    from mcncrossmodalemotions_amd import batch
    rng = np.random.default_rng(8)
    for speed, n in ((0.95, 5000), (1.0499, 16384), (1.0, 777)):
        x = rng.standard_normal(n).astype(np.float32)
        y = batch.resample(torch.from_numpy(x).cuda(), int(round(16000 / speed)), 16000).cpu().numpy()
        ref = O.resample(x, int(round(16000 / speed)), 16000)
        assert y.shape == ref.shape
        close(y, ref, 1e-5, "resample speed %.4f" % speed)


def test_wgrad_side_stream_is_bit_identical(gpu):
    """DagNN.wgradStream: filter / bias derivatives on a side HIP stream -- same kernels, same
    inputs, so one SGD step leaves bit-identical parameters."""
    import torch
    from mcncrossmodalemotions_amd import train, vl, zoo
    rng = np.random.default_rng(5)
    x = O.F(rng.standard_normal((512, 100, 1, 4)))
    lg = O.F(rng.standard_normal((1, 1, 8, 4)) * 3)
    res = []
    for side in (False, True):
        net = zoo.emoVoxZoo(numSeconds=1, seed=11, width_mult=0.125)
        net.pack_params()
        if side:
            net.wgradStream = torch.cuda.Stream()
        opts = train.TrainOpts(batchSize=4)
        xd, lgd = vl.from_numpy(x), vl.from_numpy(lg)
        for it in range(3):
            train.train_step(net, ["data", xd, "logitTarget", lgd, "maxLabel", vl.max_label(lgd)], opts, it,
                             None, 4)
        torch.cuda.synchronize()
        res.append(net._flat.val.clone())
    assert torch.equal(res[0], res[1])


def test_side_stream_ordering_under_lag(gpu, monkeypatch):
    """Ordering between the main stream and DagNN.wgradStream, provoked with artificial lag (a host that runs one or
    two steps ahead of the GPU sees exactly these interleavings):
      * the filter transposition the forward pass enqueues on the side stream (vl.conv_prepare_backward) must not
        read the filters before the previous step's xm_sgd_update -- a sleep in front of every update on the MAIN
        stream makes a missing wait visible as stale transposed filters in the next dgrad;
      * a filter derivative enqueued on the side stream must be complete before anything on the main stream consumes
        the flat derivative buffer -- a sleep in front of every prepare on the SIDE stream makes it lag.
    Three steps with both lags leave parameters bit-identical to three steps without a side stream."""
    import torch
    from mcncrossmodalemotions_amd import train, vl, zoo
    rng = np.random.default_rng(5)
    x = O.F(rng.standard_normal((512, 100, 1, 4)))
    lg = O.F(rng.standard_normal((1, 1, 8, 4)) * 3)
    res = []
    real_sgd, real_prep = vl.sgd_update, vl.conv_prepare_backward
    for side in (False, True):
        net = zoo.emoVoxZoo(numSeconds=1, seed=11, width_mult=0.125)
        net.pack_params()
        if side:
            net.wgradStream = torch.cuda.Stream()
            assert net.prepareBackward

            def slow_sgd(*a, **k):
                torch.cuda._sleep(30_000_000)      # ~15 ms on the stream the update runs on
                return real_sgd(*a, **k)

            def slow_prep(*a, **k):
                torch.cuda._sleep(3_000_000)       # the side stream falls behind the forward pass
                return real_prep(*a, **k)
            monkeypatch.setattr(vl, "sgd_update", slow_sgd)
            monkeypatch.setattr(vl, "conv_prepare_backward", slow_prep)
        opts = train.TrainOpts(learningRate=[1e-1], batchSize=4)    # a large step: stale filters change the bits
        xd, lgd = vl.from_numpy(x), vl.from_numpy(lg)
        for it in range(3):
            train.train_step(net, ["data", xd, "logitTarget", lgd, "maxLabel", vl.max_label(lgd)], opts, it,
                             None, 4)
        torch.cuda.synchronize()
        res.append(net._flat.val.clone())
    assert torch.equal(res[0], res[1])


@pytest.mark.parametrize("lossType", ["euclidean", "huber", "softmaxlog"])
def test_student_alternative_loss_heads(gpu, lossType):
    """configureForRegression's other heads (emoVoxZoo.m:138-150): loss value and every parameter
    derivative of the 1/8-width student against the oracle; euclidean also divides the last filter
    bank by 10 (:141-145)."""
    from mcncrossmodalemotions_amd import vl, zoo
    rng = np.random.default_rng(23)
    N, W = 3, 100
    net = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=6, lossType=lossType)
    if lossType == "euclidean":
        ref = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=6)
        a, b = net.params[net.getLayer("fc8").params[0]].value, ref.params[ref.getLayer("fc8").params[0]].value
        assert np.allclose(np.asarray(a) * 10, np.asarray(b), rtol=1e-6)
    P0 = oracle_net.host_params(net)
    data, lgo, lab = _student_inputs(rng, W, N)
    wts = O.F(np.ones((1, 1, 1, N)))
    feed = {"data": data, "logitTarget": lgo, "maxLabel": lab, "instanceWeights": wts}
    V = oracle_net.forward(net, feed, P0, mode="normal")
    _, DP = oracle_net.backward(net, V, {"objective": np.float32(1)}, P0, mode="normal")
    net.pack_params()
    inputs = []
    for k, v in feed.items():
        if k in net.vars:
            inputs += [k, vl.from_numpy(v)]
    net.mode = "normal"
    net.eval(inputs, ["objective", 1])
    close(vl.to_numpy(net.vars["objective"].value).ravel()[0], V["objective"], 1e-5, "objective " + lossType)
    for name, ref in DP.items():
        got = vl.to_numpy(net.params[name].der)
        close(got.reshape(ref.shape, order="F"), ref, 2e-4, "der " + name)


def test_run_distillation_driver(gpu, tmp_path):
    """run_distillation -> cnn_train_dag mirror (run_distillation.m:71-182): mini-epochs, validation
    pass in test mode, extractStats keys, checkpoint + resume ('cont')."""
    from mcncrossmodalemotions_amd.run_distillation import run_distillation
    from mcncrossmodalemotions_amd import zoo
    kw = dict(gpus=[0], numSeconds=1, batchSize=4, miniEpochRatio=0.5, miniVal=0.5, numTracks=24,
              widthMult=0.125, dataDir=str(tmp_path), learningRate=[1e-3, 1e-3, 1e-3])
    net, info = run_distillation(numEpochs=2, **kw)
    assert len(info["train"]) == 2 and len(info["val"]) == 2
    tr = info["train"][-1]
    for k in ["objective", "classerror", "meanAcc", "num", "time"] + zoo.EMOTIONS + [e + "Pop" for e in zoo.EMOTIONS]:
        assert k in tr, k
    assert tr["num"] == 9          # 18 training tracks x 0.5
    assert info["val"][-1]["num"] == 3
    assert np.isfinite(tr["objective"]) and 0.0 <= tr["classerror"] <= 1.0 and 0.0 <= tr["meanAcc"] <= 1.0
    assert abs(sum(tr[e + "Pop"] for e in zoo.EMOTIONS) - 1.0) < 1e-6
    exp = [d for d in tmp_path.iterdir()]
    assert len(exp) == 1 and exp[0].name == ("voxceleb-senet50-ferplus-emovoxceleb-student-hot-cross-ent-scratch-"
                                              "1sec-8emo-agg-max-temp2")
    assert (exp[0] / "net-epoch-2.pt").exists()
    # resume: epochs 1-2 come from the checkpoint, only epoch 3 runs
    net2, info2 = run_distillation(numEpochs=3, **kw)
    assert len(info2["train"]) == 3
    assert info2["train"][:2] == info["train"]
    # a fresh run without 'cont' reproduces the first epochs exactly (seeded shuffles and crops)
    net3, info3 = run_distillation(numEpochs=2, cont=False, **kw)
    for a, b in zip(info3["train"], info["train"]):
        assert a["objective"] == b["objective"] and a["meanAcc"] == b["meanAcc"]
    # the euclidean head trains through the same driver
    _, info4 = run_distillation(numEpochs=1, lossType="euclidean", cont=False, **kw)
    assert np.isfinite(info4["train"][0]["objective"])


def test_compute_audio_feats_variable_width(gpu):
    """external/compute_audio_feats.m:116-136,160-185: whole-clip row normalisation, centre crop to the
    bucket width, pool6 resized per clip; one-by-one and bucket-batched evaluation vs the oracle."""
    from mcncrossmodalemotions_amd import external, vl, zoo
    rng = np.random.default_rng(41)
    net = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=9)
    widths = [100, 137, 250, 205, 333, 1012, 299]
    specs = [O.F(np.abs(rng.standard_normal((512, T))) + 0.1) for T in widths]
    # oracle: same arithmetic on the host
    ref = []
    onet = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=9)
    zoo.strip_losses(onet)
    P0 = oracle_net.host_params(onet)
    for sp, T in zip(specs, widths):
        n = O.spec_rownorm(sp.reshape(512, T, 1, 1, order="F"))
        rsize = max(w for w in external.BUCKETS_WIDTH if w <= T)
        rstart = int(np.floor((T - rsize) / 2.0 + 0.5)) or 1
        crop = np.asfortranarray(n[:, rstart - 1:rstart - 1 + rsize])
        onet.getLayer("pool6").block.poolSize = [1, external.BUCKETS_POOL[external.BUCKETS_WIDTH.index(rsize)]]
        V = oracle_net.forward(onet, {"data": crop}, P0, mode="test")
        ref.append(V["prediction"].ravel())
    ref = np.stack(ref)
    dspecs = [vl.from_numpy(sp) for sp in specs]
    got = external.compute_audio_feats(net, dspecs)
    close(got, ref, 1e-4, "one clip at a time")
    got_b = external.compute_audio_feats(net, dspecs, batch_by_bucket=True)
    close(got_b, ref, 1e-4, "bucket-batched")
    close(got_b, got, 1e-5, "batched vs single")
    got_g = external.compute_audio_feats(net, dspecs, use_graphs=True)
    close(got_g, ref, 1e-4, "HIP-graph replay")
    close(external.compute_audio_feats(net, dspecs, use_graphs=True), got_g, 0, "graph replay is repeatable")
    with pytest.raises(ValueError):
        external.compute_audio_feats(net, [vl.from_numpy(O.F(np.ones((512, 60))))])


def test_compute_visual_feats_splits_tracks(gpu):
    """external/compute_visual_feats.m:60-116: flattened frames -> teacher minibatches -> per-track logits."""
    from mcncrossmodalemotions_amd import external, vl, zoo
    rng = np.random.default_rng(43)
    net = zoo.ferPlusZoo("resnet50-ferplus", seed=7, width_mult=0.125, blocks=(1, 1, 1, 1))
    net.getLayer("pool5").block.poolSize = [2, 2]
    counts = [3, 1, 5, 2]
    tracks = [O.F(rng.standard_normal((64, 64, 3, c)) * 40) for c in counts]
    onet = zoo.ferPlusZoo("resnet50-ferplus", seed=7, width_mult=0.125, blocks=(1, 1, 1, 1))
    zoo.strip_losses(onet)
    onet.getLayer("pool5").block.poolSize = [2, 2]
    P0 = oracle_net.host_params(onet)
    feats = external.compute_visual_feats(net, [vl.from_numpy(t) for t in tracks], batchSize=4)
    assert [f.shape for f in feats] == [(c, 8) for c in counts]
    for t, f in zip(tracks, feats):
        V = oracle_net.forward(onet, {"data": t}, P0, mode="test")
        close(f, V["prediction"].reshape(8, -1, order="F").T, 1e-4, "track logits")


def test_bucketed_gradient_exchange(gpu):
    """train.GradBuckets: buckets are cut from the back of the filter segment at parameter boundaries
    (student: [fc6f fc7f fc8f] on fc6 = 82 % of the bytes, then the conv filters), the ranges tile the flat buffer
    exactly once, and a step with the overlapped exchange -- through torch.distributed AND through the library's own
    communicator behind the C ABI (xm_parserv_push / xm_parserv_sync), single-rank groups: the collective is an
    identity -- leaves bit-identical parameters to a step with one exchange at the end / no exchange."""
    import torch
    import torch.distributed as dist
    from mcncrossmodalemotions_amd import train, vl, zoo
    net = zoo.emoVoxZoo(numSeconds=1, seed=11, width_mult=0.125)
    net.pack_params()
    bk = train.GradBuckets(net, target_bytes=64 << 10)
    total = int(net._flat.der.numel())
    rs = sorted(bk.ranges())
    assert rs[0][0] == 0 and rs[-1][1] == total and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
    full = zoo.emoVoxZoo(numSeconds=3, seed=1)       # full width: the first bucket carries 82 % of the bytes
    full.pack_params()
    bf = train.GradBuckets(full)
    f6, f8 = full.params["fc6f"], full.params["fc8f"]
    a, b, trig = bf.buckets[0]
    assert (a, b) == (f6._flat_off, f8._flat_off + (int(f8.value.numel()) + 3) // 4 * 4) and trig == "fc6"
    assert 0.80 < (b - a) / float(full._flat.der.numel()) < 0.84
    rs = sorted(bf.ranges())
    assert rs[0][0] == 0 and rs[-1][1] == int(full._flat.der.numel()) and all(x[1] == y[0] for x, y in zip(rs, rs[1:]))
    # config 5: the SE-ResNet-50 teacher's 104 MB go out in several buckets along the backward pass
    tnet = zoo.ferPlusZoo("senet50-ferplus")
    tnet.removeLayer("top1error")
    tnet.pack_params()
    bt = train.GradBuckets(tnet)
    assert 3 <= len(bt.buckets) <= 6 and all(4 * (b - a) >= (8 << 20) for a, b, _ in bt.buckets[:-1])
    order = {l.name: i for i, l in enumerate(tnet.layers)}
    trig = [order[t] for _, _, t in bt.buckets]
    assert trig == sorted(trig, reverse=True)            # pushed in the order the backward pass reaches them
    rs = sorted(bt.ranges())
    assert rs[0][0] == 0 and rs[-1][1] == int(tnet._flat.der.numel()) and all(x[1] == y[0] for x, y in zip(rs, rs[1:]))
    own_group = not dist.is_initialized()
    if own_group:
        dist.init_process_group("nccl", rank=0, world_size=1, init_method="tcp://127.0.0.1:29571",
                                device_id=torch.device("cuda", 0))
    try:
        rng = np.random.default_rng(5)
        x = O.F(rng.standard_normal((512, 100, 1, 4)))
        lg = O.F(rng.standard_normal((1, 1, 8, 4)) * 3)
        res = []
        for mode in ("none", "end", "overlap", "overlap+side", "capi-end", "capi-overlap+side"):
            n = zoo.emoVoxZoo(numSeconds=1, seed=11, width_mult=0.125)
            n.pack_params()
            if mode.endswith("+side"):
                n.wgradStream = torch.cuda.Stream()
            ps = None
            if mode != "none":
                ps = train.ParameterServer("rccl-capi" if mode.startswith("capi") else "torch")
                ps.force = True
                ps.start()
                ps.overlap = "overlap" in mode
                assert ps.comm_count() == 1
            opts = train.TrainOpts(batchSize=4)
            xd, lgd = vl.from_numpy(x), vl.from_numpy(lg)
            pushed = []
            for it in range(3):
                train.train_step(n, ["data", xd, "logitTarget", lgd, "maxLabel", vl.max_label(lgd)], opts, it, ps, 4)
                if ps is not None and ps.overlap and it == 0:
                    n._grad_buckets.log = pushed
            torch.cuda.synchronize()
            if pushed:   # two logged steps: every element pushed exactly once per step
                pr = sorted(pushed)
                half = pr[::2]
                assert pr[::2] == pr[1::2]
                assert half[0][0] == 0 and half[-1][1] == int(n._flat.der.numel())
                assert all(u[1] == v[0] for u, v in zip(half, half[1:]))
            res.append(n._flat.val.clone())
            if ps is not None:
                ps.stop()
        for r in res[1:]:
            assert torch.equal(res[0], r)
    finally:
        if own_group:
            dist.destroy_process_group()


def test_profiler_names_are_the_kernels_that_exist(gpu):
    """bench.py's roofline object names kernels through xm_prof_kernel_name; every name a real step produces must be an
    instantiated kernel of the library (the symbol rocprofv3 prints) -- round 3 decoded the merged strided-dgrad kernel's
    key with the wrong divisor and reported an instantiation that had not run.  A distillation step on narrow networks
    (every kernel family: implicit GEMM, LDS-DMA, halo, merged dgrad, wgrad, stem + its fused filter derivative)."""
    import subprocess
    import torch
    from mcncrossmodalemotions_amd import _lib, batch as xbatch, prof, train, vl, zoo
    L = _lib.load()
    syms = subprocess.run(["nm", "-C", _lib.SO_PATH], capture_output=True, text=True).stdout
    teacher = zoo.ferPlusZoo("resnet50-ferplus", seed=1, width_mult=0.25, blocks=(1, 1, 1, 1))
    zoo.strip_losses(teacher)
    teacher.move("gpu")
    teacher.mode = "test"
    teacher.vars["prediction"].precious = True
    student = zoo.emoVoxZoo(numSeconds=3, width_mult=0.5, seed=2)
    student.pack_params()
    faces = xbatch.getImageBatch(8, seed=4)
    spec = vl.spec_rownorm(torch.randn((8, 1, 300, 512), device="cuda").abs_().permute(3, 2, 1, 0))
    opts = train.TrainOpts(batchSize=8)
    with prof.recording(L):
        teacher.eval(["data", faces])
        tl = teacher.vars["prediction"].value
        train.train_step(student, ["data", spec, "logitTarget", tl, "maxLabel", vl.max_label(tl)], opts, 0, None, 8)
    rows = prof.collect(L)      # a key without a name raises
    assert len(rows) >= 6
    names = {r.name for r in rows}
    for r in rows:
        assert ("xm::%s(" % r.name) in syms, "%r (key %d) is not a kernel of %s" % (r.name, r.key, _lib.SO_PATH)
    fam = {nm.split("<")[0] for nm in names}
    assert {"conv_gemm_kernel", "conv_wgrad_kernel", "conv_stem_bnpool_fwd_kernel", "conv_stem_wgrad_pool_kernel", "stem_gram_kernel"} <= fam \
        and len(fam) >= 6, fam
    # the merged strided dgrad (the kernel whose key was mis-decoded): the student's conv2 geometry at 16 samples (the
    # classes merge into one launch when they have >= 512 tiles together)
    x = torch.randn((16, 96, 73, 126), device="cuda").permute(3, 2, 1, 0)
    f = (torch.randn((256, 96, 5, 5), device="cuda") * 0.05).permute(3, 2, 1, 0)
    dzdy = torch.randn((16, 256, 36, 62), device="cuda").permute(3, 2, 1, 0)
    _, rows = prof.kernels_run(lambda: vl.vl_nnconv(x, f, None, dzdy, stride=2, pad=1, no_der_filters=True), L)
    merged = [r.name for r in rows]
    for m in merged:
        assert ("xm::%s(" % m) in syms, m
    assert any("multi" in m for m in merged), merged


def test_shipped_tuning_table_covers_the_bench_step(gpu):
    """Every convolution shape of the default bench step (full ResNet-50 teacher forward on 32 faces, full-width student
    step on 32 spectrograms 512x300, wgrad side stream as in bench.py) is in the shipped tile-configuration table: the
    step adds no measured entry, so tile choices -- and with them the summation order / the bits of every result -- are
    the same in every process (include/xmodal.h, xm_tune_load)."""
    import ctypes as C
    import torch
    from mcncrossmodalemotions_amd import _lib, batch as xbatch, train, vl, zoo
    L = _lib.load()
    if os.environ.get("XM_TUNE_FILE") is not None or os.environ.get("XM_AUTOTUNE") == "0":
        pytest.skip("non-default tuning table")
    teacher = zoo.ferPlusZoo("resnet50-ferplus", seed=100)
    zoo.strip_losses(teacher)
    teacher.move("gpu")
    teacher.mode = "test"
    teacher.vars["prediction"].precious = True
    student = zoo.emoVoxZoo("emovoxceleb-student", scratch=1, lossType="hot-cross-ent", numSeconds=3, numOutputs=8, seed=200)
    student.pack_params()
    student.wgradStream = torch.cuda.Stream()
    faces = xbatch.getImageBatch(32, seed=4)
    raw = torch.randn((32, 1, 300, 512), device="cuda").abs_()
    spec = vl.spec_rownorm(raw.permute(3, 2, 1, 0))
    tot, new0, new1 = C.c_int(), C.c_int(), C.c_int()
    L.xm_tune_load(None)          # (an earlier test of this process may have pointed the loader at another file)
    L.xm_tune_entries(C.byref(tot), C.byref(new0))
    opts = train.TrainOpts(batchSize=32)
    for it in range(2):
        teacher.eval(["data", faces])
        tl = teacher.vars["prediction"].value
        train.train_step(student, ["data", spec, "logitTarget", tl, "maxLabel", vl.max_label(tl)], opts, it, None, 32)
    torch.cuda.synchronize()
    L.xm_tune_entries(C.byref(tot), C.byref(new1))
    assert new1.value == new0.value, "the bench step measured %d tile configurations that the shipped table lacks" % (
        new1.value - new0.value)
