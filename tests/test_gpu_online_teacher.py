"""GPU: teacherMode='online' -- the frozen teacher run inside getBatchEmoVoxCeleb (batch.OnlineTeacher, xm_window_targets).
  kernel     vl.window_targets bit-equal to aggregate_logits on the transposed copy + channel cut + max_label, guard words
             around both outputs
  plumbing   a teacher that is pure indexing (logit e of a face = one fixed pixel of it) does not depend on the batch a
             face sits in: the cached batch (buildImdb, batches of 16) and the online one are bit-equal
  training   two train_steps of the full-width student: cached, online overlapped, online on the calling stream
  teacher    the real ResNet-50 stand-in: online targets within 2e-4 max|cached logits| of the cached ones
  launches   an online step records the kernels of a cached step + the teacher's + the JPEG decode's
  driver     run_distillation(teacherMode='online') trains, checkpoints, and never shares a directory with a cached run
The frames are the files of tests/golden/jpeg_small.npz served through batch.JpegDenseFrames (all but the 1 x 1 one,
whose 1/1.6 centre crop is empty -- as in tests/test_gpu_jpeg.py)."""
import collections
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_jpeg_cpu import GOLDEN

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, -12345.0
AVG = (131.0912, 103.8827, 91.4953)


def bits(t):
    from mcncrossmodalemotions_amd import vl
    return vl.to_numpy(t).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the kernel
def guarded(n, device):
    t = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=device)
    return t, t[GUARD:GUARD + n]


def window_targets_guarded(gpu, lg, first, last, agg, P):
    """xm_window_targets into buffers with guard words on both sides -> (out P x N, labels N) as uint32 / float"""
    from mcncrossmodalemotions_amd import _lib, vl
    E, n, N = int(lg.shape[2]), int(lg.shape[3]), int(first.numel())
    go, out = guarded(P * N, gpu)
    gl, lab = guarded(N, gpu)
    _lib.check(_lib.load().xm_window_targets(C.c_void_p(lg.data_ptr()), E, n, C.c_void_p(first.data_ptr()),
                                             C.c_void_p(last.data_ptr()), N, vl._AGG[agg], P, C.c_void_p(out.data_ptr()),
                                             C.c_void_p(lab.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for g in (go, gl):
        assert bool((g[:GUARD] == SENTINEL).all()) and bool((g[-GUARD:] == SENTINEL).all())
    return out.cpu().numpy().view(np.uint32).reshape(N, P).T, lab.cpu().numpy()


def composed(lg, first, last, agg, P):
    """the three steps xm_window_targets stands for, as getBatchEmoVoxCeleb runs them on cached logits"""
    from mcncrossmodalemotions_amd import vl
    E, n = int(lg.shape[2]), int(lg.shape[3])
    fl = lg.permute(3, 2, 1, 0).reshape(n, E).t().contiguous().t()                     # the n x E mat, a transposed copy
    lgo, lab = vl.aggregate_logits(fl, first, last, agg)
    if P != E:
        lgo = lgo[:, :, :P, :].permute(3, 2, 1, 0).contiguous().permute(3, 2, 1, 0)
        lab = vl.max_label(lgo)
    return bits(lgo).reshape(P, -1, order="F"), vl.to_numpy(lab).ravel()


@pytest.fixture(scope="module")
def frame_logits(gpu):
    """1 x 1 x 8 x 230 teacher logits: quarter-integer values (ties within a frame and between frames), row 40 all NaN,
    single NaN entries, a +Inf and a -Inf; and the windows of the N = 70 case"""
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(12)
    n = 230
    x = (np.round(rng.standard_normal((1, 1, 8, n)) * 8) / 4).astype(np.float32)
    x[0, 0, :, 40] = np.nan
    x[0, 0, 2, 77] = np.nan
    x[0, 0, 7, 78] = np.nan
    x[0, 0, 5, 120], x[0, 0, 1, 121] = np.inf, -np.inf
    x[0, 0, :, 150:153] = 1.25                                                         # a window of nothing but ties
    kinds = [(1, 1), (5, 24), (9, 8), (12, 9), (40, 40), (30, 49), (77, 78), (150, 152), (115, 125), (230, 230), (211, 230)]
    first, last = [], []
    for k in range(70):
        if k < len(kinds):
            a, b = kinds[k]
        else:
            a = int(rng.integers(1, n + 1))
            b = min(n, a + int(rng.integers(0, 30)))
        first.append(a)
        last.append(b)
    return vl.from_numpy(x, gpu), np.array(first, np.int32), np.array(last, np.int32)


@pytest.mark.parametrize("P", [8, 7])
@pytest.mark.parametrize("agg", ["max", "mean"])
def test_window_targets_equals_the_three_steps_70_pairs(gpu, frame_logits, agg, P):
    from mcncrossmodalemotions_amd import vl
    lg, first, last = frame_logits
    df, dl = torch.from_numpy(first).to(gpu), torch.from_numpy(last).to(gpu)
    assert (last - first + 1 == 20).any() and (last == first).any() and (last < first).sum() == 2   # 20 rows, 1 row, empty
    out, lab = window_targets_guarded(gpu, lg, df, dl, agg, P)
    ref, rlab = composed(lg, df, dl, agg, P)
    assert np.array_equal(out, ref) and np.array_equal(lab, rlab)
    assert np.isnan(out.view(np.float32)).any() == (agg == "mean") and len(set(lab)) > 3
    o2, l2 = vl.window_targets(lg, df, dl, agg, P)                                       # the wrapper: the same bits, as mats
    assert tuple(o2.shape) == (1, 1, P, 70) and tuple(l2.shape) == (1, 1, 1, 70)
    assert np.array_equal(bits(o2).reshape(P, 70, order="F"), ref) and np.array_equal(vl.to_numpy(l2).ravel(), rlab)


@pytest.mark.parametrize("window", [(33, 33), (21, 40), (40, 40), (35, 34), (36, 33)], ids=["1row", "20rows", "nan-row", "empty",
                                                                                              "empty-3"])
def test_window_targets_equals_the_three_steps_one_pair(gpu, frame_logits, window):
    lg = frame_logits[0]
    df = torch.tensor([window[0]], dtype=torch.int32, device=gpu)
    dl = torch.tensor([window[1]], dtype=torch.int32, device=gpu)
    for agg in ("max", "mean"):
        for P in (8, 7):
            out, lab = window_targets_guarded(gpu, lg, df, dl, agg, P)
            ref, rlab = composed(lg, df, dl, agg, P)
            assert np.array_equal(out, ref) and np.array_equal(lab, rlab), (agg, P)


def test_window_targets_wrapper_refuses(gpu, frame_logits):
    from mcncrossmodalemotions_amd import vl
    lg = frame_logits[0]
    one = torch.ones(1, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match="aggregator"):
        vl.window_targets(lg, one, one, "peak")
    with pytest.raises(ValueError, match="numPredEmotions"):
        vl.window_targets(lg, one, one, "max", 9)
    with pytest.raises(ValueError, match="int32"):
        vl.window_targets(lg, one.long(), one)
    o, l = vl.window_targets(lg, one[:0], one[:0])
    assert tuple(o.shape) == (1, 1, 8, 0) and tuple(l.shape) == (1, 1, 1, 0)


# ------------------------------------------------------------------------------------------------ plumbing, exact
class PixelTeacher:
    """logit e of a face is the pixel PIX[e] of it: pure indexing, the same bits whatever batch the face sits in"""
    imageSize, averageImage = (24, 24), AVG
    PIX = [(3, 4, 0), (12, 12, 1), (20, 5, 2), (7, 19, 0), (23, 23, 1), (0, 0, 2), (11, 2, 0), (16, 17, 1)]

    def __init__(self):
        self.calls = []

    def logits(self, faces):
        n = int(faces.shape[3])
        self.calls.append(n)
        t = torch.stack([faces[h, w, c, :] for h, w, c in self.PIX], 1).contiguous()     # n x 8
        return t.reshape(n, 8, 1, 1).permute(3, 2, 1, 0)


def six_tracks(min_seconds, max_seconds, seed=4):
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe
    return fe.src_imdb(batch.SyntheticEmoVoxImdb(num_tracks=6, seed=seed, min_seconds=min_seconds, max_seconds=max_seconds,
                                                 val_fraction=0.34))


@pytest.fixture(scope="module")
def jpeg_world(gpu):
    """(imdb with frame lists, its JpegDenseFrames, the cached imdb built with the PixelTeacher in batches of 16)"""
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe
    golden = np.load(GOLDEN)
    use = [str(n) for n in golden["names"] if str(n) != "s420_1x1"]
    src = six_tracks(3.5, 6.0)
    frames = batch.JpegDenseFrames(src, [golden["bytes_" + n].tobytes() for n in use])
    imdb = fe.addFramesToImdb(src, frames.lister, find=frames.find)
    assert 80 <= len(imdb.images["denseFrames"]) <= 160 and (imdb.set == 2).sum() == 2
    cached = fe.buildImdb(PixelTeacher(), imdb, read=frames.read, batchSize=16)
    assert np.unique(np.concatenate(cached.wavLogits, 0), axis=0).shape[0] >= 8     # a face per file, (nearly) all different
    return imdb, frames, cached


@pytest.fixture(scope="module")
def pixel_world(gpu):
    """the same over decoded pixels (batch.SyntheticDenseFrames): frames= instead of read="""
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe
    src = six_tracks(3.5, 6.0, seed=8)
    frames = batch.SyntheticDenseFrames(src, frameSize=(40, 48))
    imdb = fe.addFramesToImdb(src, frames.lister, find=frames.find)
    return imdb, frames, fe.buildImdb(PixelTeacher(), imdb, frames, batchSize=16)


def get_batch(imdb, sel, gpu, online=None, agg="max", P=8, W=300, seed=3, lossType="hot-cross-ent"):
    from mcncrossmodalemotions_amd import batch
    inputs = batch.getBatchEmoVoxCeleb(imdb, sel, imageSize=(512, W), numPredEmotions=P, logitAggregator=agg,
                                       lossType=lossType, rng=np.random.default_rng(seed), device=gpu, onlineTeacher=online)
    torch.cuda.synchronize()
    return inputs, dict(zip(inputs[::2], inputs[1::2]))


def assert_same_batch(a, b):
    assert list(a) == list(b)
    for k in a:
        assert tuple(a[k].shape) == tuple(b[k].shape) and np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("P", [8, 7])
@pytest.mark.parametrize("agg", ["max", "mean"])
@pytest.mark.parametrize("sel", [[4], [1, 5, 2]], ids=["N1", "N3"])
def test_online_batch_equals_cached_batch(gpu, jpeg_world, sel, agg, P):
    from mcncrossmodalemotions_amd import batch
    imdb, frames, cached = jpeg_world
    online = batch.OnlineTeacher(PixelTeacher(), imdb, read=frames.read)
    ci, c = get_batch(cached, sel, gpu, agg=agg, P=P)
    oi, o = get_batch(imdb, sel, gpu, online, agg=agg, P=P)
    assert_same_batch(c, o)
    assert tuple(o["logitTarget"].shape) == (1, 1, P, len(sel)) and len(set(bits(o["logitTarget"]).ravel())) > len(sel)
    assert type(ci) is list and isinstance(oi, batch.BatchInputs)
    assert set(oi.input_events) == {"logitTarget", "maxLabel"} and oi.input_events["maxLabel"].query()
    assert len(online.model.calls) == 1 and 10 * len(sel) <= online.model.calls[0] <= 14 * len(sel)   # W = 300: 13 rows a pair


@pytest.mark.parametrize("how", ["split64", "no-overlap", "chunk5", "softmaxlog", "euclidean"])
def test_online_batch_equals_cached_batch_options(gpu, jpeg_world, how):
    from mcncrossmodalemotions_amd import batch
    imdb, frames, cached = jpeg_world
    kw = {"split64": dict(split=64), "no-overlap": dict(overlap=False), "chunk5": dict(chunk=5)}.get(how, {})
    loss = how if how in ("softmaxlog", "euclidean") else "hot-cross-ent"
    online = batch.OnlineTeacher(PixelTeacher(), imdb, read=frames.read, **kw)
    sel = [1, 5, 2]
    _, c = get_batch(cached, sel, gpu, lossType=loss)
    oi, o = get_batch(imdb, sel, gpu, online, lossType=loss)
    assert_same_batch(c, o)
    if how == "no-overlap":
        assert oi.input_events is None and online.stream is None
    if how == "chunk5":
        assert len(online.model.calls) >= 7 and max(online.model.calls) == 5 and sum(online.model.calls) >= 30
    if how == "euclidean":
        assert list(o) == ["data", "logitTarget", "instanceWeights", "maxLabel"]


def test_online_batch_from_decoded_pixels_and_frames_per_pair(gpu, pixel_world):
    from mcncrossmodalemotions_amd import batch
    imdb, frames, cached = pixel_world
    online = batch.OnlineTeacher(PixelTeacher(), imdb, frames=frames)
    assert np.unique(np.concatenate(cached.wavLogits, 0), axis=0).shape[0] >= len(imdb.images["denseFrames"]) - 2   # a face per frame
    for agg in ("mean", "max"):
        _, c = get_batch(cached, [0, 3, 4], gpu, agg=agg)
        _, o = get_batch(imdb, [0, 3, 4], gpu, online, agg=agg)
        assert_same_batch(c, o)
    # one frame a pair (BASELINE's definition): the same spectrograms, the target is one of the window's cached rows
    one = batch.OnlineTeacher(PixelTeacher(), imdb, frames=frames, framesPerPair=1, seed=5)
    _, o1 = get_batch(imdb, [0, 3, 4], gpu, one)
    assert one.model.calls == [3] and np.array_equal(bits(o1["data"]), bits(c["data"]))
    _, _, first, last = batch.wav_batch_plan(cached, [0, 3, 4], 300, "I", np.random.default_rng(3))
    cat = np.concatenate(cached.wavLogits, 0).view(np.uint32)
    got = bits(o1["logitTarget"]).reshape(8, 3, order="F")
    for k in range(3):
        assert (cat[first[k] - 1:last[k]] == got[:, k]).all(1).any(), k
    with pytest.raises(ValueError, match="numPredEmotions exceeds"):
        get_batch(imdb, [0], gpu, online, P=9)


# ------------------------------------------------------------------------------------------------ training
def test_two_train_steps_cached_online_overlapped_and_not(gpu, jpeg_world):
    """the full-width student, N = 3, W = 300: the flat parameter buffer after two steps is the same in all three"""
    from mcncrossmodalemotions_amd import batch, train, zoo
    imdb, frames, cached = jpeg_world
    ways = {"cached": (cached, None), "overlap": (imdb, dict(overlap=True)), "serial": (imdb, dict(overlap=False))}
    flat = {}
    for name, (db, kw) in ways.items():
        student = zoo.emoVoxZoo("emovoxceleb-student", scratch=1, lossType="hot-cross-ent", numSeconds=3, numOutputs=8,
                                seed=200)
        student.pack_params()
        online = batch.OnlineTeacher(PixelTeacher(), imdb, read=frames.read, **kw) if kw is not None else None
        rng = np.random.default_rng(6)
        opts = train.TrainOpts(batchSize=3)
        for it, sel in enumerate(([1, 5, 2], [0, 2, 4])):
            inputs = batch.getBatchEmoVoxCeleb(db, sel, imageSize=(512, 300), rng=rng, device=gpu, onlineTeacher=online)
            assert (getattr(inputs, "input_events", None) is not None) == (name == "overlap")
            train.train_step(student, inputs, opts, it, None, 3, input_events=getattr(inputs, "input_events", None))
        torch.cuda.synchronize()
        flat[name] = student._flat.val.clone()
        del student
    assert bool(torch.isfinite(flat["cached"]).all())
    assert torch.equal(flat["cached"], flat["overlap"]) and torch.equal(flat["cached"], flat["serial"])


# ------------------------------------------------------------------------------------------------ the real teacher
def test_real_teacher_online_targets_within_twice_the_forward_criterion(gpu):
    """resnet50-ferplus (seeded stand-in, calibrated moments), ~40 frames in 6 short tracks: the cached logits come from
    batches of 16, the online ones from the 3 clips' frames in one batch.  Each HIP forward value is within 1e-4 of the
    oracle relative to the tensor's largest entry (the project's standing criterion), so two batch partitions of the
    same kernels differ by at most twice that; max and mean of values within d are within d."""
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe, vl, zoo
    golden = np.load(GOLDEN)
    use = [str(n) for n in golden["names"] if str(n) != "s420_1x1"]
    src = six_tracks(1.2, 1.9, seed=2)
    frames = batch.JpegDenseFrames(src, [golden["bytes_" + n].tobytes() for n in use])
    imdb = fe.addFramesToImdb(src, frames.lister, find=frames.find)
    assert 30 <= len(imdb.images["denseFrames"]) <= 48
    net = zoo.ferPlusZoo("resnet50-ferplus", seed=100)
    zoo.strip_losses(net)
    net.move("gpu")
    zoo.calibrate_moments(net, ["data", batch.getImageBatch(16, seed=999, device=gpu)])
    net.mode = "test"
    cached = fe.buildImdb(net, imdb, read=frames.read, batchSize=16)
    online = batch.OnlineTeacher(net, imdb, read=frames.read)
    scale = float(np.abs(np.concatenate(cached.wavLogits, 0)).max())
    assert np.isfinite(scale) and scale > 0
    sel = [0, 3, 5]
    for agg in ("max", "mean"):
        _, c = get_batch(cached, sel, gpu, agg=agg)
        _, o = get_batch(imdb, sel, gpu, online, agg=agg)
        assert np.array_equal(bits(c["data"]), bits(o["data"]))
        err = float(np.abs(vl.to_numpy(c["logitTarget"]) - vl.to_numpy(o["logitTarget"])).max())
        print("real teacher, %s: max |online - cached| %.3e, bound %.3e (max |cached logits| %.3f)" % (agg, err, 2e-4 * scale,
                                                                                                        scale))
        assert err <= 2e-4 * scale


# ------------------------------------------------------------------------------------------------ no hidden work
def test_an_online_step_launches_a_cached_step_plus_teacher_plus_decode(gpu, jpeg_world):
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe, prof, train, vl, zoo
    imdb, frames, _ = jpeg_world
    net = zoo.ferPlusZoo("resnet50-ferplus", seed=5, width_mult=0.25, blocks=(1, 1, 1, 1))
    cached = fe.buildImdb(net, imdb, read=frames.read, batchSize=16)
    online = batch.OnlineTeacher(net, imdb, read=frames.read, lanes=1)
    student = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=9)
    student.pack_params()
    opts = train.TrainOpts(batchSize=3)
    sel = [1, 5, 2]

    def step(db, provider):
        inputs = batch.getBatchEmoVoxCeleb(db, sel, imageSize=(512, 100), rng=np.random.default_rng(3), device=gpu,
                                           onlineTeacher=provider)
        train.train_step(student, inputs, opts, 0, None, 3, input_events=getattr(inputs, "input_events", None))

    _, _, first, last = batch.wav_batch_plan(imdb, sel, 100, "I", np.random.default_rng(3))
    paths = batch.online_frame_plan(imdb, first, last)[0]
    decode = lambda: vl.imreadjpeg(frames.read(paths), resize=(224, 224), crop_size=1 / 1.6, average_image=AVG)
    faces = decode()
    def count(fn):
        c = collections.Counter()
        for r in prof.kernels_run(fn)[1]:
            c[r.name] += int(r.launches)
        return c

    for fn in (lambda: step(cached, None), lambda: step(imdb, online), lambda: online.model.logits(faces), decode):
        fn()                                                         # every shape has its tile configuration
    torch.cuda.synchronize()
    c, o = count(lambda: step(cached, None)), count(lambda: step(imdb, online))
    t, d = count(lambda: online.model.logits(faces)), count(decode)
    assert sum(c.values()) > 10 and sum(t.values()) > 10 and sum(d.values()) > 0
    assert o == c + t + d, {k: (o[k], (c + t + d)[k]) for k in set(o) | set(c + t + d) if o[k] != (c + t + d)[k]}


# ------------------------------------------------------------------------------------------------ the driver
def test_run_distillation_online_trains_checkpoints_and_keeps_its_own_directory(gpu, jpeg_world, tmp_path):
    from mcncrossmodalemotions_amd.run_distillation import run_distillation
    imdb, frames, cached = jpeg_world
    kw = dict(gpus=[0], numSeconds=1, batchSize=2, miniEpochRatio=1.0, miniVal=1.0, widthMult=0.125, dataDir=str(tmp_path),
              learningRate=[1e-3], numEpochs=1)
    net, info = run_distillation(imdb=imdb, teacherMode="online", teacherNet=PixelTeacher(), read=frames.read, **kw)
    assert len(info["train"]) == 1 and np.isfinite(info["train"][0]["objective"]) and info["train"][0]["num"] == 4
    assert len(info["val"]) == 1 and np.isfinite(info["val"][0]["objective"]) and info["val"][0]["num"] == 2
    dirs = sorted(os.listdir(tmp_path))
    assert len(dirs) == 1 and dirs[0].endswith("-online") and os.path.exists(tmp_path / dirs[0] / "net-epoch-1.pt")
    # the cached run of the same options: another directory, trained from its first epoch
    net2, info2 = run_distillation(imdb=cached, **kw)
    dirs2 = sorted(os.listdir(tmp_path))
    assert len(dirs2) == 2 and dirs[0] == dirs2[0] + "-online" and len(info2["train"]) == 1
    assert os.path.exists(tmp_path / dirs2[0] / "net-epoch-1.pt")
    # the same teacher, the same frames, the same generators: the two runs trained on the same batches
    assert info2["train"][0]["objective"] == info["train"][0]["objective"]
    # resuming the online run finds its checkpoint and trains nothing more; one frame a pair is a third directory
    _, info3 = run_distillation(imdb=imdb, teacherMode="online", teacherNet=PixelTeacher(), read=frames.read, **kw)
    assert info3["train"] == info["train"]
    run_distillation(imdb=imdb, teacherMode="online", teacherNet=PixelTeacher(), read=frames.read, framesPerPair=1,
                     overlapTeacher=False, **kw)
    assert sorted(os.listdir(tmp_path))[-1].endswith("-online-fpp1") and len(os.listdir(tmp_path)) == 3
