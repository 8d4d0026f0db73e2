"""GPU: vl.vl_imreadjpeg / xm_imread_transform_batch against the float64 restatement of tests/test_imread_aug_cpu.py on the
decoded pixels of the committed JPEG fixtures and of images PIL encodes here (1 x 1, 2 x 3, grey 17 x 23, 37 x 53, 96 x 96
and 300 x 200, which reduced to 8 x 8 takes 151 bicubic taps and two chunks of output rows):
  * every filter, with and without antialias, mirrored and not, centred and random windows, with and without the colour
    options, within the derived per-pixel tolerance (Ty + Tx + 4) 2^-24 sum |wy| |wx| |p| (ref_apply adds the colour terms);
  * the same bits on a second run, for an image alone and in a batch, and behind each of the three decoders;
  * the launch counts of xm_imread_geometry for one image and for all;
  * the narrow path: rounded, the new stage at 'bilinear' without antialias equals vl.imreadjpeg wherever the unrounded
    value is farther from k + 1/2 than the derived tolerance, and at most 1 % of an image's pixels are that close;
  * Contrast keeps the channel means, Saturation keeps a grey image; seeds fix the batch and Flip does not move windows;
  * batch.getBatchJpegFaces feeds train.cnn_train_dag reproducibly; getImageBatch with a filter equals the default path."""
import io

import numpy as np
import pytest
import torch

from test_imread_aug_cpu import FILTERS, U24, jpeg_bytes, opts_vector, ref_apply, ref_plan
from test_jpeg_cpu import GOLDEN

pytestmark = pytest.mark.gpu
AVG = (131.0912, 103.8827, 91.4953)
BRIGHT = np.diag([6.0, 4.0, 5.0]) + 0.5


@pytest.fixture(scope="module")
def files():
    """name -> JPEG bytes: the baseline fixtures that decode without a status bit, and the images encoded here"""
    from PIL import Image
    g = dict(np.load(GOLDEN))
    out = {str(n): g["bytes_" + str(n)].tobytes() for n in g["names"]}
    rng = np.random.default_rng(17)

    def smooth(H, W):   # low-pass noise: JPEG keeps it, and neighbouring pixels still differ
        a = rng.integers(0, 256, (H // 4 + 2, W // 4 + 2, 3)).astype(np.float64)
        a = np.kron(a, np.ones((4, 4, 1)))[:H, :W] + rng.integers(-20, 21, (H, W, 3))
        return np.clip(a, 0, 255).astype(np.uint8)

    for H, W in ((1, 1), (2, 3), (37, 53), (96, 96), (300, 200)):
        out["new_%dx%d" % (H, W)] = jpeg_bytes(smooth(H, W))
    fh = io.BytesIO()
    Image.fromarray(smooth(17, 23)[:, :, 0], mode="L").save(fh, "JPEG", quality=90)
    out["new_grey_17x23"] = fh.getvalue()
    return out


@pytest.fixture(scope="module")
def decoded(gpu, files):
    """name -> H x W x 3 float64 pixels as the device decodes them (the reference's input; computed once)"""
    from mcncrossmodalemotions_amd import vl
    imgs, status = vl.imreadjpeg(list(files.values()), return_status=True)
    assert not status.cpu().numpy().any()
    return {n: t.cpu().numpy().astype(np.float64) for n, t in zip(files, imgs)}


def run(blobs, o, draws=None, avg=None, split=None, progressive=False):
    """the stage through its pieces (jpeg_plan, jpeg_decode, imread_plan, imread_transform) with explicit draws:
    -> (list of Ho x Wo x 3 float32 numpy, rows)"""
    from mcncrossmodalemotions_amd import vl
    buf, plan = vl.jpeg_plan(blobs, stage=vl._pinned, progressive=progressive)
    pixels, _, status, desc = vl.jpeg_decode(buf, plan, want_pixels=True, split=split)
    rows, sizes = vl.imread_plan(desc[:, [2, 3, 21]], opts_vector(dict(o, avg=0 if avg is None else 1 if np.size(avg) == 3 else 2)), draws)
    flat = vl.imread_transform(pixels, rows, sizes, None if avg is None else np.asarray(avg, np.float32))
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    flat = flat.cpu().numpy()
    return [flat[int(r[5]):int(r[5]) + 3 * int(r[3]) * int(r[4])].reshape(3, int(r[4]), int(r[3])).transpose(2, 1, 0) for r in rows], rows


def draws_for(seed, N):
    from mcncrossmodalemotions_amd import vl
    return vl.imread_draws(np.random.default_rng(seed), N)


def check(got, imgs, o, draws, avg=None):
    """every image within the derived tolerance -> the worst ratio to it"""
    worst = 0.0
    for k, (g, img) in enumerate(zip(got, imgs)):
        p = ref_plan(img.shape[0], img.shape[1], o, draws[k] if draws is not None else np.array([0.5] * 7 + [0.0] * 3))
        ref, tol, _ = ref_apply(img, p, avg)
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        err = np.abs(g.astype(np.float64) - ref)
        bad = err > tol
        assert not bad.any(), (k, o, float(err[bad].max()), float(tol[bad].min()))
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    return worst


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("name", list(FILTERS))
def test_every_filter_against_the_restatement(gpu, files, decoded, name, antialias):
    names = list(files)
    blobs, imgs = [files[n] for n in names], [decoded[n] for n in names]
    N = len(names)
    worst = {}
    # centred whole-image window, no draws; the 300 x 200 image reduced to 8 x 8 walks two chunks of output rows
    o = dict(resize=(8, 8), filter=name, antialias=antialias)
    got, rows = run(blobs, o)
    worst["centre 8x8"] = check(got, imgs, o, None)
    big = names.index("new_300x200")
    if antialias:
        assert rows[big, 13] == {"box": 39, "bilinear": 76, "bicubic": 151}[name] and (rows[big, 33] < 8) == (name == "bicubic")
    # random windows, ranges, mirrored and not
    o = dict(resize=(24, 20), filter=name, antialias=antialias, random=True, flip=True, size=(0.5, 1.0), aniso=(0.75, 4 / 3))
    d = draws_for(3, N)
    got, rows = run(blobs, o, d)
    assert 0 < rows[:, 10].sum() < N
    worst["random 24x20"] = check(got, imgs, o, d)
    # the colour options on top, Contrast included (the two-pass path), and ragged outputs of a scalar Resize
    o = dict(resize=12, filter=name, antialias=antialias, random=True, flip=True, size=(0.35, 1.0), contrast=0.4, saturation=0.3,
             brightness=BRIGHT)
    d = draws_for(4, N)
    got, rows = run(blobs, o, d, avg=AVG)
    assert len({(int(r[3]), int(r[4])) for r in rows}) > 3
    worst["colour S=12"] = check(got, imgs, o, d, AVG)
    o = dict(resize=(16, 20), filter=name, antialias=antialias, saturation=0.5, brightness=BRIGHT, size=(0.625, 0.625))
    avg_img = np.random.default_rng(8).uniform(80, 140, (16, 20, 3)).astype(np.float32)
    got, _ = run(blobs, o, d, avg=avg_img)
    worst["average image"] = check(got, imgs, o, d, avg_img)
    print("%s antialias=%s: worst ratio to the tolerance %s" % (name, antialias, {k: round(v, 3) for k, v in worst.items()}))


def test_public_entry_takes_matconvnet_option_lists(gpu, files, decoded):
    from mcncrossmodalemotions_amd import vl
    names = list(files)
    blobs, imgs = [files[n] for n in names], [decoded[n] for n in names]
    out = vl.vl_imreadjpeg(blobs, "Pack", "Resize", [24, 20], "Flip", "CropSize", [0.5, 1], "cropanisotropy", [0.75, 4 / 3],
                           "CropLocation", "random", "Interpolation", "bicubic", "NumThreads", 4, "Verbose",
                           rng=np.random.default_rng(3), antialias=True)
    assert tuple(out.shape) == (24, 20, 3, len(names)) and out.dtype == torch.float32 and vl.is_mat(out)
    o = dict(resize=(24, 20), filter="bicubic", antialias=True, random=True, flip=True, size=(0.5, 1.0), aniso=(0.75, 4 / 3))
    got = vl.to_numpy(out)
    check([got[..., k] for k in range(len(names))], imgs, o, draws_for(3, len(names)))
    # no Resize, no Pack: a list at the images' own sizes; at 'bilinear' that is the decoded image up to the tolerance
    lst, status = vl.vl_imreadjpeg(blobs, return_status=True)
    assert [tuple(t.shape) for t in lst] == [i.shape for i in imgs] and not status.cpu().numpy().any()
    check([t.cpu().numpy() for t in lst], imgs, dict(), None)
    assert vl.vl_imreadjpeg([]) == []
    # SubtractAverage through the option list, three values and an image
    a = vl.vl_imreadjpeg(blobs[:3], "Pack", "Resize", [8, 8], "SubtractAverage", list(AVG))
    b = vl.vl_imreadjpeg(blobs[:3], "Pack", "Resize", [8, 8], "SubtractAverage", np.tile(np.float32(AVG), (8, 8, 1)))
    assert torch.equal(a, b)
    check([vl.to_numpy(a)[..., k] for k in range(3)], imgs[:3], dict(resize=(8, 8)), None, AVG)


def test_bits_repeat_alone_in_a_batch_and_behind_every_decoder(gpu, files):
    from mcncrossmodalemotions_amd import vl
    names = [n for n in files]
    blobs = [files[n] for n in names]
    o = dict(resize=(24, 20), filter="bicubic", antialias=True, random=True, flip=True, size=(0.5, 1.0), contrast=0.4, saturation=0.3,
             brightness=BRIGHT)
    d = draws_for(5, len(names))
    first, _ = run(blobs, o, d, avg=AVG)
    again, _ = run(blobs, o, d, avg=AVG)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    for k in (0, names.index("new_300x200"), names.index("new_1x1"), len(names) - 1):
        alone, _ = run(blobs[k:k + 1], o, d[k:k + 1], avg=AVG)
        assert np.array_equal(alone[0], first[k]), names[k]
    mixed = [5, 0, len(names) - 1, 5]                                    # another order, another neighbourhood, a repeat
    sub, _ = run([blobs[k] for k in mixed], dict(o, resize=14), d[mixed], avg=AVG)
    alone = [run(blobs[k:k + 1], dict(o, resize=14), d[k:k + 1], avg=AVG)[0][0] for k in mixed]
    assert all(np.array_equal(a, b) for a, b in zip(sub, alone)) and np.array_equal(sub[0], sub[3])
    # the other two decoders write the same pixels, so the stage gives the same bits behind them
    split, _ = run(blobs, o, d, avg=AVG, split=32)
    prog, _ = run(blobs, o, d, avg=AVG, progressive=True)
    assert all(np.array_equal(a, b) for a, b in zip(first, split)) and all(np.array_equal(a, b) for a, b in zip(first, prog))
    opts = ("Pack", "Resize", [24, 20], "Interpolation", "bicubic", "Contrast", 0.4, "Flip")
    base = vl.vl_imreadjpeg(blobs, *opts, rng=np.random.default_rng(6))
    assert torch.equal(base, vl.vl_imreadjpeg(blobs, *opts, rng=np.random.default_rng(6), split=32))
    assert torch.equal(base, vl.vl_imreadjpeg(blobs, *opts, rng=np.random.default_rng(6), progressive=True))


def test_launch_counts_are_those_of_the_geometry(gpu, files):
    from mcncrossmodalemotions_amd import _lib, prof, vl
    L = _lib.load()
    blobs = list(files.values())
    launches, with_contrast, _, _ = vl.imread_geometry()
    mine = lambda rows: {r.name: r.launches for r in rows if r.name.startswith("imread_")}   # noqa: E731
    for some in (blobs[:1], blobs):
        plain = mine(prof.kernels_run(lambda: vl.vl_imreadjpeg(some, "Resize", 9, "Interpolation", "bicubic"), L)[1])
        assert plain == {"imread_table_kernel": 1, "imread_resample_kernel<false>": 1} and sum(plain.values()) == launches
        jit = mine(prof.kernels_run(lambda: vl.vl_imreadjpeg(some, "Resize", [9, 7], "Contrast", 0.3, "Pack",
                                                             rng=np.random.default_rng(1)), L)[1])
        assert jit == {"imread_table_kernel": 1, "imread_resample_kernel<true>": 1, "imread_colour_kernel": 1}
        assert sum(jit.values()) == with_contrast


@pytest.mark.parametrize("shape,size", [((37, 53), (24, 24)), ((17, 23), (224, 224)), ((96, 96), (224, 224))])
def test_rounded_it_is_the_narrow_path(gpu, files, decoded, shape, size):
    from mcncrossmodalemotions_amd import vl
    name = {(37, 53): "new_37x53", (17, 23): "new_grey_17x23", (96, 96): "new_96x96"}[shape]
    blob, img = files[name], decoded[name]
    assert img.shape[:2] == shape
    narrow = vl.to_numpy(vl.imreadjpeg([blob], resize=size, crop_size=1 / 1.6))[..., 0]
    new = vl.vl_imreadjpeg([blob], "Pack", "Resize", list(size), "CropSize", 1 / 1.6, "CropLocation", "center", "Interpolation",
                           "bilinear")
    got = vl.to_numpy(new)[..., 0].astype(np.float64)
    o = dict(resize=size, size=(0.625, 0.625))
    ref, tol, _ = ref_apply(img, ref_plan(shape[0], shape[1], o))
    assert (np.abs(got - ref) <= tol).all()
    near_tie = np.abs(ref - np.floor(ref) - 0.5) <= tol                   # the reference alone decides what is excluded
    share = near_tie.mean()
    print("%s -> %s: %.3f %% of the pixels are within the tolerance of k + 1/2" % (shape, size, 100 * share))
    assert share <= 0.01
    rounded = np.floor(got + 0.5)
    assert np.array_equal(rounded[~near_tie], narrow[~near_tie])
    assert np.array_equal(vl.to_numpy(vl.uint8_round(new))[..., 0], np.clip(rounded, 0, 255))


def test_contrast_keeps_the_means_and_saturation_keeps_grey(gpu, files, decoded):
    blob, img = files["new_96x96"], decoded["new_96x96"]
    for u5 in (0.0, 1.0):                                                  # gamma = 1 - C and 1 + C
        d = np.array([[0.5] * 5 + [u5, 0.5, 0, 0, 0]])
        o = dict(resize=(40, 36), contrast=0.6)
        got, rows = run([blob], o, d)
        assert abs(rows[0, 27] - (0.4 if u5 == 0 else 1.6)) < 1e-15
        _, _, res = ref_apply(img, ref_plan(96, 96, o, d[0]))
        mu = res.mean((0, 1))
        bound = 40 * 36 * U24 * np.abs(res).mean((0, 1))                   # an Ho Wo-term fp32 sum
        assert (np.abs(got[0].astype(np.float64).mean((0, 1)) - mu) <= bound).all(), (u5, got[0].mean((0, 1)), mu)
    grey, gimg = files["new_grey_17x23"], decoded["new_grey_17x23"]
    assert np.array_equal(gimg[:, :, 0], gimg[:, :, 1]) and np.array_equal(gimg[:, :, 0], gimg[:, :, 2])
    for u6 in (0.0, 1.0):
        d = np.array([[0.5] * 6 + [u6, 0, 0, 0]])
        o = dict(resize=(20, 30), saturation=0.8, filter="bicubic")
        got, _ = run([grey], o, d)
        plain = ref_apply(gimg, ref_plan(17, 23, dict(o, saturation=0.0), d[0]))[0]
        _, tol, _ = ref_apply(gimg, ref_plan(17, 23, o, d[0]))
        assert (np.abs(got[0] - plain) <= tol).all()


def test_a_seed_fixes_the_batch_and_flip_does_not_move_the_windows(gpu, files):
    from mcncrossmodalemotions_amd import vl
    blobs = list(files.values())[:6]
    opts = ("Pack", "Resize", [16, 20], "CropSize", [0.35, 1], "CropLocation", "random", "Brightness", [5, 5, 5])
    a = vl.vl_imreadjpeg(blobs, *opts, rng=np.random.default_rng(21))
    b = vl.vl_imreadjpeg(blobs, *opts, rng=np.random.default_rng(21))
    c = vl.vl_imreadjpeg(blobs, *opts, rng=np.random.default_rng(22))
    assert torch.equal(a, b) and not torch.equal(a, c)
    f = vl.vl_imreadjpeg(blobs, *opts, "Flip", rng=np.random.default_rng(21))
    mirrored = vl.imread_draws(np.random.default_rng(21), 6)[:, 4] < 0.5
    assert 0 < mirrored.sum() < 6
    for k in range(6):   # the same window: an image that is not mirrored keeps its bits, a mirrored one is the left-right mirror
        want = torch.flip(a[..., k], dims=[1]) if mirrored[k] else a[..., k]
        assert torch.equal(f[..., k], want), k


def test_get_batch_jpeg_faces_feeds_cnn_train_dag_reproducibly(gpu, files):
    from mcncrossmodalemotions_amd import batch, train, vl, zoo
    names = [n for n in files if n not in ("new_1x1", "new_2x3", "s420_1x1")][:8]
    blobs = [files[n] for n in names]
    labels = [1 + k % 8 for k in range(8)]

    def trained():
        net = zoo.ferPlusZoo("resnet50_ft-dag", seed=11, width_mult=0.125, blocks=(1, 1, 1, 1), lossType="softmaxlog", numOutputs=8)
        net.getLayer("pool5").block.poolSize = [2, 2]                      # 64 x 64 input (as the teacher step tests)
        net.meta["normalization"]["imageSize"] = [64, 64, 3]
        rng = np.random.default_rng(9)
        get = lambda imdb, b: batch.getBatchJpegFaces(blobs, labels, b, net, True, rng, CropSize=[0.35, 1], Flip=True,   # noqa: E731
                                                      CropAnisotropy=[0.75, 4 / 3], Brightness=[4, 4, 4], Contrast=0.3,
                                                      Saturation=0.3)
        train.cnn_train_dag(net, None, get, learningRate=[1e-3], batchSize=4, numEpochs=1, train=range(8), val=[])
        torch.cuda.synchronize()
        return net._flat.val.clone(), net
    one, net = trained()
    two, _ = trained()
    assert torch.equal(one, two) and bool(torch.isfinite(one).all())
    fresh = zoo.ferPlusZoo("resnet50_ft-dag", seed=11, width_mult=0.125, blocks=(1, 1, 1, 1), lossType="softmaxlog", numOutputs=8)
    fresh.pack_params()
    assert not torch.equal(one.cpu(), fresh._flat.val.cpu())                # the two steps moved the parameters
    # outside train mode: the centre crop of the largest CropSize, nothing drawn
    ev = batch.getBatchJpegFaces(blobs, labels, [2, 5], net, False, None, CropSize=[0.35, 1], Flip=True)
    ref = vl.normalize_face(vl.vl_imreadjpeg([blobs[2], blobs[5]], "Pack", "Resize", [64, 64]), net.meta["normalization"]["averageImage"])
    assert ev[0] == "data" and ev[2] == "label" and torch.equal(ev[1], ref) and vl.to_numpy(ev[3]).ravel().tolist() == [3.0, 6.0]


def test_evaluation_callers_with_a_filter_equal_the_default_path(gpu, files, decoded):
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    from mcncrossmodalemotions_amd import vl
    names = ["new_96x96", "s420_96x80_q50", "new_37x53", "s420_64x64_rst"]
    # 47 x 41: the windows are 60, 50, 40 and 23.125 samples long, so no ratio has a small power-of-two denominator; ratios
    # such as 60 / 48 put samples on exact quarters, where bilinear values of integer pixels are true ties by the hundred
    norm = fe._Norm((47, 41), AVG)
    read = lambda paths: [files[p] for p in paths]   # noqa: E731
    default = vl.to_numpy(fe.getImageBatch(names, norm, read=read))
    new = vl.to_numpy(fe.getImageBatch(names, norm, read=read, interpolation="bilinear", antialias=False))
    assert default.shape == new.shape == (47, 41, 3, 4)
    for k, n in enumerate(names):
        img = decoded[n]
        ref, tol, _ = ref_apply(img, ref_plan(img.shape[0], img.shape[1], dict(resize=(47, 41), size=(0.625, 0.625))))
        near_tie = (np.abs(ref - np.floor(ref) - 0.5) <= tol).any(2)
        # the grey value is rounded once more, from a three-term fp32 sum of the rounded values (<= 4 * 2^-24 * 255 off)
        grey = np.floor(ref + 0.5) @ np.array([0.2989, 0.5870, 0.1140])
        near_tie |= np.abs(grey - np.floor(grey) - 0.5) <= 4 * U24 * 255
        assert near_tie.mean() <= 0.01, (n, near_tie.mean())
        assert np.array_equal(default[..., k][~near_tie], new[..., k][~near_tie]), n
    # another filter and antialias reach the stage through both callers
    bic = vl.to_numpy(fe.getImageBatch(names, norm, read=read, interpolation="bicubic", antialias=True, crop_size=1.0))
    rgb = vl.vl_imreadjpeg([files[n] for n in names], "Pack", "Resize", [47, 41], "Interpolation", "bicubic", antialias=True)
    assert np.array_equal(bic, vl.to_numpy(vl.normalize_face(vl.uint8_round(rgb), AVG)))
