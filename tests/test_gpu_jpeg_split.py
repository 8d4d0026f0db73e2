"""GPU: the segment-parallel entropy decode (xm_jpeg_decode_batch_split, vl.imreadjpeg(split=)) against
xm_jpeg_decode_batch in the same process -- pixels, faces and status bit for bit -- and against PIL's pixels stored in
tests/golden/jpeg_small.npz: every fixture alone at seg_bytes 16, 32, 64 and 4096, a lane of more than two passes, restart
intervals alone and in a mixed batch, ragged batches of 70 with guard words around every output, a truncated and a
corrupted file in a batch, corruptions in a segment whose cold guess is the true state, the rounds vector, the launch
count, and buildImdb / compute_visual_feats with split= against the same functions without."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_jpeg_cpu import GOLDEN
from test_jpeg_split_cpu import ALIGNED, corrupted, patched, sweep

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, -12345.0
AVG = (131.0912, 103.8827, 91.4953)
RESIZE, CROP = (24, 20), 1 / 1.6
SEGS = (16, 32, 64, 4096)
TRUNCATED, BADCODE = 1, 2


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def names(golden):
    return [str(n) for n in golden["names"]]


def hwc(t):
    """H x W x 3 device tensor -> uint8 numpy"""
    a = t.cpu().numpy()
    assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= 255
    return a.astype(np.uint8)


def guarded(n, dtype, device):
    t = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=device)
    return t, t[GUARD:GUARD + n]


def guards_intact(t):
    return bool((t[:GUARD] == SENTINEL).all()) and bool((t[-GUARD:] == SENTINEL).all())


def decode_guarded(gpu, files, split=None, resize=RESIZE, crop=CROP, avg=AVG):
    """xm_jpeg_decode_batch (split None) or xm_jpeg_decode_batch_split into buffers with guard words on both sides ->
    (ragged pixels, faces, status, rounds, segments per lane), all numpy, guards checked"""
    from mcncrossmodalemotions_amd import _lib, vl
    L = _lib.load()
    buf, plan = vl.jpeg_plan(files)
    N, sizes = plan["N"], plan["sizes"]
    nl = int(sizes[6])
    dev = torch.from_numpy(buf).to(gpu)
    gp, pixels = guarded(int(sizes[5]), torch.float32, gpu)
    gs, status = guarded(N, torch.float32, gpu)                       # int32 words behind a float view of the same size
    gf, faces = guarded(resize[0] * resize[1] * 3 * N, torch.float32, gpu)
    gr, rounds = guarded(nl, torch.float32, gpu)
    a3 = (C.c_float * 3)(*avg)
    p = dev.data_ptr()
    args = [C.c_void_p(p), plan["nbytes"], C.c_void_p(p + plan["desc"][0]), N, C.c_void_p(p + plan["lanes"][0]), nl,
            C.c_void_p(p + plan["tables"][0]), int(sizes[1]), int(sizes[2]), int(sizes[3]), int(sizes[4]), int(sizes[5]),
            C.c_void_p(pixels.data_ptr()), C.c_void_p(faces.data_ptr()), float(crop), resize[0], resize[1], a3,
            C.c_void_p(status.data_ptr())]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if split is None:
        _lib.check(L.xm_jpeg_decode_batch(*args, stream))
    else:
        _lib.check(L.xm_jpeg_decode_batch_split(*args, int(split), C.c_void_p(rounds.data_ptr()), stream))
    torch.cuda.synchronize()
    assert guards_intact(gp) and guards_intact(gs) and guards_intact(gf) and guards_intact(gr)
    lanes = buf[plan["lanes"][0]:plan["lanes"][0] + plan["lanes"][1]].view(np.int64).reshape(nl, 4)
    segments = None if split is None else np.maximum(-(-(lanes[:, 2] - lanes[:, 1]) // int(split)), 1)
    desc = buf[plan["desc"][0]:plan["desc"][0] + plan["desc"][1]].view(np.int64).reshape(N, 24).copy()
    return dict(pixels=pixels.cpu().numpy(), faces=faces.view(torch.int32).cpu().numpy(),
                status=status.view(torch.int32).cpu().numpy(),
                rounds=None if split is None else rounds.view(torch.int32).cpu().numpy(), segments=segments, desc=desc)


def image(out, i):
    """image i of a decode_guarded result as H x W x 3 uint8"""
    d = out["desc"][i]
    H, W, o = int(d[2]), int(d[3]), int(d[21])
    a = out["pixels"][o:o + 3 * H * W].reshape(3, W, H).transpose(2, 1, 0)
    assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= 255
    return a.astype(np.uint8)


def assert_same(got, want, what):
    """pixels, faces and status of two decodes of the same files, bit for bit"""
    assert np.array_equal(got["status"], want["status"]), (what, got["status"], want["status"])
    assert np.array_equal(got["pixels"].view(np.uint32), want["pixels"].view(np.uint32)), what
    assert np.array_equal(got["faces"], want["faces"]), what
    assert (got["rounds"] >= 1).all() and (got["rounds"] <= got["segments"]).all(), (what, got["rounds"], got["segments"])


@pytest.fixture(scope="module")
def unsplit(gpu, golden, names):
    """every supported fixture decoded alone by xm_jpeg_decode_batch"""
    return {n: decode_guarded(gpu, [golden["bytes_" + n].tobytes()]) for n in names}


@pytest.mark.parametrize("k", range(11))
def test_every_fixture_alone(gpu, golden, names, unsplit, k):
    name = names[k]
    data = golden["bytes_" + name].tobytes()
    for seg in SEGS:
        got = decode_guarded(gpu, [data], split=seg)
        assert_same(got, unsplit[name], (name, seg))
        assert got["status"][0] == 0 and np.array_equal(image(got, 0), golden["pix_" + name]), (name, seg)
        if seg == 4096:                                       # one segment per lane: the first round is the only one
            assert (got["segments"] == 1).all() and (got["rounds"] == 1).all(), name
    if name in ("grey_8x8", "s420_1x1"):                      # lanes shorter than two segments
        assert decode_guarded(gpu, [data], split=16)["segments"].tolist() == [2 if name == "grey_8x8" else 1]


def test_a_lane_of_more_than_two_passes(gpu, golden, unsplit):
    from mcncrossmodalemotions_amd import vl
    per_pass, _ = vl.jpeg_split_geometry()
    assert 224 > 2 * per_pass                                 # else this file does not exercise the carry: fail, not skip
    got = decode_guarded(gpu, [golden["bytes_s420_50x50_q100"].tobytes()], split=16)
    assert got["segments"].tolist() == [225]                  # 3,593 entropy bytes
    assert_same(got, unsplit["s420_50x50_q100"], "s420_50x50_q100")
    assert np.array_equal(image(got, 0), golden["pix_s420_50x50_q100"])
    print("rounds of 225 segments in passes of %d: %d" % (per_pass, got["rounds"][0]))


def test_restart_intervals_alone_and_mixed(gpu, golden, unsplit):
    rst = golden["bytes_s420_64x64_rst"].tobytes()
    alone = decode_guarded(gpu, [rst], split=16)
    assert alone["segments"].size == 6 and alone["segments"].min() >= 8 and alone["segments"].max() <= 22
    assert_same(alone, unsplit["s420_64x64_rst"], "alone")
    mix = ["s420_96x80_q50", "s420_64x64_rst", "grey_17x23", "s420_64x64_rst", "s444_37x29_opt"]
    files = [golden["bytes_" + n].tobytes() for n in mix]
    want = decode_guarded(gpu, files)
    for seg in (16, 64):
        got = decode_guarded(gpu, files, split=seg)
        assert got["rounds"].size == 3 + 2 * 6
        assert_same(got, want, ("mixed", seg))
        for j, n in enumerate(mix):
            assert np.array_equal(image(got, j), golden["pix_" + n]), (n, seg)


@pytest.mark.parametrize("seed", [0, 1])
def test_one_ragged_batch_of_70(gpu, golden, names, seed):
    order = np.random.default_rng(seed).permutation(70) % len(names)
    files = [golden["bytes_" + names[i]].tobytes() for i in order]
    want = decode_guarded(gpu, files)
    assert not want["status"].any()
    for seg in (16, 64):
        got = decode_guarded(gpu, files, split=seg)
        assert_same(got, want, (seed, seg))
        for j, i in enumerate(order):
            assert np.array_equal(image(got, j), golden["pix_" + names[i]]), (j, names[i], seg)


def test_truncated_file_in_a_batch(gpu, golden):
    files = [golden["bytes_s420_16x16"].tobytes(), golden["bytes_truncated"].tobytes(),
             golden["bytes_grey_17x23"].tobytes(), golden["bytes_s420_96x80_q50"].tobytes()]
    want = decode_guarded(gpu, files)
    assert want["status"].tolist() == [0, TRUNCATED, 0, 0]
    for seg in SEGS:
        got = decode_guarded(gpu, files, split=seg)
        assert got["status"].tolist() == [0, TRUNCATED, 0, 0], seg
        assert_same(got, want, seg)                           # the whole truncated image, the rows past the cut included
        for j, n in ((0, "s420_16x16"), (2, "grey_17x23"), (3, "s420_96x80_q50")):
            assert np.array_equal(image(got, j), golden["pix_" + n]), (n, seg)


def test_corrupted_file_in_a_batch(gpu, golden):
    files = [golden["bytes_s420_41x35_opt"].tobytes(), corrupted(golden), golden["bytes_s444_37x29_opt"].tobytes()]
    want = decode_guarded(gpu, files)
    assert want["status"].tolist() == [0, BADCODE, 0]
    assert not np.array_equal(image(want, 1), golden["pix_s444_37x29_opt"])
    for seg in SEGS:
        got = decode_guarded(gpu, files, split=seg)
        assert got["status"].tolist() == [0, BADCODE, 0], seg
        assert_same(got, want, seg)
        assert np.array_equal(image(got, 0), golden["pix_s420_41x35_opt"]), seg       # the neighbours are untouched
        assert np.array_equal(image(got, 2), golden["pix_s444_37x29_opt"]), seg


def test_corruption_where_a_cold_guess_is_the_true_state(gpu, golden):
    """a thread whose guessed entry is the true state and whose segment holds the invalid symbol: its recovered decode
    must not become final (test_jpeg_split_cpu.ALIGNED)"""
    for seg in sorted({a[1] for a in ALIGNED}):
        files = [patched(golden, name, offset, value) for name, s, offset, value in ALIGNED if s == seg]
        files.insert(1, golden["bytes_s420_16x16"].tobytes())
        want = decode_guarded(gpu, files)
        assert want["status"].tolist() == [BADCODE, 0] + [BADCODE] * (len(files) - 2), seg
        assert_same(decode_guarded(gpu, files, split=seg), want, seg)


def test_corruption_sweep_in_one_batch(gpu, golden):
    files = sweep(golden)
    want = decode_guarded(gpu, files)
    assert (want["status"] & BADCODE).any() and len(files) >= 40
    for seg in (16, 32, 64):
        assert_same(decode_guarded(gpu, files, split=seg), want, seg)


def test_imreadjpeg_and_jpeg_decode_take_split(gpu, golden, names):
    from mcncrossmodalemotions_amd import vl
    files = [golden["bytes_" + n].tobytes() for n in names]
    plain, st0 = vl.imreadjpeg(files, return_status=True)
    imgs, st1 = vl.imreadjpeg(files, return_status=True, split=32)
    assert torch.equal(st0, st1) and all(torch.equal(a, b) for a, b in zip(plain, imgs))
    faces0 = vl.imreadjpeg(files, resize=RESIZE, crop_size=CROP, average_image=AVG)
    faces1 = vl.imreadjpeg(files, resize=RESIZE, crop_size=CROP, average_image=AVG, split=32)
    assert torch.equal(faces0.contiguous().view(torch.int32), faces1.contiguous().view(torch.int32))
    buf, plan = vl.jpeg_plan(files)
    out = vl.jpeg_decode(buf, plan, split=16, return_rounds=True)
    assert len(out) == 5 and out[4].dtype == torch.int32 and out[4].numel() == int(plan["sizes"][6])
    assert len(vl.jpeg_decode(buf, plan, split=16)) == 4 and int(out[4].min()) >= 1
    for bad in (0, 8, 24, 65552, 16.5):
        with pytest.raises(ValueError, match="multiple of 16"):
            vl.imreadjpeg(files, split=bad)
    with pytest.raises(ValueError, match="needs split"):
        vl.jpeg_decode(buf, plan, return_rounds=True)


def _launches(L, fn):
    from mcncrossmodalemotions_amd import prof
    return {r.name: r.launches for r in prof.kernels_run(fn, L)[1]}


def test_launch_count_is_the_geometrys(gpu, golden, names):
    from mcncrossmodalemotions_amd import _lib, vl
    L = _lib.load()
    _, launches = vl.jpeg_split_geometry()
    files = [golden["bytes_" + names[i % len(names)]].tobytes() for i in range(70)]
    vl.imreadjpeg(files, resize=(24, 24), average_image=AVG, split=16)             # the workspace exists
    one = _launches(L, lambda: vl.imreadjpeg(files[8:9], resize=(24, 24), average_image=AVG, split=16))
    all70 = _launches(L, lambda: vl.imreadjpeg(files, resize=(24, 24), average_image=AVG, split=16))
    print("launches:", all70)
    assert one == all70 and sum(all70.values()) == launches
    assert set(all70) == {"jpeg_clear_kernel", "jpeg_entropy_split_kernel", "jpeg_idct_kernel", "jpeg_colour_kernel",
                          "crop_resize_face_ragged_kernel"}


# ------------------------------------------------------------------------------------------------ buildImdb, compute_visual_feats
@pytest.fixture(scope="module")
def teacher(gpu):
    """the quarter-width ResNet-50 teacher of tests/test_gpu_imdb.py"""
    from mcncrossmodalemotions_amd import zoo
    return zoo.ferPlusZoo("resnet50-ferplus", seed=5, width_mult=0.25, blocks=(1, 1, 1, 1))


def jpeg_imdb(golden, names):
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe
    syn = batch.SyntheticEmoVoxImdb(num_tracks=5, seed=4, min_seconds=0.8, max_seconds=1.6)
    src = fe.src_imdb(syn)
    use = [n for n in names if n != "s420_1x1"]
    frames = batch.JpegDenseFrames(src, [golden["bytes_" + n].tobytes() for n in use], frameless=(2,), unclaimed=3)
    return fe.addFramesToImdb(src, frames.lister, find=frames.find), frames


def test_build_imdb_with_split(gpu, golden, names, teacher):
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    imdb, frames = jpeg_imdb(golden, names)
    ref = fe.buildImdb(teacher, imdb, read=frames.read, batchSize=7)
    got = fe.buildImdb(teacher, imdb, read=frames.read, batchSize=7, split=64)
    assert len(got.wavLogits) == len(ref.wavLogits) == 4
    for a, b in zip(got.wavLogits, ref.wavLogits):
        assert a.shape == b.shape and a.shape[0] > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    with pytest.raises(ValueError, match="needs `read`"):
        fe.buildImdb(teacher, imdb, lambda paths, device: None, split=64)


def test_compute_visual_feats_with_split(gpu, golden, names, teacher):
    from mcncrossmodalemotions_amd import external
    imdb, frames = jpeg_imdb(golden, names)
    ids, wavIds, paths = imdb.images["id"], imdb.images["denseFramesWavIds"], imdb.images["denseFrames"]
    tracks = [[p for p, w in zip(paths, wavIds) if w == i] for i in ids]
    ref = external.compute_visual_feats(teacher, tracks, batchSize=6, read=frames.read)
    got = external.compute_visual_feats(teacher, tracks, batchSize=6, read=frames.read, split=64)
    assert len(got) == len(ref) == len(tracks)
    for a, b in zip(got, ref):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
