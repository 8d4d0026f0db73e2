"""GPU: vl.imreadjpeg(progressive=True) / xm_jpeg_decode_batch_prog against PIL's pixels stored in
tests/golden/jpeg_progressive.npz -- exactly, the decode is integer arithmetic throughout -- alone and in ragged batches
that mix baseline and progressive files, with guard words around every output; baseline files through the progressive
path against the default path; the fused face tensor against vl.crop_resize_face bit for bit; files that end after a
scan; a truncated file between two good ones; the launch count; and buildImdb fed the progressive bytes against
buildImdb fed the baseline bytes of the same images."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_jpeg_cpu import GOLDEN, TRUNCATED
from test_jpeg_prog_cpu import GOLDEN_PROG, PARTIAL, np_decode_prog

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, -12345.0
AVG = (131.0912, 103.8827, 91.4953)


@pytest.fixture(scope="module")
def prog():
    return dict(np.load(GOLDEN_PROG))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def names(prog):
    return [str(n) for n in prog["names"]]


@pytest.fixture(scope="module")
def base_names(golden):
    return [str(n) for n in golden["names"]]


def hwc(t):
    """H x W x 3 device tensor -> uint8 numpy"""
    a = t.cpu().numpy()
    assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= 255
    return a.astype(np.uint8)


@pytest.fixture(scope="module")
def singles(gpu, prog, golden, names, base_names):
    """every fixture decoded alone: the progressive ones (and the partial files) with progressive=True, the baseline
    ones of jpeg_small.npz by the default path.  name -> (H x W x 3 uint8, status)"""
    from mcncrossmodalemotions_amd import vl
    out = {}
    for n in names + PARTIAL:
        imgs, status = vl.imreadjpeg([prog["bytes_" + n].tobytes()], return_status=True, progressive=True)
        out[n] = (hwc(imgs[0]), int(status.cpu()[0]))
    for n in base_names:
        imgs, status = vl.imreadjpeg([golden["bytes_" + n].tobytes()], return_status=True)
        out["base:" + n] = (hwc(imgs[0]), int(status.cpu()[0]))
    return out


def guarded(n, dtype, device):
    t = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=device)
    return t, t[GUARD:GUARD + n]


def guards_intact(t):
    return bool((t[:GUARD] == SENTINEL).all()) and bool((t[-GUARD:] == SENTINEL).all())


def decode_guarded(gpu, files, resize=None, crop=1 / 1.6, avg=AVG):
    """xm_jpeg_decode_batch_prog into buffers with guard words on both sides -> (images, faces, status), guards checked"""
    from mcncrossmodalemotions_amd import _lib, vl
    L = _lib.load()
    buf, plan = vl.jpeg_plan(files, progressive=True)
    N, sizes = plan["N"], plan["sizes"]
    dev = torch.from_numpy(buf).to(gpu)
    gp, pixels = guarded(int(sizes[5]), torch.float32, gpu)
    gs, status = guarded(N, torch.float32, gpu)                       # int32 words behind a float view of the same size
    gf, faces = (None, None) if resize is None else guarded(resize[0] * resize[1] * 3 * N, torch.float32, gpu)
    a3 = (C.c_float * 3)(*avg)
    p = dev.data_ptr()
    _lib.check(L.xm_jpeg_decode_batch_prog(
        C.c_void_p(p), plan["nbytes"], C.c_void_p(p + plan["desc"][0]), N, C.c_void_p(p + plan["lanes"][0]), int(sizes[6]),
        C.c_void_p(p + plan["tables"][0]), int(sizes[1]), int(sizes[2]), int(sizes[3]), int(sizes[4]), int(sizes[5]),
        C.c_void_p(pixels.data_ptr()), C.c_void_p(faces.data_ptr()) if faces is not None else None, float(crop),
        resize[0] if resize else 0, resize[1] if resize else 0, a3, C.c_void_p(status.data_ptr()),
        C.c_void_p(p + plan["scans"][0]), int(sizes[8]), int(sizes[9]), int(sizes[10]),
        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert guards_intact(gp) and guards_intact(gs) and (gf is None or guards_intact(gf))
    desc = buf[plan["desc"][0]:plan["desc"][0] + plan["desc"][1]].view(np.int64).reshape(N, 24)
    imgs = [pixels[int(d[21]):int(d[21]) + 3 * int(d[2]) * int(d[3])].view(3, int(d[3]), int(d[2])).permute(2, 1, 0) for d in desc]
    if faces is not None:
        faces = faces.view(N, 3, resize[1], resize[0]).permute(3, 2, 1, 0)
    return imgs, faces, status.view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("k", range(11))
def test_every_fixture_equals_pil(singles, prog, names, k):
    got, status = singles[names[k]]
    want = prog["pix_" + names[k]]
    assert status == 0 and got.shape == want.shape, names[k]
    assert np.array_equal(got, want), (names[k], int(np.abs(got.astype(int) - want).max()))


@pytest.mark.parametrize("seed", [0, 1])
def test_one_ragged_batch_of_baseline_and_progressive(gpu, prog, golden, names, base_names, singles, seed):
    pool = [(n, prog["bytes_" + n].tobytes()) for n in names] + [("base:" + n, golden["bytes_" + n].tobytes()) for n in base_names]
    order = np.random.default_rng(seed).permutation(44) % len(pool)              # every file twice, any order
    imgs, _, status = decode_guarded(gpu, [pool[i][1] for i in order])
    assert not status.any()
    for j, i in enumerate(order):
        assert np.array_equal(hwc(imgs[j]), singles[pool[i][0]][0]), (j, pool[i][0])


def test_baseline_files_through_the_progressive_path(gpu, golden, base_names):
    from mcncrossmodalemotions_amd import vl
    files = [golden["bytes_" + n].tobytes() for n in base_names] + [golden["bytes_truncated"].tobytes()]
    assert len(base_names) == 11
    a, sa = vl.imreadjpeg(files, return_status=True)
    b, sb = vl.imreadjpeg(files, return_status=True, progressive=True)
    assert torch.equal(sa, sb) and sa.cpu().tolist() == [0] * 11 + [TRUNCATED]
    for n, x, y in zip(base_names + ["truncated"], a, b):
        assert torch.equal(x, y), n
    fa = vl.imreadjpeg(files, resize=(24, 20), crop_size=1 / 1.6, average_image=AVG)
    fb = vl.imreadjpeg(files, resize=(24, 20), crop_size=1 / 1.6, average_image=AVG, progressive=True)
    assert torch.equal(fa.contiguous().view(torch.int32), fb.contiguous().view(torch.int32))


def test_faces_equal_crop_resize_face_per_image(gpu, prog, names):
    from mcncrossmodalemotions_amd import vl
    files = [prog["bytes_" + n].tobytes() for n in names + PARTIAL]
    for resize, crop in (((24, 20), 1 / 1.6), ((7, 9), 1.0)):
        imgs, faces, status = decode_guarded(gpu, files, resize=resize, crop=crop)
        assert not status.any() and tuple(faces.shape) == resize + (3, len(files))
        for j, im in enumerate(imgs):
            one = vl.crop_resize_face(vl.from_numpy(im.cpu().numpy()[..., None], gpu), AVG, resize, crop=crop)
            assert torch.equal(faces[..., j].contiguous().view(torch.int32), one[..., 0].contiguous().view(torch.int32)), \
                ((names + PARTIAL)[j], resize)


@pytest.mark.parametrize("name", PARTIAL)
def test_partial_files_equal_pil(singles, prog, name):
    got, status = singles[name]
    want = prog["pix_" + name]
    print(name, "largest difference from PIL", int(np.abs(got.astype(int) - want).max()))
    assert status == 0 and np.array_equal(got, want), name


@pytest.mark.parametrize("name", PARTIAL)
def test_partial_files_in_a_batch_equal_the_restatement(gpu, prog, singles, name):
    files = [prog["bytes_s420_16x16"].tobytes(), prog["bytes_" + name].tobytes(), prog["bytes_s420_41x35"].tobytes()]
    imgs, _, status = decode_guarded(gpu, files)
    assert not status.any() and np.array_equal(hwc(imgs[1]), np_decode_prog(files[1]))
    assert np.array_equal(hwc(imgs[0]), prog["pix_s420_16x16"]) and np.array_equal(hwc(imgs[2]), prog["pix_s420_41x35"])


def test_truncated_file_between_two_good_ones(gpu, prog):
    files = [prog["bytes_s420_41x35"].tobytes(), prog["bytes_truncated"].tobytes(), prog["bytes_grey_17x23"].tobytes()]
    imgs, faces, status = decode_guarded(gpu, files, resize=(24, 20))
    assert status[0] == 0 and status[2] == 0 and status[1] & TRUNCATED
    assert tuple(imgs[1].shape) == (96, 80, 3) and hwc(imgs[1]).shape == (96, 80, 3)        # the call completed, values 0 .. 255
    for j, n in ((0, "s420_41x35"), (2, "grey_17x23")):
        assert np.array_equal(hwc(imgs[j]), prog["pix_" + n]), n


def _launches(L, fn):
    from mcncrossmodalemotions_amd import prof
    return {r.name: r.launches for r in prof.kernels_run(fn, L)[1]}


def test_launch_count_does_not_depend_on_n(gpu, prog, names):
    from mcncrossmodalemotions_amd import _lib, vl
    L = _lib.load()
    files = [prog["bytes_" + names[i % len(names)]].tobytes() for i in range(70)]
    read = lambda fs: vl.imreadjpeg(fs, resize=(24, 24), average_image=AVG, progressive=True)
    read(files)                                                                  # the workspace exists
    three = _launches(L, lambda: read(files[4:7]))
    all70 = _launches(L, lambda: read(files))
    print("launches:", all70)
    assert three == all70 == {"jpeg_clear_kernel": 1, "jpeg_entropy_prog_kernel": 3, "jpeg_idct_kernel": 1, "jpeg_colour_kernel": 1,
                              "crop_resize_face_ragged_kernel": 1}                # one entropy launch per level
    plain = _launches(L, lambda: vl.imreadjpeg(files, progressive=True))
    assert sum(plain.values()) == 6 and "crop_resize_face_ragged_kernel" not in plain
    # a file that ends early brings the two smoothing launches, once per call
    part = [prog["bytes_partial_5"].tobytes()]
    assert _launches(L, lambda: read(files[:3] + part)) == _launches(L, lambda: read(part + files)) == dict(
        all70, jpeg_smooth_kernel=1, jpeg_smooth_dc_kernel=1)


def test_build_imdb_from_progressive_bytes(gpu, prog, names):
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe, zoo
    teacher = zoo.ferPlusZoo("resnet50-ferplus", seed=5, width_mult=0.25, blocks=(1, 1, 1, 1))
    use = [n for n in names if n != "s420_1x1"]
    out = {}
    for kind in ("bytes_", "base_"):
        syn = batch.SyntheticEmoVoxImdb(num_tracks=5, seed=4, min_seconds=0.8, max_seconds=1.6)
        src = fe.src_imdb(syn)
        frames = batch.JpegDenseFrames(src, [prog[kind + n].tobytes() for n in use], frameless=(2,), unclaimed=3,
                                       progressive=kind == "bytes_")
        imdb = fe.addFramesToImdb(src, frames.lister, find=frames.find)
        out[kind] = fe.buildImdb(teacher, imdb, read=frames.read, batchSize=7, progressive=frames.progressive)
    got, ref = out["bytes_"].wavLogits, out["base_"].wavLogits
    assert len(got) == len(ref) == 4
    for a, b in zip(got, ref):
        assert a.shape == b.shape and a.shape[0] > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    with pytest.raises(Exception, match="SOF2"):                                 # the default still refuses
        fe.getImageBatch(["x"], fe._Norm((24, 24), AVG), read=lambda ps: [prog["bytes_grey_8x8"].tobytes()])
