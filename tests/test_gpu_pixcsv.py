"""GPU: xm_pixcsv_decode_batch / vl.pixcsv_decode / batch.getFerPlusImdb.  The reference for every pixel is
np.array(field.split()) on the same bytes; the values are integers, so every comparison is exact.  Every direct call
decodes into a buffer with guard words on both sides, reads bytes that are surrounded by DIGITS the kernel has to mask
(before the field, behind it, in the padding of the buffer), and checks the guards.  Aimed at the kernel's seams with
xm_pixcsv_geometry: the 16 alignments of a field, numbers of one to three digits that end within four bytes of a
thread's 16-byte group and of a pass boundary, separator runs, a field that ends with the buffer, 1 / 2 / 257 rows in
one launch, both layouts, images on both sides of the LDS staging limit, every status word, skipped and permuted rows,
chunked uploads; then the CSV pair end to end through getFerPlusImdb, getBatchFerPlus, ferplus_baselines and
benchmark_ferplus_models."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, 0xDEADBEEF - (1 << 32)
GUARD_WORD = np.uint32(SENTINEL & 0xFFFFFFFF)
BADCHAR, RANGE, COUNT, NOFIT = 1, 2, 4, 8


# ------------------------------------------------------------------------------------------------ helpers
def ref_image(field, H, W, transpose):
    """the numpy restatement: the numbers of the field at their documented positions, 0 elsewhere"""
    v = np.array(field.split()).astype(np.float32) if field.split() else np.zeros(0, np.float32)
    img = np.zeros(H * W, np.float32)
    k = np.arange(min(len(v), H * W))
    img[(k % W) * H + k // W if transpose else k] = v[:H * W]
    return img


def rand_number(rng, width=None):
    width = width or int(rng.integers(1, 4))
    lo, hi = ((0, 10), (10, 100), (100, 256))[width - 1]
    return b"%d" % int(rng.integers(lo, hi))


def rand_field(rng, count):
    return b" ".join(rand_number(rng) for _ in range(count))


def pack(fields, align=None, between=b"99,99"):
    """one buffer holding the fields, digits between them; align=16 puts every field at a 16-byte boundary, align=k < 16
    at k past one.  Returns (blob, rows)"""
    blob, rows = b"", []
    for i, f in enumerate(fields):
        blob += between
        if align is not None:
            blob += b"8" * ((align - len(blob)) % 16)
        rows.append([len(blob), len(blob) + len(f), -1, -1, i + 1, i, 0, 0])
        blob += f
    return blob, np.array(rows, np.int64).reshape(len(fields), 8)


def run(gpu, blob, rows, H, W, transpose, images=None, tail=b"77"):
    """xm_pixcsv_decode_batch on blob (+ `tail` digits, + digits up to the next multiple of 16; nbytes counts blob and tail)
    -> (uint32 images x H*W, status N x 2); guards checked"""
    from mcncrossmodalemotions_amd import _lib
    rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 8)
    N = len(rows)
    images = N if images is None else images
    body = blob + tail
    padded = body + b"5" * ((-len(body)) % 16)
    dev = torch.from_numpy(np.frombuffer(padded, np.uint8).copy()).to(gpu)
    desc = torch.from_numpy(rows).to(gpu)
    n = images * H * W
    out = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=gpu)
    status = torch.full((max(N, 1), 2), -7, dtype=torch.int32, device=gpu)
    _lib.check(_lib.load().xm_pixcsv_decode_batch(C.c_void_p(dev.data_ptr()), len(body), C.c_void_p(desc.data_ptr()), N, H, W,
                                                  int(transpose), C.c_void_p(out.data_ptr() + 4 * GUARD), n,
                                                  C.c_void_p(status.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint32)
    assert (host[:GUARD] == GUARD_WORD).all() and (host[GUARD + n:] == GUARD_WORD).all()
    return host[GUARD:GUARD + n].reshape(images, H * W), status.cpu().numpy()[:N]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_fields(gpu, fields, H, W, transpose, align=None, tail=b"77"):
    blob, rows = pack(fields, align)
    got, st = run(gpu, blob, rows, H, W, transpose, tail=tail)
    for i, f in enumerate(fields):
        assert np.array_equal(got[i], bits(ref_image(f, H, W, transpose))), (i, f[:60])
        assert st[i].tolist() == [len(f.split()), 0 if len(f.split()) == H * W else COUNT], (i, st[i])
    return got, st


@pytest.fixture(scope="module")
def P():
    from mcncrossmodalemotions_amd import vl
    bpp, launches = vl.pixcsv_geometry()
    assert launches == 1 and bpp % 16 == 0
    return bpp


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("transpose", [0, 1])
def test_every_alignment_of_the_field(gpu, transpose):
    rng = np.random.default_rng(3)
    for a in range(16):
        f = rand_field(rng, 15)
        blob, rows = pack([f], align=a, between=b"1234567 ")
        assert rows[0, 0] % 16 == a
        got, st = run(gpu, blob, rows, 3, 5, transpose)
        assert np.array_equal(got[0], bits(ref_image(f, 3, 5, transpose))), a
        assert st[0].tolist() == [15, 0]


def seam_field(rng, count, targets):
    """`count` numbers; for every (byte, width) of `targets` a number of that width whose LAST digit is field byte `byte`"""
    out, todo = b"", sorted(targets)
    n = 0
    while n < count:
        if todo:
            T, w = todo[0]
            start = T - w + 1
            nxt = rand_number(rng)
            if len(out) + len(nxt) + 1 <= start and n < count - len(todo):
                out += nxt + b" "
            else:
                assert len(out) <= start, (len(out), start)
                out += b" " * (start - len(out)) + rand_number(rng, w) + b" "
                assert out[T:T + 1].isdigit() and out[T + 1:T + 2] == b" "
                todo.pop(0)
        else:
            out += rand_number(rng) + b" "
        n += 1
    assert not todo
    return out[:-1]


def test_numbers_that_end_near_a_group_or_pass_seam(gpu, P):
    """for d in -4 .. 4 and 1, 2 and 3 digits: a number whose last digit is field byte 16 j + d, P + d and 2 P + d of a
    field that starts at a 16-byte boundary, so that those are bytes of a thread's group / of a pass"""
    rng = np.random.default_rng(11)
    H, W = 50, 60
    fields = []
    for d in range(-4, 5):
        for w in (1, 2, 3):
            j = 4 + (d + 4)
            f = seam_field(rng, H * W, [(16 * j + d, w), (16 * 40 + d, w), (P + d, w), (2 * P + d, w)])
            assert len(f) > 2 * P + 16 and len(f.split()) == H * W
            fields.append(f)
    for transpose in (0, 1):
        check_fields(gpu, fields, H, W, transpose, align=16)
    # the same fields at an odd alignment: the seams then fall elsewhere in the numbers
    check_fields(gpu, fields[:6], H, W, 1, align=7)


def test_a_number_that_ends_with_the_field_at_a_seam(gpu, P):
    """the closing separator is the byte AT the field's end: fields whose last digit is the last byte of a group / a pass"""
    rng = np.random.default_rng(12)
    fields = []
    for end in (16, 32, P - 1, P, P + 1, 2 * P):
        for w in (1, 2, 3):
            f = seam_field(rng, end, [(end - 1, w)])[:end]
            assert len(f) == end and f[-w:].isdigit() and (w == end or f[-w - 1:-w] == b" ")
            fields.append(f)
    blob, rows = pack(fields, align=16)
    HW = max(len(f.split()) for f in fields)
    got, st = run(gpu, blob, rows, 1, HW, 0)
    for i, f in enumerate(fields):
        assert np.array_equal(got[i], bits(ref_image(f, 1, HW, 0))), i
        assert st[i, 0] == len(f.split())


def test_separator_runs(gpu):
    fields = [b"  1 2 3   4 5\t6", b"\t\t 10  20\t30 \t 40   50 60 \t ", b"1 2 3 4 5 6      ", b"      1 2 3 4 5 6",
              b" " * 40 + b"7 8 9 10 11 12" + b"\t" * 33, b"255\t0\t255\t0\t255\t0"]
    for transpose in (0, 1):
        for align in (None, 16, 13):
            check_fields(gpu, fields, 2, 3, transpose, align=align)


@pytest.mark.parametrize("fill", [0, 5, 15])
def test_field_ends_at_the_last_byte_of_the_buffer(gpu, fill):
    rng = np.random.default_rng(20 + fill)
    f = rand_field(rng, 12)
    lead = b"9" * ((fill - len(f)) % 16)                   # len(lead + f) % 16 == fill: 0 leaves no padding at all
    blob = lead + f
    assert len(blob) % 16 == fill
    rows = [[len(lead), len(blob), -1, -1, 1, 0, 0, 0]]
    for transpose in (0, 1):
        got, st = run(gpu, blob, rows, 4, 3, transpose, tail=b"")
        assert np.array_equal(got[0], bits(ref_image(f, 4, 3, transpose))) and st[0].tolist() == [12, 0]


@pytest.mark.parametrize("H,W", [(3, 5), (5, 3), (1, 7), (7, 1), (48, 48)])
def test_layouts(gpu, H, W):
    rng = np.random.default_rng(H * 100 + W)
    fields = [rand_field(rng, H * W) for _ in range(3)]
    t0, _ = check_fields(gpu, fields, H, W, 0)
    t1, _ = check_fields(gpu, fields, H, W, 1)
    for a, b in zip(t0, t1):      # transpose=1 is the MATLAB (column-major) H x W array of the row-major image
        assert np.array_equal(b.reshape(W, H), a.reshape(H, W).T)


@pytest.mark.parametrize("H,W", [(64, 64), (17, 241), (65, 64)])
def test_images_on_both_sides_of_the_staging_limit(gpu, H, W):
    """4096 floats are assembled in LDS, 4097 and more are stored from the threads"""
    rng = np.random.default_rng(H + W)
    fields = [rand_field(rng, H * W), rand_field(rng, H * W - 5), rand_field(rng, H * W + 3)]
    for transpose in (0, 1):
        check_fields(gpu, fields, H, W, transpose, align=3)


def _launches(L, fn):
    from mcncrossmodalemotions_amd import prof
    return {r.name: r.launches for r in prof.kernels_run(fn, L)[1]}


def csv_text(fields, usages=None, quote=lambda i: i % 3 == 0, eol=b"\n"):
    lines = [b"emotion,pixels,Usage"]
    for i, f in enumerate(fields):
        u = (usages[i] if usages is not None else "Training").encode()
        lines.append(b"%d," % (i % 7) + (b'"' + f + b'"' if quote(i) else f) + b"," + u)
    return eol.join(lines) + eol


@pytest.fixture(scope="module")
def faces():
    """257 rows of 48 x 48 with random values of 1 .. 3 digits, as CSV text, and their numpy parse"""
    rng = np.random.default_rng(48)
    fields = [rand_field(rng, 48 * 48) for _ in range(257)]
    want = np.stack([ref_image(f, 48, 48, 1) for f in fields])
    return fields, want


@pytest.mark.parametrize("N", [1, 2, 257])
def test_batch_sizes_in_one_launch(gpu, faces, N):
    from mcncrossmodalemotions_amd import _lib, vl
    fields, want = faces
    data = csv_text(fields[:N])
    plan = vl.pixcsv_plan(data)
    assert plan["N"] == N and [bytes(data[r[0]:r[1]]) for r in plan["rows"][:2]] == fields[:min(N, 2)]
    res = {}
    launches = _launches(_lib.load(), lambda: res.update(r=vl.pixcsv_decode(data, plan)))
    print("launches:", launches)
    assert launches == {"pixcsv_decode_kernel": 1}
    images, st = res["r"]
    assert tuple(images.shape) == (48, 48, 1, N) and images.permute(3, 2, 1, 0).is_contiguous()
    assert np.array_equal(st, np.tile(np.array([[2304, 0]], np.int32), (N, 1)))
    got = images.permute(3, 2, 1, 0).reshape(N, -1).cpu().numpy()
    assert np.array_equal(bits(got), bits(want[:N]))
    # as the H x W x 1 x N array: image n, row r, column c is number r * 48 + c of the field
    k = 5 * 48 + 7
    assert float(images[5, 7, 0, N - 1]) == float(fields[N - 1].split()[k])


def test_status_words_and_documented_values(gpu):
    cases = [
        (b"1 2a3 4", [1, 2, 3, 4], [4, BADCHAR]),                   # the byte separates like a blank
        (b"1,2 3 4", [1, 2, 3, 4], [4, BADCHAR]),
        (b"1 -2 3.5", [1, 2, 3, 5], [4, BADCHAR]),
        (b"1 2 \r3 4", [1, 2, 3, 4], [4, BADCHAR]),
        (b"1 256 3 4", [1, 255, 3, 4], [4, RANGE]),
        (b"1 0255 3 4", [1, 255, 3, 4], [4, RANGE]),
        (b"999 1000 00001 255", [255, 255, 255, 255], [4, RANGE]),
        (b"0 00 000 255", [0, 0, 0, 255], [4, 0]),                   # leading zeros within three digits are values
        (b"1 2 3", [1, 2, 3, 0], [3, COUNT]),
        (b"1 2 3 4 5", [1, 2, 3, 4], [5, COUNT]),
        (b"", [0, 0, 0, 0], [0, COUNT]),
        (b"   \t ", [0, 0, 0, 0], [0, COUNT]),
        (b"1 2 300 x", [1, 2, 255, 0], [3, BADCHAR | RANGE | COUNT]),
        (b"12345678901234567890 7", [255, 7, 0, 0], [2, RANGE | COUNT]),
    ]
    blob, rows = pack([c[0] for c in cases])
    for transpose in (0, 1):
        got, st = run(gpu, blob, rows, 2, 2, transpose)
        for i, (f, vals, want) in enumerate(cases):
            img = np.zeros(4, np.float32)
            k = np.arange(4)
            img[(k % 2) * 2 + k // 2 if transpose else k] = vals
            assert np.array_equal(got[i], bits(img)), (f, got[i].view(np.float32))
            assert st[i].tolist() == want, (f, st[i])
    # zero fill at the transposed positions of a 2 x 3 image with four of six numbers
    got, st = run(gpu, *pack([b"9 8 7 6"]), 2, 3, 1)
    assert got[0].view(np.float32).tolist() == [9, 6, 8, 0, 7, 0] and st[0].tolist() == [4, COUNT]


def test_skipped_permuted_and_unfitting_rows(gpu):
    rng = np.random.default_rng(5)
    fields = [rand_field(rng, 12) for _ in range(7)]
    blob, rows = pack(fields)
    want = np.stack([bits(ref_image(f, 3, 4, 1)) for f in fields])
    # a permutation into 9 slots: two slots are named by no row and stay untouched, one row is skipped
    slots = np.array([8, 3, -1, 0, 6, 1, 4])
    rows[:, 5] = slots
    got, st = run(gpu, blob, rows, 3, 4, 1, images=9)
    for i, s in enumerate(slots):
        if s >= 0:
            assert np.array_equal(got[s], want[i]) and st[i].tolist() == [12, 0]
    assert st[2].tolist() == [0, 0]
    for s in (2, 5, 7):
        assert (got[s] == GUARD_WORD).all()
    # an index whose image does not lie inside out_floats: flagged, nothing written (the guards are checked by run)
    rows[:, 5] = [0, 7, 2, 3, 1 << 40, 5, 6]
    got, st = run(gpu, blob, rows, 3, 4, 1, images=7)
    assert st[:, 1].tolist() == [0, NOFIT, 0, 0, NOFIT, 0, 0] and st[[1, 4], 0].tolist() == [0, 0]
    assert (got[1] == GUARD_WORD).all() and (got[4] == GUARD_WORD).all() and np.array_equal(got[0], want[0])


def test_vl_decode_placement_strictness_and_refusals(gpu, faces):
    from mcncrossmodalemotions_amd import _lib, vl
    fields, want = faces
    data = csv_text([fields[0][:100], fields[1], b"1 2 x", fields[2]])
    plan = vl.pixcsv_plan(data)
    with pytest.raises(_lib.XmError, match=r"line 2: \d+ numbers where 48 x 48 = 2304 are expected \(2 rows flagged\)"):
        vl.pixcsv_decode(data, plan)
    images, st = vl.pixcsv_decode(data, plan, strict=False)
    assert st[:, 1].tolist() == [COUNT, 0, BADCHAR | COUNT, 0] and st[2, 0] == 2
    assert np.array_equal(bits(images[:, :, 0, 3].contiguous().cpu().numpy().ravel()), bits(ref_image(fields[2], 48, 48, 0)))
    # image_base and out: rows land behind the images already there; skipped rows do not move the others
    rows = plan["rows"].copy()
    rows[:, 5] = [-1, 1, -1, 0]
    out = torch.full((5 * 2304,), 7.0, device=gpu)
    images, st = vl.pixcsv_decode(data, dict(plan, rows=rows), out=out, image_base=2)
    assert images.data_ptr() == out.data_ptr() and tuple(images.shape) == (48, 48, 1, 5) and st[:, 1].tolist() == [0, 0, 0, 0]
    flat = out.view(5, 2304).cpu().numpy()
    assert (flat[[0, 1, 4]] == 7).all() and np.array_equal(flat[3], want[1]) and np.array_equal(flat[2], want[2])
    with pytest.raises(_lib.XmError, match="line 3: image 5 of 48 x 48 does not fit OUT"):
        vl.pixcsv_decode(data, dict(plan, rows=rows), out=out, image_base=4)
    with pytest.raises(ValueError, match="byte ranges"):
        vl.pixcsv_decode(data[:200], plan)
    with pytest.raises(ValueError, match="OUT must be"):
        vl.pixcsv_decode(data, plan, out=out.cpu())


def test_chunked_decode_equals_the_single_call(gpu, faces):
    from mcncrossmodalemotions_amd import _lib, vl
    fields, want = faces
    n = 23
    data = csv_text(fields[:n], eol=b"\r\n")
    plan = vl.pixcsv_plan(data)
    single, st1 = vl.pixcsv_decode(data, plan)
    for chunk in (3 * plan["longest"] + 100, plan["longest"], 1):
        cuts = vl._pix_chunks(plan["rows"], chunk)
        assert len(cuts) >= 3
        res = {}
        launches = _launches(_lib.load(), lambda: res.update(r=vl.pixcsv_decode(data, plan, chunk_bytes=chunk)))
        assert launches == {"pixcsv_decode_kernel": len(cuts)}
        parts, st = res["r"]
        assert torch.equal(parts.contiguous().view(torch.int32), single.contiguous().view(torch.int32)) and np.array_equal(st, st1)
    assert np.array_equal(bits(single.permute(3, 2, 1, 0).reshape(n, -1).cpu().numpy()), bits(want[:n]))


# ------------------------------------------------------------------------------------------------ end to end
VOTE_HEADER = "Usage,Image name,neutral,happiness,surprise,sadness,anger,disgust,fear,contempt,unknown,NF"


@pytest.fixture(scope="module")
def fer_dir(tmp_path_factory, faces):
    """a CSV pair of 70 rows: 64 images (48 Training, 8 PublicTest, 8 PrivateTest), 3 rows FER+ removed, 3 rows without
    a vote among the eight emotions; and the host restatement of what getFerPlusImdb makes of it"""
    fields, want = faces
    rng = np.random.default_rng(64)
    d = str(tmp_path_factory.mktemp("fer2013+"))
    usages, names, votes = [], [], []
    for i in range(70):
        usages.append("Training" if i < 52 else "PublicTest" if i < 61 else "PrivateTest")
        v = rng.multinomial(10, rng.dirichlet(np.full(10, 0.3)))
        if v[:8].sum() == 0:
            v[int(rng.integers(0, 8))] += 1
        names.append("fer%07d.png" % i)
        if i in (4, 30, 55):
            names[-1], v = "", np.zeros(10, int)
        if i in (9, 40, 65):
            v = np.array([0] * 8 + [6, 4])
        votes.append(v)
    with open(os.path.join(d, "fer2013.csv"), "wb") as fh:
        fh.write(csv_text(fields[:70], usages))
    with open(os.path.join(d, "fer2013new.csv"), "w") as fh:
        fh.write(VOTE_HEADER + "\n" + "".join("%s,%s,%s\n" % (u, n, ",".join(map(str, v))) for u, n, v in zip(usages, names, votes)))
    keep = np.array([i not in (4, 30, 55, 9, 40, 65) for i in range(70)])
    votes = np.array(votes, float)[keep]
    host = dict(data=np.asfortranarray(want[:70][keep].reshape(64, 48, 48).transpose(2, 1, 0)[:, :, None, :]),   # H x W x 1 x N
                votes=votes, set=np.array([1] * 48 + [2] * 8 + [3] * 8),
                hardLabels=(votes[:, :8].argmax(1) + 1).reshape(1, 64).astype(np.float64),
                ferLabels=(np.arange(70) % 7)[keep].astype(float), row=(np.arange(70) + 2)[keep])
    return d, host, fields


def test_get_ferplus_imdb_equals_the_host_restatement(gpu, fer_dir):
    from mcncrossmodalemotions_amd import batch
    d, host, fields = fer_dir
    imdb = batch.getFerPlusImdb(d, "CNTK", chunk_bytes=5 * 9000)
    im = imdb.images
    assert im["data"].is_cuda and tuple(im["data"].shape) == (48, 48, 1, 64)
    # image 0, row 2, column 9 is number 2 * 48 + 9 of the first row's field
    assert float(im["data"][2, 9, 0, 0]) == float(fields[0].split()[2 * 48 + 9])
    from mcncrossmodalemotions_amd import vl
    assert np.array_equal(bits(vl.to_numpy(im["data"])), bits(host["data"]))
    for k in ("votes", "set", "hardLabels", "ferLabels", "row"):
        assert np.array_equal(np.asarray(im[k]), host[k]), k
    assert imdb.meta["classes"] == batch.FERPLUS_CLASSES
    full = batch.getFerPlusImdb(d, "full")
    assert tuple(full.images["data"].shape) == (48, 48, 1, 67) and full.images["row"].tolist() == [i + 2 for i in range(70) if i not in (4, 30, 55)]
    # getBatchFerPlus on it equals getBatchFerPlus on an imdb that holds the numpy parse, with the same draws
    ref = batch.SyntheticFerPlusImdb.__new__(batch.SyntheticFerPlusImdb)
    ref.images = {k: host[k] for k in ("data", "votes", "set", "hardLabels")}
    ref.meta, ref._dev = {"classes": list(batch.FERPLUS_CLASSES)}, {}
    for idx, loss in ((list(range(3, 19)), "distributions"), (list(range(48, 56)), "distributions"), ([60, 56, 63], "softmaxlog")):
        a = batch.getBatchFerPlus(imdb, idx, lossType=loss, rng=np.random.default_rng(8), device=gpu)
        b = batch.getBatchFerPlus(ref, idx, lossType=loss, rng=np.random.default_rng(8), device=gpu)
        assert a[0::2] == b[0::2] and len(a) == (6 if loss == "distributions" else 4)
        for x, y in zip(a[1::2], b[1::2]):
            assert x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def test_a_bad_pixel_field_names_its_line(gpu, fer_dir, tmp_path):
    from mcncrossmodalemotions_amd import _lib, batch
    d, _, _ = fer_dir
    txt = open(os.path.join(d, "fer2013.csv"), "rb").read().split(b"\n")
    txt[12] = txt[12].replace(b" ", b" 300 ", 1)
    (tmp_path / "fer2013.csv").write_bytes(b"\n".join(txt))
    (tmp_path / "fer2013new.csv").write_bytes(open(os.path.join(d, "fer2013new.csv"), "rb").read())
    with pytest.raises(_lib.XmError, match="line 13: a number above 255.*2305 numbers where 48 x 48 = 2304"):
        batch.getFerPlusImdb(str(tmp_path))


def test_ferplus_baselines_and_benchmark_from_the_csv_pair(gpu, fer_dir, tmp_path, monkeypatch):
    from mcncrossmodalemotions_amd import batch
    from mcncrossmodalemotions_amd import benchmark_ferplus_models as bm
    from mcncrossmodalemotions_amd import ferplus_baselines as fb
    d, host, _ = fer_dir
    made = []
    real = batch.getFerPlusImdb
    monkeypatch.setattr(batch, "getFerPlusImdb", lambda *a, **k: made.append(real(*a, **k)) or made[-1])
    narrow = dict(widthMult=0.125, blocks=(1, 1, 1, 1))
    net, info = fb.ferplus_baselines(dataDir=d, numEpochs=1, batchSize=8, expRoot=str(tmp_path / "exp"), **narrow)
    assert len(made) == 1 and made[0].images["data"].is_cuda
    assert len(info["train"]) == 1 and info["train"][0]["num"] == 48 and info["val"][0]["num"] == 8
    for st in info["train"] + info["val"]:
        assert np.isfinite(st["objective"]) and 0 <= st["classerror"] <= 1
    assert os.listdir(str(tmp_path / "exp" / "senet50_ft-dag-distributions-CNTK-dropout-0.5-aug")) == ["net-epoch-1.pt"]
    # benchmark_ferplus_models on the same directory: two models, val and test, cached and reused
    cache = str(tmp_path / "benchCache")
    res = bm.benchmark_ferplus_models(dataDir=d, benchmarkCacheDir=cache, verbose=False, **narrow)
    assert len(made) == 5 and sorted(res) == ["resnet50-ferplus", "senet50-ferplus"]
    for s in res.values():
        assert 0 <= s["valAcc"] <= 1 and 0 <= s["testAcc"] <= 1 and round(s["valAcc"] * 8) == pytest.approx(s["valAcc"] * 8)
    assert sorted(os.listdir(cache)) == ["resnet50-ferplus.json", "senet50-ferplus.json"]
    again = bm.benchmark_ferplus_models(dataDir=d, benchmarkCacheDir=cache, verbose=False, **narrow)
    assert again == res and len(made) == 5
