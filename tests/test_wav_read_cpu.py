"""CPU: the host side of vl.audioread.  A numpy restatement of the RIFF / WAVE parse and of the sample conversions is
written here (np_parse, np_decode); it equals the samples stored in tests/golden/wav_small.npz (computed by
make_golden_wav.py from the values the files were written from) and, where scipy imports, scipy.io.wavfile.read
normalised by 2^(container bits - 1).  vl.audioinfo and the descriptors, offsets and sizes of xm_wav_plan equal the
restatement for the whole set in two orders, with ranges, with a channel and with an out_base; every rejection gives its
documented code and names the file's index.  Nothing here opens a device.  tests/wav_plan_check.cpp -- csrc/wav_plan.h
alone, every truncation and single-byte mutation of a valid file per format -- is built with the address and
undefined-behaviour sanitizers and run as a program of its own."""
import ctypes as C
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wav_small.npz")
U8, S16, S24, S32, F32, F64 = range(6)
EINVAL, ENOTSUP = 1, 5


# ---------------------------------------------------------------------------------------------------- the restatement
def np_parse(data):
    """audioinfo of one file: dict(begin, end, rate, nch, bits, fmt, align, total, truncated)"""
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE"
    pos, info = 12, None
    while True:
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = pos + 8
        if tag == b"fmt " and info is None:
            code, nch, rate, _, align, bits = struct.unpack("<HHIIHH", data[body:body + 16])
            if code == 0xFFFE:
                code = struct.unpack("<H", data[body + 24:body + 26])[0]
            fmt = {(1, 8): U8, (1, 16): S16, (1, 24): S24, (1, 32): S32, (3, 32): F32, (3, 64): F64}[(code, bits)]
            info = dict(rate=rate, nch=nch, bits=bits, fmt=fmt, align=align)
        elif tag == b"data":
            end = min(body + size, len(data))
            info.update(begin=body, end=end, truncated=int(body + size > len(data)), total=(end - body) // info["align"])
            return info
        pos = body + size + (size & 1)


def np_decode(data, rng=None, channel=None):
    """float32 samples of audioread(file, rng)(:, channel + 1), flattened in MATLAB layout"""
    w = np_parse(data)
    raw = np.frombuffer(data, np.uint8)[w["begin"]:w["begin"] + w["total"] * w["align"]]
    nch, total = w["nch"], w["total"]
    if w["fmt"] == U8:
        y = (raw.astype(np.float64) - 128) / 128
    elif w["fmt"] == S16:
        y = raw.view("<i2").astype(np.float64) / 2.0 ** 15
    elif w["fmt"] == S24:
        b = raw.reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        y = (v - ((v >> 23) << 24)).astype(np.float64) / 2.0 ** 23
    elif w["fmt"] == S32:
        y = raw.view("<i4").astype(np.float64) / 2.0 ** 31
    elif w["fmt"] == F32:
        y = raw.view("<f4")
    else:
        y = raw.view("<f8")
    with np.errstate(over="ignore", under="ignore"):
        y = y.astype(np.float32).reshape(total, nch)
    a, b = (1, total) if rng is None else (int(rng[0]), total if rng[1] == -1 else int(rng[1]))
    y = y[a - 1:b]
    if channel is not None:
        y = y[:, channel:channel + 1]
    return np.ascontiguousarray(y.T).reshape(-1)


def np_plan(files, ranges=None, channel=None, out_base=0):
    """the N x 16 descriptor table and [floats, N] of xm_wav_plan"""
    rows, off, out = [], 0, out_base
    for i, f in enumerate(files):
        w = np_parse(f)
        a, b = (1, w["total"]) if ranges is None else (int(ranges[i][0]), w["total"] if ranges[i][1] == -1 else int(ranges[i][1]))
        cw = w["nch"] if channel is None else 1
        rows.append([off + w["begin"], off + w["end"], w["rate"], w["nch"], w["bits"], w["fmt"], w["total"], a - 1, b - a + 1, cw,
                     -1 if channel is None else channel, out, w["truncated"], w["align"], 0, 0])
        out += (b - a + 1) * cw
        off += len(f)
    return np.array(rows, np.int64).reshape(len(files), 16), [out - out_base, len(files)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def names(golden):
    return [str(n) for n in golden["names"]]


def files_of(golden, names):
    return [golden["bytes_" + n].tobytes() for n in names]


def c_plan(files, ranges=None, channel=-1, out_base=0):
    """xm_wav_plan through ctypes on plain host memory -> (rc, desc N x 16, sizes, message)"""
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    N = len(files)
    blob = np.frombuffer(b"".join(files) + b"\0", np.uint8).copy()
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    desc = np.full((max(N, 1), 16), -7, np.int64)
    sizes = np.full(2, -7, np.int64)
    r = None if ranges is None else np.ascontiguousarray(ranges, np.int64)
    rc = L.xm_wav_plan(C.c_void_p(blob.ctypes.data), C.c_void_p(offsets.ctypes.data), N,
                       None if r is None else C.c_void_p(r.ctypes.data), channel, out_base, C.c_void_p(desc.ctypes.data),
                       C.c_void_p(sizes.ctypes.data))
    return rc, desc[:N], sizes, L.xm_last_error().decode()


# ---------------------------------------------------------------------------------------------------- tests
def test_fixture_set_is_what_the_generator_promises(golden, names):
    assert os.path.getsize(GOLDEN) < 200 * 1024
    for f in ("u8", "s16", "s24", "s32", "f32", "f64"):
        for n in (1, 5, 64, 257):
            assert "%s_m%d" % (f, n) in names
    for n in ("s16_m1023", "s16_m1024", "s16_m1025", "s16_m4097", "s16_st33", "s24_st21", "f32_st17", "u8_3ch19", "ext_s16_st9",
              "ext_s24_m10", "ext_f32_m11", "chunks_s16_m40", "streamed_s16_m30", "empty_s16", "edge_s16", "edge_s32", "edge_f64",
              "edge_f32"):
        assert n in names
    s = golden["bytes_streamed_s16_m30"]
    assert len(s) & 1 and golden["meta_streamed_s16_m30"][5] == 1 and (len(s) - 44) == 61
    assert len(golden["bad_names"]) == 21


def test_restatement_equals_the_stored_samples(golden, names):
    for n in names:
        data = golden["bytes_" + n].tobytes()
        w, meta = np_parse(data), golden["meta_" + n]
        assert [w["rate"], w["nch"], w["bits"], w["fmt"], w["total"], w["truncated"]] == list(meta), n
        got = bits(np_decode(data))
        assert got.shape == golden["exp_" + n].shape and np.array_equal(got, golden["exp_" + n]), n
    # the values the issue names
    e = golden["exp_edge_s16"].view(np.float32)
    assert e[0] == -1.0 and e[1] == np.float32(32767 / 32768)
    e = golden["exp_edge_s32"].view(np.float32)
    assert e[0] == 1.0 and e[1] == -1.0 and e[2] == np.float32(2.0 ** -7) and e[3] == np.float32((2 ** 24 + 4) / 2.0 ** 31)
    e = golden["exp_edge_f64"]
    assert e[0] == 0x3EAAAAAB and e[2] == 0 and e[5] == 1 and e[6] == 0 and e[7] == 1 and e[8] == 2 and e[9] == 2
    assert list(golden["exp_edge_f32"][:4]) == [0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FA00000]


def test_restatement_equals_scipy(golden, names):
    wavfile = pytest.importorskip("scipy.io.wavfile")
    checked = 0
    for n in names:
        if n.startswith(("edge_f", "streamed", "empty")):     # NaN payloads and the cut file are not scipy's business
            continue
        data = golden["bytes_" + n].tobytes()
        w = np_parse(data)
        rate, v = wavfile.read(io.BytesIO(data))
        v = v.reshape(w["total"], w["nch"])
        if w["fmt"] == U8:
            y = (v.astype(np.float64) - 128) / 128
        elif w["fmt"] in (F32, F64):
            y = v.astype(np.float64)
        else:
            # 24-bit comes back as int32 shifted left by 8: the same value over 2^31
            y = v.astype(np.float64) / 2.0 ** ((32 if w["fmt"] == S24 else w["bits"]) - 1)
        assert rate == w["rate"]
        assert np.array_equal(bits(np.ascontiguousarray(y.astype(np.float32).T).reshape(-1)), golden["exp_" + n]), n
        checked += 1
    assert checked >= 35


def test_audioinfo_equals_the_restatement(golden, names, tmp_path):
    import torch
    from mcncrossmodalemotions_amd import vl
    before = torch.cuda.is_initialized()
    files = files_of(golden, names)
    info = vl.audioinfo(files)
    assert len(info) == len(files)
    for n, f, i in zip(names, files, info):
        w = np_parse(f)
        assert (i["SampleRate"], i["TotalSamples"], i["NumChannels"], i["BitsPerSample"]) == (w["rate"], w["total"], w["nch"], w["bits"]), n
        assert i["Duration"] == w["total"] / w["rate"] and i["Truncated"] == bool(w["truncated"])
    p = tmp_path / "a.wav"
    p.write_bytes(files[3])
    assert vl.audioinfo([str(p)]) == info[3:4] and vl.audioinfo([]) == []
    assert torch.cuda.is_initialized() == before


@pytest.mark.parametrize("seed", [0, 1])
def test_plan_equals_the_restatement(golden, names, seed):
    import torch
    before = torch.cuda.is_initialized()
    order = np.random.default_rng(seed).permutation(len(names)) if seed else np.arange(len(names))
    files = files_of(golden, [names[i] for i in order])
    want, wsizes = np_plan(files)
    rc, desc, sizes, _ = c_plan(files)
    assert rc == 0 and np.array_equal(desc, want) and list(sizes) == wsizes
    assert wsizes[0] == sum(len(golden["exp_" + names[i]]) for i in order)
    # out_base shifts the output offsets only
    want, wsizes = np_plan(files, out_base=12345)
    rc, desc, sizes, _ = c_plan(files, out_base=12345)
    assert rc == 0 and np.array_equal(desc, want) and list(sizes) == wsizes and desc[0, 11] == 12345
    # ranges ([2 T-1] where the file has three frames, [1 -1] = the whole file elsewhere) and a channel
    nz = [f for f in files if np_parse(f)["total"] > 0]
    ranges = [(2, np_parse(f)["total"] - 1) if np_parse(f)["total"] >= 3 else (1, -1) for f in nz]
    for channel in (None, 0):
        want, wsizes = np_plan(nz, ranges, channel, 3)
        rc, desc, sizes, _ = c_plan(nz, ranges, -1 if channel is None else 0, 3)
        assert rc == 0 and np.array_equal(desc, want) and list(sizes) == wsizes
    st = [f for f in files if np_parse(f)["nch"] >= 2]
    want, wsizes = np_plan(st, None, 1)
    rc, desc, sizes, _ = c_plan(st, None, 1)
    assert len(st) == 5 and rc == 0 and np.array_equal(desc, want) and list(sizes) == wsizes
    assert c_plan([])[0] == 0 and list(c_plan([])[2]) == [0, 0]
    assert torch.cuda.is_initialized() == before


def test_vl_wav_plan_lays_the_staging_buffer_out(golden, names):
    from mcncrossmodalemotions_amd import vl
    files = files_of(golden, names)
    buf, plan = vl.wav_plan(files, out_base=5)
    want, wsizes = np_plan(files, out_base=5)
    assert np.array_equal(plan["rows"], want) and plan["floats"] == wsizes[0] and plan["N"] == len(files)
    assert bytes(buf[:plan["nbytes"]]) == b"".join(files)
    assert plan["desc"][0] % 16 == 0 and plan["desc"][0] > plan["nbytes"] and plan["total"] % 16 == 0
    assert plan["total"] >= plan["desc"][0] + plan["desc"][1] and buf.size == plan["total"]
    _, one = vl.wav_plan(files[:3], ranges=[1, float("inf")])
    assert np.array_equal(one["rows"], np_plan(files[:3])[0])


def test_every_rejection_gives_its_code_and_names_the_file(golden, names):
    good = golden["bytes_s16_m5"].tobytes()
    for n in (str(b) for b in golden["bad_names"]):
        data, code = golden["bad_" + n].tobytes(), int(golden["badcode_" + n])
        for k, files in ((0, [data]), (2, [good, good, data, good])):
            rc, _, _, msg = c_plan(files)
            assert rc == code, (n, rc, msg)
            assert "file %d:" % k in msg, (n, msg)
    not_sup = {n for n in (str(b) for b in golden["bad_names"]) if int(golden["badcode_" + n]) == ENOTSUP}
    assert not_sup == {"rf64", "bw64", "rifx", "alaw", "mulaw", "adpcm", "mpeg", "ext_valid20", "pcm12", "float16"}


def test_ranges_outside_the_file_are_errors(golden):
    from mcncrossmodalemotions_amd import _lib, vl
    f, e = golden["bytes_s16_m64"].tobytes(), golden["bytes_empty_s16"].tobytes()
    for r in ((0, 5), (1, 65), (6, 5), (65, 65), (-3, -1), (1, -2)):
        rc, _, _, msg = c_plan([f, f], [(1, 64), r])
        assert rc == EINVAL and "file 1:" in msg and "range" in msg, (r, msg)
    for r in ((1, 64), (64, 64), (1, 1), (1, -1), (64, -1)):
        assert c_plan([f], [r])[0] == 0
    assert c_plan([e], [(1, -1)])[0] == EINVAL              # audioread(file, [1 0]) of an empty file fails in MATLAB too
    rc, _, _, msg = c_plan([f, f], None, 1)
    assert rc == EINVAL and "file 0:" in msg and "channel" in msg
    assert c_plan([f], None, -2)[0] == EINVAL and c_plan([f], None, -1, -1)[0] == EINVAL
    with pytest.raises(_lib.XmError, match="file 1"):
        vl.audioinfo([f, golden["bad_alaw"].tobytes()])
    L = _lib.load()
    assert L.xm_version() >= 114
    # the device entry validates its arguments before any device call
    assert L.xm_wav_decode_batch(None, 0, None, 0, None, 0, None) == 0
    assert L.xm_wav_decode_batch(None, 16, None, 1, None, 4, None) == EINVAL
    assert L.xm_wav_decode_batch(None, -1, None, 0, None, 0, None) == EINVAL
    assert L.xm_wav_decode_batch(None, 0, None, -1, None, 0, None) == EINVAL
    assert L.xm_wav_decode_batch(None, 0, None, 0, None, -1, None) == EINVAL


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_wav_plan_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wav_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "wav_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    assert int(r.stdout.split()[0]) > 5000      # every truncation and mutation ran


def wav_bytes(fmt, v, rate=16000):
    """a plain WAV file of a frames x channels array of the format's own values (S24 as int32) -- for the tests that need
    files the fixture set does not hold"""
    v = np.asarray(v)
    v = v.reshape(v.shape[0], -1)
    bits_ = {U8: 8, S16: 16, S24: 24, S32: 32, F32: 32, F64: 64}[fmt]
    if fmt == S24:
        body = np.ascontiguousarray(v.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3]).tobytes()
    else:
        body = np.ascontiguousarray(v.astype({U8: "u1", S16: "<i2", S32: "<i4", F32: "<f4", F64: "<f8"}[fmt])).tobytes()
    nch, align = v.shape[1], v.shape[1] * bits_ // 8
    head = struct.pack("<HHIIHH", 3 if fmt in (F32, F64) else 1, nch, rate, rate * align, align, bits_)
    riff = b"WAVE" + b"fmt " + struct.pack("<I", 16) + head + b"data" + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")
    return b"RIFF" + struct.pack("<I", len(riff)) + riff


def random_values(rng, fmt, frames, nch=1):
    if fmt in (F32, F64):
        return (rng.standard_normal((frames, nch)) * 0.3).astype(np.float32 if fmt == F32 else np.float64)
    b = {U8: 8, S16: 16, S24: 24, S32: 32}[fmt]
    lo = 0 if fmt == U8 else -2 ** (b - 1)
    return rng.integers(lo, lo + 2 ** b, (frames, nch)).astype(np.uint8 if fmt == U8 else np.int16 if fmt == S16 else np.int32)


def test_wav_bytes_helper_round_trips():
    rng = np.random.default_rng(3)
    for fmt in range(6):
        v = random_values(rng, fmt, 9, 2)
        w = np_parse(wav_bytes(fmt, v))
        assert (w["fmt"], w["nch"], w["total"], w["truncated"]) == (fmt, 2, 9, 0)
        if fmt in (S16, S24, S32):
            want = (v.astype(np.float64) / 2.0 ** (w["bits"] - 1)).astype(np.float32)
            assert np.array_equal(np_decode(wav_bytes(fmt, v)), want.T.reshape(-1))
