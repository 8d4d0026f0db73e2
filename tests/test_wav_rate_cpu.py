"""CPU: the host side of vl.audioread(fs=) -- xm_wav_plan_fs.  For 48000, 44100, 22050, 11025, 8000, 32000, 192000 and
16000 Hz files brought to 16000 Hz: p, q = fs / SampleRate in lowest terms (slots 14, 15), ceil(frames p / q) output
floats per channel written, the output offsets and `sizes`, at frame counts whose product with p leaves 0, 1 and q - 1
modulo q, for empty files, for 2- and 3-channel files with and without a channel, with ranges, an out_base and files
cut short; the other slots are xm_wav_plan's.  The three refusals of a ratio name the file; the symbols are declared,
typed and exported; the device entry checks its arguments before any device call; vl.audioinfo(fs=) and the lengths of
batch.WavFileEmoVoxImdb(resample=True) come from the plan alone.  Nothing here opens a device.
tests/wav_rate_plan_check.cpp -- the header alone over truncations and mutations of such files -- is built with the
address and undefined-behaviour sanitizers and run as a program of its own."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from test_wav_read_cpu import EINVAL, ENOTSUP, F32, ROOT, S16, S24, U8, c_plan, np_parse, random_values, wav_bytes

FS = 16000
RATES = [48000, 44100, 22050, 11025, 8000, 32000, 192000, 16000]
RATIO = {48000: (1, 3), 44100: (160, 441), 22050: (320, 441), 11025: (640, 441), 8000: (2, 1), 32000: (1, 2),
         192000: (1, 12), 16000: (1, 1)}
SAME = [k for k in range(16) if k not in (8, 9, 10, 11, 14, 15)]     # the slots that are xm_wav_plan's whatever fs is


def c_plan_fs(files, fs=FS, ranges=None, channel=-1, out_base=0):
    """xm_wav_plan_fs through ctypes on plain host memory -> (rc, desc N x 16, sizes, message)"""
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    N = len(files)
    blob = np.frombuffer(b"".join(files) + b"\0", np.uint8).copy()
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    desc = np.full((max(N, 1), 16), -7, np.int64)
    sizes = np.full(2, -7, np.int64)
    r = None if ranges is None else np.ascontiguousarray(ranges, np.int64)
    rc = L.xm_wav_plan_fs(C.c_void_p(blob.ctypes.data), C.c_void_p(offsets.ctypes.data), N,
                          None if r is None else C.c_void_p(r.ctypes.data), channel, fs, out_base, C.c_void_p(desc.ctypes.data),
                          C.c_void_p(sizes.ctypes.data))
    return rc, desc[:N], sizes, L.xm_last_error().decode()


def ceil_div(a, b):
    return -(-a // b)


def frames_with_remainder(p, q, r, at_least=5):
    """the smallest frame count >= at_least with frames * p % q == r, or None when no count has it"""
    for n in range(at_least, at_least + q + 1):
        if n * p % q == r:
            return n
    return None


def pcm(frames, nch=1, rate=FS, fmt=S16, seed=0):
    if frames == 0:                                  # wav_bytes needs a frame: its header with an empty data chunk
        one = wav_bytes(fmt, random_values(np.random.default_rng(seed), fmt, 1, nch), rate)
        return one[:4] + struct.pack("<I", 36) + one[8:40] + struct.pack("<I", 0)
    return wav_bytes(fmt, random_values(np.random.default_rng(seed), fmt, frames, nch), rate)


def test_symbols_are_declared_typed_and_exported():
    from mcncrossmodalemotions_amd import _lib, vl
    L = _lib.load()
    assert L.xm_version() >= 122
    hdr = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    assert "122 = + xm_wav_plan_fs, xm_wav_decode_resample_batch, xm_wav_resample_geometry" in hdr
    for name, nargs in (("xm_wav_plan_fs", 9), ("xm_wav_decode_resample_batch", 7), ("xm_wav_resample_geometry", 2)):
        assert "int %s(" % name in hdr
        assert len(_lib.SIGNATURES[name]) == nargs and getattr(L, name).restype is C.c_int
    assert _lib.SIGNATURES["xm_wav_plan_fs"][5] is C.c_longlong and _lib.SIGNATURES["xm_wav_plan_fs"][6] is C.c_longlong
    assert _lib.SIGNATURES["xm_wav_decode_resample_batch"] == _lib.SIGNATURES["xm_wav_decode_batch"]
    import torch
    before = torch.cuda.is_initialized()
    tile, launches = vl.wav_resample_geometry()
    assert tile >= 256 and tile % 256 == 0 and launches == 2
    assert L.xm_wav_resample_geometry(None, None) == 0
    assert torch.cuda.is_initialized() == before


@pytest.mark.parametrize("rate", RATES)
def test_ratio_counts_and_offsets(rate):
    p, q = RATIO[rate]
    g = math.gcd(FS, rate)
    assert (p, q) == (FS // g, rate // g)
    counts = sorted({n for n in (frames_with_remainder(p, q, r) for r in (0, 1, q - 1)) if n is not None} | {0, 1, 2, 3})
    assert {n * p % q for n in counts if n >= 5} == {r for r in (0, 1, q - 1) if r < q}
    for nch, channel in ((1, None), (1, 0), (2, None), (2, 0), (2, 1), (3, None), (3, 0), (3, 1)):
        files = [pcm(n, nch, rate, seed=n) for n in counts]
        sel = -1 if channel is None else channel
        rc, desc, sizes, msg = c_plan_fs(files, FS, None, sel, 11)
        assert rc == 0, msg
        rc0, plain, sizes0, _ = c_plan(files, None, sel, 11)
        assert rc0 == 0 and np.array_equal(desc[:, SAME], plain[:, SAME]) and (plain[:, 14:] == 0).all()
        cw = nch if channel is None else 1
        out = 11
        for n, d in zip(counts, desc):
            assert (d[14], d[15]) == (p, q) and d[2] == rate
            assert (d[8], d[9], d[10]) == (n, cw, sel)                  # slot 8 stays the SOURCE frames decoded
            assert d[11] == out, (n, nch, channel)
            out += ceil_div(n * p, q) * cw
        assert list(sizes) == [out - 11, len(files)]
        if rate == FS:
            assert np.array_equal(desc[:, :14], plain[:, :14]) and list(sizes) == list(sizes0)


def test_mixed_rates_in_one_batch():
    frames = [1000, 441, 0, 882, 77, 3, 4097, 12]
    files = [pcm(n, 1 + k % 2, r, (U8, S16, S24, F32)[k % 4], k) for k, (n, r) in enumerate(zip(frames, RATES))]
    rc, desc, sizes, msg = c_plan_fs(files)
    assert rc == 0, msg
    plain = c_plan(files)[1]
    assert np.array_equal(desc[:, SAME], plain[:, SAME])
    out = 0
    for n, r, d in zip(frames, RATES, desc):
        assert (d[14], d[15]) == RATIO[r] and d[11] == out
        out += ceil_div(n * d[14], d[15]) * d[9]
    assert sizes[0] == out
    # another target rate: 44100 -> 22050 is 1 / 2, 16000 -> 22050 is 441 / 320
    rc, desc, sizes, _ = c_plan_fs(files, 22050)
    assert rc == 0 and [(int(d[14]), int(d[15])) for d in desc] == [(147, 320), (1, 2), (1, 1), (2, 1), (441, 160), (441, 640), (147, 1280), (441, 320)]
    assert c_plan_fs([])[0] == 0 and list(c_plan_fs([])[2]) == [0, 0]


def test_ranges_out_base_and_truncated_files():
    T = 1000
    f44, f48 = pcm(T, 2, 44100, seed=1), pcm(T, 1, 48000, S24, seed=2)
    ranges = [(1, -1), (1, T), (2, T - 1), (T, T), (442, 882), (1, 441), (100, 540), (7, 9)]
    for data, (p, q) in ((f44, (160, 441)), (f48, (1, 3))):
        for channel in (-1, 0):
            rc, desc, sizes, msg = c_plan_fs([data] * len(ranges), FS, ranges, channel, 1 << 33)
            assert rc == 0, msg
            plain = c_plan([data] * len(ranges), ranges, channel, 1 << 33)[1]
            assert np.array_equal(desc[:, SAME], plain[:, SAME]) and np.array_equal(desc[:, 7:11], plain[:, 7:11])
            out = 1 << 33
            for (a, b), d in zip(ranges, desc):
                n = (T if b == -1 else b) - a + 1
                assert (d[7], d[8], d[11]) == (a - 1, n, out)           # the range is in SOURCE frames
                out += ceil_div(n * p, q) * d[9]
            assert sizes[0] == out - (1 << 33)
    for r in ((0, 5), (1, T + 1), (6, 5)):
        rc, _, _, msg = c_plan_fs([f48, f48], FS, [(1, T), r])
        assert rc == EINVAL and "file 1:" in msg and "range" in msg
    # a file cut short: what is there is decoded, flagged, and counted at the new rate
    w = np_parse(f48)
    cut = f48[:w["begin"] + 3 * 601 + 2]                                  # 601 frames and two bytes of the next
    rc, desc, sizes, _ = c_plan_fs([f48, cut, f48])
    assert rc == 0 and list(desc[:, 12]) == [0, 1, 0] and desc[1, 8] == desc[1, 6] == 601
    assert list(desc[:, 11]) == [0, 334, 334 + 201] and sizes[0] == 334 + 201 + 334
    streamed = bytearray(f44)
    b44 = np_parse(f44)["begin"]
    streamed[b44 - 4:b44] = b"\xff\xff\xff\xff"                          # a streamed writer's data size
    rc, desc, sizes, _ = c_plan_fs([bytes(streamed)], FS, None, 1)
    assert rc == 0 and desc[0, 12] == 1 and desc[0, 8] == T and sizes[0] == ceil_div(T * 160, 441)
    # negative or zero fs, and the plain plan's refusals word for word
    assert c_plan_fs([f48], 0)[0] == EINVAL and c_plan_fs([f48], -16000)[0] == EINVAL
    assert c_plan_fs([f48], FS, None, -2)[0] == EINVAL and c_plan_fs([f48], FS, None, -1, -1)[0] == EINVAL
    rc, _, _, msg = c_plan_fs([f48, f48], FS, None, 1)
    assert rc == EINVAL and msg == c_plan([f48, f48], None, 1)[3] and "file 0:" in msg and "channel" in msg
    golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "wav_small.npz")))
    for n in ("alaw", "rf64"):
        bad = golden["bad_" + n].tobytes()
        rc, _, _, msg = c_plan_fs([f48, bad])
        assert rc == ENOTSUP and "file 1:" in msg and msg == c_plan([f48, bad])[3]


def test_each_refusal_of_a_ratio_names_the_file():
    ok = pcm(10, 1, 48000)
    cases = [(1048577, FS, "2^20"),                 # 16000 / 1048577 in lowest terms: q above 2^20
             (272000, FS, "below 1 / 16"),           # 1 / 17
             (1000, 17000, "above 16 times")]        # 17 / 1
    for rate, fs, what in cases:
        bad = pcm(10, 1, rate)
        for k, files in ((0, [bad]), (2, [ok, ok, bad, ok])):
            rc, _, _, msg = c_plan_fs(files, fs)
            assert rc == ENOTSUP and "file %d:" % k in msg and what in msg, (rate, fs, msg)
            assert c_plan(files)[0] == 0                                   # the file itself is fine
    rc, desc, _, _ = c_plan_fs([pcm(10, 1, 256000), pcm(10, 1, 1000), pcm(10, 1, 1048575)], FS)
    assert rc == ENOTSUP                                                   # 640 / 41943: terms below 2^20, yet under 1 / 16
    rc, desc, sizes, _ = c_plan_fs([pcm(10, 1, 256000), pcm(10, 1, 1000)], FS)
    assert rc == 0 and [(int(d[14]), int(d[15])) for d in desc] == [(1, 16), (16, 1)] and list(desc[:, 11]) == [0, 1] and sizes[0] == 161
    rc, desc, _, _ = c_plan_fs([pcm(10, 1, 1048575)], 1048576)
    assert rc == 0 and (desc[0, 14], desc[0, 15]) == (1048576, 1048575)
    rc, _, _, msg = c_plan_fs([pcm(10, 1, 1048576), pcm(10, 1, 1048577)], 1048576)
    assert rc == ENOTSUP and "file 1:" in msg and "2^20" in msg


def test_device_entry_checks_its_arguments_without_a_device():
    import torch
    from mcncrossmodalemotions_amd import _lib
    before = torch.cuda.is_initialized()
    L = _lib.load()
    fn = L.xm_wav_decode_resample_batch
    assert fn(None, 0, None, 0, None, 0, None) == 0
    assert fn(None, 16, None, 1, None, 4, None) == EINVAL
    assert fn(None, -1, None, 0, None, 0, None) == EINVAL
    assert fn(None, 0, None, -1, None, 0, None) == EINVAL
    assert fn(None, 0, None, 0, None, -1, None) == EINVAL
    host = np.zeros(64, np.int64)                                          # aligned host memory: never dereferenced
    a = host.ctypes.data
    assert a % 8 == 0
    a16 = (a + 15) & ~15
    for args in ((a16 + 1, 16, a16 + 64, 1, a16 + 128, 4), (a16, 16, a16 + 68, 1, a16 + 128, 4), (a16, 16, a16 + 64, 1, a16 + 130, 4)):
        assert fn(C.c_void_p(args[0]), args[1], C.c_void_p(args[2]), args[3], C.c_void_p(args[4]), args[5], None) == EINVAL
        assert "aligned" in L.xm_last_error().decode()
    assert torch.cuda.is_initialized() == before


def test_audioinfo_and_imdb_lengths_come_from_the_plan():
    import torch
    from mcncrossmodalemotions_amd import _lib, batch as xbatch, vl
    before = torch.cuda.is_initialized()
    files = [pcm(44100, 2, 44100, seed=1), pcm(16001, 1, 16000, seed=2), pcm(30000, 2, 48000, S24, seed=3), pcm(0, 1, 22050)]
    info = vl.audioinfo(files, fs=FS)
    assert [i["ResampledSamples"] for i in info] == [16000, 16001, 10000, 0]
    assert [(i["SampleRate"], i["TotalSamples"], i["NumChannels"]) for i in info] == [(44100, 44100, 2), (16000, 16001, 1), (48000, 30000, 2), (22050, 0, 1)]
    plain = vl.audioinfo(files)
    assert all("ResampledSamples" not in i for i in plain)
    assert [{k: v for k, v in i.items() if k != "ResampledSamples"} for i in info] == plain
    assert vl.audioinfo([], fs=FS) == []
    with pytest.raises(_lib.XmError, match="file 1"):
        vl.audioinfo([files[0], pcm(10, 1, 272000)], fs=FS)
    buf, plan = vl.wav_plan(files, channel=0, out_base=7, fs=FS)
    assert plan["fs"] == FS and list(plan["out_frames"]) == [16000, 16001, 10000, 0] and plan["floats"] == 42001
    assert list(plan["rows"][:, 11]) == [7, 16007, 32008, 42008]
    assert "fs" not in vl.wav_plan(files)[1]
    # the imdb: lengths at the imdb's rate, noise too; the defaults keep both refusals word for word
    tracks = {"a.wav": files[0], "b.wav": files[1], "c.wav": files[2]}
    logits = [np.zeros((3, 8), np.float32)] * 3
    noise = [pcm(96000, 1, 48000, seed=5), pcm(40000, 2, 16000, seed=6)]
    imdb = xbatch.WavFileEmoVoxImdb(tracks, logits, noise=noise, resample=True, channel=0)
    assert imdb.fs == FS and list(imdb.num_samples) == [16000, 16001, 10000] and list(imdb.wav_offsets()) == [0, 16000, 32001, 42001]
    assert list(imdb.noise_samples) == [32000, 40000] and imdb.noiselen == 32000 and imdb.noisenum == 2
    with pytest.raises(ValueError) as e:
        xbatch.WavFileEmoVoxImdb(tracks, logits)
    assert str(e.value) == "WavFileEmoVoxImdb: track 'a.wav' is sampled at 44100 Hz, the imdb at 16000"
    with pytest.raises(ValueError) as e:
        xbatch.WavFileEmoVoxImdb({"b.wav": files[1], "s.wav": noise[1]}, logits[:2])
    assert str(e.value) == "WavFileEmoVoxImdb: track 's.wav' has 2 channels, one is required"
    with pytest.raises(ValueError, match="one is required"):
        xbatch.WavFileEmoVoxImdb(tracks, logits, resample=True)            # resampling alone does not pick a channel
    with pytest.raises(ValueError, match="44100 Hz"):
        xbatch.WavFileEmoVoxImdb(tracks, logits, channel=0)                # a channel alone does not resample
    with pytest.raises(ValueError, match="channel 1 was asked for"):
        xbatch.WavFileEmoVoxImdb(tracks, logits, resample=True, channel=1)
    assert torch.cuda.is_initialized() == before


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_rate_plan_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wav_rate_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "wav_rate_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    words = r.stdout.split()
    assert int(words[0]) > 5000 and int(words[7]) > 100      # every truncation and mutation ran; rates were mutated into refusals
