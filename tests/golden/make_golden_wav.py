"""Writes tests/golden/wav_small.npz: small WAV files (their bytes) next to the float32 samples audioread returns for
them, as uint32 bit patterns in MATLAB layout (channel c of a frames x channels matrix at + c * frames), and one file
per rejection of xm_wav_plan with the code it must give.  numpy, struct and wave only; seeded.

    python tests/golden/make_golden_wav.py

The expected samples are computed from the integers / floats the files were written from, never by parsing the files:
single(double(v) / 2^(bits - 1)) for PCM (8-bit: (v - 128) / 128), the float32 bits themselves, single(double)."""
import io
import os
import struct
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
U8, S16, S24, S32, F32, F64 = range(6)
BITS = {U8: 8, S16: 16, S24: 24, S32: 32, F32: 32, F64: 64}
EINVAL, ENOTSUP = 1, 5
PCM_GUID = struct.pack("<H", 1) + bytes([0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])
FLT_GUID = struct.pack("<H", 3) + PCM_GUID[2:]


def draw(rng, fmt, frames, nch):
    """frames x nch values of the format's own type"""
    n = (frames, nch)
    if fmt == U8:
        return rng.integers(0, 256, n).astype(np.uint8)
    if fmt == S16:
        return rng.integers(-2 ** 15, 2 ** 15, n).astype(np.int16)
    if fmt == S24:
        return rng.integers(-2 ** 23, 2 ** 23, n).astype(np.int32)
    if fmt == S32:
        return rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    if fmt == F32:
        return (rng.standard_normal(n) * 0.3).astype(np.float32)
    return rng.standard_normal(n) * 0.3


def payload(fmt, v):
    """interleaved little-endian sample bytes of a frames x nch array"""
    if fmt == S24:
        b = v.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3]
        return np.ascontiguousarray(b).tobytes()
    dt = {U8: "u1", S16: "<i2", S32: "<i4", F32: "<f4", F64: "<f8"}[fmt]
    return np.ascontiguousarray(v.astype(dt)).tobytes()


def expected(fmt, v):
    """uint32 bits of single(audioread's double), MATLAB layout"""
    if fmt == U8:
        y = ((v.astype(np.float64) - 128) / 128).astype(np.float32)
    elif fmt == F32:
        y = v.astype(np.float32)
    elif fmt == F64:
        with np.errstate(over="ignore", under="ignore"):
            y = v.astype(np.float64).astype(np.float32)
    else:
        y = (v.astype(np.float64) / 2.0 ** (BITS[fmt] - 1)).astype(np.float32)
    return np.ascontiguousarray(y.T).reshape(-1).view(np.uint32)


def fmt_chunk(tag, nch, rate, bits, align=None, extensible=None, valid=None):
    align = nch * bits // 8 if align is None else align
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, nch, rate, rate * align, align, bits)
    if extensible:
        body += struct.pack("<HHI", 22, bits if valid is None else valid, 0) + extensible
    return b"fmt " + struct.pack("<I", len(body)) + body


def chunk(tag, body, size=None):
    return tag + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 and size is None else b"")


def riff(*chunks, magic=b"RIFF", form=b"WAVE"):
    body = form + b"".join(chunks)
    return magic + struct.pack("<I", len(body) & 0xFFFFFFFF) + body


def simple(fmt, v, rate=16000, **kw):
    tag = 3 if fmt in (F32, F64) else 1
    return riff(fmt_chunk(tag, v.shape[1], rate, BITS[fmt], **kw), chunk(b"data", payload(fmt, v)))


def by_wave_module(v, rate=16000):
    """16-bit PCM through the standard library's writer"""
    bio = io.BytesIO()
    with wave.open(bio, "wb") as w:
        w.setnchannels(v.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(payload(S16, v))
    return bio.getvalue()


def main():
    rng = np.random.default_rng(20240611)
    good, bad = [], []

    def add(name, data, fmt, v, rate=16000, truncated=0):
        good.append((name, data, expected(fmt, v), [rate, v.shape[1], BITS[fmt], fmt, v.shape[0], truncated]))

    tags = {U8: "u8", S16: "s16", S24: "s24", S32: "s32", F32: "f32", F64: "f64"}
    for fmt in range(6):
        for frames in (1, 5, 64, 257):
            v = draw(rng, fmt, frames, 1)
            add("%s_m%d" % (tags[fmt], frames), simple(fmt, v), fmt, v)
    for frames in (1023, 1024, 1025, 4097):
        v = draw(rng, S16, frames, 1)
        add("s16_m%d" % frames, by_wave_module(v), S16, v)
    v = draw(rng, S16, 33, 2)
    add("s16_st33", by_wave_module(v, 44100), S16, v, rate=44100)
    v = draw(rng, S24, 21, 2)
    add("s24_st21", simple(S24, v, 48000), S24, v, rate=48000)
    v = draw(rng, F32, 17, 2)
    add("f32_st17", simple(F32, v), F32, v)
    v = draw(rng, U8, 19, 3)
    add("u8_3ch19", simple(U8, v, 8000), U8, v, rate=8000)
    v = draw(rng, S16, 9, 2)
    add("ext_s16_st9", simple(S16, v, extensible=PCM_GUID), S16, v)
    v = draw(rng, S24, 10, 1)
    add("ext_s24_m10", simple(S24, v, extensible=PCM_GUID), S24, v)
    v = draw(rng, F32, 11, 1)
    add("ext_f32_m11", simple(F32, v, extensible=FLT_GUID), F32, v)
    # an odd-sized LIST chunk and a fact chunk before the data, a LIST behind it that is not sample data
    v = draw(rng, S16, 40, 1)
    add("chunks_s16_m40", riff(fmt_chunk(1, 1, 16000, 16), chunk(b"LIST", b"INFOx"), chunk(b"fact", struct.pack("<I", 40)),
                               chunk(b"data", payload(S16, v)), chunk(b"LIST", b"INFOISFT\x04\0\0\0abc\0")), S16, v)
    # a streamed writer: data size 0xFFFFFFFF, 30 frames and one more byte present, odd file length
    v = draw(rng, S16, 30, 1)
    data = riff(fmt_chunk(1, 1, 16000, 16), chunk(b"data", payload(S16, v) + b"\x7f", size=0xFFFFFFFF))
    assert len(data) & 1
    add("streamed_s16_m30", data, S16, v, truncated=1)
    v = draw(rng, S16, 0, 1)
    add("empty_s16", simple(S16, v), S16, v)
    # extreme values
    v = np.array([[-32768], [32767], [0], [-1], [1], [-32767]], np.int16)
    add("edge_s16", simple(S16, v), S16, v)
    v = np.array([[2 ** 31 - 1], [-2 ** 31], [2 ** 24 + 1], [2 ** 24 + 3], [-(2 ** 24) - 1], [2 ** 25 + 2], [2 ** 25 + 6],
                  [2 ** 30 + 65], [2 ** 31 - 129], [2 ** 31 - 64], [1], [-1], [0]], np.int64).astype(np.int32)
    add("edge_s32", simple(S32, v), S32, v)
    t = 2.0 ** -149
    v = np.array([[1 / 3], [-1 / 3], [5e-324], [1e-310], [1e-40], [t], [t / 2], [t / 2 * (1 + 2.0 ** -52)], [1.5 * t], [2.5 * t],
                  [2.0 ** -126], [2.0 ** -126 * (1 - 2.0 ** -25)], [3.4e38], [3.5e38], [(2 - 2.0 ** -24) * 2.0 ** 127],
                  [(2 - 2.0 ** -24) * 2.0 ** 127 * (1 - 2.0 ** -53)], [1e39], [1 + 2.0 ** -24], [1 + 3 * 2.0 ** -24], [0.0], [-0.0],
                  [np.inf], [-np.inf], [np.nan]], np.float64)
    add("edge_f64", simple(F64, v), F64, v)
    v = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FA00000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000,
                  0x3F800000], np.uint32).view(np.float32).reshape(-1, 1)
    data = riff(fmt_chunk(3, 1, 16000, 32), chunk(b"data", v.tobytes()))
    good.append(("edge_f32", data, np.ascontiguousarray(v.T).reshape(-1).view(np.uint32), [16000, 1, 32, F32, v.shape[0], 0]))

    # ---- rejections -------------------------------------------------------------------------------------------------
    s16 = draw(rng, S16, 8, 1)
    ok = simple(S16, s16)
    d16 = chunk(b"data", payload(S16, s16))
    bad += [("rf64", riff(fmt_chunk(1, 1, 16000, 16), d16, magic=b"RF64"), ENOTSUP),
            ("bw64", riff(fmt_chunk(1, 1, 16000, 16), d16, magic=b"BW64"), ENOTSUP),
            ("rifx", riff(fmt_chunk(1, 1, 16000, 16), d16, magic=b"RIFX"), ENOTSUP),
            ("alaw", riff(fmt_chunk(6, 1, 8000, 8), chunk(b"data", bytes(16))), ENOTSUP),
            ("mulaw", riff(fmt_chunk(7, 1, 8000, 8), chunk(b"data", bytes(16))), ENOTSUP),
            ("adpcm", riff(fmt_chunk(2, 1, 16000, 4, align=256), chunk(b"data", bytes(256))), ENOTSUP),
            ("mpeg", riff(fmt_chunk(0x50, 1, 16000, 0, align=1), chunk(b"data", bytes(16))), ENOTSUP),
            ("ext_valid20", simple(S24, draw(rng, S24, 4, 1), extensible=PCM_GUID, valid=20), ENOTSUP),
            ("pcm12", riff(fmt_chunk(1, 1, 16000, 12, align=2), d16), ENOTSUP),
            ("float16", riff(fmt_chunk(3, 1, 16000, 16), d16), ENOTSUP),
            ("no_riff", b"JUNK" + ok[4:], EINVAL),
            ("no_wave", riff(fmt_chunk(1, 1, 16000, 16), d16, form=b"AVI "), EINVAL),
            ("cut_in_riff_header", ok[:10], EINVAL),
            ("cut_in_chunk_header", ok[:17], EINVAL),
            ("cut_in_fmt", ok[:30], EINVAL),
            ("short_fmt", riff(b"fmt " + struct.pack("<I", 14) + struct.pack("<HHIIH", 1, 1, 16000, 32000, 2), d16), EINVAL),
            ("data_before_fmt", riff(d16, fmt_chunk(1, 1, 16000, 16)), EINVAL),
            ("no_data", riff(fmt_chunk(1, 1, 16000, 16), chunk(b"LIST", b"INFO")), EINVAL),
            ("bad_align", riff(fmt_chunk(1, 2, 16000, 16, align=2), d16), EINVAL),
            ("zero_channels", riff(fmt_chunk(1, 0, 16000, 16, align=0), d16), EINVAL),
            ("zero_rate", riff(fmt_chunk(1, 1, 0, 16), d16), EINVAL)]

    out = {"names": np.array([g[0] for g in good]), "bad_names": np.array([b[0] for b in bad])}
    for name, data, exp, meta in good:
        out["bytes_" + name] = np.frombuffer(data, np.uint8)
        out["exp_" + name] = exp
        out["meta_" + name] = np.array(meta, np.int64)
    for name, data, code in bad:
        out["bad_" + name] = np.frombuffer(data, np.uint8)
        out["badcode_" + name] = np.array(code, np.int64)
    path = os.path.join(HERE, "wav_small.npz")
    np.savez_compressed(path, **out)
    print("%s: %d files, %d rejections, %d bytes" % (path, len(good), len(bad), os.path.getsize(path)))


if __name__ == "__main__":
    main()
