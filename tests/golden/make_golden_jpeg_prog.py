"""Writes tests/golden/jpeg_progressive.npz: the file bytes of a few small progressive (SOF2) JPEGs and the pixels PIL
(libjpeg-turbo, default integer path) decodes from them.  The tests read only the .npz.

    python tests/golden/make_golden_jpeg_prog.py

Content and encoder are those of make_golden_jpeg.py, with seeds of its own and progressive=True: libjpeg's standard
progression, 10 scans for colour (3 levels of successive approximation) and 6 for grey, a DHT in front of every scan
that needs one.  For every case the progressive and the baseline encoding of the same image hold the same quantised
coefficients, so they decode to identical pixels; the generator asserts it and stores the baseline bytes as base_<name>.
  partial_K   the 41 x 35 file cut in front of the DHT of scan K (counted from 0) plus FF D9: a valid file that ends
              before all bits have arrived, with the pixels PIL gives for it
  truncated   the 96 x 80 file cut at 60 % of the entropy data of its sixth scan (bytes only)
"""
import io
import os

import numpy as np

from make_golden_jpeg import encode, pil_decode

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jpeg_progressive.npz")

# name, H, W, mode ('L' | 'RGB'), PIL subsampling (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0), save options
CASES = [
    ("grey_8x8", 8, 8, "L", None, {}),
    ("grey_17x23", 17, 23, "L", None, {}),
    ("s444_16x16", 16, 16, "RGB", 0, {}),
    ("s422_33x47_opt", 33, 47, "RGB", 1, {"optimize": True}),
    ("s420_16x16", 16, 16, "RGB", 2, {}),
    ("s420_41x35", 41, 35, "RGB", 2, {}),
    ("s420_96x80_q10", 96, 80, "RGB", 2, {"quality": 10}),
    ("s420_50x50_q100", 50, 50, "RGB", 2, {"quality": 100}),
    ("s420_64x64_rst3", 64, 64, "RGB", 2, {"restart_marker_blocks": 3}),
    ("s420_1x1", 1, 1, "RGB", 2, {}),
]
FLAT = ("flat_64x64", 64, 64, (90, 140, 200))
SUPPORTED = [c[0] for c in CASES] + [FLAT[0]]
PARTIAL_OF, PARTIAL_AT = "s420_41x35", (1, 5, 9)
TRUNC_OF, TRUNC_SCAN, TRUNC_AT = "s420_96x80_q10", 5, 0.6


def segments(data):
    """[(marker, offset of its FF, offset past its segment and entropy data)] of the whole file"""
    out, pos, n = [], 2, len(data)
    while pos < n:
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        if m == 0xD9:
            out.append((m, pos, pos + 2))
            break
        end = pos + 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
        if m == 0xDA:                                        # entropy data: up to the next marker but 00 / RSTn
            while not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
                end += 1
        out.append((m, pos, end))
        pos = end
    return out


def scan_cut(data, k):
    """offset of the first DHT of the run of DHT segments in front of SOS number k (from 0)"""
    segs = segments(data)
    at = [i for i, s in enumerate(segs) if s[0] == 0xDA][k]
    first = at
    while segs[first - 1][0] == 0xC4:
        first -= 1
    assert first < at, "scan %d has no DHT of its own" % k
    return segs[first][1]


def flat_bytes(progressive):
    from PIL import Image
    name, H, W, rgb = FLAT
    buf = io.BytesIO()
    Image.fromarray(np.broadcast_to(np.array(rgb, np.uint8), (H, W, 3)).copy(), "RGB").save(
        buf, "JPEG", quality=90, subsampling=2, progressive=progressive)
    return buf.getvalue()


def cases():
    """{key: array} exactly as stored in the .npz"""
    import PIL
    out = {"names": np.array(SUPPORTED), "pil_version": np.array(PIL.__version__)}
    files = {}
    for k, (name, H, W, mode, ss, opts) in enumerate(CASES):
        files[name] = (encode(300 + k, H, W, mode, ss, dict(opts, progressive=True)), encode(300 + k, H, W, mode, ss, opts))
    files[FLAT[0]] = (flat_bytes(True), flat_bytes(False))
    for name, (prog, base) in files.items():
        assert b"\xff\xc2" in prog and b"\xff\xc2" not in base, name
        nscans = sum(1 for s in segments(prog) if s[0] == 0xDA)
        assert nscans == (6 if name.startswith("grey") else 10), (name, nscans)
        pix = pil_decode(prog)
        assert np.array_equal(pix, pil_decode(base)), name       # the same coefficients, the same pixels
        out["bytes_" + name] = np.frombuffer(prog, np.uint8).copy()
        out["base_" + name] = np.frombuffer(base, np.uint8).copy()
        out["pix_" + name] = pix
    whole = files[PARTIAL_OF][0]
    for k in PARTIAL_AT:
        part = whole[:scan_cut(whole, k)] + b"\xff\xd9"
        out["bytes_partial_%d" % k] = np.frombuffer(part, np.uint8).copy()
        out["pix_partial_%d" % k] = pil_decode(part)
    whole = files[TRUNC_OF][0]
    sos = [s for s in segments(whole) if s[0] == 0xDA][TRUNC_SCAN]
    data0 = sos[1] + 2 + int.from_bytes(whole[sos[1] + 2:sos[1] + 4], "big")
    out["bytes_truncated"] = np.frombuffer(whole[:data0 + int(TRUNC_AT * (sos[2] - data0))], np.uint8).copy()
    return out


if __name__ == "__main__":
    c = cases()
    np.savez_compressed(OUT, **c)
    print("%s: %d bytes, %d JPEG bytes" % (OUT, os.path.getsize(OUT),
                                           sum(v.size for k, v in c.items() if k.startswith("bytes_"))))
    whole = c["pix_" + PARTIAL_OF].astype(int)
    print("partial: largest difference from the whole file",
          [int(np.abs(c["pix_partial_%d" % k].astype(int) - whole).max()) for k in PARTIAL_AT])
