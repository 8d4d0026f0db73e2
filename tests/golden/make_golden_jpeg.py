"""Writes tests/golden/jpeg_small.npz: the file bytes of a few small JPEGs and the pixels PIL (libjpeg-turbo, default
integer path: ISLOW IDCT, fancy upsampling) decodes from them.  The GPU tests read only the .npz.

    python tests/golden/make_golden_jpeg.py

Every image is seeded smooth-plus-noise content.  Cases: see CASES; default quality 90.  `progressive` is there to be
rejected (bytes only), `truncated` is the 4:2:0 96 x 80 file cut at 60 % of its scan, with the pixels of the whole file.
"""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jpeg_small.npz")

# name, H, W, mode ('L' | 'RGB'), PIL subsampling (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0), save options
CASES = [
    ("grey_8x8", 8, 8, "L", None, {}),
    ("grey_17x23", 17, 23, "L", None, {}),
    ("s444_16x16", 16, 16, "RGB", 0, {}),
    ("s444_37x29_opt", 37, 29, "RGB", 0, {"optimize": True}),
    ("s422_33x47", 33, 47, "RGB", 1, {}),
    ("s420_16x16", 16, 16, "RGB", 2, {}),
    ("s420_41x35_opt", 41, 35, "RGB", 2, {"optimize": True}),
    ("s420_96x80_q50", 96, 80, "RGB", 2, {"quality": 50}),
    ("s420_50x50_q100", 50, 50, "RGB", 2, {"quality": 100}),
    ("s420_64x64_rst", 64, 64, "RGB", 2, {"restart_marker_blocks": 3}),
    ("s420_1x1", 1, 1, "RGB", 2, {}),
]
SUPPORTED = [c[0] for c in CASES]
TRUNC_OF = "s420_96x80_q50"


def smooth_noise(seed, H, W, channels):
    """a few low-frequency waves per channel plus Gaussian noise, uint8"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((H, W, channels))
    for c in range(channels):
        v = 128 + 20 * rng.standard_normal()
        for _ in range(4):
            fy, fx, ph = rng.uniform(0, 0.25), rng.uniform(0, 0.25), rng.uniform(0, 6.28)
            v = v + rng.uniform(10, 45) * np.sin(fy * y + fx * x + ph)
        out[:, :, c] = v + 12 * rng.standard_normal((H, W))
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def encode(seed, H, W, mode, subsampling, opts):
    from PIL import Image
    a = smooth_noise(seed, H, W, 1 if mode == "L" else 3)
    im = Image.fromarray(a[:, :, 0] if mode == "L" else a, mode)
    kw = dict(quality=90)
    kw.update(opts)
    if subsampling is not None:
        kw["subsampling"] = subsampling
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_decode(data):
    """H x W x 3 uint8; a grey file gives R = G = B = Y"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    a = np.asarray(im)
    return np.ascontiguousarray(np.repeat(a[:, :, None], 3, 2) if a.ndim == 2 else a)


def scan_start(data):
    """offset of the first entropy-coded byte"""
    i = data.index(b"\xff\xda")
    return i + 2 + int.from_bytes(data[i + 2:i + 4], "big")


def cases():
    """{key: array} exactly as stored in the .npz"""
    import PIL
    out = {"names": np.array(SUPPORTED), "pil_version": np.array(PIL.__version__)}
    for k, (name, H, W, mode, ss, opts) in enumerate(CASES):
        data = encode(100 + k, H, W, mode, ss, opts)
        out["bytes_" + name] = np.frombuffer(data, np.uint8).copy()
        out["pix_" + name] = pil_decode(data)
    out["bytes_progressive"] = np.frombuffer(encode(200, 32, 32, "RGB", 2, {"progressive": True}), np.uint8).copy()
    whole = out["bytes_" + TRUNC_OF].tobytes()
    s0 = scan_start(whole)
    cut = s0 + int(0.6 * (len(whole) - 2 - s0))
    out["bytes_truncated"] = np.frombuffer(whole[:cut], np.uint8).copy()
    out["pix_truncated"] = out["pix_" + TRUNC_OF]
    return out


if __name__ == "__main__":
    c = cases()
    np.savez_compressed(OUT, **c)
    print("%s: %d bytes, %d JPEG bytes" % (OUT, os.path.getsize(OUT),
                                           sum(v.size for k, v in c.items() if k.startswith("bytes_"))))
