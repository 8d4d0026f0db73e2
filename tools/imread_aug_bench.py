#!/usr/bin/env python
"""Timing of vl.vl_imreadjpeg's crop / flip / filter / colour stage (xm_imread_transform_batch), in one call.
usage: python tools/imread_aug_bench.py [--reps 20]
The 128 files of tools/jpeg_bench.py (256 x 256, 4:2:0, quality 90).  Prints
 (a) the stage to 224 x 224 on the decoded batch, per kernel and in all, for 'bilinear' and 'bicubic', each with and
     without antialias, whole image and the centre crop 1/1.6 -- next to crop_resize_face_ragged_kernel on the same
     decoded batch (the narrow path's resampler) and a device copy of the bytes the stage moves;
 (b) the same with Contrast (three launches), against (a);
 (c) vl.vl_imreadjpeg with the training options (random crop 0.35 .. 1, anisotropy 3/4 .. 4/3, flip, brightness,
     contrast, saturation) at split=512, files to tensor, against PIL decode + crop + resize + flip on ten threads feeding
     the same tensor -- the comparison of DESIGN section 15."""
import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from jpeg_bench import kernel_ms, make_files, timeit  # noqa: E402
from mcncrossmodalemotions_amd import _lib, vl  # noqa: E402

FILTER = {"box": 0, "bilinear": 1, "bicubic": 2}


def opts(filter, antialias, size=1.0, contrast=0.0):
    v = np.zeros(vl.IMREAD_OPTS)
    v[0:3] = (1, 224, 224)
    v[5:7] = size
    v[9], v[10], v[11] = FILTER[filter], antialias, contrast
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.load()
    files, have_pil = make_files(128)
    N = len(files)
    buf, plan = vl.jpeg_plan(files, stage=vl._pinned)
    pixels, _, _, desc = vl.jpeg_decode(buf, plan, want_pixels=True)
    hw = desc[:, [2, 3, 21]]
    in_bytes, out_bytes = 4.0 * pixels.numel() / N, 4.0 * 3 * 224 * 224
    print("%d files decoded: %.0f kB of pixels read and %.0f kB written per image at most" % (N, in_bytes / 1e3, out_bytes / 1e3))
    src = torch.empty(int((in_bytes + out_bytes) * N / 8), dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    copy_ms = timeit(lambda: dst.copy_(src), a.reps) * 1e3
    print("a device copy that reads and writes as many bytes (%.1f MB each way)      %8.3f ms" % (src.numel() * 4 / 1e6, copy_ms))
    # the yardstick: the narrow path's resampler, timed inside its own decode by the profiler hook
    for crop in (1.0, 1 / 1.6):
        ms = kernel_ms(L, lambda: vl.imreadjpeg(files, resize=(224, 224), crop_size=crop), a.reps)
        print("crop_resize_face_ragged_kernel, crop %.3f (inside vl.imreadjpeg)             %8.3f ms" % (crop, ms["crop_resize_face_ragged_kernel"]))
    print("(a), (b) the stage on the decoded batch, ms per batch of %d (profiler hook per kernel; back to back in all)" % N)
    print("    %-9s %-5s %-6s %-8s %8s %8s %8s %8s %9s" % ("filter", "aa", "crop", "contrast", "table", "resample", "colour", "all", "x copy"))
    for crop in (1.0, 1 / 1.6):
        for filter in ("bilinear", "bicubic"):
            for aa in (0, 1):
                for contrast in (0.0, 0.4):
                    draws = vl.imread_draws(np.random.default_rng(1), N) if contrast else None
                    rows, sizes = vl.imread_plan(hw, opts(filter, aa, crop, contrast), draws)
                    fn = lambda: vl.imread_transform(pixels, rows, sizes)                      # noqa: E731
                    ms = kernel_ms(L, fn, a.reps)
                    res = ms.get("imread_resample_kernel<true>", ms.get("imread_resample_kernel<false>"))
                    whole = timeit(fn, a.reps) * 1e3
                    print("    %-9s %-5d %-6.3f %-8.1f %8.3f %8.3f %8.3f %8.3f %9.2f" % (
                        filter, aa, crop, contrast, ms["imread_table_kernel"], res, ms.get("imread_colour_kernel", 0.0), whole, whole / copy_ms))
    # ---- (c) files to tensor with the training options ----------------------------------------------------------------
    train = ("Pack", "Resize", [224, 224], "CropSize", [0.35, 1], "CropAnisotropy", [0.75, 4 / 3], "CropLocation", "random", "Flip",
             "Brightness", [8, 8, 8], "Contrast", 0.4, "Saturation", 0.4)
    rng = np.random.default_rng(2)
    dev = lambda: vl.vl_imreadjpeg(files, *train, rng=rng, split=512)                          # noqa: E731
    dev()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        dev()
    torch.cuda.synchronize()
    t_dev = (time.perf_counter() - t0) / a.reps
    print("(c) files -> 224 x 224 x 3 x %d training tensor" % N)
    print("    vl.vl_imreadjpeg, training options, split=512   %9.1f img/s  (%.3f ms per batch)" % (N / t_dev, t_dev * 1e3))
    if have_pil:
        from PIL import Image
        pool = ThreadPoolExecutor(10)

        def one(args):
            b, u = args
            im = Image.open(io.BytesIO(b)).convert("RGB")
            s = 0.35 + 0.65 * u[1]
            w, h = im.size
            cw, ch = s * w, s * h
            x0, y0 = u[3] * (w - cw), u[2] * (h - ch)
            im = im.resize((224, 224), Image.BILINEAR, box=(x0, y0, x0 + cw, y0 + ch))
            arr = np.asarray(im)
            return arr[:, ::-1] if u[4] < 0.5 else arr

        def pil():
            d = vl.imread_draws(rng, N)
            a8 = np.ascontiguousarray(np.stack(list(pool.map(one, zip(files, d))), 0))
            t = torch.from_numpy(a8).pin_memory().to("cuda", non_blocking=True)
            return t.to(torch.float32).permute(0, 3, 2, 1).contiguous().permute(3, 2, 1, 0)
        pil()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            pil()
        torch.cuda.synchronize()
        t_pil = (time.perf_counter() - t0) / a.reps
        print("    PIL decode + crop + resize + flip, 10 threads     %9.1f img/s  (%.3f ms per batch; no colour jitter)" % (N / t_pil, t_pil * 1e3))
        print("    device path against the PIL-fed tensor: %.2f x" % (t_pil / t_dev))


if __name__ == "__main__":
    main()
