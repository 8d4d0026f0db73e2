#!/usr/bin/env python
"""Timing of vl.imreadjpeg (xm_jpeg_plan / xm_jpeg_decode_batch) in front of the frozen teacher.
usage: python tools/jpeg_bench.py [--teacher senet50-ferplus] [--batches 12] [--reps 10] [--split | --progressive]
128 files of 256 x 256, 4:2:0, quality 90, smooth-plus-noise content (made with PIL when it is importable; otherwise the
golden files of tests/golden/jpeg_small.npz repeated, and the PIL lines are left out).  Prints
 (a) ms per batch of each decode kernel (the library's profiler hook) and of the host parse and the enqueue;
 (b) PIL decoding the same files on 10 and on 16 threads, img/s, twice;
 (c) buildImdb's loop at batch 128 fed prepared decoded frames, PIL on 10 threads, and the device JPEG path, next to the
     teacher alone measured in the same process.
--split prints instead, in one call on the same files, the table of the segment-parallel entropy decode (imreadjpeg's
split=): the entropy kernel's time unsplit and at seg_bytes 64 / 128 / 256 / 512 with the mean and the maximum of the
rounds per lane, the whole decode back to back, and buildImdb's loop unsplit, split and fed by PIL on 10 threads.
--progressive prints, in one call, the same images encoded baseline and progressive (imreadjpeg's progressive=; needs
PIL): the entropy stage per batch of each (the progressive one is a launch per level), the launches per call, the whole
decode back to back, and buildImdb's loop fed each."""
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
from mcncrossmodalemotions_amd import _lib, fetch_emovoxceleb_imdb as fe, prof, vl, zoo  # noqa: E402


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def make_files(n, progressive=False):
    try:
        from PIL import Image
    except ImportError:
        g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_small.npz"))
        names = [str(x) for x in g["names"]]
        return [g["bytes_" + names[i % len(names)]].tobytes() for i in range(n)], False
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_jpeg as mk
    out = []
    for i in range(n):
        buf = io.BytesIO()
        Image.fromarray(mk.smooth_noise(5000 + i, 256, 256, 3), "RGB").save(buf, "JPEG", quality=90, subsampling=2,
                                                                            progressive=progressive)
        out.append(buf.getvalue())
    return out, True


def pil_rate(files, threads):
    from PIL import Image
    dec = lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))     # noqa: E731
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(dec, files))
        t0 = time.perf_counter()
        for _ in range(4):
            list(ex.map(dec, files))
        return 4 * len(files) / (time.perf_counter() - t0)


def kernel_ms(L, fn, reps):
    with prof.recording(L):
        for _ in range(reps):
            fn()
    return {r.name: r.ms / max(r.launches, 1) for r in prof.collect(L)}


def loop_rate(teacher, imdb, numIms, **src):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fe.buildImdb(teacher, imdb, batchSize=128, **src)
    torch.cuda.synchronize()
    return numIms / (time.perf_counter() - t0)


SPLITS = (64, 128, 256, 512)


def loop_setup(a, faces):
    """the imdb of 128 * batches frames that name the 128 files, the frozen teacher and its rate alone"""
    n = 128 * a.batches
    images = {"name": ["id%05d/v/1.wav" % i for i in range(1, n // 32 + 1)], "id": np.arange(1, n // 32 + 1),
              "set": np.ones(n // 32, int), "numSamples": np.full(n // 32, 8 * 16000),
              "denseFrames": ["%d" % (i % 128) for i in range(n)], "denseFramesWavIds": np.arange(n) // 32 + 1}
    imdb = fe.EmoVoxImdb(images)
    net = zoo.ferPlusZoo(a.teacher)
    zoo.strip_losses(net)
    net.mode = "test"
    net.move("gpu")
    teacher = zoo.FrozenTeacher(net, lanes=2)
    teacher.imageSize, teacher.averageImage = (224, 224), fe.AVERAGE_IMAGE
    for _ in range(a.batches):
        teacher.logits(faces)
    alone = max(128 / timeit(lambda: teacher.logits(faces), a.batches) for _ in range(3))
    return teacher, imdb, n, alone


def split_table(a, L, files, have_pil):
    face = dict(resize=(224, 224), crop_size=1 / 1.6, average_image=fe.AVERAGE_IMAGE)
    faces = vl.imreadjpeg(files, **face)
    print("entropy stage per batch of 128 (the library's profiler hook), rounds per lane, the whole decode back to back")
    print("    %-10s %-26s %10s %12s %8s %8s %12s" % ("seg_bytes", "kernel", "ms", "segs / lane", "rounds", "max", "decode ms"))
    best, best_ms, base_ms = None, None, None
    for seg in (None,) + SPLITS:
        fn = lambda: vl.imreadjpeg(files, split=seg, **face)                                   # noqa: E731
        got = fn()
        assert torch.equal(got.contiguous().view(torch.int32), faces.contiguous().view(torch.int32)), seg
        name = "jpeg_entropy_kernel" if seg is None else "jpeg_entropy_split_kernel"
        ms = kernel_ms(L, fn, a.reps)[name]
        whole = timeit(fn, a.reps) * 1e3
        if seg is None:
            base_ms = ms
            print("    %-10s %-26s %10.3f %12s %8s %8s %12.3f" % ("unsplit", name, ms, "1", "-", "-", whole))
            continue
        buf, plan = vl.jpeg_plan(files, stage=vl._pinned)
        rounds = vl.jpeg_decode(buf, plan, want_pixels=False, resize=(224, 224), crop=1 / 1.6,
                                average_image=fe.AVERAGE_IMAGE, split=seg, return_rounds=True)[4].cpu().numpy()
        lanes = buf[plan["lanes"][0]:plan["lanes"][0] + plan["lanes"][1]].view(np.int64).reshape(-1, 4)
        segs = np.maximum(-(-(lanes[:, 2] - lanes[:, 1]) // seg), 1)
        print("    %-10d %-26s %10.3f %12.1f %8.1f %8d %12.3f   (%.1f x the unsplit kernel)" % (
            seg, name, ms, segs.mean(), rounds.mean(), rounds.max(), whole, base_ms / ms))
        if best_ms is None or ms < best_ms:
            best, best_ms = seg, ms
    teacher, imdb, n, alone = loop_setup(a, faces)
    read = lambda paths: [files[int(p)] for p in paths]                                        # noqa: E731
    print("buildImdb loop, %s, batch 128, %d frames" % (a.teacher, n))
    print("    FrozenTeacher.logits alone (prepared faces)   %9.1f img/s  = %.3f ms per batch" % (alone, 128 / alone * 1e3))
    rates = {}
    srcs = [("device JPEG decode, unsplit", dict(read=read)), ("device JPEG decode, split=%d" % best, dict(read=read, split=best))]
    if have_pil:
        srcs.append(("PIL on 10 threads", dict(frames=pil_frames_fn(files))))
    for label, src in srcs:
        fe.buildImdb(teacher, imdb, batchSize=128, **src)
        for rep in range(2):
            r = loop_rate(teacher, imdb, n, **src)
            rates[label] = max(r, rates.get(label, 0.0))
            print("    %-45s %9.1f img/s  (%+.1f %% vs alone)" % (label, r, 100 * (r / alone - 1)))
    keys = list(rates)
    print("    split=%d against the unsplit device decode: %.2f x" % (best, rates[keys[1]] / rates[keys[0]]))
    if have_pil:
        print("    split=%d against the PIL-fed loop:           %.2f x" % (best, rates[keys[1]] / rates[keys[2]]))


def progressive_table(a, L, files):
    prog, _ = make_files(128, progressive=True)
    print("the same images progressive: %.1f kB on average" % (sum(map(len, prog)) / 128e3))
    face = dict(resize=(224, 224), crop_size=1 / 1.6, average_image=fe.AVERAGE_IMAGE)
    want = vl.imreadjpeg(files, **face)
    runs = [("baseline files, default path", lambda: vl.imreadjpeg(files, **face)),
            ("baseline files, progressive=True", lambda: vl.imreadjpeg(files, progressive=True, **face)),
            ("progressive files, progressive=True", lambda: vl.imreadjpeg(prog, progressive=True, **face))]
    print("per batch of 128 (the library's profiler hook): the entropy stage, all launches of a call, the whole decode back to back")
    print("    %-38s %12s %10s %10s %12s" % ("", "entropy ms", "launches", "calls ms", "decode ms"))
    for label, fn in runs:
        got = fn()
        assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)), label
        with prof.recording(L):
            for _ in range(a.reps):
                fn()
        rows = prof.collect(L)
        entropy = sum(r.ms for r in rows if "entropy" in r.name) / a.reps
        print("    %-38s %12.3f %10d %10.3f %12.3f" % (label, entropy, sum(r.launches for r in rows) // a.reps,
                                                       sum(r.ms for r in rows) / a.reps, timeit(fn, a.reps) * 1e3))
    teacher, imdb, n, alone = loop_setup(a, want)
    print("buildImdb loop, %s, batch 128, %d frames" % (a.teacher, n))
    print("    FrozenTeacher.logits alone (prepared faces)   %9.1f img/s  = %.3f ms per batch" % (alone, 128 / alone * 1e3))
    for label, src in [("baseline files, default path", dict(read=lambda ps: [files[int(p)] for p in ps])),
                       ("progressive files, progressive=True", dict(read=lambda ps: [prog[int(p)] for p in ps], progressive=True))]:
        fe.buildImdb(teacher, imdb, batchSize=128, **src)
        for rep in range(2):
            r = loop_rate(teacher, imdb, n, **src)
            print("    %-45s %9.1f img/s  (%+.1f %% vs alone)" % (label, r, 100 * (r / alone - 1)))


def pil_frames_fn(files):
    """frames(paths, device) for buildImdb: PIL on 10 host threads, uploaded from pinned memory"""
    from PIL import Image
    pool = ThreadPoolExecutor(10)
    dec = lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))                       # noqa: E731

    def pil_frames(paths, device):
        a8 = np.stack(list(pool.map(dec, [files[int(p)] for p in paths])), 0)                  # n x H x W x 3
        t = torch.from_numpy(a8).pin_memory().to(device, non_blocking=True)
        return t.to(torch.float32).permute(0, 3, 2, 1).contiguous().permute(3, 2, 1, 0)         # MATLAB layout
    return pil_frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--teacher", default="senet50-ferplus")
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--split", action="store_true", help="the table of the segment-parallel entropy decode")
    ap.add_argument("--progressive", action="store_true", help="baseline against progressive encodings of the same images")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    L = _lib.load()
    files, have_pil = make_files(128)
    print("128 files, %s, %.1f kB on average" % ("256 x 256 4:2:0 quality 90 (PIL)" if have_pil else
                                                  "the golden files repeated (PIL is not importable)",
                                                  sum(map(len, files)) / 128e3))
    if a.split:
        return split_table(a, L, files, have_pil)
    if a.progressive:
        if not have_pil:
            raise SystemExit("--progressive needs PIL to encode the files")
        return progressive_table(a, L, files)
    full = lambda: vl.imreadjpeg(files, resize=(224, 224), crop_size=1 / 1.6, average_image=fe.AVERAGE_IMAGE)   # noqa: E731
    full()
    torch.cuda.synchronize()
    print("(a) per batch of 128")
    for k, v in kernel_ms(L, full, a.reps).items():
        print("    %-34s %8.3f ms" % (k, v))
    t0 = time.perf_counter()
    for _ in range(a.reps):
        vl.jpeg_plan(files, stage=vl._pinned)
    t_plan = (time.perf_counter() - t0) / a.reps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        full()
    t_host = (time.perf_counter() - t0) / a.reps
    torch.cuda.synchronize()
    print("    %-34s %8.3f ms" % ("host: copy into pinned + xm_jpeg_plan", t_plan * 1e3))
    print("    %-34s %8.3f ms" % ("host: whole imreadjpeg call", t_host * 1e3))
    print("    %-34s %8.3f ms" % ("device: whole call, back to back", timeit(full, a.reps) * 1e3))
    if have_pil:
        print("(b) PIL on the same files")
        for rep in range(2):
            print("    10 threads %9.1f img/s    16 threads %9.1f img/s" % (pil_rate(files, 10), pil_rate(files, 16)))
    # ---- (c) the loop ------------------------------------------------------------------------------------------------
    teacher, imdb, n, alone = loop_setup(a, full())
    read = lambda paths: [files[int(p)] for p in paths]                                        # noqa: E731
    imgs = vl.imreadjpeg(files)
    uniform = len({tuple(i.shape) for i in imgs}) == 1
    print("(c) %s, batch 128, %d frames" % (a.teacher, n))
    print("    FrozenTeacher.logits alone (prepared faces)   %9.1f img/s  = %.3f ms per batch" % (alone, 128 / alone * 1e3))
    if uniform:
        one = torch.stack([i.permute(2, 1, 0) for i in imgs], 0).permute(3, 2, 1, 0)
        prepared = lambda paths, device: one[..., :len(paths)]                                 # noqa: E731
        fe.buildImdb(teacher, imdb, prepared, batchSize=128)
        r = max(loop_rate(teacher, imdb, n, frames=prepared) for _ in range(3))
        print("    buildImdb loop, prepared decoded frames       %9.1f img/s  (%+.1f %% vs alone)" % (r, 100 * (r / alone - 1)))
    if have_pil and uniform:
        pil_frames = pil_frames_fn(files)
        fe.buildImdb(teacher, imdb, pil_frames, batchSize=128)
        for rep in range(2):
            r = loop_rate(teacher, imdb, n, frames=pil_frames)
            print("    buildImdb loop, PIL on 10 threads             %9.1f img/s  (%+.1f %% vs alone)" % (r, 100 * (r / alone - 1)))
    fe.buildImdb(teacher, imdb, read=read, batchSize=128)
    for rep in range(2):
        r = loop_rate(teacher, imdb, n, read=read)
        print("    buildImdb loop, device JPEG decode            %9.1f img/s  (%+.1f %% vs alone)" % (r, 100 * (r / alone - 1)))


if __name__ == "__main__":
    main()
