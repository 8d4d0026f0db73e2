#!/usr/bin/env python
"""The distillation step as the package runs it with teacherMode='online' (batch.OnlineTeacher inside
getBatchEmoVoxCeleb, train.train_step), next to bench.py's own figures taken in the same call.
usage: python tools/online_distill_bench.py [--seconds 1.0] [--no-bench]
Prints, one line each (ms per step on the wall clock between two device synchronisations, pairs/s, the host's share):
 (0) bench.py's default line and its north_star_b256 (a child `python bench.py --full --no-cpu-baseline --no-roofline`);
 (a) the cached-mode step: getBatchEmoVoxCeleb over imdb.wavLogits + train_step, 32 pairs, resident spectrograms;
 (b) the online step on resident decoded frames (frames=): 32 pairs x 1 frame with the resnet50 teacher -- overlapped,
     on the calling stream, and without the student's wgrad side stream, which run_distillation does not set up -- and
     256 pairs x 1 frame with the senet50 teacher (north_star's configuration);
 (c) the online step from the 128 JPEG files of tools/jpeg_bench.py (read=): 1 and 13 frames per pair, split=None and
     split=512, 32 pairs, resnet50 teacher.
Every step plans its batch on the host (wav_batch_plan, online_frame_plan), which bench.py does not: its inputs are
resident and its teacher works one batch ahead (--teacher-prefetch)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mcncrossmodalemotions_amd import batch as xbatch, fetch_emovoxceleb_imdb as fe, train, vl, zoo  # noqa: E402

W = 300


def bench_lines():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline", "--no-roofline"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600, cwd=ROOT)
    try:
        d = json.loads(r.stdout.decode().strip().splitlines()[-1])
    except (ValueError, IndexError):
        print("(0) bench.py gave no result line (exit %d)" % r.returncode)
        return
    line("(0) bench.py default: resnet50 teacher, 32 pairs", d["ms_per_step"], 32)
    ns = d.get("north_star_b256") or {}
    if "ms_per_step" in ns:
        line("(0) bench.py north_star_b256: senet50 teacher, 256 pairs", ns["ms_per_step"], 256)
    else:
        print("(0) bench.py north_star_b256: %s" % ns)


def line(label, ms, pairs, host_ms=None):
    print("%-78s %9.3f ms/step %9.1f pairs/s%s" % (label, ms, pairs / ms * 1e3,
                                                    "" if host_ms is None else "   host %7.3f ms/step" % host_ms), flush=True)


def teacher_net(name, dev):
    net = zoo.ferPlusZoo("%s-ferplus" % name, seed=100)
    zoo.strip_losses(net)
    net.move("gpu")
    zoo.calibrate_moments(net, ["data", xbatch.getImageBatch(16, seed=999, device=dev)])
    net.mode = "test"
    return net


def framed_imdb(num_tracks, paths_of=None):
    """(imdb with frame lists, the same with seeded wavLogits): tracks of 6 .. 12 s"""
    import copy
    syn = xbatch.SyntheticEmoVoxImdb(num_tracks=num_tracks, seed=1, min_seconds=6.0, max_seconds=12.0)
    src = fe.src_imdb(syn)
    dense = xbatch.SyntheticDenseFrames(src)
    imdb = fe.addFramesToImdb(src, dense.lister)
    if paths_of is not None:
        imdb.images["denseFrames"] = [paths_of(i) for i in range(len(imdb.images["denseFrames"]))]
    cached = copy.copy(imdb)
    cached.wavLogits = syn.wavLogits
    return imdb, cached


def measure(label, student, imdb, pairs, spec, seconds, online=None):
    """steps of getBatchEmoVoxCeleb + train_step over random batches of `pairs` tracks, at most two in flight"""
    rng, pick = np.random.default_rng(3), np.random.default_rng(4)
    opts = train.TrainOpts(batchSize=pairs)
    T = len(imdb.set)
    ahead = train._RunAhead(student.device)
    host = [0.0]

    def step(it):
        t0 = time.perf_counter()
        sel = pick.choice(T, pairs, replace=False)
        inputs = xbatch.getBatchEmoVoxCeleb(imdb, sel, imageSize=(512, W), rng=rng, spec_source=spec, onlineTeacher=online)
        train.train_step(student, inputs, opts, it, None, pairs, input_events=getattr(inputs, "input_events", None))
        host[0] += time.perf_counter() - t0
        ahead.tick()

    tw = time.perf_counter()
    it = 0
    while it < 6 or time.perf_counter() - tw < 1.5:          # tile choices, the clock's steady state (bench.py's settle)
        step(it)
        it += 1
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(3):
        step(it)
    torch.cuda.synchronize()
    K = max(10, int(np.ceil(seconds / ((time.perf_counter() - t1) / 3))))
    host[0] = 0.0
    t0 = time.perf_counter()
    for k in range(K):
        step(it + k)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    line(label, dt / K * 1e3, pairs, host[0] / K * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="length of every timed region")
    ap.add_argument("--no-bench", action="store_true", help="leave out the child bench.py of (0)")
    a = ap.parse_args()
    if not a.no_bench:
        bench_lines()                                        # before this process opens the device
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    student = zoo.emoVoxZoo("emovoxceleb-student", scratch=1, lossType="hot-cross-ent", numSeconds=W / 100.0, numOutputs=8,
                            seed=200)
    student.pack_params()
    side = torch.cuda.Stream(device=dev)
    student.wgradStream = side                               # as bench.py --wgrad-stream 1
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    spec256 = torch.randn((256, 1, W, 512), generator=g, device=dev, dtype=torch.float32).abs_().permute(3, 2, 1, 0)
    spec32 = spec256[..., :32]
    imdb, cached = framed_imdb(512)
    measure("(a) cached: getBatch over imdb.wavLogits + train_step, 32 pairs", student, cached, 32, spec32, a.seconds)

    # ---- (b) resident decoded frames ------------------------------------------------------------------------------
    raw = torch.randint(0, 256, (256, 3, 358, 358), generator=g, device=dev).to(torch.float32).permute(3, 2, 1, 0)
    resident = lambda paths, device: raw[..., :len(paths)]                                     # noqa: E731
    res = teacher_net("resnet50", dev)
    for label, kw, wgrad in [("overlapped, wgrad side stream", dict(overlap=True), True),
                             ("calling stream, wgrad side stream", dict(overlap=False), True),
                             ("overlapped, no wgrad side stream (run_distillation)", dict(overlap=True), False),
                             ("calling stream, no wgrad side stream", dict(overlap=False), False)]:
        student.wgradStream = side if wgrad else None
        online = xbatch.OnlineTeacher(res, imdb, frames=resident, framesPerPair=1, **kw)
        measure("(b) online, resident frames, resnet50, 32 pairs x 1 frame: %s" % label, student, imdb, 32, spec32, a.seconds,
                online)
    student.wgradStream = side
    se = teacher_net("senet50", dev)
    for label, kw in [("overlapped", dict(overlap=True)), ("calling stream", dict(overlap=False))]:
        online = xbatch.OnlineTeacher(se, imdb, frames=resident, framesPerPair=1, chunk=256, **kw)
        measure("(b) online, resident frames, senet50, 256 pairs x 1 frame: %s" % label, student, imdb, 256, spec256, a.seconds,
                online)
    del se, raw

    # ---- (c) JPEG files -------------------------------------------------------------------------------------------
    import jpeg_bench
    files, have_pil = jpeg_bench.make_files(128)
    if not have_pil:
        files = [f for f in files if len(f) != 633]          # the 1 x 1 golden file has no 1/1.6 crop
    print("(c) %d files, %s, %.1f kB on average" % (len(files), "256 x 256 4:2:0 quality 90 (PIL)" if have_pil else
                                                    "the golden files repeated (PIL is not importable)",
                                                    sum(map(len, files)) / len(files) / 1e3))
    jimdb, _ = framed_imdb(512, paths_of=lambda i: "%d" % (i % len(files)))
    read = lambda paths: [files[int(p)] for p in paths]                                        # noqa: E731
    for fpp in (1, 13):
        for split in (None, 512):
            online = xbatch.OnlineTeacher(res, jimdb, read=read, framesPerPair=fpp, split=split)
            measure("(c) online, JPEG files, resnet50, 32 pairs x %d frame%s, split=%s" % (fpp, "" if fpp == 1 else "s", split),
                    student, jimdb, 32, spec32, a.seconds, online)
    # where the JPEG time goes: the decode of one step's files alone, back to back
    for n in (32, 416):
        batch = [files[i % len(files)] for i in range(n)]
        for split in (None, 512):
            fn = lambda: vl.imreadjpeg(batch, resize=(224, 224), crop_size=1 / 1.6, average_image=fe.AVERAGE_IMAGE,   # noqa: E731
                                       split=split)
            t0 = time.perf_counter()
            for _ in range(5):
                fn()
            th = (time.perf_counter() - t0) / 5
            print("    vl.imreadjpeg of %3d files alone, split=%-4s  device %8.3f ms   host (parse + enqueue) %8.3f ms" % (
                n, split, jpeg_bench.timeit(fn, 10) * 1e3, th * 1e3), flush=True)


if __name__ == "__main__":
    main()
