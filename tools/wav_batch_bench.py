#!/usr/bin/env python
"""The waveform front-end of the student's batch provider, clip by clip and batched.
usage: python tools/wav_batch_bench.py [--clips 64] [--width 300] [--reps 9]
For transformations I, IS, ISN at `clips` clips of W = `width` (the student's real batch: 64 x 300) it prints medians
over `reps` batches, each with fresh draws from one seeded stream, the two paths alternating in the same process:
  plan      batch.wav_batch_plan: the host draws and the descriptor table (shared by both paths)
  per-clip  batch.wav_clips: slice, host filter design + upload + xm_resample ('S'), xm_scale_axpy ('N') per clip
  batched   vl.wav_batch: one pinned upload + xm_wav_batch (two launches); `device` is the event time of the same call
  runSpec   the STFT behind either (one convolution + the magnitude kernel)
Wall times are host clocks around work that ends in a device synchronise."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcncrossmodalemotions_amd import batch, vl  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--width", type=int, default=300)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    imdb = batch.SyntheticEmoVoxImdb(num_tracks=max(a.clips, 64), seed=0)
    L = int(round(batch.aud_samples(a.width)))
    wav, _ = imdb.device_wav_bank(dev)
    noise, _ = imdb.device_noise_bank(dev)
    med = statistics.median
    print("%d clips, W = %d (L = %d samples), medians of %d batches, ms" % (a.clips, a.width, L, a.reps))
    print("%-4s %8s %10s %10s %10s %9s %9s %12s" % ("", "plan", "per-clip", "batched", "(device)", "runSpec", "ratio",
                                                     "max|diff|"))
    for tr in ("I", "IS", "ISN"):
        rng = np.random.default_rng(11)
        pick = np.random.default_rng(12)
        rows = []
        for rep in range(a.reps + 1):                        # the first batch warms every shape up and is dropped
            idx = [int(i) for i in pick.permutation(len(imdb.num_samples))[:a.clips]]
            t0 = time.perf_counter()
            desc, ratio, _, _ = batch.wav_batch_plan(imdb, idx, a.width, tr, rng)
            t_plan = (time.perf_counter() - t0) * 1e3
            nz = noise if "N" in tr else None
            t_clip, z1 = wall(lambda: batch.wav_clips(imdb, idx, desc, ratio, L, dev))
            t_bat, z2 = wall(lambda: vl.wav_batch(wav, nz, desc, ratio, L))
            t_dev = device_ms(lambda: vl.wav_batch(wav, nz, desc, ratio, L))
            t_spec, _ = wall(lambda: batch.runSpec(z2, {"fs": imdb.fs}))
            diff = float((z1 - z2).abs().max())
            if rep:
                rows.append((t_plan, t_clip, t_bat, t_dev, t_spec, diff))
        c = [med(r[i] for r in rows) for i in range(5)]
        print("%-4s %8.3f %10.3f %10.3f %10.3f %9.3f %8.1fx %12.2e" % (tr, c[0], c[1], c[2], c[3], c[4], c[1] / c[2],
                                                                     max(r[5] for r in rows)))
        lo, hi = [min(r[i] for r in rows) for i in (1, 2)], [max(r[i] for r in rows) for i in (1, 2)]
        print("     spread over the batches: per-clip %.3f .. %.3f, batched %.3f .. %.3f" % (lo[0], hi[0], lo[1], hi[1]))


if __name__ == "__main__":
    main()
