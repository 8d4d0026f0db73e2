#!/usr/bin/env python
"""Timing of the FER+ batch path (getBatchFerPlus, teacher/ferplus_baselines.m:182-213) at N = 128, 48 -> 224:
the fused xm_ferplus_batch against the standalone pair vl_nnaffinegrid + vl_nnbilinearsampler (on an already
normalised RGB batch, as the reference's host loop leaves it), and the sampler's backward (dX atomics + dGrid).
usage: python tools/ferplus_bench.py [--n 128] [--reps 50]
Prints us per call and the effective rate over the ALGORITHMIC bytes (each tensor once; for the backward also the
rate of the float-atomic adds, 4 B per nonzero tap weight)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcncrossmodalemotions_amd import batch, vl  # noqa: E402


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    N, H, Ho = a.n, 48, 224
    avg = (131.0912, 103.8827, 91.4953)
    imdb = batch.SyntheticFerPlusImdb(num_images=N, seed=0)
    rng = np.random.default_rng(0)
    augs = batch.computeAugs(N, rng)
    A = np.stack([batch.affine_params(augs[:, :, i]) for i in range(N)], 1).astype(np.float32)
    Ad = vl.from_numpy(A.reshape(1, 1, 6, N))
    flips = torch.from_numpy((rng.random(N) > 0.5).astype(np.int32)).cuda()
    grey = vl.from_numpy(imdb.images["data"])
    rgb = vl.from_numpy(np.repeat(imdb.images["data"], 3, axis=2) - np.asarray(avg, np.float32).reshape(1, 1, 3, 1))
    out_b, grey_b = Ho * Ho * 3 * N * 4, H * H * N * 4
    t = timeit(lambda: vl.ferplus_batch(grey, Ad, flips, avg, (Ho, Ho)), a.reps)
    print("xm_ferplus_batch        %8.1f us  %6.2f TB/s  (writes %.1f MB, reads %.2f MB)"
          % (t, (out_b + grey_b) / t * 1e-6, out_b / 1e6, grey_b / 1e6))
    grid = vl.vl_nnaffinegrid(Ad, [Ho, Ho])
    tg = timeit(lambda: vl.vl_nnaffinegrid(Ad, [Ho, Ho]), a.reps)
    ts = timeit(lambda: vl.vl_nnbilinearsampler(rgb, grid), a.reps)
    g_b = 2 * Ho * Ho * N * 4
    print("vl_nnaffinegrid         %8.1f us  %6.2f TB/s" % (tg, g_b / tg * 1e-6))
    print("vl_nnbilinearsampler    %8.1f us  %6.2f TB/s" % (ts, (out_b + g_b + 3 * grey_b) / ts * 1e-6))
    print("standalone pair         %8.1f us  (fused: %.2fx faster)" % (tg + ts, (tg + ts) / t))
    dy = vl.from_numpy(np.random.default_rng(1).standard_normal((Ho, Ho, 3, N)).astype(np.float32))
    # nonzero tap weights = the atomic adds of dX
    g = vl.to_numpy(grid).astype(np.float64)
    adds = 0
    for k, S in ((0, H), (1, H)):
        p = (g[k] + 1) * 0.5 * (S - 1)
        g[k] = p
    sy, sx = np.floor(g[0]), np.floor(g[1])
    wy, wx = g[0] - sy, g[1] - sx
    for ay in (0, 1):
        for bx in (0, 1):
            iy, ix = sy + ay, sx + bx
            w = (wy if ay else 1 - wy) * (wx if bx else 1 - wx)
            adds += int(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < H) & (w != 0)).sum())
    adds *= 3
    tb = timeit(lambda: vl.vl_nnbilinearsampler(rgb, grid, dy), a.reps)
    print("sampler backward        %8.1f us  atomic adds %.1f MB -> %.2f TB/s (%.0f %% of the 1.3 TB/s atomic rate)"
          % (tb, adds * 4 / 1e6, adds * 4 / tb * 1e-6, adds * 4 / tb * 1e-6 / 1.3 * 100))


if __name__ == "__main__":
    main()
