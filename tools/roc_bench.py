#!/usr/bin/env python
"""Timing of the ranking step of emoVoxCeleb/student_stats.m on the device: vl_roc for the three EmoVoxCeleb partitions
(118,485 / 30,496 / 4,505 tracks) x 8 emotions in one xm_roc call, fp32 softmax scores of N(0, 3) logits, and the
dominant-emotion histogram of teacher_stats.m at 5,078,961 frames x 8 (xm_label_hist).
usage: python tools/roc_bench.py [--reps 20] [--host-reps 3]
Prints (1) the device time of vl.roc without and with the curve outputs (events around the call, averaged over --reps,
index sets uploaded beforehand; the line "with set upload" includes the host check and the copy of the sets) and of
vl.label_hist; (2) the time of the numpy restatement of vl_roc on the same scores, serial and on 16 threads; (3) the
bytes the pass structure moves through HBM per call over the measured time, next to 6.3 TB/s; (4) the kernel launches
of one call for (G, E) = (1, 1), (3, 8), (6, 8) (torch.profiler device events; xm_roc_launches() is what the library
states)."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcncrossmodalemotions_amd import _lib, vl  # noqa: E402

SIZES = (118485, 30496, 4505)          # misc/generateBaseImdb.m:46-56
FRAMES = 5078961                       # teacher_stats.m: rows of vertcat(imdb.wavLogits{:})
HBM = 6.3e12                           # achievable bytes / s


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def launches(fn):
    """device kernels the call enqueues (None if the profiler records no device activity)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if getattr(ev, "device_type", None) is not None
             and str(ev.device_type).endswith("CUDA") and "Memcpy" not in ev.name and "Memset" not in ev.name]
    return len(names) if names else None


def np_auc(lab, sc):
    """vl_roc restated (stable descending sort, cumulative sums, floating trapezoid): what a user runs on the host"""
    perm = np.argsort(-sc, kind="stable")
    pos = lab[perm] > 0
    ret = int((sc > -np.inf).sum())
    tp = np.concatenate([[0], np.cumsum(pos)[:ret]]).astype(np.float64)
    fp = np.arange(ret + 1, dtype=np.float64) - tp
    tpr, fpr = tp / max(pos.sum(), 1e-10), fp / max((~pos).sum(), 1e-10)
    return 0.5 * np.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]))


def roc_bytes(nnz, E, curve):
    """HBM traffic of one xm_roc call from its pass structure, 4-byte words per entry of the nnz x E problem: keys
    (rows, score, class in; key, position out) 5, each of 4 radix passes (histogram: key in; scatter: key, position
    in and out) 5, positives per tile (position, row, class) 3, curve (key, position, row, class; + perm, tp) 4 (+ 2)"""
    return 4 * nnz * E * (5 + 4 * 5 + 3 + 4 + (2 if curve else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    n, E = sum(SIZES), 8
    logits = (rng.standard_normal((n, E)) * 3).astype(np.float32)
    cls = np.where(rng.random(n) < 0.5, rng.integers(1, E + 1, n), logits.argmax(1) + 1).astype(np.int32)
    order = rng.permutation(n) + 1
    ends = np.cumsum(SIZES)
    sets = [order[e - s:e] for s, e in zip(SIZES, ends)]
    scores = vl.vl_nnsoftmaxt(vl.from_numpy(np.asfortranarray(logits), dev), dim=2)
    dcls = torch.from_numpy(cls).to(dev)
    pre = vl.roc_sets(sets, n, dev)

    t0 = timeit(lambda: vl.roc(scores, dcls, pre), a.reps)
    t1 = timeit(lambda: vl.roc(scores, dcls, pre, want_curve=True), a.reps)
    t2 = timeit(lambda: vl.roc(scores, dcls, sets, want_curve=True), a.reps)
    print("xm_roc, %d + %d + %d rows x %d emotions, one call (%d launches stated by the library)"
          % (SIZES + (E, _lib.load().xm_roc_launches())))
    for label, t, curve in (("auc only", t0, False), ("with curve outputs", t1, True)):
        b = roc_bytes(n, E, curve)
        print("  %-22s %9.1f us   %6.1f MB through HBM -> %6.1f GB/s (%.1f %% of %.1f TB/s; floor %.1f us)"
              % (label, t, b / 1e6, b / t / 1e3, 100 * b / (t * 1e-6) / HBM, HBM / 1e12, b / HBM * 1e6))
    print("  %-22s %9.1f us   (host check and copy of the index sets included)" % ("with set upload", t2))

    host = vl.to_numpy(scores)
    probs = [(np.where(cls[s - 1] == c + 1, 1, -1), np.ascontiguousarray(host[s - 1, c])) for s in sets for c in range(E)]
    got = vl.roc(scores, dcls, pre)["auc"].cpu().numpy().reshape(-1)
    ts, tt = [], []
    for _ in range(a.host_reps):
        t = time.perf_counter()
        ref = [np_auc(*p) for p in probs]
        ts.append(time.perf_counter() - t)
        with ThreadPoolExecutor(16) as ex:
            t = time.perf_counter()
            ref = list(ex.map(lambda p: np_auc(*p), probs))
            tt.append(time.perf_counter() - t)
    print("numpy restatement on the same scores: serial %.1f ms, 16 threads %.1f ms (best of %d); max |auc - device| = %.2e"
          % (min(ts) * 1e3, min(tt) * 1e3, a.host_reps, np.abs(np.array(ref) - got).max()))
    print("  device / host (16 threads): %.3f" % (t0 * 1e-6 / min(tt)))

    for G, Ec in ((1, 1), (3, 8), (6, 8)):
        sc = scores[:, :Ec] if Ec == E else scores[:, :1].contiguous()
        st = (sets * 2)[:G]
        pr = vl.roc_sets(st, n, dev)
        vl.roc(sc, dcls, pr, want_curve=True)
        print("  kernel launches, G = %d, E = %d: %s" % (G, Ec, launches(lambda: vl.roc(sc, dcls, pr, want_curve=True))))

    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.randn(E, FRAMES, generator=g, device=dev, dtype=torch.float32).t()
    bins = torch.zeros(E, dtype=torch.int64, device=dev)
    th = timeit(lambda: vl.label_hist(x, bins=bins), a.reps)
    b = 4 * FRAMES * E
    print("xm_label_hist, %d frames x %d: %9.1f us   %6.1f MB -> %6.1f GB/s (%.1f %% of %.1f TB/s), launches %s"
          % (FRAMES, E, th, b / 1e6, b / th / 1e3, 100 * b / (th * 1e-6) / HBM, HBM / 1e12,
             launches(lambda: vl.label_hist(x, bins=bins))))
    xh = x.cpu().numpy()
    t = time.perf_counter()
    np.bincount(xh.argmax(1), minlength=E)
    print("  numpy argmax + bincount on the host: %.1f ms" % ((time.perf_counter() - t) * 1e3))


if __name__ == "__main__":
    main()
