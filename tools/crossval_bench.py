#!/usr/bin/env python
"""Timing of the cross-validation step of external/run_cross_val.m + emo_benchmarks.m on the device: aggregation of
per-frame logits (xm_aggregate_logits, 'peak'), the fits of all folds (xm_mnrfit, one launch) and the scoring of all
folds (xm_mnrval, one launch), at an RML-like size (700 tracks, p = 8, k = 6) and an AFEW-like size (1156 tracks,
k = 7), non-separable planted features, 1 .. 20 frames per track.
usage: python tools/crossval_bench.py [--folds 10] [--reps 20]
Prints the device time per stage (events around each call, averaged over --reps) and the number of kernel launches per
stage for 1 fold and for --folds folds (torch.profiler device events): the shape does not depend on the fold count."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcncrossmodalemotions_amd import emo_benchmarks as eb, vl  # noqa: E402


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


def problem(n, k, folds, seed):
    rng = np.random.default_rng(seed)
    y = rng.permutation(np.arange(n) % k) + 1
    mu = rng.standard_normal((k, 8)) * 0.8
    counts = rng.integers(1, 21, n)
    frames = np.concatenate([mu[y[i] - 1] + rng.standard_normal((c, 8)) for i, c in enumerate(counts)], 0)
    last = np.cumsum(counts).astype(np.int32)
    first = (last - counts + 1).astype(np.int32)
    tr, va = eb.cross_val_folds(rng.permutation(n) + 1, folds)
    return (vl.from_numpy(np.asfortranarray(frames.astype(np.float32))), torch.from_numpy(first).cuda(),
            torch.from_numpy(last).cuda(), torch.from_numpy(y.astype(np.int32)).cuda(), tr, va, int(counts.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for name, n, k in (("RML-like", 700, 6), ("AFEW-like", 1156, 7)):
        fl, first, last, y, tr, va, F = problem(n, k, a.folds, n)
        X = vl.aggregate_logits(fl, first, last, "peak")[0]
        B, st, it, dv = vl.mnrfit(X, y, tr, k)
        ta = timeit(lambda: vl.aggregate_logits(fl, first, last, "peak"), a.reps)
        tf = timeit(lambda: vl.mnrfit(X, y, tr, k), a.reps)
        tv = timeit(lambda: vl.mnrval(B, X, va, y), a.reps)
        iters = it.cpu().numpy()
        print("%-9s %4d tracks (%5d frames), p = 8, k = %d, %d folds: status %s, Newton iterations %d..%d"
              % (name, n, F, k, a.folds, sorted(set(st.cpu().numpy().tolist())), iters.min(), iters.max()))
        print("  aggregate ('peak')  %9.1f us" % ta)
        print("  mnrfit  (all folds) %9.1f us  (%.1f us per Newton iteration of the slowest fold)"
              % (tf, tf / max(1, iters.max())))
        print("  mnrval  (all folds) %9.1f us" % tv)
        print("  total               %9.1f us" % (ta + tf + tv))
        for label, trs, vas in (("1 fold", tr[:1], va[:1]), ("%d folds" % a.folds, tr, va)):
            Bg = _first_sets(B, len(vas))
            c = [launches(lambda: vl.aggregate_logits(fl, first, last, "peak")),
                 launches(lambda: vl.mnrfit(X, y, trs, k)),
                 launches(lambda: vl.mnrval(Bg, X, vas, y))]
            print("  kernel launches, %-8s aggregate %s, mnrfit %s, mnrval %s" % (label + ":", *c))


def _first_sets(B, G):
    """the first G coefficient sets as a (p+1) x (k-1) x G MATLAB-layout tensor."""
    return B.permute(2, 1, 0)[:G].contiguous().permute(2, 1, 0)


if __name__ == "__main__":
    main()
