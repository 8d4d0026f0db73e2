#!/usr/bin/env python
"""ms per update of the full-width student's flat parameter buffer: xm_sgd_update against every kind of xm_solver_update
(cnn_train_dag's 'solver' option and the nesterovUpdate arm), in one process and one call.
usage: python tools/solver_bench.py [--reps 50] [--rounds 5] [--width 1.0] [--out FILE]

One update = one launch per 'gradient' segment of the flat buffer, as train.accumulate_gradients issues them.  The kinds are
timed in alternation (`rounds` windows of `reps` updates each, device events around a window); the figure is the median
window.  The kernels are pure streaming: floats moved per element are 5 (w, state, der read; w, state written) for SGD,
adagrad, rmsprop and nesterov and 7 for adadelta and adam (a second state read and written), so the expected time ratio to
xm_sgd_update is 1.0 and 1.4.  GB/s is over those algorithmic bytes; "share" is that rate over the 6.3 TB/s a float4 copy
reaches on an MI355X (8 TB/s peak)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcncrossmodalemotions_amd import vl, zoo  # noqa: E402

ACHIEVABLE_GBS = 6300.0
FLOATS = {"sgd": 5, "adagrad": 5, "rmsprop": 5, "nesterov": 5, "adadelta": 7, "adam": 7}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("solver_bench: needs a GPU (a timing taken elsewhere says nothing)")
    net = zoo.emoVoxZoo(numSeconds=4, seed=0, width_mult=a.width)
    flat = net.pack_params()
    segs = [(lm, wm, s, e) for (method, lm, wm), s, e in flat.segments if method == "gradient" and e > s]
    n = sum(e - s for _, _, s, e in segs)
    torch.manual_seed(0)
    flat.der.copy_(torch.randn_like(flat.der) * 1e-3)
    kinds = ["sgd", "adagrad", "rmsprop", "nesterov", "adadelta", "adam"]
    # every kind keeps states of its own (a momentum is no second moment: adagrad on SGD's state takes sqrt of negatives)
    state1 = {k: torch.zeros_like(flat.mom) for k in kinds}
    state2 = {k: torch.zeros_like(flat.mom) for k in kinds if k != "sgd" and vl.SOLVERS[k][2]}
    lr, wd, batch = 1e-4, 5e-4, 64.0
    t = {"adam": 0}

    def update(kind):
        if kind == "adam":
            t["adam"] += 1
        for lm, wm, s, e in segs:
            w, m, d = flat.val[s:e], state1[kind][s:e], flat.der[s:e]
            if kind == "sgd":
                vl.sgd_update(w, m, d, lr * lm, 0.9, wd * wm, batch)
            else:
                s2 = state2[kind][s:e] if kind in state2 else None
                vl.solver_update(kind, w, m, s2, d, lr * lm, wd * wm, batch, t=max(t["adam"], 1))

    for k in kinds:                      # warm up: code objects, the allocator
        for _ in range(3):
            update(k)
    torch.cuda.synchronize()
    windows = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for k in kinds:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.reps):
                update(k)
            e.record()
            torch.cuda.synchronize()
            windows[k].append(s.elapsed_time(e) / a.reps)
    assert bool(torch.isfinite(flat.val).all()) and all(bool(torch.isfinite(v).all()) for v in state1.values())
    res = {"elements": n, "segments": len(segs), "reps": a.reps, "rounds": a.rounds, "kinds": {}}
    base = statistics.median(windows["sgd"])
    print("%d elements in %d segments (%.1f MB per buffer); %d rounds of %d updates" % (n, len(segs), n * 4 / 1e6, a.rounds,
                                                                                       a.reps))
    print("%-9s %9s %9s %9s %7s %9s %7s %7s" % ("kind", "ms", "min", "max", "floats", "GB/s", "share", "x sgd"))
    for k in kinds:
        ms = statistics.median(windows[k])
        gbs = FLOATS[k] * 4 * n / ms / 1e6
        res["kinds"][k] = {"ms": ms, "min_ms": min(windows[k]), "max_ms": max(windows[k]), "floats_per_element": FLOATS[k],
                           "GBps": gbs, "share_of_achievable": gbs / ACHIEVABLE_GBS, "ratio_to_sgd": ms / base,
                           "byte_ratio_to_sgd": FLOATS[k] / FLOATS["sgd"]}
        print("%-9s %9.4f %9.4f %9.4f %7d %9.0f %7.2f %7.2f" % (k, ms, min(windows[k]), max(windows[k]), FLOATS[k], gbs,
                                                                gbs / ACHIEVABLE_GBS, ms / base))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
