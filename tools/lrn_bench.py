#!/usr/bin/env python
"""vl_nnnormalize against the copy that moves the same bytes, and the frozen VGG-Face teacher.

norm1 / norm2 of VGG-M at 128 faces (109 x 109 x 96 and 26 x 26 x 256, PARAM [5 2 1e-4 0.75]): device time of the forward and
of the backward call and of a hipMemcpyAsync device-to-device copy of one tensor (read once, written once: the forward's
traffic; the backward moves three tensors, so its line is 1.5 x the copy), all from HIP events in this one process, the three
alternating, over buffer sets that together exceed the 256 MiB last-level cache.  Then the frozen 'vgg-vd-face-fer' and
'resnet50-ferplus' stand-ins at 128 faces: images per second and the share of the fp32 MFMA peak that the convolutions'
FLOPs (counted here from the graph) amount to.
usage: python tools/lrn_bench.py [--faces 128] [--rounds 7] [--skip-teachers]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mcncrossmodalemotions_amd import _lib, batch, dagnn, vl, zoo

PEAK_FP32_MFMA = 157.3e12       # MI355X, dense fp32 matrix rate (flop/s)
PARAM = [5, 2, 1e-4, 0.75]
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
D2D = 3


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps          # ms per call


def lrn_case(name, shape, rounds):
    n = int(np.prod(shape))
    sets = max(2, -(-(1 << 30) // (12 * n)))            # x, dzdy, out of every set: more than 1 GiB in all
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    xs = [torch.randn(tuple(reversed(shape)), generator=g, device="cuda").permute(3, 2, 1, 0) for _ in range(sets)]
    ds = [torch.randn(tuple(reversed(shape)), generator=g, device="cuda").permute(3, 2, 1, 0) for _ in range(sets)]
    ys = [vl.mat_empty(*shape) for _ in range(sets)]
    # the C ABI directly, with the pointers made beforehand: a 26 x 26 x 256 x 128 call takes tens of microseconds, and the
    # host must not be what the events measure
    L = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    px, pd, py = ([C.c_void_p(t.data_ptr()) for t in ts] for ts in (xs, ds, ys))
    dims = [int(v) for v in shape]
    prm = (int(PARAM[0]), C.c_float(PARAM[1]), C.c_float(PARAM[2]), C.c_float(PARAM[3]))
    runs = {"copy": lambda i: hip.hipMemcpyAsync(py[i % sets], px[i % sets], 4 * n, D2D, st),
            "forward": lambda i: L.xm_nnnormalize_forward(px[i % sets], *dims, *prm, py[i % sets], st),
            "backward": lambda i: L.xm_nnnormalize_backward(px[i % sets], pd[i % sets], *dims, *prm, py[i % sets], st)}
    assert runs["forward"](0) == 0 and runs["backward"](0) == 0
    reps = max(4 * sets, int(2e11 // (8 * n)))          # ~40 ms of copy per timing
    ms = {k: [] for k in runs}
    for k, fn in runs.items():
        timed(fn, sets)                                 # warm-up
    for _ in range(rounds):
        for k, fn in runs.items():
            ms[k].append(timed(fn, reps))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (min(v), max(v)) for k, v in ms.items()}
    gb = 8 * n / 1e9
    print("%s %s x %d sets, %d calls per timing, %d timings each (median [min .. max] ms per call)" % (name, shape, sets, reps, rounds))
    for k in runs:
        traffic = gb * (1.5 if k == "backward" else 1.0)
        print("  %-8s %8.4f [%8.4f .. %8.4f] ms   %6.2f TB/s" % (k, med[k], spread[k][0], spread[k][1], traffic / med[k]))
    print("  forward / copy = %.3f    backward / (1.5 x copy) = %.3f" % (med["forward"] / med["copy"],
                                                                        med["backward"] / (1.5 * med["copy"])))


def graph_flops(net, size, n):
    """2 * FH * FW * FC * K per output pixel of every convolution of a chain or ResNet graph, for n size x size inputs"""
    hw, total = {v: size for v in net.getInputs()}, 0.0
    for l in net.layers:
        b, h = l.block, hw.get(l.inputs[0])
        if isinstance(b, dagnn.Conv):
            p = vl._pad4(b.pad)
            h = vl.out_size(h, p[0], p[1], b.size[0], b.dilate[0], b.stride[0])
            total += 2.0 * b.size[0] * b.size[1] * b.size[2] * b.size[3] * h * h * n
        elif isinstance(b, dagnn.GlobalPooling):
            h = 1
        elif isinstance(b, dagnn.Pooling):
            p = vl._pad4(b.pad)
            h = vl.out_size(h, p[0], p[1], b.poolSize[0], 1, vl._pair(b.stride, "STRIDE")[0])
        elif isinstance(b, dagnn.Axpy):
            h = hw.get(l.inputs[1])
        for v in l.outputs:
            hw[v] = h
    return total


def teacher_case(name, faces, rounds):
    net = zoo.ferPlusZoo(name)
    zoo.strip_losses(net)
    net.mode = "test"
    net.move("gpu")
    avg = net.meta["normalization"]["averageImage"]
    data = batch.getImageBatch(faces, averageImage=avg, seed=2)
    teacher = zoo.FrozenTeacher(net, lanes=2)
    for _ in range(3):
        teacher.logits(data)                            # first sight of the shapes: tile configurations are measured
    torch.cuda.synchronize()
    reps, ts = 10, []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            teacher.logits(data)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / reps)
    t = float(np.median(ts))
    fl = graph_flops(net, 224, faces)
    print("%-18s %4d faces: %8.1f img/s [%.1f .. %.1f]   %.1f GFLOP per call   %.1f %% of the fp32 MFMA peak" % (
        name, faces, faces / t, faces / max(ts), faces / min(ts), fl / 1e9, 100 * fl / t / PEAK_FP32_MFMA))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-teachers", action="store_true")
    args = ap.parse_args()
    print("vl_nnnormalize geometry (pixels per block, channels per pass, window in registers): %s" % (vl.nnnormalize_geometry(),))
    lrn_case("norm1", (109, 109, 96, args.faces), args.rounds)
    lrn_case("norm2", (26, 26, 256, args.faces), args.rounds)
    if not args.skip_teachers:
        teacher_case("vgg-vd-face-fer", args.faces, args.rounds)
        teacher_case("resnet50-ferplus", args.faces, args.rounds)
