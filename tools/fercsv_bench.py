#!/usr/bin/env python
"""Timing of the FER2013 CSV path (xm_pixcsv_plan / xm_pixcsv_decode_batch, vl.pixcsv_decode) on a synthetic file of the
real size, built in memory: 35,887 rows of 2,304 values, uniform 0 .. 255, `emotion,pixels,Usage` with a header.
usage: python tools/fercsv_bench.py [--rows 35887] [--reps 7] [--chunk-mb 64] [--out profiles/fercsv/fercsv_bench.txt]
Prints, and writes verbatim to --out, from ONE call:
 (a) plan + chunked upload + decode to the finished device image array (host clock to a device synchronise), with the
     plan, the staging copies and the rest apart;
 (b) the host restatement -- np.fromstring(field, sep=' ') per row, transpose, one upload -- the thing to beat, once;
 (c) the decode kernel alone on the whole file resident on the device (device events, median) against a device-to-device
     copy of the same input bytes, alternating, and the bytes the kernel reads and writes per second.
Warm-up before every timed window; medians over --reps; only numbers of this call are compared with each other."""
import argparse
import ctypes as C
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcncrossmodalemotions_amd import _lib, vl  # noqa: E402

H = W = 48


def make_file(rows, seed=0):
    """the CSV as one uint8 array, and the values (rows x 2304 uint8)"""
    rng = np.random.default_rng(seed)
    table = np.zeros((256, 4), np.uint8)                       # "v " padded with 0 to four bytes
    for v in range(256):
        s = b"%d " % v
        table[v, :len(s)] = np.frombuffer(s, np.uint8)
    usages = [b",Training\n", b",PublicTest\n", b",PrivateTest\n"]
    parts, vals = [b"emotion,pixels,Usage\n"], []
    for r0 in range(0, rows, 1024):
        v = rng.integers(0, 256, (min(1024, rows - r0), H * W), dtype=np.uint8)
        vals.append(v)
        for i in range(len(v)):
            t = table[v[i]].ravel()
            parts.append(b"%d," % ((r0 + i) % 7))
            parts.append(t[t != 0][:-1].tobytes())             # without the trailing blank
            parts.append(usages[0 if (r0 + i) % 10 < 8 else 1 + (r0 + i) % 2])
    return np.frombuffer(b"".join(parts), np.uint8), np.concatenate(vals)


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return float(np.median(out)), float(min(out)), float(max(out))


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=35887)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fercsv", "fercsv_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fercsv_bench: no GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    L = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    data, vals = make_file(a.rows)
    nbytes, nout = int(data.size), 4 * a.rows * H * W
    say("synthetic fer2013.csv: %d rows of %d values, %.1f MB of text, %.1f MB of float32 images (built in %.1f s)"
        % (a.rows, H * W, nbytes / 1e6, nout / 1e6, time.perf_counter() - t0))
    chunk = a.chunk_mb << 20

    # ---- (a) the whole path ------------------------------------------------------------------------------------------
    out = torch.empty(a.rows * H * W, dtype=torch.float32, device=dev)
    holder = {}

    def whole():
        holder["plan"] = vl.pixcsv_plan(data)
        holder["res"] = vl.pixcsv_decode(data, holder["plan"], out=out, chunk_bytes=chunk)

    whole()                                                                  # warm-up: pinned and device buffers, code object
    t_plan = host_ms(lambda: vl.pixcsv_plan(data), 3)
    plan = holder["plan"]
    t_dec = host_ms(lambda: vl.pixcsv_decode(data, plan, out=out, chunk_bytes=chunk), a.reps)
    t_all = host_ms(whole, a.reps)
    nchunks = len(vl._pix_chunks(plan["rows"], chunk))
    say("(a) plan + upload in %d chunks of <= %d MB + decode, host clock to a device synchronise, median of %d (min .. max):"
        % (nchunks, a.chunk_mb, a.reps))
    say("    whole path            %9.1f ms (%.1f .. %.1f) = %.2f GB/s of text" % (t_all + (nbytes / t_all[0] / 1e6,)))
    say("    xm_pixcsv_plan alone  %9.1f ms (%.1f .. %.1f)" % t_plan)
    say("    vl.pixcsv_decode      %9.1f ms (%.1f .. %.1f)  (copy into pinned staging, upload, %d launches, status download)"
        % (t_dec + (nchunks,)))
    images, st = holder["res"]
    ok = bool((st[:, 0] == H * W).all() and not st[:, 1].any())
    pick = np.random.default_rng(1).integers(0, a.rows, 64)
    got = images[:, :, 0, torch.from_numpy(pick).to(dev)].permute(2, 0, 1).cpu().numpy()
    ok = ok and np.array_equal(got.reshape(64, -1), vals[pick].astype(np.float32))
    say("    every status (2304, 0) and 64 sampled images equal to the values written: %s" % ok)

    # ---- (b) the host restatement --------------------------------------------------------------------------------------
    rows = plan["rows"]
    raw = data.tobytes()

    def host_path():
        imgs = np.empty((a.rows, H * W), np.float32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            for i, r in enumerate(rows):
                imgs[i] = np.fromstring(raw[r[0]:r[1]], dtype=np.float32, sep=" ")
        t = np.ascontiguousarray(imgs.reshape(a.rows, H, W).transpose(0, 2, 1))        # N x W x H: the device layout
        return torch.from_numpy(t).to(dev)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = host_path()
    torch.cuda.synchronize()
    t_host = (time.perf_counter() - t0) * 1e3
    say("(b) host restatement, np.fromstring per row + transpose + one upload, once: %9.1f ms = %.1f x the whole device path"
        % (t_host, t_host / t_all[0]))
    say("    equal to the device result bit for bit: %s"
        % bool(torch.equal(ref.view(-1).view(torch.int32), out.view(torch.int32))))
    del ref

    # ---- (c) the kernel alone ---------------------------------------------------------------------------------------------
    up = (nbytes + 15) & ~15
    staged = torch.zeros(up + 8 * vl.PIX_DESC * a.rows, dtype=torch.uint8, device=dev)
    staged[:nbytes].copy_(torch.from_numpy(data))
    staged[up:].copy_(torch.from_numpy(rows.view(np.uint8).reshape(-1)))
    status = torch.empty((a.rows, 2), dtype=torch.int32, device=dev)
    p = staged.data_ptr()
    kern = lambda: _lib.check(L.xm_pixcsv_decode_batch(C.c_void_p(p), nbytes, C.c_void_p(p + up), a.rows, H, W, 1,   # noqa: E731
                                                       C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(status.data_ptr()),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    src = staged[:nbytes]
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)                                                        # noqa: E731
    say("(c) pixcsv_decode_kernel on the whole file in one launch (%d blocks), device events, median of %d (min .. max),"
        " alternating with a device-to-device copy of the same %.1f MB" % (a.rows, a.reps, nbytes / 1e6))
    for rep in range(3):
        k = median_ms(kern, a.reps)
        c = median_ms(copy, a.reps)
        say("    kernel %8.3f ms (%.3f .. %.3f) = %7.1f GB/s of text read, %7.1f GB/s read + written | copy %8.3f ms (%.3f .. %.3f)"
            " = %7.1f GB/s read + written | kernel time / copy time %.2f"
            % (k + (nbytes / k[0] / 1e6, (nbytes + nout) / k[0] / 1e6) + c + (2 * nbytes / c[0] / 1e6, k[0] / c[0])))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
