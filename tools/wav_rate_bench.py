#!/usr/bin/env python
"""Timing of vl.audioread(fs=16000) (xm_wav_plan_fs / xm_wav_decode_resample_batch): 256 PCM16 files of 4 - 12 s in one
call, (1) at 44.1 kHz stereo read by channel 0 and (2) at 48 kHz mono.
usage: python tools/wav_rate_bench.py [--files 256] [--reps 5] [--out profiles/wav/wav_rate_bench.txt]
Prints, and writes verbatim to --out, per set
 (a) the whole call, host clock to a device synchronise, medians of --reps runs with both arms alternating in the same
     process: the fused vl.audioread(files, channel=0, fs=16000) against what there was before -- vl.audioread at the
     file's own rate (one launch for the batch) followed by batch.resample per file (a float64 filter design on the host,
     its upload and one xm_resample launch each) --, and the floats of the native-rate bank the second arm needs;
 (b) the two kernels (the library's profiler hook) and the data kernel back to back, next to a device-to-device copy of
     the output bytes timed in the same loop (the floor of anything that writes the bank), with the taps per second;
 (c) the largest difference between the two arms over max|x| (the per-file arm rounds its filter to float32)."""
import argparse
import ctypes as C
import os
import statistics
import struct
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcncrossmodalemotions_amd import _lib, batch as xbatch, prof, vl  # noqa: E402

FS = 16000


def wav_file(frames, nch, rate, rng):
    body = rng.integers(-20000, 20000, frames * nch).astype("<i2").tobytes()
    align = 2 * nch
    head = struct.pack("<HHIIHH", 1, nch, rate, rate * align, align, 16)
    riff = b"WAVE" + b"fmt " + struct.pack("<I", 16) + head + b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", len(riff)) + riff


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wav", "wav_rate_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wav_rate_bench: no GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    L = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    for name, rate, nch in (("44.1 kHz stereo, channel 0", 44100, 2), ("48 kHz mono", 48000, 1)):
        frames = rng.integers(4 * rate, 12 * rate, a.files)
        files = [wav_file(int(n), nch, rate, rng) for n in frames]
        g = np.gcd(FS, rate)
        p, q = FS // g, rate // g
        nout = int(sum(-(-int(n) * p // q) for n in frames))
        taps = 2 * 10 * max(p, q) // p + 1
        say("%d PCM16 files of 4 - 12 s at %s: %.1f MB of files, %.1f MB of float32 at the file's rate (one channel), %.1f MB at 16 kHz;"
            " p / q = %d / %d, %d taps per output" % (a.files, name, sum(map(len, files)) / 1e6, 4 * int(frames.sum()) / 1e6, 4 * nout / 1e6,
                                                     p, q, taps))

        fused = lambda: vl.audioread(files, channel=0, fs=FS)                                   # noqa: E731

        def per_file():
            bank, offs = vl.audioread(files, channel=0)
            return [xbatch.resample(bank[int(offs[k]):int(offs[k + 1])], FS, rate) for k in range(len(files))]

        fused(), per_file()                                                                     # warm both arms
        t_f, t_p = [], []
        for _ in range(a.reps):
            t_f.append(host_clock(fused))
            t_p.append(host_clock(per_file))
        mf, mp = statistics.median(t_f), statistics.median(t_p)
        say("(a) whole call, median of %d alternating runs: fused vl.audioread(fs=16000) %9.3f ms (min %9.3f) | audioread + batch.resample per"
            " file %9.3f ms (min %9.3f) | %.1f x" % (a.reps, mf, min(t_f), mp, min(t_p), mp / mf))

        # ---- (b) the kernels alone: staged bytes already on the device ---------------------------------------------
        buf, plan = vl.wav_plan(files, channel=0, fs=FS)
        d = torch.from_numpy(buf).to(dev)
        out = torch.empty(plan["floats"], dtype=torch.float32, device=dev)
        ptr = d.data_ptr()
        call = lambda: _lib.check(L.xm_wav_decode_resample_batch(C.c_void_p(ptr), plan["nbytes"], C.c_void_p(ptr + plan["desc"][0]),   # noqa: E731
                                                                  plan["N"], C.c_void_p(out.data_ptr()), out.numel(),
                                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        src = torch.empty(4 * nout, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for rep in range(3):
            with prof.recording(L):
                for _ in range(a.reps):
                    call()
            k = {r.name: r.ms / max(r.launches, 1) for r in prof.collect(L)}
            t = device_ms(call, a.reps)
            c = device_ms(lambda: dst.copy_(src), a.reps)
            say("(b) wav_rate_gain_kernel %7.4f ms, wav_resample_kernel %8.4f ms (profiler hook); both back to back %8.4f ms = %6.1f G taps/s"
                " | copy of the %.1f MB written %7.4f ms | data kernel / copy %.1f" %
                (k["wav_rate_gain_kernel"], k["wav_resample_kernel"], t, nout * taps / t / 1e6, 4 * nout / 1e6, c, k["wav_resample_kernel"] / c))

        # ---- (c) the two arms against each other ---------------------------------------------------------------------
        got, offs = fused()
        ref = torch.cat(per_file())
        say("(c) fused against the per-file arm: %d floats each, max |difference| / max |x| = %.2e" %
            (got.numel(), float((got - ref).abs().max() / ref.abs().max())))
        del d, out, src, dst, got, ref
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
