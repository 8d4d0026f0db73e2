#!/usr/bin/env python
"""Timing of the imdb build of emoVoxCeleb/fetch_emovoxceleb_imdb.m and of the peak search of sample_audio.m on the device.
usage: python tools/imdb_bench.py [--teacher senet50-ferplus] [--batches 12] [--reps 10] [--frame 256] [--skip-loop]
Prints (1) frames/s of buildImdb's loop at batch 128 (decoded frames -> crop_resize_face -> FrozenTeacher.logits ->
xm_scatter_rows, nothing synchronised inside) next to FrozenTeacher.logits alone on prepared faces in the same process,
with the decoded frames taken from a prepared device tensor and from batch.SyntheticDenseFrames (which hashes every pixel
on the device per batch); (2) the device time of xm_group_rows, of the regrouping (xm_gather_rows + xm_scatter_rows) and
of xm_track_peaks at 5,078,961 rows and 153,486 tracks, against the bytes each must move at least, next to 6.3 TB/s."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe, vl, zoo  # noqa: E402

FRAMES, TRACKS, E = 5078961, 153486, 8      # fetch_emovoxceleb_imdb.m:223; misc/generateBaseImdb.m:46-56 (all partitions)
HBM = 6.3e12


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


def loop_rate(teacher, imdb, frames, numIms):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fe.buildImdb(teacher, imdb, frames, batchSize=128)      # ends with the download of the logits: the device is idle
    torch.cuda.synchronize()
    return numIms / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--teacher", default="senet50-ferplus")
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frame", type=int, default=256)
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if not a.skip_loop:
        n = 128 * a.batches
        # n frames in tracks of 32: ids are sorted, as addFramesToImdb leaves them
        images = {"name": ["id%05d/v/1.wav" % i for i in range(1, n // 32 + 1)], "id": np.arange(1, n // 32 + 1),
                  "set": np.ones(n // 32, int), "numSamples": np.full(n // 32, 8 * 16000),
                  "denseFrames": ["id%05d/1.6/v/1/%05d.jpg" % (i // 32 + 1, i % 32 + 1) for i in range(n)],
                  "denseFramesWavIds": np.arange(n) // 32 + 1}
        imdb = fe.EmoVoxImdb(images)
        synth = batch.SyntheticDenseFrames(imdb, frameSize=(a.frame, a.frame))
        net = zoo.ferPlusZoo(a.teacher)
        zoo.strip_losses(net)
        net.mode = "test"
        net.move("gpu")
        teacher = zoo.FrozenTeacher(net, lanes=2)
        teacher.imageSize, teacher.averageImage = (224, 224), fe.AVERAGE_IMAGE
        one = synth(images["denseFrames"][:128], dev)
        faces = vl.crop_resize_face(one, fe.AVERAGE_IMAGE, (224, 224))
        for _ in range(a.batches):                                  # the same warm-up the loop lines get
            teacher.logits(faces)
        alone = max(128 / timeit(lambda: teacher.logits(faces), a.batches) for _ in range(3))
        prepared = lambda paths, device: one[..., :len(paths)]     # noqa: E731
        fe.buildImdb(teacher, imdb, prepared, batchSize=128)      # warm-up (workspace growth, first shapes)
        r_prep = max(loop_rate(teacher, imdb, prepared, n) for _ in range(3))
        r_syn = max(loop_rate(teacher, imdb, synth, n) for _ in range(3))
        t_crop = timeit(lambda: vl.crop_resize_face(one, fe.AVERAGE_IMAGE, (224, 224)), a.reps)
        t_syn = timeit(lambda: synth(images["denseFrames"][:128], dev), a.reps)
        print("%s, batch 128, %d frames of %d x %d" % (a.teacher, n, a.frame, a.frame))
        print("  FrozenTeacher.logits alone (prepared faces)      %9.1f img/s" % alone)
        print("  buildImdb loop, prepared decoded frames          %9.1f img/s  (%+.1f %% vs alone)" %
              (r_prep, 100 * (r_prep / alone - 1)))
        print("  buildImdb loop, SyntheticDenseFrames per batch   %9.1f img/s  (%+.1f %% vs alone)" %
              (r_syn, 100 * (r_syn / alone - 1)))
        print("  per batch of 128: crop_resize_face %.3f ms, SyntheticDenseFrames %.3f ms, teacher %.3f ms" %
              (t_crop * 1e3, t_syn * 1e3, 128 / alone * 1e3))
    # ---- grouping, regrouping and peaks at the size of the dataset -----------------------------------------------
    rng = np.random.default_rng(0)
    lens = rng.multinomial(FRAMES - TRACKS, np.full(TRACKS, 1.0 / TRACKS)) + 1
    ids_sorted = np.repeat(np.arange(1, TRACKS + 1), lens).astype(np.int32)
    keys = np.arange(1, TRACKS + 1)
    logits = vl.mat_empty(FRAMES, E, device=dev)
    logits.normal_()
    grouped = vl.mat_empty(FRAMES, E, device=dev)
    print("%d rows x %d, %d tracks" % (FRAMES, E, TRACKS))
    for name, ids in (("sorted ids", ids_sorted), ("shuffled ids", rng.permutation(ids_sorted))):
        d = torch.from_numpy(ids).to(dev)
        t = timeit(lambda: vl.group_rows(d, keys, TRACKS), a.reps)
        # at least: read the ids, write the rows and the offsets; the radix passes move 16 n per pass on top
        least = 4.0 * FRAMES * 2 + 4.0 * TRACKS
        moved = least + 4 * (4 + 16) * FRAMES + 8.0 * FRAMES
        print("  xm_group_rows (%s, with the key upload)  %8.3f ms   least %.0f MB = %.1f %% of HBM rate, passes move %.0f MB = %.1f %%"
              % (name, t * 1e3, least / 1e6, 100 * least / t / HBM, moved / 1e6, 100 * moved / t / HBM))
    off, rows, nnz = vl.group_rows(torch.from_numpy(ids_sorted).to(dev), keys, TRACKS)
    t = timeit(lambda: vl.scatter_rows(vl.gather_rows(logits, rows), grouped), a.reps)
    least = 2.0 * 4 * E * FRAMES + 4.0 * FRAMES
    print("  regroup: xm_gather_rows + xm_scatter_rows          %8.3f ms   least %.0f MB = %.1f %% (the two launches move %.0f MB = %.1f %%)"
          % (t * 1e3, least / 1e6, 100 * least / t / HBM, 2 * least / 1e6, 200 * least / t / HBM))
    t = timeit(lambda: vl.track_peaks(grouped, off), a.reps)
    least = 4.0 * E * FRAMES + 4.0 * (E + 3) * TRACKS
    print("  xm_track_peaks (contiguous tracks)                  %8.3f ms   least %.0f MB = %.1f %%" %
          (t * 1e3, least / 1e6, 100 * least / t / HBM))
    first = (off[:-1] + 1).contiguous()
    last = off[1:].contiguous()
    t2 = timeit(lambda: (vl.aggregate_logits(grouped, first, last, "peak"), vl.aggregate_logits(grouped, first, last, "max")),
                a.reps)
    print("  xm_aggregate_logits peak + max (one thread a track) %8.3f ms" % (t2 * 1e3))
    t = timeit(lambda: vl.track_peaks(logits, off, rows), a.reps)
    print("  xm_track_peaks (through the row list)               %8.3f ms" % (t * 1e3))


if __name__ == "__main__":
    main()
