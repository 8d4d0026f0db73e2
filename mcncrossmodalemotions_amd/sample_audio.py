"""sample_audio mirror (emoVoxCeleb/sample_audio.m): audio samples per emotion with their peak frames.

    sample_audio('teacher', 'senet50-ferplus', 'ignore', {'disgust', 'contempt', 'fear'})

Same options and flow as sample_audio.m:35-199: the imdb of fetch_emovoxceleb_imdb(teacher), per track the position and
emotion of its largest logit and the per-emotion maxima (:69-74; all tracks in ONE xm_track_peaks launch), per emotion
not in `ignore` the tracks tagged with it (:86), min(numel, 20) of them drawn (:89), and per sample the folder
<dest>/<emotion>/<jj>/ (:103-198).

What differs, because there are neither media nor MATLAB here:
  * MATLAB's rng(0) / randsample stream (:80,89) cannot be reproduced: the picks are the first min(numel, 20) entries of
    numpy.random.default_rng(0).permutation(numel), one generator for the whole run as upstream;
  * files are recorded, not copied: manifest.json holds, for the wav, the avi, the peak frame (samplePeaks) and the
    sorted frame list (sampleFrameSeq), the source path and the destination name the reference copies to (:123-135,
    :167-196);
  * distribution.json stands for distribution.png (:137-164): the eight values, the eight colours, the tick stubs and
    ylim = [min(-3, min(dist)), max(10, max(dist))];
  * there is no prompt (:202-221): an existing destination without `clobber` returns None before anything is sampled,
    as the answer 'n' does; `clobber` removes <dest> and nothing else;
  * `dest` (keyword-only) replaces vl_rootnn/data/mcnCrossModalEmotions/samples/<teacher>; `imdb` passes a built imdb.
meta.txt is byte for byte what the reference's fprintf calls write (:118-120), see format_meta.
"""
import json
import os
import shutil

import numpy as np
import torch

from . import vl, zoo

EMOTIONS = list(zoo.EMOTIONS)                                                            # :62-63
COLORS = [[202, 202, 202], [250, 190, 190], [230, 190, 255], [88, 112, 209], [230, 88, 88], [32, 162, 102],
          [0, 128, 128], [0, 0, 0]]                                                      # :51-60
SAMPLES_PER_EMO = 20                                                                     # :75


def _num(v):
    """MATLAB's %.4f of a non-finite value"""
    v = float(v)
    if np.isnan(v):
        return "NaN"
    if np.isinf(v):
        return "Inf" if v > 0 else "-Inf"
    return "%.4f" % v


def format_meta(aviPath, logits):
    """fprintf(fid, 'aviPath: %s\\n', p) ; fprintf(fid, [repmat('%.4f ', 1, 7) '\\n'], logits) (:118-120).  MATLAB
    recycles a template over the data and stops before the first conversion that is left without data: eight logits
    give seven values and a newline, then the eighth value and one space."""
    vals = list(np.asarray(logits, dtype=np.float64).reshape(-1))
    s = "aviPath: %s\n" % aviPath
    for i, v in enumerate(vals):
        s += _num(v) + " "
        if i % 7 == 6:
            s += "\n"
    return s


def track_peaks(imdb, device=None):
    """[frameIdx, tags] and maxedLogits of :69-74 for every track: host arrays (int, int, T x E float32)"""
    device = device or torch.device("cuda", torch.cuda.current_device())
    logits, offs = imdb.device_logits(device)
    offsets = torch.from_numpy(np.asarray(offs, dtype=np.int32)).to(device)
    frameIdx, tags, maxed = vl.track_peaks(logits, offsets)
    E = int(logits.shape[1])
    return (frameIdx.cpu().numpy().astype(int), tags.cpu().numpy().astype(int),
            vl.to_numpy(maxed).reshape(E, -1, order="F").T.copy())


def sample_audio(vis=False, clobber=False, samplePeaks=True, sampleFrameSeq=False,
                 ignore=("disgust", "contempt", "fear"), teacher="senet50-ferplus",
                 wavDir="data/datasets/voxceleb1/voxceleb_all", aviDir="/datasets/voxceleb1/avi",
                 faceDir="data/datasets/voxceleb1/unzippedIntervalFaces", *, imdb=None, dest=None, root="data",
                 verbose=True):
    """Options as in sample_audio.m:35-45 (`vis` is parsed and unused: nothing is drawn).  Returns None when the
    destination exists and `clobber` is off, else {'dest', 'frameIdx', 'tags', 'maxedLogits', 'samples': {emotion:
    [{'track' (0-based), 'id', 'dir', 'wav', 'peakFrame', 'frames'}]}}."""
    dest = dest or os.path.join(root, "mcnCrossModalEmotions", "samples", teacher)       # :47-48
    emotionIdx = [i + 1 for i, e in enumerate(EMOTIONS) if e not in set(ignore)]         # :64-65
    # confirmSamplingProcess (:81,202-221) comes first here: the answer 'n' needs neither the imdb nor the device
    if os.path.isdir(dest) and not clobber:
        if verbose:
            print("destination directory at %s already exists\nexiting sampler" % dest, flush=True)
        return None
    if not torch.cuda.is_available():
        raise RuntimeError("sample_audio needs a GPU; this build has no CPU path")
    if imdb is None:
        from .fetch_emovoxceleb_imdb import fetch_emovoxceleb_imdb
        imdb = fetch_emovoxceleb_imdb(teacher)                                           # :66
    frameIdx, tags, maxedLogits = track_peaks(imdb)                                      # :69-74
    rng = np.random.default_rng(0)                                                       # rng(0), :80
    if os.path.isdir(dest):                                                              # clobber: rm -rf <dest> (:205-207)
        shutil.rmtree(dest)
    images = imdb.images
    wavIds = np.asarray(images["denseFramesWavIds"])
    out = {"dest": dest, "frameIdx": frameIdx, "tags": tags, "maxedLogits": maxedLogits, "samples": {}}
    stubs = [e[0].upper() + e[1:3].lower() for e in EMOTIONS]                            # :146
    for emoIdx in emotionIdx:                                                            # :84-100
        emo = EMOTIONS[emoIdx - 1]
        tagged = np.nonzero(tags == emoIdx)[0]
        num = min(tagged.size, SAMPLES_PER_EMO)
        if verbose:
            print("found %d audio segments for %s, picking %d" % (tagged.size, emo, SAMPLES_PER_EMO), flush=True)
        samples = tagged[rng.permutation(tagged.size)[:num]]                             # randsample, :89-90
        recs = []
        for jj, ti in enumerate(samples, 1):                                             # :103-197
            sub = os.path.join(dest, emo, str(jj))
            os.makedirs(sub, exist_ok=True)
            wavPath = images["name"][ti]
            origAviPath = os.path.splitext(wavPath)[0] + ".avi"                          # :111-114
            dist = maxedLogits[ti]
            with open(os.path.join(sub, "meta.txt"), "w", newline="") as f:              # :115-121
                f.write(format_meta(origAviPath, dist))
            allFrames = [p for p, w in zip(images["denseFrames"], wavIds) if w == images["id"][ti]]   # :93-95
            rec = {"track": int(ti), "id": int(images["id"][ti]), "dir": sub,
                   "wav": {"src": os.path.join(wavDir, wavPath), "dest": wavPath.replace("/", "-")},            # :123-129
                   "avi": {"src": os.path.join(aviDir, origAviPath), "dest": origAviPath.replace("/", "-")},    # :131-135
                   "peakFrame": None, "frames": None}
            lo, hi = float(np.min(dist)), float(np.max(dist))
            with open(os.path.join(sub, "distribution.json"), "w") as f:                 # :137-164
                json.dump({"values": [float(v) for v in dist], "colors": COLORS, "xticklabels": stubs,
                           "xlim": [0.5, 8.5], "ylim": [min(-3.0, lo), max(10.0, hi)]}, f, indent=1)
            if samplePeaks:                                                              # :96-97, :167-178
                rec["peakFrame"] = {"src": os.path.join(faceDir, allFrames[frameIdx[ti] - 1]),
                                    "path": allFrames[frameIdx[ti] - 1], "dest": "peakFrame.jpg"}
            if sampleFrameSeq:                                                           # :180-196
                rec["frames"] = [{"src": os.path.join(faceDir, p), "dest": os.path.join("frames", "%05d.jpg" % kk)}
                                 for kk, p in enumerate(sorted(allFrames), 1)]
            with open(os.path.join(sub, "manifest.json"), "w") as f:
                json.dump({k: v for k, v in rec.items() if k != "dir"}, f, indent=1)
            recs.append(rec)
        out["samples"][emo] = recs
    return out
