"""student_stats / teacher_stats mirror (emoVoxCeleb/student_stats.m, emoVoxCeleb/teacher_stats.m).

    student_stats('partition', 'all', 'student', 'emovoxceleb-student', 'ignore', {'fear', 'contempt', 'disgust'})
    teacher_stats('figurePath', ...)

student_stats answers "does the voice student agree with the face teacher?": one ROC curve and one AUC per emotion and
per partition of EmoVoxCeleb, the label of a track being the teacher's dominant emotion max(max(wavLogits{i}, [], 1))
(:97) and the score the student's softmax output (:95).  Same option names, defaults and flow as the reference: student
logits from the feature cache or compute_audio_feats (:52-64), partitions train / unheardVal / heardVal = imdb set
1 / 2 / 3 (:79-87), vl_roc per emotion (:109-115), the '%s: %g' printout and meanAuc over the represented emotions
that are not ignored (:127-145), and the cache file emovoxceleb-student-stats.mat that receives a partition's AUC row
only when it does not hold one yet (:134-149).  The arithmetic runs on the device: softmax (xm_nnsoftmaxt), the
teacher labels of all tracks in one xm_aggregate_logits launch, every partition x emotion ranking problem in ONE
xm_roc call, the histograms through xm_label_hist.  teacher_stats is the histogram of the
teacher's dominant emotion over all face frames of EmoVoxCeleb next to that of a second logit list (:28-43,57-58).

What differs, because there is neither MATLAB, vlfeat nor the dataset here:
  * the data is a batch.SyntheticEmoVoxImdb (keyword-only `imdb`; heard_fraction > 0 gives it the third set) -- the
    reference loads fetch_emovoxceleb_imdb(teacher); `root` stands for vl_rootnn, `net` for emoVoxZoo(student);
  * the feature cache <root>/mcnCrossModalEmotions/cachedFeats-audio/<student>-emovoxceleb-feats.mat is written with
    scipy.io.savemat through emo_benchmarks.save_feats (tracks, faceLogits) plus the cell `wavLogits` that :97 reads
    from it and `set`; `refresh` recomputes it (upstream the option is parsed and never read);
  * student features come from imdb.device_wav -> batch.runSpec -> external.compute_audio_feats (batch_by_bucket):
    whole clips, as compute_audio_feats.m does; the files themselves are read by a batch.WavFileEmoVoxImdb passed as
    `imdb` (vl.audioread);
  * vl_roc is vlfeat's [EXT]: restated from its documentation, AUC = S / (p n) with S an exact
    integer; the reference's -1 labels for every other class are kept, no label is 0 here;
  * figures are data, not .jpg: figDir/<emotion>-<partition>.json holds auc, p, n, retrieved and the curve thinned to
    at most CURVE_POINTS points plus both end points, for the emotions not in `ignore` (:121); visHist writes the two
    histograms to figDir/hist-student.json and figDir/hist-teacher-<partition>.json (:67-71,99-102); no plotting;
  * an unknown partition raises ValueError (a containers.Map key error upstream);
  * meanAuc of an empty selection is NaN, as mean([]) is;
  * the cache keeps MATLAB's semantics, including that a second run leaves an existing partition's row untouched;
  * teacher_stats: the AFEW logits are a download upstream (:32-41); here `afew` is a list of F_i x 8 arrays (default a
    seeded synthetic stand-in, or the faceLogits of the .mat file `afewLogits` when it exists), and the figure is
    written as JSON next to figurePath (<figurePath minus extension>.json).
Extensions are keyword-only.
"""
import json
import os

import numpy as np
import torch

from . import batch as xbatch
from . import emo_benchmarks as eb
from . import external, vl, zoo

PARTITIONS = {"train": 1, "unheardVal": 2, "heardVal": 3}            # student_stats.m:79-81
EMOTIONS = list(zoo.EMOTIONS)                                         # net.meta.classes.name, :106-107
FERPLUS_EMOTIONS = ["Neutral", "Happiness", "Surprise", "Sadness", "Anger", "Disgust", "Fear", "Contempt"]   # teacher_stats.m:50-51
CURVE_POINTS = 256
CACHE_NAME = "emovoxceleb-student-stats.mat"


def partition_list(partition):
    """:83-87: one partition or, for 'all', the three keys in order."""
    if partition == "all":
        return list(PARTITIONS)
    if partition not in PARTITIONS:
        raise ValueError("unknown partition %s (one of %s or 'all')" % (partition, ", ".join(PARTITIONS)))
    return [partition]


def mean_auc(auc, teacherMaxLogits, emotions, ignore):
    """:141-144: representedEmotions = unique(labels) minus the ignored ones (1-based), meanAuc over them."""
    represented = np.unique(np.asarray(teacherMaxLogits, dtype=np.int64))
    drop = [i + 1 for i, e in enumerate(emotions) if e in set(ignore)]
    represented = represented[~np.isin(represented, drop)]
    auc = np.asarray(auc, dtype=np.float64).reshape(-1)
    return (float(auc[represented - 1].mean()) if represented.size else float("nan")), represented


def update_cache(cachePath, emotions, partition, auc):
    """:131-149: create the cache with `emotions` or load it; add the partition's 1 x E row unless it has one; save."""
    from scipy.io import loadmat, savemat
    os.makedirs(os.path.dirname(cachePath) or ".", exist_ok=True)
    if not os.path.exists(cachePath):
        cache = {"emotions": np.array(list(emotions), dtype=object).reshape(1, -1)}
    else:
        cache = {k: v for k, v in loadmat(cachePath).items() if not k.startswith("__")}
    if partition not in cache:
        cache[partition] = np.asarray(auc, dtype=np.float64).reshape(1, -1)
    savemat(cachePath, cache)
    return cache


def thin_curve(retrieved, max_points=CURVE_POINTS):
    """indices into the retrieved + 1 curve points: both end points and at most max_points evenly spaced ones between,
    strictly increasing."""
    npts = int(retrieved) + 1
    if npts <= max_points + 2:
        return np.arange(npts)
    return np.unique(np.concatenate([[0], np.round(np.linspace(0, npts - 1, max_points + 2)).astype(np.int64),
                                     [npts - 1]]))


def curve_points(tp, p, n, retrieved, max_points=CURVE_POINTS):
    """tp: positives among the first i + 1 ranked rows -> thinned (tpr, tnr) of vl_roc (fp = rank - tp)."""
    tp = np.concatenate([[0], np.asarray(tp[:int(retrieved)], dtype=np.float64)])
    idx = thin_curve(retrieved, max_points)
    tpr = tp[idx] / max(p, 1e-10)
    fpr = (idx - tp[idx]) / max(n, 1e-10)
    return idx, tpr, 1.0 - fpr


def save_student_feats(path, imdb, logits):
    """the struct compute_audio_feats saves for EmoVoxCeleb: tracks, faceLogits (the student's rows, :62-64) and the
    teacher's wavLogits."""
    from scipy.io import loadmat, savemat
    N = len(imdb.wavLogits)
    tracks = {"set": np.asarray(imdb.set), "labels": np.zeros(N, int), "id": np.arange(1, N + 1)}
    eb.save_feats(path, tracks, [logits[i:i + 1] for i in range(N)])
    m = {k: v for k, v in loadmat(path).items() if not k.startswith("__")}
    cell = np.empty((1, N), dtype=object)
    for i, l in enumerate(imdb.wavLogits):
        cell[0, i] = np.asarray(l, dtype=np.float32)
    m["wavLogits"] = cell
    savemat(path, m)


def load_student_feats(path):
    """-> (set, studentLogits N x E float32, list of F_i x E float32 teacher logits)."""
    from scipy.io import loadmat
    tracks, faceLogits = eb.load_feats(path)
    wav = [np.asarray(c, dtype=np.float32) for c in loadmat(path)["wavLogits"].reshape(-1)]
    return tracks["set"], np.concatenate(faceLogits, 0), wav


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("student_stats needs a GPU; this build has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _write_json(path, obj):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1)
    return path


def _hist_json(path, title, counts, emotions):
    return _write_json(path, {"title": title, "emotions": list(emotions), "counts": [int(v) for v in counts]})


def student_stats(refresh=False, visHist=False, partition="all", student="emovoxceleb-student",
                  teacher="senet50-ferplus", ignore=("fear", "contempt", "disgust"), figDir="data/emovoxceleb-figs",
                  cachePath=None, expRoot=None, *, imdb=None, net=None, root="data", verbose=True, wavBatch=False,
                  modelDir=None):
    """Options as in student_stats.m:39-50 (cachePath defaults to <root>/mcnCrossModalEmotions/cache/
    emovoxceleb-student-stats.mat, expRoot to <root>/xEmo18; expRoot is parsed and unused, as upstream).
    Returns {partition: {'auc' (E doubles), 'meanAuc', 'represented' (1-based), 'counts' {'p', 'n', 'retrieved'},
    'status', 'emotions', 'figPaths', 'histPaths', 'cachePath', 'featPath'}}.
    Extensions (keyword-only): `imdb` (default a three-set SyntheticEmoVoxImdb), `net` (default
    zoo.emoVoxZoo(student)), `root` (vl_rootnn), `verbose` (the reference's printout), `wavBatch` (the features come from
    external.compute_audio_feats_wav on imdb.device_wav_bank -- one xm_spec_bucket_batch call per bucket -- instead of
    the per-clip runSpec loop; off by default), `modelDir` (without `net`: the student of <modelDir>/<student>.mat)."""
    partitions = partition_list(partition)
    cachePath = cachePath or os.path.join(root, "mcnCrossModalEmotions", "cache", CACHE_NAME)
    expRoot = expRoot or os.path.join(root, "xEmo18")
    device = _device()
    featPath = eb.cached_feats_path(root, "audio", student, "emovoxceleb")               # :52-55
    if refresh or not os.path.exists(featPath):                                          # :56-58
        if imdb is None:
            imdb = xbatch.SyntheticEmoVoxImdb(num_tracks=96, val_fraction=0.25, heard_fraction=0.125)
        dag = net if net is not None else zoo.inference_student(student, modelDir)
        if wavBatch:
            wav, offsets = imdb.device_wav_bank(device)
            logits = external.compute_audio_feats_wav(dag, wav, offsets, numEmotions=len(EMOTIONS))
        else:
            specs = [xbatch.runSpec(imdb.device_wav(i, device))[:, :, 0, 0] for i in range(len(imdb.wavLogits))]
            logits = external.compute_audio_feats(dag, specs, numEmotions=len(EMOTIONS), batch_by_bucket=True)
        save_student_feats(featPath, imdb, logits)
    elif verbose:
        print("found features at %s... skipping" % featPath, flush=True)
    sets, studentLogits, wavLogits = load_student_feats(featPath)                        # :60-64
    emotions = list(net.meta.get("classes", {}).get("name", EMOTIONS)) if net is not None else list(EMOTIONS)
    emotions = [e.lower() for e in emotions][:studentLogits.shape[1]]
    E = len(emotions)

    dlogits = vl.from_numpy(np.asfortranarray(studentLogits), device)                    # N x E
    histPaths = {}
    if visHist:                                                                          # :65-71
        h = vl.label_hist(dlogits).cpu().numpy()
        histPaths["student"] = _hist_json(os.path.join(figDir, "hist-student.json"),
                                          "histogram of dominant emotions (predicted by student)", h, emotions)
    normedLogits = vl.vl_nnsoftmaxt(dlogits, dim=2)                                      # :95
    # teacher label per track = the column of max(max(y, [], 1)) (:97): aggregate_logits' maxLabel, one launch
    counts = np.array([l.shape[0] for l in wavLogits])
    last = np.cumsum(counts).astype(np.int32)
    first = (last - counts + 1).astype(np.int32)
    cat = np.asfortranarray(np.concatenate(wavLogits, 0)[:, :E])
    logitTarget, maxLabel = vl.aggregate_logits(vl.from_numpy(cat, device), torch.from_numpy(first).to(device),
                                      torch.from_numpy(last).to(device), "max")
    dcls = maxLabel.reshape(-1).to(torch.int32)
    aggregated = vl.to_numpy(logitTarget).reshape(E, -1, order="F")
    keepSets = [np.nonzero(sets == PARTITIONS[p])[0] + 1 for p in partitions]            # :94
    # every partition x emotion problem: one call
    r = vl.roc(normedLogits, dcls, keepSets, want_curve=True)
    auc = r["auc"].cpu().numpy()
    cnt = {k: r[k].cpu().numpy() for k in ("p", "n", "retrieved")}
    status = r["status"].cpu().numpy()
    tp = r["tp"].cpu().numpy()
    teacherMax = dcls.cpu().numpy()
    offs = r["offsets"]

    out = {}
    for ii, part in enumerate(partitions):
        if verbose:
            print("compute stats for %s (%d/%d)..." % (part, ii + 1, len(partitions)), flush=True)
        teacherMaxLogits = teacherMax[keepSets[ii] - 1]
        if visHist:                                                                      # :99-102
            kept = np.asfortranarray(aggregated[:, keepSets[ii] - 1].reshape(1, 1, E, -1))
            hist = vl.label_hist(vl.from_numpy(kept, device), dim=3).cpu().numpy()
            histPaths[part] = _hist_json(os.path.join(figDir, "hist-teacher-%s.json" % part),
                                         "dominant emotion of the teacher (%s)" % part, hist, emotions)
        figPaths = {}
        for jj, emo in enumerate(emotions):                                              # :109-125
            if emo in ignore:
                continue
            p, n, ret = (int(cnt[k][ii, jj]) for k in ("p", "n", "retrieved"))
            idx, tpr, tnr = curve_points(tp[jj, int(offs[ii]):int(offs[ii + 1])], p, n, ret)
            figPaths[emo] = _write_json(os.path.join(figDir, "%s-%s.json" % (emo, part)), {
                "title": "%s (%s)" % (emo, part), "auc": None if np.isnan(auc[ii, jj]) else float(auc[ii, jj]),
                "p": p, "n": n, "retrieved": ret, "rank": idx.tolist(), "tpr": tpr.tolist(), "tnr": tnr.tolist()})
        if verbose:
            for jj, emo in enumerate(emotions):                                          # :127-129
                print("%s: %g" % (emo, auc[ii, jj]))
        update_cache(cachePath, emotions, part, auc[ii])                                 # :131-149
        meanAuc, represented = mean_auc(auc[ii], teacherMaxLogits, emotions, ignore)     # :141-145
        if verbose:
            print("meanAuc: %g" % meanAuc, flush=True)
        out[part] = {"auc": auc[ii].copy(), "meanAuc": meanAuc, "represented": represented,
                     "counts": {k: cnt[k][ii].copy() for k in cnt}, "status": status[ii].copy(), "emotions": emotions,
                     "figPaths": figPaths, "histPaths": dict(histPaths), "cachePath": cachePath, "featPath": featPath}
    return out


def synthetic_afew_logits(num_tracks=40, seed=1, num_emotions=8):
    """stand-in for afew-logits.mat (teacher_stats.m:32-41): a list of F_i x 8 single arrays."""
    rng = np.random.default_rng(seed)
    return [np.asfortranarray(rng.standard_normal((int(f), num_emotions)).astype(np.float32) * 3)
            for f in rng.integers(4, 40, num_tracks)]


def teacher_stats(figurePath="data/emoVoxCeleb/emovoxceleb-figure.pdf", afewLogits="data/emoVoxCeleb/afew-logits.mat",
                  *, imdb=None, afew=None, verbose=True):
    """Options as in teacher_stats.m:20-23.  Returns {'emoCeleb', 'compared' (8 int64 counts each, histcounts(preds,
    0.5:8.5), :57-58), 'emotions', 'labels', 'path'}.  Extensions (keyword-only): `imdb` (default a SyntheticEmoVoxImdb),
    `afew` (a list of F_i x 8 logit arrays; default the faceLogits of `afewLogits` when that file exists, else a seeded
    synthetic list), `verbose`."""
    device = _device()
    if imdb is None:
        imdb = xbatch.SyntheticEmoVoxImdb(num_tracks=96)
    if afew is None:
        if os.path.exists(afewLogits):
            from scipy.io import loadmat
            afew = [np.asarray(c, dtype=np.float32) for c in loadmat(afewLogits)["faceLogits"].reshape(-1)]
        else:
            afew = synthetic_afew_logits()
    hists = []
    for logits in (imdb.wavLogits, afew):                                                # :28-29, :40-41
        allLogits = np.asfortranarray(np.concatenate([np.asarray(l, np.float32) for l in logits], 0))
        hists.append(vl.label_hist(vl.from_numpy(allLogits, device)).cpu().numpy())
    E = len(hists[0])
    path = os.path.splitext(figurePath)[0] + ".json"
    _write_json(path, {"emotions": FERPLUS_EMOTIONS[:E], "labels": ["EmoVoxCeleb", "Afew 6.0"],
                       "ylabel": "Number of frames", "emoCeleb": [int(v) for v in hists[0]],
                       "compared": [int(v) for v in hists[1]]})
    if verbose:
        for name, h in zip(("EmoVoxCeleb", "Afew 6.0"), hists):
            print("%s: %s" % (name, " ".join(str(int(v)) for v in h)), flush=True)
    return {"emoCeleb": hists[0], "compared": hists[1], "emotions": FERPLUS_EMOTIONS[:E],
            "labels": ["EmoVoxCeleb", "Afew 6.0"], "path": path}
