"""emo_benchmarks mirror (external/run_cross_val.m, external/emo_benchmarks.m): score a model on external benchmarks.

    [miniImdb, expDirs, valIdxSets] = run_cross_val('numFolds', 10, 'aggregator', 'max', 'targetDataset', 'rml', ...)
    emo_benchmarks('modality', 'audio', 'datasets', {'rml', 'enterface'}, 'modelName', 'emovoxceleb-student')

Same option names, defaults and flow as the reference.  run_cross_val seeds the stream at 0 (:55), computes and caches
the model's logits on the target dataset unless the cache file exists (:71-86), aggregates each track's logit rows
('mean1' | 'max' | 'peak', :128-135), cuts numFolds contiguous validation slices out of randperm (:92-108; AFEW: the
existing train / val split) and fits mnrfit per fold (:137-145).  emo_benchmarks scores every fold with mnrval, prints
the fold accuracies, their mean and N-1 std and the summed confusion matrix (:36-126).  The arithmetic runs on the
device: aggregation in one xm_aggregate_logits launch, all folds' fits in one xm_mnrfit launch (fp64 Newton-Raphson),
all folds' scoring in one xm_mnrval launch -- three launches whatever numFolds is.

What differs, because there is neither MATLAB nor benchmark data here:
  * the data is a batch.SyntheticBenchmarkImdb per dataset (keyword-only `imdbs` / `imdb`) -- the RML, eNTERFACE and
    AFEW imdbs are built by functions that are not part of the reference; `root` stands for vl_rootnn;
  * the MATLAB random stream is a numpy Generator seeded with 0, in the reference's draw order (the 'random' model's
    randn(numTracks, numEmotions), column-major, then randperm), as in batch.py;
  * the feature cache <root>/mcnCrossModalEmotions/cachedFeats-<modality>/<modelName>-<dataset>-feats.mat is written
    with scipy.io.savemat and holds `tracks` (set, labels, id) and the cell `faceLogits`;
  * a class absent from a fold's training rows makes mnrfit drop that category and shift the columns; here the fit's
    status flags it and run_cross_val raises with the fold number;
  * separable data: mnrfit warns; here the fit reports the iteration limit, its coefficients stay finite and
    run_cross_val warns with the fold number (also for a Hessian that is not positive definite);
  * an unknown aggregator is rejected before any feature is computed (the reference fails inside the fold loop);
  * the confusion figure is written as JSON and text (figDir/confmat/<dataset>-<modelName>.json / .txt: the normalised
    matrix, the summed counts and the canonical labels), not as a PDF: plotting is out of scope;
  * compute_visual_feats has no 'random' branch upstream (ferPlusZoo('random') fails), so neither has this one.
Parity with MATLAB's mnrfit is unpinned: for non-separable data the maximum-likelihood estimate is unique and only the
stopping rule (statset('mnrfit') as documented: 100 iterations, TolX 1e-6) can move bits, below the tolerance.
Extensions are keyword-only.
"""
import json
import math
import os
import warnings

import numpy as np
import torch

from . import batch as xbatch
from . import external, vl, zoo

MODEL_EMO_LABELS = ["neutral", "happiness", "surprise", "sadness", "anger", "disgust", "fear", "contempt"]   # :46-48
_SIX = ["Angry", "Disgust", "Fear", "Happy", "Sad", "Surprise"]
# dataset -> (datasetLabels, numFolds, useExstingVal, adjustmentFactor), emo_benchmarks.m:57-75
DATASETS = {"rml": (_SIX, 10, False, 1.0), "enterface": (_SIX, 10, False, 1.0),
            "afew": (_SIX + ["Neutral"], 1, True, 381 / 383)}
_CANONICAL = {"Fear": "Fear", "Sad": "Sadness", "Angry": "Anger", "Neutral": "Neutral", "Happy": "Happiness",
              "Disgust": "Disgust", "Surprise": "Surprise"}
AGGREGATORS = {"mean1": "mean", "max": "max", "peak": "peak"}   # run_cross_val.m:128-133 -> vl.aggregate_logits
TARGET_DATASETS = ("rml", "afew", "afew-6", "enterface")


def matlab_round(x):
    """MATLAB round: halves away from zero."""
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def canonicalLabels(labels):
    """emo_benchmarks.m:129-145: dataset label names in the FER2013+ form."""
    return [_CANONICAL[l] for l in labels]


def cross_val_folds(sampleOrder, numFolds):
    """run_cross_val.m:97-107: splits = round(linspace(0, n, K + 1)); fold ii validates on the contiguous slice
    sampleOrder(splits(ii)+1 : splits(ii+1)) and trains on the rest of sampleOrder, in that order.
    Returns (trainIdxSets, valIdxSets) of 1-based index arrays."""
    sampleOrder = np.asarray(sampleOrder)
    splits = [matlab_round(v) for v in np.linspace(0, len(sampleOrder), int(numFolds) + 1)]
    trainIdxSets, valIdxSets = [], []
    for ii in range(int(numFolds)):
        valIdx = sampleOrder[splits[ii]:splits[ii + 1]]
        valIdxSets.append(valIdx)
        trainIdxSets.append(sampleOrder[~np.isin(sampleOrder, valIdx)])
    return trainIdxSets, valIdxSets


def fold_summary(foldAccs):
    """mean(foldAccs) and MATLAB's std (N - 1 normalisation; 0 for a single fold)."""
    a = np.asarray(foldAccs, dtype=np.float64)
    return float(a.mean()), (float(a.std(ddof=1)) if a.size > 1 else 0.0)


def normalise_confusion(confSum):
    """bsxfun(@rdivide, confSum, sum(confSum, 2)): rows sum to 1, a row without samples is 0/0 = NaN."""
    c = np.asarray(confSum, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / c.sum(1, keepdims=True)


def cached_feats_path(root, modality, modelName, targetDataset):
    """run_cross_val.m:71-77."""
    return os.path.join(root, "mcnCrossModalEmotions", "cachedFeats-%s" % modality,
                        "%s-%s-feats.mat" % (modelName, targetDataset))


def save_feats(path, tracks, faceLogits):
    """the imdb struct compute_*_feats save: tracks (set, labels, id) and faceLogits, a cell of F_i x E single."""
    from scipy.io import savemat
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    cell = np.empty((1, len(faceLogits)), dtype=object)
    for i, l in enumerate(faceLogits):
        cell[0, i] = np.asarray(l, dtype=np.float32).reshape(-1, np.shape(l)[-1])
    tr = {k: np.asarray(tracks[k], dtype=np.float64).reshape(1, -1) for k in ("set", "labels", "id")}
    savemat(path, {"tracks": tr, "faceLogits": cell})


def load_feats(path):
    """-> (tracks dict of 1-D arrays, list of F_i x E float32 arrays)."""
    from scipy.io import loadmat
    m = loadmat(path)
    tr = m["tracks"][0, 0]
    tracks = {k: np.asarray(tr[k], dtype=np.float64).reshape(-1).astype(int) for k in ("set", "labels", "id")}
    faceLogits = [np.asarray(c, dtype=np.float32) for c in m["faceLogits"].reshape(-1)]
    return tracks, faceLogits


def _compute_feats(modality, modelName, imdb, net, numSrcEmotions, rng, device, modelDir=None):
    """compute_audio_feats / compute_visual_feats with the file I/O left out: one logit row per track (audio) or
    per face frame (visual)."""
    N = len(imdb.tracks["set"])
    if modality == "audio":
        if modelName == "random":                                # compute_audio_feats.m:95-99
            logits = rng.standard_normal(N * numSrcEmotions).reshape((N, numSrcEmotions), order="F")
            logits = logits.astype(np.float32)
        else:
            dag = net if net is not None else zoo.inference_student(modelName, modelDir)
            specs = [imdb.device_spec(i, device) for i in range(N)]
            logits = external.compute_audio_feats(dag, specs, numEmotions=numSrcEmotions, batch_by_bucket=True)
        return [logits[i:i + 1] for i in range(N)]
    if modelName == "random":
        raise ValueError("compute_visual_feats has no 'random' model")
    dag = net if net is not None else zoo.ferPlusZoo(modelName, modelDir=modelDir)
    frames = [imdb.device_faces(i, device) for i in range(N)]
    return external.compute_visual_feats(dag, frames, numEmotions=numSrcEmotions)


def run_cross_val(numFolds=10, aggregator="max", targetDataset="rml", numTargetEmotions=6, numSrcEmotions=8,
                  labelType="labels", useExstingVal=False, modality="visual", modelName="emovoxceleb-student", *,
                  imdb=None, net=None, root="data", maxIter=100, tolX=1e-6, verbose=False, modelDir=None):
    """Options as in run_cross_val.m:44-52.  Returns (miniImdb, expDirs, valIdxSets): miniImdb = {'labels',
    'fusedLogits' (N x numSrcEmotions single), 'images': {'set'}}, one experiment directory per fold holding
    mnr-params.mat (`coefficients`, (numSrcEmotions + 1) x (numTargetEmotions - 1) double), 1-based validation indices.
    Extensions (keyword-only): `imdb` (default a SyntheticBenchmarkImdb of numTargetEmotions classes), `net` (the
    network to extract features with, default zoo.emoVoxZoo / zoo.ferPlusZoo(modelName); 'random' builds none),
    `root` (vl_rootnn), `maxIter` / `tolX` (statset('mnrfit')), `verbose`, `modelDir` (the zoo reads the model file from
    there when no `net` is passed)."""
    rng = np.random.default_rng(0)                                                       # rng(0), :55
    if targetDataset not in TARGET_DATASETS:
        raise ValueError("unknown dataset %s" % targetDataset)
    if modality not in ("visual", "audio"):
        raise ValueError("unknown modality %s" % modality)
    if aggregator not in AGGREGATORS:
        raise ValueError("aggregator: %s unrecognised" % aggregator)
    if useExstingVal and numFolds != 1:
        raise AssertionError("when using an existing val set, only one fold should be specified")
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    imdbPath = cached_feats_path(root, modality, modelName, targetDataset)
    if not os.path.exists(imdbPath):                                                     # :80-86
        if imdb is None:
            imdb = xbatch.SyntheticBenchmarkImdb(num_classes=numTargetEmotions, modality=modality,
                                                 val_fraction=0.5 if useExstingVal else 0.0)
        if device is None and modelName != "random":
            raise RuntimeError("computing features needs a GPU; this build has no CPU path")
        feats = _compute_feats(modality, modelName, imdb, net, numSrcEmotions, rng, device, modelDir)
        save_feats(imdbPath, imdb.tracks, feats)
    elif verbose:
        print("found features at %s... skipping" % imdbPath, flush=True)
    tracks, faceLogits = load_feats(imdbPath)                                            # :88-90
    sets = tracks["set"]
    if useExstingVal:                                                                    # :92-96
        trainIdxSets = [np.nonzero(sets == 1)[0] + 1]
        valIdxSets = [np.nonzero(sets == 2)[0] + 1]
    else:
        sampleOrder = rng.permutation(len(sets)) + 1                                     # randperm, :98
        trainIdxSets, valIdxSets = cross_val_folds(sampleOrder, numFolds)
    expRoot = os.path.join(root, "%s-%s" % (targetDataset, modality))
    expDirs = [os.path.join(expRoot, "%s-%s-foldNum-%d" % (modelName, aggregator, f + 1)) for f in range(numFolds)]
    if device is None:
        raise RuntimeError("run_cross_val needs a GPU; this build has no CPU path")

    # aggregation: every track's F_i x E block in one launch (fusedLogits = 1 x 1 x E x N on the device)
    counts = np.array([l.shape[0] for l in faceLogits])
    last = np.cumsum(counts).astype(np.int32)
    first = (last - counts + 1).astype(np.int32)
    cat = np.asfortranarray(np.concatenate(faceLogits, 0)[:, :numSrcEmotions])
    X, _ = vl.aggregate_logits(vl.from_numpy(cat, device), torch.from_numpy(first).to(device),
                               torch.from_numpy(last).to(device), AGGREGATORS[aggregator])
    labels = np.asarray(tracks[labelType]).reshape(-1)
    dlabels = torch.from_numpy(labels.astype(np.int32)).to(device)
    # the fits of all folds: one launch
    B, status, iters, dev = vl.mnrfit(X, dlabels, trainIdxSets, numTargetEmotions, maxIter=maxIter, tolX=tolX)
    coefs = vl.to_numpy(B).reshape(numSrcEmotions + 1, numTargetEmotions - 1, numFolds, order="F")
    status, iters = status.cpu().numpy(), iters.cpu().numpy()
    from scipy.io import savemat
    for f in range(numFolds):
        if verbose:
            print("finetuning with fold %d/%d" % (f + 1, numFolds), flush=True)
        if status[f] == vl.MNR_BADINPUT:
            raise ValueError("fold %d: a class of 1..%d is absent from the training rows (or a label is outside "
                             "that range); mnrfit would drop the category" % (f + 1, numTargetEmotions))
        if status[f] == vl.MNR_ITERLIMIT:
            warnings.warn("fold %d: mnrfit reached the iteration limit (%d); the data may be separable"
                          % (f + 1, int(iters[f])))
        elif status[f] == vl.MNR_NOTPD:
            warnings.warn("fold %d: mnrfit stopped at iteration %d, the Hessian is not positive definite"
                          % (f + 1, int(iters[f])))
        os.makedirs(expDirs[f], exist_ok=True)
        savemat(os.path.join(expDirs[f], "mnr-params.mat"), {"coefficients": coefs[:, :, f]})
    fused = vl.to_numpy(X).reshape(numSrcEmotions, -1, order="F").T
    miniImdb = {"labels": labels, "fusedLogits": np.ascontiguousarray(fused), "images": {"set": sets}}
    return miniImdb, expDirs, valIdxSets


def _write_confmat(normed, confSum, labels, dataset, figDir, modelName):
    """generate_confmatrix_fig's output as data: figDir/confmat/<dataset>-<modelName>.json and .txt."""
    d = os.path.join(figDir, "confmat")
    os.makedirs(d, exist_ok=True)
    base = os.path.join(d, "%s-%s" % (dataset, modelName))
    rows = [[None if not np.isfinite(v) else float(v) for v in r] for r in normed]
    with open(base + ".json", "w") as f:
        json.dump({"dataset": dataset, "modelName": modelName, "labels": labels, "normalized": rows,
                   "confusion": np.asarray(confSum).astype(int).tolist()}, f, indent=1)
    with open(base + ".txt", "w") as f:
        f.write("\t" + "\t".join(labels) + "\n")
        for lab, r in zip(labels, normed):
            f.write(lab + "\t" + "\t".join("%0.2f" % v for v in r) + "\n")
    return base + ".json"


def emo_benchmarks(modality="audio", datasets=("rml", "enterface"), modelName="emovoxceleb-student",
                   figDir="data/affine-figs-audio-splits", *, net=None, imdbs=None, root="data", verbose=True,
                   modelDir=None):
    """Options as in emo_benchmarks.m:36-40.  Returns {dataset: {'foldAccs', 'mean', 'std', 'confSum', 'normed',
    'labels' (canonical), 'adjustmentFactor', 'expDirs', 'valIdxSets', 'preds', 'confPath'}}.
    Extensions (keyword-only): `net` (a trained or reduced network instead of the zoo's), `imdbs` ({dataset: imdb},
    default SyntheticBenchmarkImdb), `root` (vl_rootnn), `verbose` (the reference's printout), `modelDir` (as in
    run_cross_val)."""
    if isinstance(datasets, str):
        datasets = [datasets]
    out = {}
    for dataset in datasets:
        if verbose:
            print("learning classifier weights...", flush=True)
        if dataset not in DATASETS:
            raise ValueError("unknown dataset %s" % dataset)
        datasetLabels, numFolds, useExstingVal, adjustmentFactor = DATASETS[dataset]
        numTargetEmotions = len(datasetLabels)
        miniImdb, expDirs, valIdxSets = run_cross_val(
            modelName=modelName, targetDataset=dataset, numSrcEmotions=len(MODEL_EMO_LABELS),
            useExstingVal=useExstingVal, numFolds=numFolds, numTargetEmotions=numTargetEmotions, modality=modality,
            imdb=(imdbs or {}).get(dataset), net=net, root=root, verbose=verbose, modelDir=modelDir)
        from scipy.io import loadmat
        coefs = [loadmat(os.path.join(e, "mnr-params.mat"))["coefficients"] for e in expDirs]   # :92-93
        device = torch.device("cuda", torch.cuda.current_device())
        B = torch.from_numpy(np.stack([np.asarray(c, np.float64).T for c in coefs], 0)).to(device).permute(2, 1, 0)
        X = vl.from_numpy(miniImdb["fusedLogits"].T, device)
        labels = miniImdb["labels"]
        dlabels = torch.from_numpy(labels.astype(np.int32)).to(device)
        # the scoring of all folds: one launch
        probs, preds, conf = vl.mnrval(B, X, valIdxSets, dlabels)
        conf = conf.cpu().numpy()
        preds = [p.cpu().numpy() for p in preds]
        foldAccs = np.zeros(len(expDirs))
        confSum = np.zeros((numTargetEmotions, numTargetEmotions), dtype=np.int64)
        for ee in range(len(expDirs)):                                                   # :87-107
            valIdx = valIdxSets[ee]
            matches = preds[ee] == labels[np.asarray(valIdx, dtype=np.int64) - 1]
            acc = (matches.sum() / matches.size if matches.size else float("nan")) * adjustmentFactor
            confSum += conf[ee]
            if verbose:
                print("(fold %d/%d) recomputed accuracy: %.1f" % (ee + 1, len(expDirs), 100 * acc))
                print("(fold %d/%d) accuracy for %s: %.1f" % (ee + 1, len(expDirs), modelName, acc))
            foldAccs[ee] = acc
        mean, std = fold_summary(foldAccs)
        normed = normalise_confusion(confSum)
        canon = canonicalLabels(datasetLabels)
        if verbose:
            print("-----------------------------")
            print("DATASET: %s" % dataset)
            print("MODEL: %s" % modelName)
            print("cross-validation score: %g, std %g " % (mean, std))
            print("-----------------------------")
            print("confusion matrix:")
            print(confSum)
            print("-----------------------------")
            print("normalized confusion matrix:")
            print(normed, flush=True)
        confPath = _write_confmat(normed, confSum, canon, dataset, figDir, modelName)
        out[dataset] = {"foldAccs": foldAccs, "mean": mean, "std": std, "confSum": confSum, "normed": normed,
                        "labels": canon, "adjustmentFactor": adjustmentFactor, "expDirs": expDirs,
                        "valIdxSets": valIdxSets, "preds": preds, "confPath": confPath}
    return out
