"""ferplus_baselines mirror (teacher/ferplus_baselines.m): fine-tune the FER+ face teachers.

    [net, info] = ferplus_baselines('modelName', 'senet50_ft-dag', 'dataType', 'CNTK', ...)

Same option names, defaults and flow as the reference (:59-80): name the experiment directory (buildExpDirName,
:297-309), pick 8 or 10 classes from `dataType`, build the network with ferPlusZoo's training branch, optionally
evaluate only (the set remapping of :120-136), bind getBatchFerPlus and call cnn_train_dag with batch 128 and the
3 x 60-epoch learning-rate schedule.  What differs, because there is no MatConvNet here: the imdb comes from
batch.getFerPlusImdb when `dataDir` holds fer2013.csv and fer2013new.csv (the function is not in the reference; its
rules are written down there) and is the seeded batch.SyntheticFerPlusImdb otherwise, the weights are synthetic, and
`gpus` is the torchrun world as in run_distillation.  `evaluateOnly.fromCkpt` picks the checkpoint whose saved info has the lowest
validation classerror; unlike the external findBestEpoch it prunes no file.  Extensions are keyword-only.
"""
import copy
import os

import numpy as np

from . import batch as xbatch
from . import train, zoo

LEARNING_RATE = np.concatenate([np.full(60, 0.01), np.full(60, 0.001), np.full(60, 0.0001)])   # :77-79


PRETRAINED = ("resnet50-ferplus", "senet50-ferplus")      # ferPlusZoo.m:60-63


def pretrained_heads(dag, lossType):
    """The published FER+ teachers are checkpoints of this very training and are loaded with its heads: 'loss' ->
    objective and 'classerror' -> classerror (benchmark_ferplus_models.m:55-56 reads val.classerror).  The synthetic
    stand-ins of zoo.ferPlusZoo carry the heads of the architecture they are built from (softmaxlog / top1error on
    'label'); they are replaced by what configureForClassification (ferPlusZoo.m:239-263) attaches for `lossType`."""
    from . import dagnn
    zoo.strip_losses(dag)
    if lossType == "softmaxlog":
        layer, hard = dagnn.Loss("softmaxlog"), "label"
    elif lossType == "distributions":
        layer, hard = dagnn.SoftmaxCELoss(temperature=1, logitTargets=False), "hardlabel"
    else:
        raise ValueError("unrecognised loss: %s" % lossType)
    dag.addLayer("loss", layer, ["prediction", "label"], "objective")
    dag.addLayer("classerror", dagnn.Loss("classerror"), ["prediction", hard], "classerror")
    dag._flat = None
    return dag


def buildExpDirName(modelName="senet50_ft-dag", lossType="distributions", dataType="CNTK", dropoutRate=0.5,
                    dataAug=True, root="data/grimaces/fer2013+"):
    """ferplus_baselines.m:297-309 (`root` stands for fullfile(vl_rootnn, 'data/grimaces/fer2013+'))."""
    expDir = os.path.join(root, "%s-%s" % (modelName, lossType))
    if dataType in ("full", "CNTK"):
        expDir += "-" + dataType
    if dropoutRate > 0:
        expDir += "-dropout-%g" % dropoutRate
    if dataAug:
        expDir += "-aug"
    return expDir


def best_checkpoint(expDir, metric="classerror"):
    """epoch of the net-epoch-<n>.pt in expDir whose saved info has the lowest validation `metric` at that epoch
    (what findBestEpoch(expDir, 'priorityMetric', 'classerror') selects; no file is pruned).  None if there is none."""
    import torch
    best, best_val = None, None
    for name in os.listdir(expDir) if os.path.isdir(expDir) else []:
        if not (name.startswith("net-epoch-") and name.endswith(".pt")):
            continue
        try:
            e = int(name[len("net-epoch-"):-len(".pt")])
        except ValueError:
            continue
        ck = torch.load(os.path.join(expDir, name), map_location="cpu", weights_only=True)
        val = (ck.get("info") or {}).get("val") or []
        if len(val) < e or metric not in val[e - 1]:
            continue
        v = float(val[e - 1][metric])
        if best_val is None or v < best_val or (v == best_val and e < best):
            best, best_val = e, v
    return best


def ferplus_baselines(dev=False, useBnorm=1, dataAug=True, dataType="CNTK", lossType="distributions",
                      modelName="senet50_ft-dag", dataDir="data/datasets/fer2013+", evaluateOnly=None, gpus=1,
                      finetuneLR=0.1, dropoutRate=0.5, cont=True, batchSize=128, learningRate=None, numEpochs=300,
                      *, imdb=None, expRoot="data/grimaces/fer2013+", widthMult=1.0, blocks=(3, 4, 6, 3), seed=0,
                      numImages=512, verbose=False, modelDir=None, solver=None, solverOpts=None, nesterovUpdate=False,
                      momentum=0.9, weightDecay=5e-4):
    """Options as in ferplus_baselines.m:59-80 (`cont` is opts.train.continue, `gpus` / `batchSize` /
    `learningRate` are opts.train.*; `numEpochs` is cnn_train_dag's default, 300, with the last rate held after
    epoch 180).  `evaluateOnly` = {'subset': '' | 'val' | 'test', 'fromCkpt': bool}.  `dataDir` holds the FER2013 and
    FER+ CSVs (fer2013.csv, fer2013new.csv): when both are there and no `imdb` is given, getFerPlusImdb reads them.
    Extensions (keyword-only): `imdb` (a prepared imdb; without it and without the CSVs a SyntheticFerPlusImdb of
    `numImages` images), `expRoot` (root of the experiment directories), `widthMult` / `blocks` (narrow networks for
    tests), `seed` (synthetic weights, imdb and batch draws), `modelDir` (zoo.ferPlusZoo reads the model file from there
    instead of building the seeded stand-in), `solver` / `solverOpts` / `nesterovUpdate` / `momentum` / `weightDecay`
    (further fields of opts.train, handed to cnn_train_dag as :140-141 hands the whole struct; the defaults are
    cnn_train_dag's)."""
    ev = {"subset": "", "fromCkpt": False}
    ev.update(evaluateOnly or {})
    if learningRate is None:
        learningRate = LEARNING_RATE
    expDir = buildExpDirName(modelName, lossType, dataType, dropoutRate, dataAug, expRoot)
    numOutputs = xbatch.ferplus_num_classes(dataType)                                   # :88-93
    dag = zoo.ferPlusZoo(modelName, seed=100 + seed, width_mult=widthMult, blocks=blocks, useBnorm=useBnorm,
                         finetuneLR=finetuneLR, dropoutRate=dropoutRate, lossType=lossType,
                         numOutputs=numOutputs, modelDir=modelDir)                       # :95-100
    if modelName in PRETRAINED:
        pretrained_heads(dag, lossType)
    if imdb is None:                                                                    # :103-110
        if all(os.path.isfile(os.path.join(dataDir, f)) for f in ("fer2013.csv", "fer2013new.csv")):
            imdb = xbatch.getFerPlusImdb(dataDir, dataType)
        else:
            imdb = xbatch.SyntheticFerPlusImdb(num_images=numImages, seed=seed)
    sets = np.array(imdb.images["set"], copy=True)
    if dev:                                                                             # :112-118
        sample = 1000
        sets[:] = 4
        sets[:sample] = 1
        sets[sample:2 * sample] = 2
        numEpochs = 1
    evaluating = ev["subset"] in ("val", "test")
    if evaluating:                                                                      # :120-136
        if ev["fromCkpt"]:
            best = best_checkpoint(expDir)
            if best is None:
                raise FileNotFoundError("no checkpoint with validation statistics in %s" % expDir)
            ckptPath = os.path.join(expDir, "net-epoch-%d.pt" % best)
            if verbose:
                print("loading from checkpointing %s..." % ckptPath, flush=True)
            train.load_checkpoint(dag, ckptPath)
        sets[sets == 1] = 4
        if ev["subset"] == "test":
            sets[sets == 2] = 4
            sets[sets == 3] = 2
        numEpochs = 1
        cont = False
    imdb = copy.copy(imdb)                       # the caller's imdb keeps its sets (a MATLAB struct is a value)
    imdb.images = dict(imdb.images, set=sets)
    norm = dag.meta["normalization"]
    brng = np.random.default_rng(seed + 31)

    def getBatch(imdb_, batch):                                                         # :138
        return xbatch.getBatchFerPlus(imdb_, batch, dataType=dataType, lossType=lossType, dataAug=dataAug,
                                      imageSize=tuple(norm["imageSize"][:2]), averageImage=norm["averageImage"],
                                      rng=brng)

    dag.meta["classes"]["name"] = list(imdb.meta["classes"])                            # :139
    trainSamples = [i for i in range(len(sets)) if sets[i] == 1]
    valSamples = [i for i in range(len(sets)) if sets[i] == 2]
    # evaluation only: no training samples and no checkpoint written (cnn_train_dag's evaluateMode saves no state)
    return train.cnn_train_dag(dag, imdb, getBatch, learningRate=learningRate, batchSize=batchSize,
                               numEpochs=numEpochs, train=trainSamples, val=valSamples, cont=cont,
                               expDir=None if evaluating else expDir, extractStatsFn=train.extractStats,
                               verbose=verbose, solver=solver, solverOpts=solverOpts, nesterovUpdate=nesterovUpdate,
                               momentum=momentum, weightDecay=weightDecay)
