"""benchmark_ferplus_models mirror (teacher/benchmark_ferplus_models.m): evaluate the FER+ teachers on the FER+
validation and test sets.

    benchmark_ferplus_models('refresh', false, 'dataDir', ..., 'benchmarkCacheDir', ...)

Same options, defaults and flow as the reference (:22-64): the two (modelName, lossType) pairs of :31-34, for each a cache
file <benchmarkCacheDir>/<modelName>.json (the reference's .mat) that is honoured unless `refresh`; otherwise
ferplus_baselines evaluates the model twice with train.batchSize 32 -- evaluateOnly.subset 'val' (PublicTest) and 'test'
(PrivateTest) -- and valAcc / testAcc = 1 - val.classerror are cached and printed with the reference's text.  `dataDir`
holds fer2013.csv and fer2013new.csv (:15-17); ferplus_baselines reads them through batch.getFerPlusImdb.

WITHOUT `modelDir` THE ACCURACIES ARE MEANINGLESS: the weights are then the seeded synthetic stand-ins of zoo.ferPlusZoo
and what is mirrored is the flow, the data path and the cache.  With `modelDir` the published teachers are read from
<modelDir>/<modelName>.mat (dagnn.load_mat); nobody has run that against the published figures yet.
Extensions are keyword-only.
"""
import json
import os
import time

from .ferplus_baselines import ferplus_baselines

PRETRAINED = (("resnet50-ferplus", "softmaxlog"), ("senet50-ferplus", "distributions"))   # :31-34


def benchmark_ferplus_models(refresh=False, dataDir="data/datasets/fer2013+", benchmarkCacheDir="data/ferPlus/benchCache",
                             *, imdb=None, widthMult=1.0, blocks=(3, 4, 6, 3), seed=0, verbose=True, modelDir=None):
    """Options as in benchmark_ferplus_models.m:22-25.  Extensions (keyword-only): `imdb` (a prepared imdb instead of
    the CSVs of dataDir), `widthMult` / `blocks` (narrow networks for tests), `seed`, `verbose` (the printout),
    `modelDir` (the directory of resnet50-ferplus.mat / senet50-ferplus.mat: the published teachers are evaluated).
    Returns {modelName: {'valAcc': .., 'testAcc': ..}} -- the reference only prints."""
    say = (lambda *a: print(*a, end="", flush=True)) if verbose else (lambda *a: None)
    os.makedirs(benchmarkCacheDir, exist_ok=True)                                        # :27-29
    results = {}
    for modelName, lossType in PRETRAINED:                                               # :36-39
        say("-----------------------------------------------------------\n")
        cachePath = os.path.join(benchmarkCacheDir, "%s.json" % modelName)              # :40-41
        if os.path.isfile(cachePath) and not refresh:                                    # :42-44
            say("loading cached results for %s on FER...\n" % modelName)
            with open(cachePath) as fh:
                stats = json.load(fh)
        else:
            commonArgs = dict(modelName=modelName, batchSize=32, lossType=lossType, dataDir=dataDir, imdb=imdb,
                              widthMult=widthMult, blocks=blocks, seed=seed, modelDir=modelDir)   # :46-49
            say("evaluating %s on FER+...\n" % modelName)
            _, valInfo = ferplus_baselines(evaluateOnly={"subset": "val"}, **commonArgs)     # :51-52
            _, testInfo = ferplus_baselines(evaluateOnly={"subset": "test"}, **commonArgs)   # :53-54
            stats = {"valAcc": 1 - float(valInfo["val"][-1]["classerror"]),              # :55-57
                     "testAcc": 1 - float(testInfo["val"][-1]["classerror"])}
            say("caching results for %s to %s ..." % (modelName, cachePath))
            tic = time.time()
            with open(cachePath, "w") as fh:
                json.dump(stats, fh)
            say("done in %g s \n" % (time.time() - tic))
        say("%s: val (%.3f), test: (%.3f)\n" % (modelName, stats["valAcc"], stats["testAcc"]))   # :62-63
        results[modelName] = stats
    return results
