"""emoVoxZoo / ferPlusZoo mirrors: the student and teacher graphs of the reference.

The reference downloads the networks as .mat files (emoVoxCeleb/emoVoxZoo.m:36-40,95-97;
teacher/ferPlusZoo.m:93-101); those files are not available offline, so by default the architectures
are restated from the published models and the weights are seeded synthetic
ones.  With `modelDir` both zoos read the model files from that directory instead
(dagnn.load_mat); nothing is ever downloaded.  The one structural pin the reference holds
-- the pool6 width table at emoVoxZoo.m:258-259 -- is reproduced exactly by `vggvox()`
(tests/test_pins.py).

Net surgery follows the reference line by line where it exists:
    prepareFromDagNN        emoVoxZoo.m:187-253   strip Loss/SoftMax, last FC -> numOutputs
    configureForRegression  emoVoxZoo.m:105-183   loss + classerror + ErrorStats layers
    updatePooling           emoVoxZoo.m:256-269   pool6 <- [1 p1] from the bucket table
    insertBNLayers          ferPlusZoo.m:123      called there, missing from the reference: built from what
                                                  ferplus_baselines.m:14-17 documents
"""
import os

import numpy as np
import torch

from . import dagnn, vl

EMOTIONS = ["neutral", "happiness", "surprise", "sadness", "anger", "disgust", "fear", "contempt"]

# emoVoxZoo.m:258-259 (also external/compute_audio_feats.m:45-46)
BUCKETS_POOL = [2, 5, 8, 11, 14, 17, 20, 23, 27, 30]
BUCKETS_WIDTH = list(range(100, 1001, 100))


# ---------------------------------------------------------------------------------------------
# raw architectures ("what the .mat files contain")
# ---------------------------------------------------------------------------------------------
def vggvox(num_classes=1251, width_mult=1.0):
    """VGGVox (VGG-M, BN variant), input 512 x W x 1 -- SURVEY Appendix B.1.
    `width_mult` < 1 shrinks the channel counts for CPU-sized tests (geometry unchanged)."""
    def c(n):
        return max(4, int(round(n * width_mult)))

    net = dagnn.DagNN()
    spec = [  # name, FH, FW, Cin, Cout, stride, pad
        ("1", 7, 7, 1, c(96), 2, 1), ("2", 5, 5, c(96), c(256), 2, 1), ("3", 3, 3, c(256), c(384), 1, 1),
        ("4", 3, 3, c(384), c(256), 1, 1), ("5", 3, 3, c(256), c(256), 1, 1),
    ]
    x = "input"
    for name, fh, fw, ci, co, s, p in spec:
        net.addLayer("conv" + name, dagnn.Conv([fh, fw, ci, co], True, (s, s), (p, p, p, p)), x,
                     "x_conv" + name, ["conv%sf" % name, "conv%sb" % name])
        net.addLayer("bn" + name, dagnn.BatchNorm(co), "x_conv" + name, "x_bn" + name,
                     ["bn%sm" % name, "bn%sb" % name, "bn%sx" % name])
        net.addLayer("relu" + name, dagnn.ReLU(), "x_bn" + name, "x_relu" + name)
        x = "x_relu" + name
        if name in ("1", "2"):
            net.addLayer("mpool" + name, dagnn.Pooling([3, 3], (2, 2), (0, 0, 0, 0), "max"), x,
                         "x_mpool" + name)
            x = "x_mpool" + name
        if name == "5":
            net.addLayer("mpool5", dagnn.Pooling([5, 3], (3, 2), (0, 0, 0, 0), "max"), x, "x_mpool5")
            x = "x_mpool5"
    net.addLayer("fc6", dagnn.Conv([9, 1, c(256), c(4096)], True), x, "x_fc6", ["fc6f", "fc6b"])
    net.addLayer("bn6", dagnn.BatchNorm(c(4096)), "x_fc6", "x_bn6", ["bn6m", "bn6b", "bn6x"])
    net.addLayer("relu6", dagnn.ReLU(), "x_bn6", "x_relu6")
    net.addLayer("pool6", dagnn.Pooling([1, 8], (1, 1), (0, 0, 0, 0), "avg"), "x_relu6", "x_pool6")
    net.addLayer("fc7", dagnn.Conv([1, 1, c(4096), c(1024)], True), "x_pool6", "x_fc7", ["fc7f", "fc7b"])
    net.addLayer("bn7", dagnn.BatchNorm(c(1024)), "x_fc7", "x_bn7", ["bn7m", "bn7b", "bn7x"])
    net.addLayer("relu7", dagnn.ReLU(), "x_bn7", "x_relu7")
    net.addLayer("fc8", dagnn.Conv([1, 1, c(1024), num_classes], True), "x_relu7", "x_fc8",
                 ["fc8f", "fc8b"])
    net.addLayer("softmax", dagnn.SoftMax(), "x_fc8", "prob")
    net.meta = {"normalization": {"imageSize": [512, 300, 1]},
                "audio": {"fs": 16000, "Tw": 25, "Ts": 10, "nfft": 1024}}
    return net


def resnet50(se=False, num_classes=8, width_mult=1.0, blocks=(3, 4, 6, 3)):
    """(SE-)ResNet-50, Caffe style (stride on the first 1x1 of a stage), input 224 x 224 x 3 --
    SURVEY Appendix B.2 / B.3.  Variable / layer names follow the Caffe imports."""
    def c(n):
        return max(4, int(round(n * width_mult)))

    net = dagnn.DagNN()
    net.addLayer("conv1", dagnn.Conv([7, 7, 3, c(64)], True, (2, 2), (3, 3, 3, 3)), "data", "conv1",
                 ["conv1_filter", "conv1_bias"])
    net.addLayer("bn_conv1", dagnn.BatchNorm(c(64), 1e-5), "conv1", "conv1_bn",
                 ["bn_conv1_mult", "bn_conv1_bias", "bn_conv1_moments"])
    net.addLayer("conv1_relu", dagnn.ReLU(), "conv1_bn", "conv1x")
    net.addLayer("pool1", dagnn.Pooling([3, 3], (2, 2), (0, 1, 0, 1), "max"), "conv1x", "pool1")
    x, cin = "pool1", c(64)
    for si, nb in enumerate(blocks):
        mid, cout = c(64 * 2 ** si), c(256 * 2 ** si)
        for bi in range(nb):
            tag = "res%d%s" % (si + 2, "abcdefgh"[bi])
            stride = 2 if (bi == 0 and si > 0) else 1
            sc = x
            if bi == 0:
                net.addLayer(tag + "_branch1", dagnn.Conv([1, 1, cin, cout], False, (stride, stride)), x,
                             tag + "_branch1", [tag + "_branch1_filter"])
                net.addLayer("bn" + tag[3:] + "_branch1", dagnn.BatchNorm(cout, 1e-5), tag + "_branch1",
                             tag + "_branch1_bn", [tag + "_b1_mult", tag + "_b1_bias", tag + "_b1_moments"])
                sc = tag + "_branch1_bn"
            y = x
            for li, (fh, ci, co, s, p) in enumerate([(1, cin, mid, stride, 0), (3, mid, mid, 1, 1),
                                                      (1, mid, cout, 1, 0)]):
                nm = tag + "_branch2" + "abc"[li]
                net.addLayer(nm, dagnn.Conv([fh, fh, ci, co], False, (s, s), (p, p, p, p)), y, nm,
                             [nm + "_filter"])
                net.addLayer("bn" + nm[3:], dagnn.BatchNorm(co, 1e-5), nm, nm + "_bn",
                             [nm + "_mult", nm + "_bias", nm + "_moments"])
                y = nm + "_bn"
                if li < 2:
                    net.addLayer(nm + "_relu", dagnn.ReLU(), y, nm + "x")
                    y = nm + "x"
            if se:
                r = max(4, cout // 16)
                net.addLayer(tag + "_global_pool", dagnn.GlobalPooling("avg"), y, tag + "_gp")
                net.addLayer(tag + "_fc1", dagnn.Conv([1, 1, cout, r], True), tag + "_gp", tag + "_fc1",
                             [tag + "_fc1_filter", tag + "_fc1_bias"])
                net.addLayer(tag + "_fc1_relu", dagnn.ReLU(), tag + "_fc1", tag + "_fc1x")
                net.addLayer(tag + "_fc2", dagnn.Conv([1, 1, r, cout], True), tag + "_fc1x", tag + "_fc2",
                             [tag + "_fc2_filter", tag + "_fc2_bias"])
                net.addLayer(tag + "_prob", dagnn.Sigmoid(), tag + "_fc2", tag + "_prob")
                net.addLayer(tag, dagnn.Axpy(), [tag + "_prob", y, sc], tag)
            else:
                net.addLayer(tag, dagnn.Sum(), [sc, y], tag)
            net.addLayer(tag + "_relu", dagnn.ReLU(), tag, tag + "x")
            x, cin = tag + "x", cout
    net.addLayer("pool5", dagnn.Pooling([7, 7], (1, 1), (0, 0, 0, 0), "avg"), x, "pool5")
    net.addLayer("classifier", dagnn.Conv([1, 1, cin, num_classes], True), "pool5", "prediction",
                 ["classifier_filter", "classifier_bias"])
    net.addLayer("loss", dagnn.Loss("softmaxlog"), ["prediction", "label"], "objective")
    net.addLayer("top1error", dagnn.Loss("classerror"), ["prediction", "label"], "top1error")
    net.meta = {"normalization": {"imageSize": [224, 224, 3], "averageImage": [131.0912, 103.8827, 91.4953]},
                "classes": {"name": list(EMOTIONS), "description": list(EMOTIONS)}}
    return net


VGG_FACE_AVERAGE = [129.1863, 104.7624, 93.5940]        # [EXT] the VGG-Face models' meta.normalization.averageImage


def _vgg_tail(net, x, cin, span, width, num_classes):
    """fc6 (spans the final map) -> relu6 -> dropout6 -> fc7 -> relu7 -> dropout7 -> fc8 -> prob of the VGG families"""
    net.addLayer("fc6", dagnn.Conv([span, span, cin, width], True), x, "fc6", ["fc6f", "fc6b"])
    net.addLayer("relu6", dagnn.ReLU(), "fc6", "relu6")
    net.addLayer("dropout6", dagnn.DropOut(rate=0.5, seed=len(net.layers)), "relu6", "dropout6")
    net.addLayer("fc7", dagnn.Conv([1, 1, width, width], True), "dropout6", "fc7", ["fc7f", "fc7b"])
    net.addLayer("relu7", dagnn.ReLU(), "fc7", "relu7")
    net.addLayer("dropout7", dagnn.DropOut(rate=0.5, seed=len(net.layers)), "relu7", "dropout7")
    net.addLayer("fc8", dagnn.Conv([1, 1, width, num_classes], True), "dropout7", "fc8", ["fc8f", "fc8b"])
    net.addLayer("prob", dagnn.SoftMax(), "fc8", "prob")


def vgg_vd_face(num_classes=2622, width_mult=1.0, image_size=224):
    """VGG-Face, the 16-layer VGG-VD [EXT: the vgg-face model of the MatConvNet model zoo]: conv1_1 .. conv5_3, 3 x 3 / pad 1
    with 64-64 / 128-128 / 256 x 3 / 512 x 3 / 512 x 3 channels, each followed by a ReLU; 2 x 2 / stride 2 max pooling after
    every stage; fc6 spans the final map (7 x 7 x 512 x 4096 at 224), dropout 0.5 behind relu6 and relu7, fc8, softmax.  No
    batch norm anywhere (insertBNLayers).  `width_mult` < 1 and `image_size` (a multiple of 32; fc6 spans image_size / 32)
    are for tests."""
    if image_size % 32 or image_size <= 0:
        raise ValueError("vgg_vd_face: image_size must be a positive multiple of 32")

    def c(n):
        return max(4, int(round(n * width_mult)))

    net = dagnn.DagNN()
    x, cin = "input", 3
    for stage, (n, ch) in enumerate([(2, 64), (2, 128), (3, 256), (3, 512), (3, 512)], 1):
        for i in range(1, n + 1):
            tag = "%d_%d" % (stage, i)
            net.addLayer("conv" + tag, dagnn.Conv([3, 3, cin, c(ch)], True, (1, 1), (1, 1, 1, 1)), x, "conv" + tag,
                         ["conv%sf" % tag, "conv%sb" % tag])
            net.addLayer("relu" + tag, dagnn.ReLU(), "conv" + tag, "relu" + tag)
            x, cin = "relu" + tag, c(ch)
        net.addLayer("pool%d" % stage, dagnn.Pooling([2, 2], (2, 2), (0, 0, 0, 0), "max"), x, "pool%d" % stage)
        x = "pool%d" % stage
    _vgg_tail(net, x, cin, image_size // 32, c(4096), num_classes)
    net.meta = {"normalization": {"imageSize": [image_size, image_size, 3], "averageImage": list(VGG_FACE_AVERAGE)}}
    return net


def vgg_m_face(bn=True, num_classes=2622, width_mult=1.0):
    """VGG-M trained on faces [EXT: Chatfield et al.'s VGG-M, imagenet-vgg-m of the MatConvNet model zoo], input 224 x 224 x 3:
    conv1 7 x 7 x 96 / stride 2, conv2 5 x 5 x 256 / stride 2 / pad 1, conv3 .. conv5 3 x 3 x 512 / pad 1, 3 x 3 / stride 2 max
    pooling behind stages 1, 2 and 5, fc6 6 x 6 x 512 x 4096, fc7, fc8.  `bn`: BatchNorm + ReLU behind conv1 .. fc7 (the
    -bn models); otherwise ReLU, with norm1 / norm2 = dagnn.LRN([5 2 1e-4 0.75]) behind relu1 / relu2 (the classic file).
    The pools pad one row / column at the bottom / right ([0 1 0 1]): 224 -> 109 -> 54 -> 26 -> 13 -> 6, so fc6 lands on a
    6 x 6 map and gives 1 x 1 (the geometry pin; tests/test_lrn_cpu.py)."""
    def c(n):
        return max(4, int(round(n * width_mult)))

    net = dagnn.DagNN()
    spec = [("1", 7, 3, c(96), 2, 0), ("2", 5, c(96), c(256), 2, 1), ("3", 3, c(256), c(512), 1, 1),
            ("4", 3, c(512), c(512), 1, 1), ("5", 3, c(512), c(512), 1, 1), ("6", 6, c(512), c(4096), 1, 0),
            ("7", 1, c(4096), c(4096), 1, 0)]
    x = "input"
    for name, f, ci, co, s, p in spec:
        lname = ("conv" if int(name) < 6 else "fc") + name
        net.addLayer(lname, dagnn.Conv([f, f, ci, co], True, (s, s), (p, p, p, p)), x, lname, [lname + "f", lname + "b"])
        x = lname
        if bn:
            net.addLayer("bn" + name, dagnn.BatchNorm(co), x, "bn" + name, ["bn%sm" % name, "bn%sb" % name, "bn%sx" % name])
            x = "bn" + name
        net.addLayer("relu" + name, dagnn.ReLU(), x, "relu" + name)
        x = "relu" + name
        if not bn and name in ("1", "2"):
            net.addLayer("norm" + name, dagnn.LRN([5, 2, 1e-4, 0.75]), x, "norm" + name)
            x = "norm" + name
        if name in ("1", "2", "5"):
            net.addLayer("pool" + name, dagnn.Pooling([3, 3], (2, 2), (0, 1, 0, 1), "max"), x, "pool" + name)
            x = "pool" + name
    net.addLayer("fc8", dagnn.Conv([1, 1, c(4096), num_classes], True), x, "fc8", ["fc8f", "fc8b"])
    net.addLayer("prob", dagnn.SoftMax(), "fc8", "prob")
    net.meta = {"normalization": {"imageSize": [224, 224, 3], "averageImage": list(VGG_FACE_AVERAGE)}}
    return net


def insertBNLayers(net):
    """dag = insertBNLayers(dag): ferPlusZoo.m:123 calls this function and the reference does not contain it; this is what
    ferplus_baselines.m:14-17 documents for `useBnorm`: "inserts batch norm layers into a model after each convolution.  If
    the model already contains any batch norm layers, this option does nothing".  One BatchNorm(K) goes directly behind
    every Conv except the one that produces 'prediction' (a normalised classifier output would pin the logits' scale), and
    the convolution's consumers read the bnorm's output instead.  Layer and variable <conv>_bn, parameters
    <conv>_bn_mult / _bias / _moments with the values and rates DagNN.initParams gives a BatchNorm (g = 1 at rate 2, b = 0,
    moments (0, 1) with trainMethod 'average' at 0.1, no weight decay).  The convolutions keep their biases.  DropOut layers
    take their new position as seed (insert_dropout's and loadobj's rule), so a saved and reloaded net draws the same masks."""
    if any(isinstance(l.block, dagnn.BatchNorm) for l in net.layers):
        return net
    for l in list(net.layers):
        if not isinstance(l.block, dagnn.Conv) or l.outputs[0] == "prediction":
            continue
        src, name = l.outputs[0], l.name + "_bn"
        if name in net.vars or net.getLayerIndex(name) is not None:
            raise ValueError("insertBNLayers: the network already has a '%s'" % name)
        readers = [q.name for q in net.layers if src in q.inputs]
        net.insertLayerAfter(l.name, name, dagnn.BatchNorm(l.block.size[3]), src, name,
                             [name + "_mult", name + "_bias", name + "_moments"])
        for q in readers:
            net.setLayerInputs(q, [name if v == src else v for v in net.getLayer(q).inputs])
        net.initLayerParams(net.getLayer(name), None)
    for pos, l in enumerate(net.layers):
        if isinstance(l.block, dagnn.DropOut):
            l.block.seed = pos          # the layers moved: insert_dropout's and loadobj's rule, seed = position
    net._flat = None
    return net


def synthetic_pretrained(net, seed):
    """Seeded stand-in for downloaded weights: He-normal filters, zero biases,
    BN g = 1, b = 0, stored moments mean ~ N(0, .1), sigma ~ U(.5, 1.5)."""
    net.initParams(seed)
    rng = np.random.default_rng(seed + 1)
    for l in net.layers:
        if isinstance(l.block, dagnn.BatchNorm):
            C = l.block.numChannels
            mom = np.zeros((C, 2), np.float32, order="F")
            mom[:, 0] = rng.standard_normal(C) * 0.1
            mom[:, 1] = rng.uniform(0.5, 1.5, C)
            net.params[l.params[2]].value = mom
    return net


def calibrate_moments(net, inputs):
    """Give a synthetic teacher realistic stored moments: one train-mode forward over `inputs`
    and copy each BatchNorm's batch moments into its `moments` parameter (what training with
    trainMethod 'average' converges to).  Runs on the GPU through the HIP kernels."""
    old_mode, old_fuse = net.mode, net.fuse
    net.mode, net.fuse = "normal", False
    try:
        if not isinstance(inputs, dict):
            inputs = {inputs[i]: inputs[i + 1] for i in range(0, len(inputs), 2)}
        for v in net.vars.values():
            v.value = None
        for k, t in inputs.items():
            if k in net.vars:
                net.vars[k].value = t
        for l in net.layers:
            if isinstance(l.block, dagnn.LossBase):
                continue
            ins = [net.vars[v].value for v in l.inputs]
            prm = [net.params[p].value for p in l.params]
            outs = l.block.forward(ins, prm)
            if isinstance(l.block, dagnn.BatchNorm):
                net.params[l.params[2]].value.copy_(l.block.moments)
                outs = l.block.forward(ins, prm)
            for v, t in zip(l.outputs, outs):
                net.vars[v].value = t
        for v in net.vars.values():
            v.value = None
    finally:
        net.mode, net.fuse = old_mode, old_fuse
    return net


# ---------------------------------------------------------------------------------------------
# ferPlusZoo (teacher)  -- teacher/ferPlusZoo.m:93-114,127-133
# ---------------------------------------------------------------------------------------------
FERPLUS_TRAINABLE = {"resnet50_ft-dag": False, "senet50_ft-dag": True}     # VGGFace2 imports -> SE or not

# the model lists of ferPlusZoo.m:37-69; only looked at when the models come from files (modelDir)
VGGFACE2_MODELS = ["resnet50_ft-dag", "resnet50_scratch-dag", "senet50_ft-dag", "senet50_scratch-dag"]
STANDARD_MODELS = ["vgg-m-face-bn-fer", "vgg-m-face-bn", "vgg-vd-face-fer", "vgg-vd-face", "vgg_face", "resnet50_ft-dag"]
FER_MODELS = ["vgg-vd-face-fer", "vgg-vd-face-sfew-dag", "vgg-m-face-bn-fer"]
SFEW_MODELS = ["vgg-vd-face-sfew", "resnet50-face-sfew"]
FERPLUS_MODELS = ["resnet50-ferplus", "senet50-ferplus"]
FERPLUS_MODELS_DEV = {"resnet50_ft-dag-dropout-0.1": "net-epoch-17",                   # :81-91
                      "resnet50_ft-dag-dropout-0.5": "net-epoch-122",
                      "senet50_ft-dag-distributions-dropout-0.5-aug": "net-epoch-98",
                      "senet50_ft-dag-distributions-CNTK-dropout-0.5-aug": "net-epoch-90"}
# the VGG face teachers that have a seeded stand-in (the SFEW names have none)
VGG_STANDINS = {"vgg-vd-face": vgg_vd_face, "vgg_face": vgg_vd_face, "vgg-vd-face-fer": vgg_vd_face,
                "vgg-m-face-bn": vgg_m_face, "vgg-m-face-bn-fer": vgg_m_face}
PUBLIC_MODELS = ["resnet50-ferplus", "senet50-ferplus", "emovoxceleb-student"]         # ensure_compatibility.m:13-15


def fixInputVarnames(net):
    """ferPlusZoo.m:127-133 / emoVoxZoo.m:65-71: an input variable called 'input' or 'x0' becomes 'data'"""
    for v in net.getInputs():
        if v in ("input", "x0"):
            net.renameVar(v, "data")
    return net


def load_model(path):
    """net = load(path) ; if isfield(net, 'net'), net = net.net ; end ; dag = dagnn.DagNN.loadobj(net).  A missing file
    raises: the reference's offer to download it (emoVoxZoo.m:74-102) is not mirrored."""
    if not os.path.isfile(path):
        raise FileNotFoundError("no model file at %s (model files are never downloaded: put it there)" % path)
    return dagnn.load_mat(path)


def ferPlusModelPath(modelName, modelDir):
    """ferPlusZoo.m:72-94: (path of the model file, name of the file without '.mat').  The VGGFace2 imports live in
    vggface2_models/, the development models in grimaces/<modelName>/net-epoch-N.mat."""
    names = VGGFACE2_MODELS + STANDARD_MODELS + FER_MODELS + SFEW_MODELS + FERPLUS_MODELS + list(FERPLUS_MODELS_DEV)
    if modelName not in names:
        raise ValueError("%s is not a recognised FER+ teacher" % modelName)                 # :72-73
    subfolder, fileName = "", modelName
    if modelName in VGGFACE2_MODELS:
        subfolder = "vggface2_models"
    elif modelName in FERPLUS_MODELS_DEV:
        subfolder, fileName = os.path.join("grimaces", modelName), FERPLUS_MODELS_DEV[modelName]
    return os.path.join(os.fspath(modelDir), subfolder, fileName + ".mat"), fileName


def ferPlusZoo(modelName, seed=100, width_mult=1.0, blocks=(3, 4, 6, 3), *, useBnorm=False, finetuneLR=1,
               dropoutRate=0, lossType="distributions", numOutputs=7, modelDir=None, image_size=224):
    """dag = ferPlusZoo(modelName, 'useBnorm', .., 'finetuneLR', .., 'dropoutRate', .., 'lossType', ..,
    'numOutputs', ..) -- teacher/ferPlusZoo.m (option defaults :30-36).

    'resnet50-ferplus' / 'senet50-ferplus': the pretrained FER+ teachers, returned as loaded (:93-114, :127-133).
    'resnet50_ft-dag' / 'senet50_ft-dag': the VGGFace2 networks configured for FER+ training (:116-124), as
    ferplus_baselines.m calls it.  That branch is broken as shipped; what is built is its evident
    intent, and these are the deviations:
      * `numOutputs` is undefined at :116 -- opts.numOutputs is used;
      * `opts.dropoout` at :119 does not exist (opts.dropooutRate is a typo'd second default) -- opts.dropoutRate is used;
      * `insertBNLayers` (:122) is not in the reference; zoo.insertBNLayers builds what ferplus_baselines.m:14-17 documents
        (a BatchNorm behind every convolution but the classifier, nothing when the model has batch norm already: the
        ResNets and vgg-m-face-bn are unchanged by useBnorm, the VGG-VD networks get 15 BatchNorms);
      * fixInputVarnames (:127-133) renames the input to 'input' although getBatchFerPlus feeds 'data'; it is 'data'
        here, as in the pretrained branch;
      * MATLAB's addLayer APPENDS the dropout layers, so layers(1:end-2) at :236 would be every layer but the two
        dropouts and the classifier would get finetuneLR too; the dropouts sit behind their convolutions here and
        layers(1:end-2) are all layers but pool5 and the classifier, which keeps its own rates ("except those used in
        the classifier", :12-14);
      * with lossType 'softmaxlog' getBatchFerPlus provides no 'hardlabel' (:215-220): the classerror head reads
        'label' then.
    Weights are seeded synthetic ones, as elsewhere (the VGGFace2 .mat files are not available), unless `modelDir`
    names the directory that holds the model files (the reference's vl_rootnn/data/models-import): then every name of
    :37-71 is read from <modelDir>/[subfolder/]<name>.mat (ferPlusModelPath), `seed` only seeds the new classifier, and
    `width_mult` / `blocks` mean nothing.  The pretrained names (ferPlusModels, ferModels, net-epoch-*) return as loaded
    after fixInputVarnames (:103-114), every other name goes through prepareFromDagNN and configureForClassification
    with the deviations above, and then insertBNLayers when `useBnorm` (:123).  A missing file raises FileNotFoundError.
    The VGG face teachers without `modelDir` (architectures restated from the public models [EXT]):
    'vgg-vd-face' / 'vgg_face' (vgg_vd_face; `image_size`, a multiple of 32, shrinks it for tests) and 'vgg-m-face-bn'
    (vgg_m_face(bn=True)) go through the training branch above; 'vgg-vd-face-fer' / 'vgg-m-face-bn-fer' are the
    pretrained FER stand-ins: the same graphs with 7 classes, as a FER training leaves them for inference -- up to the
    classifier's output 'prediction', neither loss heads nor the softmax (fetch_emovoxceleb_imdb.m:130 takes the last
    variable as the logits) -- returned after fixInputVarnames.  The SFEW names have no stand-in."""
    if modelDir is not None:
        path, fileName = ferPlusModelPath(modelName, modelDir)
        net = load_model(path)                                                     # :98-100
        if modelName in FERPLUS_MODELS or "net-epoch" in fileName or modelName in FER_MODELS:
            return fixInputVarnames(net)                                           # :103-114
        prepareFromDagNN(net, numOutputs, seed)                                    # :116
        configureForClassification(net, finetuneLR, dropoutRate, lossType)         # :118-119
        if useBnorm:
            insertBNLayers(net)                                                    # :123
        return fixInputVarnames(net)                                               # :124
    if modelName in VGG_STANDINS:
        pretrained = modelName in FER_MODELS
        build = VGG_STANDINS[modelName]
        kw = {"image_size": image_size} if build is vgg_vd_face else {}
        net = build(num_classes=7 if pretrained else 2622, width_mult=width_mult, **kw)
        synthetic_pretrained(net, seed)
        net.meta["modelName"] = modelName
        if pretrained:                                                             # :103-114
            net.removeLayer([l.name for l in net.layers if isinstance(l.block, dagnn.SoftMax)])
            net.renameVar(net.getOutputs()[-1], "prediction")
            return fixInputVarnames(net)
        prepareFromDagNN(net, numOutputs, seed)                                    # :116
        configureForClassification(net, finetuneLR, dropoutRate, lossType)         # :118-119
        if useBnorm:
            insertBNLayers(net)                                                    # :123
        return fixInputVarnames(net)                                               # :124
    if modelName in FERPLUS_TRAINABLE:
        net = resnet50(FERPLUS_TRAINABLE[modelName], numOutputs, width_mult, blocks)
        synthetic_pretrained(net, seed)
        prepareFromDagNN(net, numOutputs, seed)                                    # :116
        configureForClassification(net, finetuneLR, dropoutRate, lossType)         # :118-119
        net.meta["modelName"] = modelName
        return net
    if modelName == "resnet50-ferplus":
        net = resnet50(False, 8, width_mult, blocks)
    elif modelName == "senet50-ferplus":
        net = resnet50(True, 8, width_mult, blocks)
    else:
        raise ValueError("%s is not a recognised FER+ teacher" % modelName)  # ferPlusZoo.m:87
    synthetic_pretrained(net, seed)
    # ferPlusZoo.m:127-133: make sure the input variable is called 'data'
    for old in ("input", "x0"):
        if old in net.vars:
            net.renameVar(old, "data")
    net.meta["modelName"] = modelName
    return net


def configureForClassification(net, finetuneLR, dropout, lossType):
    """ferPlusZoo.m:202-263: dropout behind convLayers(end-2:end-1) when dropout > 0 and the net has none, finetuneLR
    on every parameter of layers(1:end-2) (BatchNorm moments included, as `deal` sets them all), then the loss heads
    {'prediction', 'label'} -> 'objective' (vl_nnsoftmaxceloss with T = 1 on probability targets for 'distributions',
    vl_nnloss softmaxlog otherwise) and classerror {'prediction', 'hardlabel'} -> 'classerror', and meta.classes."""
    if dropout and dropout > 0 and not any(isinstance(l.block, dagnn.DropOut) for l in net.layers):
        _dropout_after_last_convs(net, float(dropout))
    for l in net.layers[:-2]:
        for pname in l.params:
            net.params[pname].learningRate = float(finetuneLR)
    if lossType == "softmaxlog":
        layer, hard = dagnn.Loss("softmaxlog"), "label"
    elif lossType == "distributions":
        layer, hard = dagnn.SoftmaxCELoss(temperature=1, logitTargets=False), "hardlabel"
    else:
        raise ValueError("unrecognised loss: %s" % lossType)
    net.addLayer("loss", layer, ["prediction", "label"], "objective")
    net.addLayer("classerror", dagnn.Loss("classerror"), ["prediction", hard], "classerror")
    net.meta["classes"] = {"name": list(EMOTIONS), "description": list(EMOTIONS)}
    net._flat = None
    return net


def strip_losses(net):
    """fetch_emovoxceleb_imdb.m:101-106: remove every dagnn.Loss layer before inference."""
    names = [l.name for l in net.layers if isinstance(l.block, dagnn.LossBase)]
    net.removeLayer(names)
    return net


class FrozenTeacher:
    """The teacher loop of fetch_emovoxceleb_imdb.m:98-136 -- `dag.eval({in, data})` in test mode,
    logits = value of the last variable (:130) -- with the batch cut into `lanes` sample slices that
    run concurrently on `lanes` HIP streams (one DagNN replica per lane, parameters shared).
    A ResNet forward is a chain of ~55 dependent launches; with a single stream every launch pays its
    ramp-up and tail alone, two lanes fill each other's gaps (measured on MI355X: -7 % time at batch
    128, no gain at 32).  Samples are independent in test mode, so the logits are those of the
    single-lane evaluation up to the summation order of the tile configuration chosen per shape.
    `precision`: None leaves net.convPrecision as it is; 'fp32' / 'bf16x3' set it on the network and every lane's replica
    (dagnn.DagNN.convPrecision: the opt-in split-bf16 arm of the 1 x 1 layers).  self.precision is what the lanes run."""

    def __init__(self, net, lanes=2, output=None, precision=None):
        if net.mode != "test":
            raise ValueError("FrozenTeacher needs a test-mode network (fetch_emovoxceleb_imdb.m:107)")
        if precision not in (None, "fp32", "bf16x3"):
            raise ValueError("FrozenTeacher: precision is %r, expected None, 'fp32' or 'bf16x3'" % (precision,))
        if precision is not None:
            net.convPrecision = precision
        self.precision = net.convPrecision
        self.output = output or net.getOutputs()[-1]
        net.vars[self.output].precious = True
        self.nets = [net] + [net.replica() for _ in range(max(1, int(lanes)) - 1)]
        self.streams = [torch.cuda.Stream(device=net.device) for _ in self.nets] if len(self.nets) > 1 else []

    def logits(self, faces, input_name="data"):
        """faces: 224 x 224 x 3 x N mat -> 1 x 1 x numClasses x N mat."""
        N = int(faces.shape[3])
        L = len(self.nets)
        if L == 1 or N < 2 * L:
            self.nets[0].eval([input_name, faces])
            return self.nets[0].vars[self.output].value
        cur = torch.cuda.current_stream()
        bounds = [N * i // L for i in range(L + 1)]
        for i, (net, st) in enumerate(zip(self.nets, self.streams)):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                net.eval([input_name, faces[..., bounds[i]:bounds[i + 1]]])
        for st in self.streams:
            cur.wait_stream(st)
        outs = [net.vars[self.output].value for net in self.nets]
        C = int(outs[0].shape[2])
        out = vl.mat_empty((1, 1, C, N), device=faces.device)
        for i, o in enumerate(outs):
            out[..., bounds[i]:bounds[i + 1]].copy_(o)
        return out


# ---------------------------------------------------------------------------------------------
# emoVoxZoo (student)
# ---------------------------------------------------------------------------------------------
def prepareFromDagNN(net, numOutputs, seed=0):
    """emoVoxZoo.m:187-253: drop Loss / SoftMax layers, resize the last FC to numOutputs with
    1e-4 * randn filters (rng(0), :217-220), name the output 'prediction', input 'data'."""
    drop = [l.name for l in net.layers
            if isinstance(l.block, (dagnn.LossBase, dagnn.SoftMax))]
    net.removeLayer(drop)
    convs = [l for l in net.layers if isinstance(l.block, dagnn.Conv)]
    last = convs[-1]
    FH, FW, FC, _ = last.block.size
    last.block.size = (FH, FW, FC, numOutputs)
    rng = np.random.default_rng(seed)
    net.params[last.params[0]].value = np.asfortranarray(
        (1e-4 * rng.standard_normal((FH, FW, FC, numOutputs))).astype(np.float32))
    net.params[last.params[1]].value = np.zeros((numOutputs, 1), np.float32)
    net.renameVar(last.outputs[0], "prediction")
    inputs = net.getInputs()
    assert len(inputs) == 1, "expected a single-input network"  # emoVoxZoo.m:35
    if inputs[0] != "data":
        net.renameVar(inputs[0], "data")
    return net


def insert_dropout(net, prev, nxt, rate):
    """emoVoxZoo.m:272-277: a dagnn.DropOut named <prev>_drop between layer `prev` and its consumer `nxt`."""
    prec = net.layers[net.getLayerIndex(prev)]
    out = "%s_drop" % prev
    net.insertLayerAfter(prev, out, dagnn.DropOut(rate=rate, seed=net.getLayerIndex(prev) + 1), prec.outputs, out)
    nrec = net.layers[net.getLayerIndex(nxt)]
    net.setLayerInputs(nxt, [out if v == prec.outputs[0] else v for v in nrec.inputs])
    return net


def _dropout_after_last_convs(net, rate):
    """emoVoxZoo.m:116-135 / ferPlusZoo.m:213-232: a dropout layer behind each of convLayers(end-2:end-1)."""
    convs = [l for l in net.layers if isinstance(l.block, dagnn.Conv)]
    for sel in convs[-3:-1]:                      # convLayers(end-2:end-1): "reduce aggression"
        nxt = [l.name for l in net.layers if sel.outputs[0] in l.inputs]
        assert nxt, "target layer was not found"
        insert_dropout(net, sel.name, nxt[0], rate)
    return net


def configureForRegression(net, lossType, numOutputs, dropout=0):
    """emoVoxZoo.m:105-177 (the dropout layers of :116-135 first, then the loss heads)."""
    if dropout and dropout > 0 and not any(isinstance(l.block, dagnn.DropOut) for l in net.layers):
        _dropout_after_last_convs(net, float(dropout))
    if lossType == "softmaxlog":
        layer, inputs = dagnn.Loss("softmaxlog"), ["prediction", "maxLabel"]
    elif lossType == "hot-cross-ent":
        # emoVoxZoo.m:152 -- the temperature is hard-coded to 2 (opts.temperature only names
        # the experiment directory, run_distillation.m:85,102-104)
        layer, inputs = dagnn.SoftmaxCELoss(temperature=2, logitTargets=True), ["prediction", "logitTarget"]
    elif lossType == "euclidean":
        layer, inputs = dagnn.EuclideanLoss(), ["prediction", "logitTarget", "instanceWeights"]
        # emoVoxZoo.m:141-145: "scale down a lot to prevent exploding gradients" -- the filters of the
        # last layer are divided by 10
        p = net.params[net.layers[-1].params[0]]
        p.value = p.value / 10
        net.paramGeneration += 1   # (on the device: new storage for the filters)
    elif lossType == "huber":
        layer, inputs = dagnn.HuberLoss(sigma=1), ["prediction", "logitTarget", "instanceWeights"]
    else:
        raise ValueError("unrecognised regression loss: %s" % lossType)
    net.addLayer("loss", layer, inputs, "objective")
    net.addLayer("classerror", dagnn.VerboseLoss("classerror"), ["prediction", "maxLabel"], "classerror")
    net.addLayer("classAccs", dagnn.ErrorStats(numOutputs), ["prediction", "maxLabel"], "classAccs")
    net.meta.setdefault("classes", {})
    net.meta["classes"]["name"] = list(EMOTIONS)
    net.meta["classes"]["description"] = list(EMOTIONS)
    return net


def updatePooling(net, numSeconds):
    """emoVoxZoo.m:256-269: pool6.poolSize = [1 p1] for clips of `numSeconds` seconds."""
    width = int(round(100 * numSeconds))
    if width not in BUCKETS_WIDTH:
        raise ValueError("no pooling bucket for width %d" % width)
    p1 = BUCKETS_POOL[BUCKETS_WIDTH.index(width)]
    pools = [l for l in net.layers if l.name == "pool6"]
    assert len(pools) == 1, "expected a single pool6 layer"  # emoVoxZoo.m:268
    pools[0].block.poolSize = [1, p1]
    return net


def emoVoxZoo(modelName="emovoxceleb-student", scratch=1, lossType="hot-cross-ent", numSeconds=4,
              numOutputs=8, seed=200, width_mult=1.0, dropout=False, modelDir=None):
    """dag = emoVoxZoo(name, 'scratch', 1, 'lossType', 'hot-cross-ent', 'numSeconds', 4,
    'numOutputs', 8, 'dropout', rate) -- emoVoxZoo.m:1-62 (call site run_distillation.m:125-129).

    `modelDir` (the reference's option of that name, :22): read <modelDir>/<modelName>.mat instead of building the
    seeded stand-in.  scratch = 0 returns the file's network after fixInputVarnames (:41-48); scratch = 1 keeps its
    architecture only: prepareFromDagNN, initParams, configureForRegression, updatePooling (:50-62).  The two teacher
    names are accepted there as in the reference (:28-33).  A missing file raises FileNotFoundError."""
    if modelDir is not None:
        if modelName not in ("emovoxceleb-student", "vggvox-ver", "vggvox-ident") + tuple(FERPLUS_MODELS):
            raise ValueError("%s is not a recognised student model" % modelName)            # :33-35
        net = load_model(os.path.join(os.fspath(modelDir), modelName + ".mat"))                # :36-44
        if not scratch:
            return fixInputVarnames(net)                                                    # :45
        prepareFromDagNN(net, numOutputs)                                                   # :50
        net.initParams(seed)                                                                # :54
        configureForRegression(net, lossType, numOutputs, dropout)                          # :57-58
        updatePooling(net, numSeconds)                                                      # :61
        return fixInputVarnames(net)                                                        # :62
    if modelName not in ("emovoxceleb-student", "vggvox-ver", "vggvox-ident"):
        raise ValueError("%s is not a recognised student model" % modelName)
    net = vggvox(1251, width_mult)
    net.initParams(seed)               # stands in for the downloaded weights
    if scratch:
        prepareFromDagNN(net, numOutputs)
        net.initParams(seed)           # emoVoxZoo.m:54: re-randomise everything
        configureForRegression(net, lossType, numOutputs, dropout)
    else:
        prepareFromDagNN(net, numOutputs)
    updatePooling(net, numSeconds)
    net.meta["modelName"] = modelName
    return net


def inference_student(modelName, modelDir=None):
    """the student the evaluation drivers build when none is passed (external/compute_audio_feats.m:52, emoVoxZoo(opts.modelName)):
    the seeded stand-in, or with `modelDir` the network of <modelDir>/<modelName>.mat with its weights (scratch = 0)"""
    if modelDir is None:
        return emoVoxZoo(modelName)
    return emoVoxZoo(modelName, scratch=0, modelDir=modelDir)


def ensure_compatibility(modelDir):
    """misc/ensure_compatibility.m: every public model found in `modelDir` is loaded, the `exBackprop` field is taken out
    of its block structs (MatConvNet versions before that property refuse it) and the struct is saved back in place,
    at the top level of the file (save(modelPath, '-struct', 'net')).  Nothing else in the file changes: the struct is
    rewritten as read, not through loadobj / saveobj.  A model without a file is skipped (the reference fails there).
    Returns the paths written."""
    from . import matfile
    written = []
    for modelName in PUBLIC_MODELS:
        path = os.path.join(os.fspath(modelDir), modelName + ".mat")
        if not os.path.isfile(path):
            continue
        net = matfile.read_mat(path)
        if "net" in net:
            net = net["net"][0, 0]
            net = {f: net[f] for f in net.dtype.names}
        layers = net.get("layers")
        if layers is not None and layers.size and "block" in (layers.dtype.names or ()):
            for idx in np.ndindex(*layers.shape):
                b = layers[idx]["block"]
                if isinstance(b, np.ndarray) and b.dtype.names and "exBackprop" in b.dtype.names:
                    keep = [f for f in b.dtype.names if f != "exBackprop"]
                    nb = np.empty(b.shape, dtype=[(f, object) for f in keep])
                    for j in np.ndindex(*b.shape):
                        nb[j] = tuple(b[j][f] for f in keep)
                    layers[idx]["block"] = nb if keep else np.array([[None]], object)
        matfile.write_mat(path, matfile.rewritable(net))
        written.append(path)
    return written
