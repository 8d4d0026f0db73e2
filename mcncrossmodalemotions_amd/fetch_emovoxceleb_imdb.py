"""fetch_emovoxceleb_imdb mirror (emoVoxCeleb/fetch_emovoxceleb_imdb.m): the imdb whose wavLogits the student distils from.

    imdb = fetch_emovoxceleb_imdb('senet50-ferplus')

The reference runs the frozen teacher over every dense face frame of VoxCeleb, 128 at a time, stores
`logits(batch, :) = out'` and splits the rows per wav into imdb.wavLogits (:119-148).  Same flow here, on the device:

    addFramesToImdb (:196-285)   frames listed per track, frameless tracks removed from every images field, unclaimed
                                 frames dropped, images.denseFrames / images.denseFramesWavIds set
    buildImdb (:54-149)          losses stripped, test mode, one input; per batch: decoded frames -> vl.crop_resize_face
                                 (getImageBatch, :152-193) -> FrozenTeacher.logits -> xm_scatter_rows into ONE device
                                 matrix; nothing is synchronised or downloaded inside the loop (the reference gathers
                                 every batch, :130).  Then xm_group_rows over images.id(1:min(numWavs, limit)) (:140-147),
                                 one regrouping (xm_gather_rows + xm_scatter_rows) into the concatenated matrix that
                                 device_logits() hands to xm_aggregate_logits, and ONE download for the host cell.
    fetch_emovoxceleb_imdb (:1-51)  <imdbDir>/<teacher>-logits.mat, read / written with scipy, and a module-level cache

What differs, because there is neither the dataset nor MATLAB here:
  * the source imdb (voxceleb-imdb.mat, :84) is src_imdb(batch.SyntheticEmoVoxImdb(...)); the frame files and their
    pixels come from batch.SyntheticDenseFrames (`lister`, `find`, decoded frames);
  * the 5,078,961 assertion (:223) is the optional `expectFrames`;
  * the reference keys its cache on `opts` alone (:19), so a second teacher is handed the first one's imdb; the key here
    is (teacher, imdbDir);
  * fetchImdbFromInternet (:288-324) is not mirrored: nothing here opens a network connection, a missing file means
    "build";
  * `teacher` of buildImdb is a network (or any object with .logits(faces)), not a name: ferPlusZoo's weights are
    seeded stand-ins, so the caller says which network it means.
Extensions are keyword-only.
"""
import copy
import math
import os

import numpy as np
import torch

from . import batch as xbatch
from . import vl, zoo

NUM_EMOTIONS = 8                 # :64
AVERAGE_IMAGE = (131.0912, 103.8827, 91.4953)


class EmoVoxImdb(xbatch.SyntheticEmoVoxImdb):
    """The imdb struct of the reference: `images` (one entry per wav in every field: name, video, track, id, set,
    numSamples; after addFramesToImdb also the per-frame lists denseFrames / denseFramesWavIds) and, once built,
    `wavLogits`.  It answers what getBatchEmoVoxCeleb, run_distillation, student_stats and teacher_stats ask of a
    batch.SyntheticEmoVoxImdb (set, num_samples, fs, wavLogits, device_wav, device_noise, device_logits)."""

    PER_FRAME = ("denseFrames", "denseFramesWavIds")

    def __init__(self, images, fs=16000, seed=0, wavLogits=None, precision="fp32"):
        self.images, self.fs, self.seed = images, int(fs), int(seed)
        self.wavLogits = wavLogits
        self.precision = precision       # the arithmetic of the teacher that wrote wavLogits (buildImdb teacherPrecision)
        self._dev = None

    set = property(lambda self: np.asarray(self.images["set"]))
    num_samples = property(lambda self: np.asarray(self.images["numSamples"]))

    def device_wav(self, ii, device):
        """synthetic waveform of track ii, seeded by the track's id: dropping other tracks does not change it"""
        cache = self.__dict__.setdefault("_wav", {})
        if ii not in cache:
            g = torch.Generator(device=device)
            g.manual_seed(self.seed * 100003 + int(self.images["id"][ii]) - 1)
            cache[ii] = torch.randn(int(self.num_samples[ii]), generator=g, device=device, dtype=torch.float32) * 0.1
        return cache[ii]


def src_imdb(syn):
    """stand-in for voxceleb-imdb.mat (:84) with the fields addFramesToImdb reads (:241-245), from the sizes of a
    batch.SyntheticEmoVoxImdb: one celebrity / video / track per wav, ids 1..N."""
    N = len(syn.num_samples)
    ids = np.arange(1, N + 1)
    images = {"name": ["id%05d/video%05d/%05d.wav" % (i, i, 1) for i in ids], "video": ["video%05d" % i for i in ids],
              "track": np.ones(N, int), "id": ids, "set": np.asarray(syn.set).copy(),
              "numSamples": np.asarray(syn.num_samples).copy()}
    return EmoVoxImdb(images, fs=syn.fs, seed=syn.seed)


def addFramesToImdb(imdb, lister, *, find=None, expectFrames=None):
    """imdb = addFramesToImdb(imdb, faceDir) -- :196-285.  `lister(track) -> list of relative frame paths` stands for
    zs_getImgsInDir(fullfile(faceDir, celeb, '1.6', video, num2str(track)), 'jpg') (:246-247); `find() -> all frame
    paths` for the `find` call whose count sizes the arrays (:209-222; default: the listed frames); `expectFrames` for
    the assertion on that count (:223).  Frames are numbered in track order, wavIds is the 1-based index of the track
    (:249); the slots the tracks do not claim keep id 0 and are dropped (:270-273); tracks without frames are removed
    from every images field (:261-268).  Returns a new imdb; the argument is not modified."""
    images = imdb.images
    numWavs = len(images["name"])
    framePaths, wavIds = [], []
    for ii in range(numWavs):                                                            # :239-259
        track = {k: images[k][ii] for k in images if k not in EmoVoxImdb.PER_FRAME}
        frames = list(lister(track))
        wavIds += [ii + 1] * len(frames)
        framePaths += frames
    numIms = len(find()) if find is not None else len(framePaths)                        # :209-222
    if expectFrames is not None:
        assert numIms == int(expectFrames), "unexpected number of face images"          # :223
    if numIms < len(framePaths):
        raise ValueError("find reports %d frames, the tracks list %d" % (numIms, len(framePaths)))
    wavIds = np.asarray(wavIds + [0] * (numIms - len(framePaths)), dtype=np.int64)        # zeros(numIms, 1), :236
    framePaths = framePaths + [None] * (numIms - len(framePaths))
    withFrames = np.unique(wavIds)                                                       # :262-268
    keep = np.isin(np.arange(1, numWavs + 1), withFrames)
    out = {}
    for k, v in images.items():
        if k in EmoVoxImdb.PER_FRAME:
            continue
        out[k] = [x for x, m in zip(v, keep) if m] if isinstance(v, list) else np.asarray(v)[keep]
    claimed = wavIds != 0                                                                # :270-273
    out["denseFrames"] = [p for p, m in zip(framePaths, claimed) if m]                   # already relative (:275-283)
    out["denseFramesWavIds"] = wavIds[claimed]
    new = copy.copy(imdb)
    new.images, new.wavLogits, new._dev = out, None, None
    new.__dict__.pop("_wav", None)
    return new


def check_precision(precision, who):
    if precision not in (None, "fp32", "bf16x3"):
        raise ValueError("%s: teacher precision is %r, expected None, 'fp32' or 'bf16x3'" % (who, precision))
    return precision


def _as_teacher(teacher, lanes, precision=None):
    """:98-110: strip the losses, test mode, a single input, on the device -> (object with .logits, imageSize, avg).
    `precision` (None: as the teacher stands) goes to zoo.FrozenTeacher; an object that already has .logits keeps its own
    and must not contradict the one asked for."""
    check_precision(precision, "teacher")
    if hasattr(teacher, "logits"):
        own = getattr(teacher, "precision", "fp32")
        if precision is not None and precision != own:
            raise ValueError("the teacher object runs at precision %r, %r was asked for" % (own, precision))
        return (teacher, tuple(getattr(teacher, "imageSize", (224, 224)))[:2],
                getattr(teacher, "averageImage", AVERAGE_IMAGE))
    zoo.strip_losses(teacher)                                                            # :101-106
    teacher.mode = "test"                                                                # :107
    inVars = teacher.getInputs()
    assert len(inVars) == 1, "too many inputs"                                           # :109-110
    if teacher.device is None:
        teacher.move("gpu")                                                              # :108
    norm = teacher.meta["normalization"]
    return zoo.FrozenTeacher(teacher, lanes=lanes, precision=precision), tuple(norm["imageSize"][:2]), norm["averageImage"]


def read_files(faceDir):
    """the default `read` of getImageBatch: paths -> the bytes of fullfile(faceDir, path) (:127)"""
    def read(paths):
        out = []
        for p in paths:
            with open(os.path.join(faceDir, p), "rb") as fh:
                out.append(fh.read())
        return out
    return read


def getImageBatch(imagePaths, dag, *, read=None, faceDir=os.path.join("data", "voxceleb", "faces"), device=None,
                  split=None, progressive=False, interpolation=None, antialias=False, crop_size=1 / 1.6):
    """data = getImageBatch(imagePaths, dag) -- :152-193: vl_imreadjpeg with CropSize 1/1.6, CropLocation center,
    bilinear Resize to meta.normalization.imageSize (:160-172), rgb2gray, x3 and normalizeFace (:176-193), all on the
    device from the files' bytes (vl.imreadjpeg).  `read(paths) -> list of bytes` (default: the files under faceDir);
    `dag`: a network with meta.normalization, or an object with .imageSize / .averageImage.  Ho x Wo x 3 x n; nothing
    is synchronised.  `split`: vl.imreadjpeg's seg_bytes (the segment-parallel entropy decode; the same faces).
    `progressive`: vl.imreadjpeg's option of that name -- progressive files are read too, as vl_imreadjpeg reads them.
    `interpolation` ('box' | 'bilinear' | 'bicubic'; None: the path above, unchanged) picks the filter: the frames then go
    through vl.vl_imreadjpeg(..., 'Resize', imageSize, 'CropLocation', 'center', 'CropSize', crop_size) with `antialias`
    as given, are rounded to uint8 values as the path above rounds them, and vl.normalize_face does the rest -- the path
    for frames larger than the network's input (AFEW-sized frames, which are already tightly cropped: crop_size=1)."""
    if progressive and split is not None:
        raise ValueError("getImageBatch: progressive=True and split= exclude each other (vl.imreadjpeg)")
    if hasattr(dag, "meta"):
        imageSize, avg = tuple(dag.meta["normalization"]["imageSize"][:2]), dag.meta["normalization"]["averageImage"]
    else:
        imageSize, avg = tuple(getattr(dag, "imageSize", (224, 224)))[:2], getattr(dag, "averageImage", AVERAGE_IMAGE)
    read = read or read_files(faceDir)
    if interpolation is not None:
        rgb = vl.vl_imreadjpeg(read(list(imagePaths)), "Pack", "Resize", list(imageSize), "CropLocation", "center", "CropSize",
                               crop_size, "Interpolation", interpolation, "NumThreads", 10, antialias=antialias,
                               device=device, split=split, progressive=progressive)
        return vl.normalize_face(vl.uint8_round(rgb), avg)
    return vl.imreadjpeg(read(list(imagePaths)), resize=imageSize, crop_size=1 / 1.6, crop_location="center",
                         interpolation="bilinear", pack=True, num_threads=10, average_image=avg, device=device,
                         split=split, progressive=progressive)


class _Norm:
    def __init__(self, imageSize, averageImage):
        self.imageSize, self.averageImage = imageSize, averageImage


def buildImdb(teacher, imdb, frames=None, *, read=None, limit=math.inf, batchSize=128, lanes=2, device=None,
              split=None, progressive=False, teacherPrecision=None):
    """imdb = buildImdb(teacher) -- :54-149, for an imdb that went through addFramesToImdb.  `teacher`: a ferPlusZoo
    network (losses are stripped, test mode, one input: :101-110) or any object with .logits(faces) -> 1 x 1 x E x n;
    `frames(paths, device)` -> the decoded frames Hin x Win x 3 x n (0..255), what vl_imreadjpeg returns for
    fullfile(faceDir, denseFrames(batch)) (:127,160-172).  Returns a new imdb with
      wavLogits        host list, one F_i x E float32 array per wav (empty past `limit`), downloaded once;
      device_logits()  the same rows concatenated on the device, already in place.
    With `read(paths) -> list of bytes` instead of `frames` the batch comes from getImageBatch: the JPEG files are
    decoded on the device (frames of any sizes in one batch); `split` and `progressive` go to getImageBatch.
    `teacherPrecision` (None | 'fp32' | 'bf16x3'): zoo.FrozenTeacher's precision; the imdb records what ran (.precision).
    The loop enqueues work only; it neither synchronises nor downloads."""
    if progressive and split is not None:
        raise ValueError("buildImdb: progressive=True and split= exclude each other (vl.imreadjpeg)")
    check_precision(teacherPrecision, "buildImdb")
    if (frames is None) == (read is None):
        raise ValueError("buildImdb: give either `frames` (decoded pixels) or `read` (JPEG bytes)")
    if (split is not None or progressive) and read is None:
        raise ValueError("buildImdb: `split` and `progressive` belong to the device JPEG decode, which needs `read`")
    if not torch.cuda.is_available():
        raise RuntimeError("buildImdb needs a GPU; this build has no CPU path")
    device = device or torch.device("cuda", torch.cuda.current_device())
    images = imdb.images
    model, imageSize, avg = _as_teacher(teacher, lanes, teacherPrecision)
    wavIds = np.asarray(images["denseFramesWavIds"], dtype=np.int64)
    ids = np.asarray(images["id"], dtype=np.int64)
    # compute for the first `limit` tracks (:112-115).  The reference is asymmetric and this keeps it: the frames of the
    # tracks with id <= firstId + limit are evaluated -- limit + 1 tracks when the ids are consecutive -- while only the
    # first min(numWavs, limit) cells are filled (:142); the rows of the extra track are computed and then dropped.
    firstId = int(ids[0])
    numKeep = int((wavIds <= firstId + limit).sum())
    numIms = min(len(images["denseFrames"]), numKeep)
    E, logits = NUM_EMOTIONS, None
    for start in range(0, numIms, int(batchSize)):                                       # :122-136
        batch = range(start, min(start + int(batchSize), numIms))
        paths = [images["denseFrames"][i] for i in batch]
        if read is not None:
            faces = getImageBatch(paths, _Norm(imageSize, avg), read=read, device=device, split=split,
                                  progressive=progressive)                               # :152-193
        else:
            data = frames(paths, device)                                                 # vl_imreadjpeg (:160-172)
            faces = vl.crop_resize_face(data, avg, imageSize)                            # getImageBatch (:152-193)
        out = model.logits(faces)                                                        # dag.eval, vars(end) (:129-130)
        if logits is None:
            # zeros(numIms, numEmotions) (:119), as wide as the teacher's output: the FER teachers have 7 classes, not the
            # 8 that :64 writes down for the FER+ ones
            E = int(out.shape[2])
            logits = vl.mat_zeros(numIms, E, device=device)
        vl.scatter_rows(out, logits, row0=start)                                         # logits(batch, :) = out' (:131)
    if logits is None:
        logits = vl.mat_zeros(1, E, device=device)
    numWavs = len(images["name"])
    numLogits = int(min(numWavs, limit))                                                 # :140-142
    dids = torch.from_numpy(wavIds[:numIms].astype(np.int32)).to(device)
    key_max = int(max(ids.max(), wavIds.max() if wavIds.size else 0))
    offsets, rows, nnz = vl.group_rows(dids, ids[:numLogits], key_max)                   # :143-147, all cells at once
    h_off = offsets.cpu().numpy().astype(np.int64)                                       # the first wait for the device
    kept = int(h_off[-1])
    grouped = vl.mat_zeros(max(kept, 1), E, device=device)
    if kept:
        vl.scatter_rows(vl.gather_rows(logits, rows[:kept]), grouped)
    host = vl.to_numpy(grouped)[:kept]                                                   # the one download of logits
    cells = [np.asfortranarray(host[h_off[i]:h_off[i + 1]]) for i in range(numLogits)]
    cells += [np.zeros((0, E), np.float32, order="F") for _ in range(numWavs - numLogits)]   # [] cells past limit (:141)
    new = copy.copy(imdb)
    new.wavLogits = cells
    new.precision = getattr(model, "precision", "fp32")
    new._dev = (grouped, np.concatenate([h_off, np.full(numWavs - numLogits, kept, np.int64)]))
    return new


# ---- fetch_emovoxceleb_imdb (:1-51) -----------------------------------------------------------------------------------
_CACHE = {}          # (teacher, imdbDir) -> imdb; upstream: `global imdb`, validated against `opts` only (:16-19)


def getImdbPath(imdbDir, teacher):
    """:45-51"""
    return os.path.join(imdbDir, "%s-logits.mat" % teacher)


def save_imdb(path, imdb):
    """save(imdbPath, '-struct', 'imdb') (:32): images as a struct, wavLogits as a 1 x N cell"""
    from scipy.io import savemat
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    images = {}
    for k, v in imdb.images.items():
        images[k] = np.array(v, dtype=object).reshape(1, -1) if isinstance(v, list) else np.asarray(v).reshape(1, -1)
    cell = np.empty((1, len(imdb.wavLogits)), dtype=object)
    for i, l in enumerate(imdb.wavLogits):
        cell[0, i] = np.asarray(l, dtype=np.float32)
    savemat(path, {"images": images, "wavLogits": cell, "fs": imdb.fs, "seed": imdb.seed,
                   "precision": getattr(imdb, "precision", "fp32")})


def load_imdb(path):
    """imdb = load(imdbPath) (:26)"""
    from scipy.io import loadmat
    m = loadmat(path)
    rec = m["images"][0, 0]
    images = {}
    for k in rec.dtype.names:
        v = rec[k].reshape(-1)
        images[k] = [str(x.reshape(-1)[0]) if x.size else "" for x in v] if v.dtype == object else v.astype(np.int64)
    E = NUM_EMOTIONS
    cells = [np.asarray(c, dtype=np.float32) for c in m["wavLogits"].reshape(-1)]
    E = next((int(c.shape[1]) for c in cells if c.ndim == 2 and c.size), E)          # the width the teacher wrote
    wav = [np.asfortranarray(c.reshape(-1, E)) for c in cells]
    # (a file from before the field existed was written by the fp32 teacher)
    precision = str(np.asarray(m["precision"]).reshape(-1)[0]).strip() if "precision" in m else "fp32"
    return EmoVoxImdb(images, fs=int(m["fs"].ravel()[0]), seed=int(m["seed"].ravel()[0]), wavLogits=wav,
                      precision=precision)


def require_precision(imdb, wanted, where):
    """a cache of teacher logits is good for ONE arithmetic: mixing the targets of two silently is what this refuses"""
    have = getattr(imdb, "precision", "fp32")
    if have != wanted:
        raise ValueError("%s holds teacher logits computed at precision %r, but %r was asked for: use another imdbDir, "
                         "or ask for teacherPrecision=%r" % (where, have, wanted, have))
    return imdb


def fetch_emovoxceleb_imdb(teacher="senet50-ferplus", imdbDir=os.path.join("data", "xEmo18", "storedFeats"), *,
                           net=None, imdb=None, frames=None, read=None, split=None, progressive=False, verbose=True,
                           modelDir=None, teacherPrecision=None,
                           **buildOpts):
    """loadedImdb = fetch_emovoxceleb_imdb(teacher, 'imdbDir', ..) -- :1-51: the cached imdb of (teacher, imdbDir), else
    <imdbDir>/<teacher>-logits.mat when it exists, else buildImdb and save.  Building needs (keyword-only) `net` (default
    zoo.ferPlusZoo(teacher, modelDir=modelDir): with `modelDir` the teacher's model file), `imdb` (an imdb that went through addFramesToImdb; default a 64-track synthetic one) and
    `frames` or `read` (with `split` or `progressive`, as buildImdb); buildOpts go to buildImdb (limit, batchSize, lanes).  A loaded
    imdb uploads its logits on first use.
    The cache key and the file name hold the teacher's NAME and imdbDir, nothing else: a later call with another
    `net`, `imdb`, `frames` or `limit` under the same name and directory gets the first build back, from the module
    cache or from the file.  Use another imdbDir (or call buildImdb) for a different build.
    `teacherPrecision` (None = 'fp32' | 'bf16x3'): the arithmetic of the teacher's 1 x 1 layers (buildImdb).  The file
    records it in a `precision` field (a file without the field counts as 'fp32'); a cached or stored imdb written at
    another precision than the one asked for raises ValueError naming both."""
    if progressive and split is not None:
        raise ValueError("fetch_emovoxceleb_imdb: progressive=True and split= exclude each other (vl.imreadjpeg)")
    wanted = check_precision(teacherPrecision, "fetch_emovoxceleb_imdb") or "fp32"
    key = (str(teacher), os.path.abspath(imdbDir))
    if key in _CACHE:                                                                    # :19-20
        if verbose:
            print("found imdb in cache, re-using..", flush=True)
        return require_precision(_CACHE[key], wanted, "the imdb cached for %s" % (key,))
    imdbPath = getImdbPath(imdbDir, teacher)
    if os.path.exists(imdbPath):                                                         # :24-27
        if verbose:
            print("loading imdb ...", flush=True)
        loaded = require_precision(load_imdb(imdbPath), wanted, imdbPath)
    else:                                                                                # :28-34
        if verbose:
            print("generating imdb (this will take a long time)...", flush=True)
        if imdb is None:
            syn = xbatch.SyntheticEmoVoxImdb(num_tracks=64, val_fraction=0.25, heard_fraction=0.125)
            src = src_imdb(syn)
            frames = frames or xbatch.SyntheticDenseFrames(src)
            imdb = addFramesToImdb(src, frames.lister, find=frames.find)
        if frames is None and read is None:
            raise ValueError("fetch_emovoxceleb_imdb: building needs `frames` for the given imdb")
        loaded = buildImdb(net if net is not None else zoo.ferPlusZoo(teacher, modelDir=modelDir), imdb,
                           frames if read is None else None,
                           read=read, split=split, progressive=progressive, teacherPrecision=wanted, **buildOpts)
        save_imdb(imdbPath, loaded)
    _CACHE[key] = loaded
    return loaded
