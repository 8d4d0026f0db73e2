"""Feature-extraction drivers of the reference's evaluation code (`external/`), device side.

    compute_audio_feats   external/compute_audio_feats.m:96-136,160-185
        variable-width student inference: per clip, row-normalise the whole spectrogram, centre-crop to
        the largest bucket width <= T, resize `pool6` to that bucket, one test-mode forward.
    compute_audio_feats_wav  the same from the waveform bank: audio_feats_plan on the host, then per bucket one
        xm_spec_bucket_batch call (whole-clip STFT, row statistics, crop) and one forward.
    compute_audio_feats_files  the same from the WAV files: vl.audioread (channel 0) into the bank, then the above.
    compute_visual_feats  external/compute_visual_feats.m:60-116
        frozen teacher over the flattened frames of all tracks in minibatches, logits split per track.

The .mat imdb stays outside: the functions take device tensors (spectrogram magnitudes 512 x T, the
waveform bank, normalised faces 224 x 224 x 3 x F) or, through compute_audio_feats_files / compute_visual_feats(read=...),
the bytes of the WAV / JPEG files, which are decoded on the device.
"""
import math

import numpy as np
import torch

from . import dagnn, vl, zoo

BUCKETS_POOL = list(zoo.BUCKETS_POOL)     # compute_audio_feats.m:45-46
BUCKETS_WIDTH = list(zoo.BUCKETS_WIDTH)


def _matlab_round(x):
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def test_getinput(spec):
    """compute_audio_feats.m:160-185 minus file reading: mean/std normalisation of every frequency row
    over the WHOLE clip, then the centre crop to the largest bucket width that fits.
    spec: 512 x T device mat.  Returns (512 x rsize mat, rsize)."""
    T = int(spec.shape[1])
    fits = [w for w in BUCKETS_WIDTH if w <= T]
    if not fits:
        raise ValueError("empty audio clip: %d frames, the smallest bucket needs %d" % (T, BUCKETS_WIDTH[0]))
    rsize = fits[-1]
    n = vl.spec_rownorm(spec[:, :, None, None] if spec.dim() == 2 else spec)   # 512 x T x 1 x 1 view
    rstart = _matlab_round((T - rsize) / 2.0)
    if rstart == 0:
        rstart = 1                                   # 1-based, :183
    s0 = rstart - 1
    if s0 + rsize > T:                               # cannot happen for the bucket table; guard anyway
        s0 = T - rsize
    return n[:, s0:s0 + rsize], rsize


def _student(dag, modelDir):
    """compute_audio_feats.m:52 `dag = emoVoxZoo(opts.modelName)`: a model name instead of a network builds the zoo's (from
    <modelDir>/<name>.mat when `modelDir` is given)"""
    return zoo.inference_student(dag, modelDir) if isinstance(dag, str) else dag


def _prepare(dag):
    names = [l.name for l in dag.layers if isinstance(l.block, dagnn.LossBase)]   # :98-103
    if names:
        dag.removeLayer(names)
    dag.mode = "test"
    dag.move("gpu")
    ins = dag.getInputs()
    if len(ins) != 1:
        raise ValueError("too many inputs")          # :108
    return ins[0], dag.getLayerIndex("pool6")


class _GraphedEval:
    """One HIP graph per (bucket width, batch) shape of the student forward: a batch-1 forward is ~25
    launches of a few microseconds each -- launch-bound from Python (0.65 ms per clip) -- so the chain is
    captured once (torch.cuda.CUDAGraph drives hipStreamBeginCapture / hipGraphLaunch; the library's
    kernels are enqueued on the capturing stream like any other) and replayed per clip: copy the
    spectrogram into the static input, one graph launch.  Shapes are warmed up before capture so that the
    tile autotuner and the workspace / tap-table allocations have settled."""

    def __init__(self, dag, inp, out_name):
        self.dag, self.inp, self.out_name = dag, inp, out_name
        self.graphs = {}
        self.ws_generation = None

    def run(self, x, p1, ind1):
        from . import _lib
        L = _lib.load()
        # The library's scratch is ONE grow-only buffer per stream and every graph is captured on the same side
        # stream: warming up a larger shape may move that buffer (the old one is freed), and a graph captured
        # earlier would then write its split-K slabs / padded filters / bnorm partial sums to freed memory.  The
        # generation counter moves with every growth: all graphs captured before it are dropped and re-captured.
        gen = int(L.xm_workspace_generation())
        if self.ws_generation is not None and gen != self.ws_generation:
            self.graphs.clear()
        key = (tuple(int(v) for v in x.shape), p1)
        ent = self.graphs.get(key)
        if ent is None:
            self.dag.layers[ind1].block.poolSize = [1, p1]
            static_in = vl.mat_empty(*x.shape, device=x.device)
            static_in.copy_(x)
            side = self.__dict__.setdefault("_stream", torch.cuda.Stream(device=x.device))
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):                      # warm-up: tuning, workspace growth, tap tables
                    self.dag.eval([self.inp, static_in])
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # capture on the stream that was warmed up: the library's scratch buffer is per stream, and a
            # first use on a fresh stream would hipMalloc inside the capture
            with torch.cuda.graph(g, stream=side):
                self.dag.eval([self.inp, static_in])
                static_out = self.dag.vars[self.out_name].value
            if int(L.xm_workspace_generation()) != gen:
                # the warm-up of THIS shape grew the scratch: every older graph points at the freed buffer
                for k in [k for k in self.graphs if k != key]:
                    del self.graphs[k]
            ent = self.graphs[key] = (g, static_in, static_out)
            self.ws_generation = int(L.xm_workspace_generation())
        g, static_in, static_out = ent
        static_in.copy_(x)
        g.replay()
        return static_out.clone()


def compute_audio_feats(dag, specs, numEmotions=8, batch_by_bucket=False, use_graphs=False, *, modelDir=None):
    """logits = compute_audio_feats(dag, specs): one row of `numEmotions` logits per clip.

    specs: list of 512 x T spectrogram-magnitude device tensors (any T >= 100).
    batch_by_bucket (extension): clips that fall into the same width bucket are evaluated as ONE
    minibatch instead of one launch chain per clip -- same logits (test-mode BN, samples independent),
    far fewer launches.
    use_graphs (extension): the forward of every (bucket, batch) shape is captured into a HIP graph once
    and replayed -- same kernels, same results, no per-layer launch cost.
    `dag` may be a model name, as upstream (:52): zoo.emoVoxZoo builds it, from `modelDir` when that is given."""
    dag = _student(dag, modelDir)
    inp, ind1 = _prepare(dag)
    if ind1 is None:
        raise ValueError("the audio model has no pool6 layer")
    out_name = list(dag.vars)[-1]                    # "risky use of end variable", :127
    dag.vars[out_name].precious = True
    logits = np.zeros((len(specs), numEmotions), np.float32)
    pending = []                                     # (clip indices, device logits) -- read back once
    graphed = None
    if use_graphs:
        graphed = dag.__dict__.get("_graphed_eval")
        if graphed is None or graphed.out_name != out_name:
            graphed = dag.__dict__["_graphed_eval"] = _GraphedEval(dag, inp, out_name)
    prepared = [test_getinput(s) for s in specs]
    if batch_by_bucket:
        groups = {}
        for i, (_, rsize) in enumerate(prepared):
            groups.setdefault(rsize, []).append(i)
        work = [(idx, rsize) for rsize, idx in sorted(groups.items())]
    else:
        work = [([i], prepared[i][1]) for i in range(len(specs))]
    for idx, rsize in work:
        p1 = BUCKETS_POOL[BUCKETS_WIDTH.index(rsize)]
        dag.layers[ind1].block.poolSize = [1, p1]    # :119
        if len(idx) == 1:
            x = prepared[idx[0]][0]                  # a column range of a column-major mat: contiguous
        else:
            x = vl.mat_empty(int(prepared[idx[0]][0].shape[0]), rsize, 1, len(idx), device=prepared[idx[0]][0].device)
            for k, i in enumerate(idx):
                x[:, :, :, k].copy_(prepared[i][0][:, :, :, 0])
        if graphed is not None:
            pending.append((idx, graphed.run(x, p1, ind1)))
            continue
        dag.eval([inp, x])
        pending.append((idx, dag.vars[out_name].value))
    for idx, val in pending:
        out = vl.to_numpy(val).reshape(-1, len(idx), order="F")   # squeeze: E x N
        logits[idx, :] = out.T[:, :numEmotions]
    return logits


def audio_feats_plan(lengths, offsets, fs=16000, Tw=25, Ts=10):
    """The host side of compute_audio_feats_wav; touches no device.  lengths / offsets: samples and first sample in the
    waveform bank of every clip.  Per clip T = floor((len - Nw) / Ns) + 1, the bucket (largest BUCKETS_WIDTH <= T;
    compute_audio_feats.m:181) and the first frame of the centre crop f0 = rstart - 1, rstart = round((T - rsize) / 2)
    with halves rounded away from zero and 0 turned into 1 (:182-183).  Returns (T, rsize, f0, groups): three int64
    arrays and groups = [(rsize, clip indices, desc)] in ascending bucket order, clip order kept inside a bucket, desc
    the N x 3 {src, len, f0} table of vl.spec_bucket_batch.  A clip with fewer frames than the smallest bucket raises
    the ValueError of test_getinput."""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    offsets = np.asarray(offsets, np.int64).reshape(-1)[:lengths.size]
    if offsets.size != lengths.size:
        raise ValueError("audio_feats_plan: one offset per clip is required")
    Nw, Ns = int(round(1e-3 * Tw * fs)), int(round(1e-3 * Ts * fs))
    T = np.where(lengths >= Nw, (lengths - Nw) // Ns + 1, 0).astype(np.int64)
    widths = np.asarray(BUCKETS_WIDTH, np.int64)
    if T.size and T.min() < widths[0]:
        raise ValueError("empty audio clip: %d frames, the smallest bucket needs %d" % (int(T.min()), int(widths[0])))
    rsize = widths[np.searchsorted(widths, T, side="right") - 1] if T.size else np.zeros(0, np.int64)
    rstart = (T - rsize + 1) // 2
    f0 = np.maximum(rstart, 1) - 1
    groups = []
    for w in np.unique(rsize):
        idx = np.nonzero(rsize == w)[0]
        groups.append((int(w), idx, np.stack([offsets[idx], lengths[idx], f0[idx]], 1)))
    return T, rsize, f0, groups


def compute_audio_feats_wav(dag, wav, offsets, numEmotions=8, limit=float("inf"), maxBatch=64, *, modelDir=None):
    """logits = compute_audio_feats from the waveforms (compute_audio_feats.m:91-136,160-185): `wav` is the device bank
    of all clips back to back, `offsets` their first samples plus the bank's length (imdb.device_wav_bank).  The clips
    are planned on the host (audio_feats_plan); per bucket and chunk of `maxBatch` clips ONE vl.spec_bucket_batch call
    makes the normalised, cropped 512 x rsize x 1 x n input and ONE test-mode forward with pool6 resized follows.  The
    logits are read back once at the end.  `limit`: only the clips with id <= firstId + limit are processed (:91-93;
    ids 1, 2, ...: the first limit + 1 clips).  `dag` / `modelDir` as in compute_audio_feats."""
    dag = _student(dag, modelDir)
    inp, ind1 = _prepare(dag)
    if ind1 is None:
        raise ValueError("the audio model has no pool6 layer")
    out_name = list(dag.vars)[-1]                    # "risky use of end variable", :127
    dag.vars[out_name].precious = True
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    numKeep = offsets.size - 1
    if limit != float("inf"):
        numKeep = max(0, min(numKeep, int(limit) + 1))
    lengths = np.diff(offsets)[:numKeep]
    _, _, _, groups = audio_feats_plan(lengths, offsets[:numKeep])
    logits = np.zeros((numKeep, numEmotions), np.float32)
    pending = []                                     # (clip indices, device logits) -- read back once
    maxBatch = max(1, int(maxBatch))
    for rsize, idx, desc in groups:
        dag.layers[ind1].block.poolSize = [1, BUCKETS_POOL[BUCKETS_WIDTH.index(rsize)]]    # :119
        for s in range(0, len(idx), maxBatch):
            x = vl.spec_bucket_batch(wav, desc[s:s + maxBatch], rsize)
            dag.eval([inp, x])
            pending.append((idx[s:s + maxBatch], dag.vars[out_name].value))
    for idx, val in pending:
        out = vl.to_numpy(val).reshape(-1, len(idx), order="F")   # squeeze: E x N
        logits[idx, :] = out.T[:, :numEmotions]
    return logits


def compute_audio_feats_files(dag, files, numEmotions=8, limit=float("inf"), maxBatch=64, *, modelDir=None, fs=None):
    """logits = compute_audio_feats from the WAV files themselves (compute_audio_feats.m:116-136,172-176): `files` is a
    list of bytes or of paths.  [z, fs] = audioread(path); assert(size(z,2) <= 2, 'unexpected number of streams');
    z = z(:,1): vl.audioread with channel=0 (the left stream) decodes every file on the device into one bank, then
    compute_audio_feats_wav runs on it.  As upstream there is no check of the sample rate: with fs=None a file at another
    rate is read as if it were at the student's; fs=16000 resamples every file to it while it is decoded
    (vl.audioread(fs=)).  `limit` as there: only the first limit + 1 files are read."""
    files = list(files)
    if limit != float("inf"):
        files = files[:max(0, min(len(files), int(limit) + 1))]
    for k, i in enumerate(vl.audioinfo(files)):
        if i["NumChannels"] > 2:
            raise ValueError("unexpected number of streams: file %d has %d channels" % (k, i["NumChannels"]))   # :174
    bank, offsets = vl.audioread(files, channel=0, fs=fs)
    return compute_audio_feats_wav(dag, bank, offsets, numEmotions=numEmotions, maxBatch=maxBatch, modelDir=modelDir)


def compute_visual_feats(dag, track_frames, batchSize=128, numEmotions=8, limit=float("inf"), lanes=2, *, read=None,
                         split=None, progressive=False, modelDir=None, precision=None, interpolation=None, antialias=False,
                         crop_size=1 / 1.6):
    """faceLogits = compute_visual_feats(dag, track_frames): the frames of all tracks are flattened
    (:63-69), pushed through the frozen teacher `batchSize` at a time (:81-94) and the logits are split
    back per track (:104-109).  track_frames: list of 224 x 224 x 3 x F_i normalised face mats; with
    `read(paths) -> list of bytes` a list of frame-path lists instead, and every batch comes from
    fetch_emovoxceleb_imdb.getImageBatch (:123-164: the JPEG files decoded on the device; `split` and `progressive` go there).
    `dag` may be a model name, as upstream (:49 ferPlusZoo(opts.modelName)); `modelDir` then names the model files' directory.
    `precision`: zoo.FrozenTeacher's (None | 'fp32' | 'bf16x3': the split-bf16 arm of the teacher's 1 x 1 layers).
    `interpolation`, `antialias`, `crop_size`: getImageBatch's (with `read`): the filter for frames that are reduced to the
    network's input, as :129-135 reduces AFEW's; None leaves the path as it is."""
    if progressive and split is not None:
        raise ValueError("compute_visual_feats: progressive=True and split= exclude each other (vl.imreadjpeg)")
    if isinstance(dag, str):
        dag = zoo.ferPlusZoo(dag, modelDir=modelDir)
    _prepare(dag)
    first_ok = [i for i in range(len(track_frames)) if i <= limit]   # frameIdx <= firstId + limit, :72
    if read is not None:
        from . import fetch_emovoxceleb_imdb as fe
        counts = [len(track_frames[i]) for i in first_ok]
        paths = [p for i in first_ok for p in track_frames[i]]
        teacher = zoo.FrozenTeacher(dag, lanes=lanes, precision=precision)
        outs = [teacher.logits(fe.getImageBatch(paths[s:s + batchSize], dag, read=read, split=split,
                                                progressive=progressive, interpolation=interpolation, antialias=antialias,
                                                crop_size=crop_size))
                for s in range(0, len(paths), batchSize)]
        logits = (np.concatenate([vl.to_numpy(o).reshape(-1, int(o.shape[3]), order="F").T for o in outs], 0)
                  if outs else np.zeros((0, numEmotions), np.float32))
        faceLogits, off = [], 0
        for c in counts:
            faceLogits.append(logits[off:off + c, :numEmotions])
            off += c
        return faceLogits
    counts = [int(track_frames[i].shape[3]) for i in first_ok]
    teacher = zoo.FrozenTeacher(dag, lanes=lanes, precision=precision)
    flat = []
    for i in first_ok:
        t = track_frames[i]
        flat.append(t.permute(3, 2, 1, 0).contiguous())           # (F, C, W, H) storage order
    allf = torch.cat(flat, 0)
    numIms = int(allf.shape[0])
    outs = []
    for s in range(0, numIms, batchSize):
        data = allf[s:s + batchSize].permute(3, 2, 1, 0)
        outs.append(teacher.logits(data))
    logits = np.concatenate([vl.to_numpy(o).reshape(-1, int(o.shape[3]), order="F").T for o in outs], 0)
    faceLogits, off = [], 0
    for c in counts:
        faceLogits.append(logits[off:off + c, :numEmotions])
        off += c
    return faceLogits
