"""Batch providers: getBatchEmoVoxCeleb (student) and getImageBatch (teacher) mirrors.

The reference's providers read wav / jpeg files (emoVoxCeleb/getBatchEmoVoxCeleb.m:76-194,
emoVoxCeleb/fetch_emovoxceleb_imdb.m:152-193).  File I/O and the FFT front-end (VGGVox runSpec)
are outside the built path; what is kept is every piece of arithmetic that
shapes the tensors the hot path consumes, fed from seeded synthetic sources:

    audSamp / crop window        getBatchEmoVoxCeleb.m:67-68,109-119
    time2idx + logit slicing     getBatchEmoVoxCeleb.m:145-158,210-214
    aggregation (max | mean)     getBatchEmoVoxCeleb.m:179-188      -> HIP xm_aggregate_logits
    per-row normalisation ('I')  getBatchEmoVoxCeleb.m:164-169      -> HIP xm_spec_rownorm
    speed perturbation ('S')     getBatchEmoVoxCeleb.m:102-108,217-245 -> HIP xm_resample (filter designed on the host)
    additive noise ('N')         getBatchEmoVoxCeleb.m:123-135      -> HIP xm_scale_axpy (z + Nratio * y)
    the three above, batched     getBatchEmoVoxCeleb.m:102-135      -> HIP xm_wav_batch (wavBatch: one descriptor table per
                                                                       batch, the resampling taps evaluated in the kernel)
    audioinfo / audioread        getBatchEmoVoxCeleb.m:79,97-117,126   -> WavFileEmoVoxImdb: the bank decoded from WAV files
                                                                       on the device (vl.audioread, xm_wav_decode_batch)
    target selection + maxLabel  getBatchEmoVoxCeleb.m:30-32
    the teacher inside the batch fetch_emovoxceleb_imdb.m:98-136 per batch -> OnlineTeacher: the frames a batch's windows name
                                 (online_frame_plan) decoded, evaluated and aggregated (HIP xm_window_targets) on a
                                 stream of its own; no wavLogits cache
    face normalisation           fetch_emovoxceleb_imdb.m:176-193   -> HIP xm_normalize_face
    dense face frames            fetch_emovoxceleb_imdb.m:127,196-285 -> SyntheticDenseFrames (lister, find, decoded frames)
    FER+ batch (getBatchFerPlus) ferplus_baselines.m:153-268        -> HIP xm_ferplus_batch (grey -> flip -> x3 minus
                                                                       averageImage -> affine grid -> bilinear sampler)
    FER+ imdb (getFerPlusImdb)   ferplus_baselines.m:103-110        -> FerPlusImdb: fer2013.csv's pixel column parsed on the
                                                                       device (vl.pixcsv_decode, xm_pixcsv_decode_batch)
    JPEG face folder (getBatch)  vl_imreadjpeg's options [EXT]      -> getBatchJpegFaces: random crop, flip and jitter on the
                                                                       device (vl.vl_imreadjpeg, xm_imread_transform_batch)
"""
import math
import os

import numpy as np
import torch

from . import vl

FPS, LOGIT_STRIDE = 25, 6  # getBatchEmoVoxCeleb.m:212


def time2idx(t):
    """getBatchEmoVoxCeleb.m:210-214."""
    return int(math.floor(max(t * FPS - 1, 0) / LOGIT_STRIDE)) + 1


def aud_samples(width, Tw=25, fs=16000):
    """getBatchEmoVoxCeleb.m:67-68: audSamp = (0.01*W + 0.001*Tw - 0.001) * fs."""
    return (0.01 * width + 0.001 * Tw - 0.001) * fs


_SPEC_BANKS = {}


def _spec_filter_bank(fs, Tw, Ts, alpha, nfft, device):
    """1 x (Nw+1) x 1 x 2B filter bank = pre-emphasis * Hamming window * DFT rows (Re | Im), built in
    float64 on the host once per setting.  Tap k multiplies sample s[Ns*j - 1 + k]."""
    key = (fs, Tw, Ts, alpha, nfft, str(device))
    if key not in _SPEC_BANKS:
        Nw = int(round(1e-3 * Tw * fs))
        B = nfft // 2
        t = np.arange(Nw)
        win = 0.54 - 0.46 * np.cos(2 * np.pi * t / (Nw - 1))
        ang = 2 * np.pi * np.outer(t, np.arange(B)) / nfft            # Nw x B
        re, im = win[:, None] * np.cos(ang), -win[:, None] * np.sin(ang)
        bank = np.zeros((Nw + 1, 2 * B))
        bank[1:, :B] += re
        bank[1:, B:] += im
        bank[:-1, :B] -= alpha * re                                     # y[t] = s[t] - alpha s[t-1]
        bank[:-1, B:] -= alpha * im
        f = np.asfortranarray(bank.reshape(1, Nw + 1, 1, 2 * B).astype(np.float32))
        _SPEC_BANKS[key] = vl.from_numpy(f, device)
    return _SPEC_BANKS[key]


def runSpec(z, audio=None):
    """SPEC = runSpec(z, audio) on the device (getBatchEmoVoxCeleb.m:162, compute_audio_feats.m:176;
    [EXT] VGGVox, restated from the paper: 25 ms Hamming frames every 10 ms, pre-emphasis 0.97,
    1024-point FFT magnitude, 512 bins).  z: L x N device tensor of samples, one clip per column
    (column-major).  The whole STFT is ONE strided 1-D convolution on the MFMA path -- pre-emphasis,
    window and DFT folded into a 1 x 401 x 1 x 1024 filter bank, stride [1 160] -- followed by a
    magnitude/transposition kernel.  Returns 512 x W x 1 x N, W = floor((L - 400) / 160) + 1."""
    a = dict(fs=16000, Tw=25, Ts=10, alpha=0.97)
    a.update({k: v for k, v in (audio or {}).items() if k in a})
    nfft = 1024
    if z.dim() == 1:
        z = z[:, None]
    L, N = int(z.shape[0]), int(z.shape[1])
    Nw, Ns = int(round(1e-3 * a["Tw"] * a["fs"])), int(round(1e-3 * a["Ts"] * a["fs"]))
    if L < Nw:
        raise ValueError("runSpec: clip shorter than one analysis frame")
    bank = _spec_filter_bank(a["fs"], a["Tw"], a["Ts"], a["alpha"], nfft, z.device)
    # one leading zero per clip = the missing predecessor of the first sample (filter([1 -alpha], 1, z))
    buf = torch.zeros((N, L + 1), dtype=torch.float32, device=z.device)
    buf[:, 1:].copy_(z.t())
    x = buf.t()[None, :, None, :]                 # 1 x (L+1) x 1 x N view, column-major
    reim = vl.vl_nnconv(x, bank, None, stride=(1, Ns))
    return vl.spec_magnitude(reim)


def findSettings(transformation):
    """[chspeed, inputnorm, noisy] = findSettings(transformation, opts) -- getBatchEmoVoxCeleb.m:217-245: 'S' = speed
    perturbation, 'I' = per-row input normalisation, 'N' = additive noise; 'v' (validation) switches S and N off."""
    isVal = "v" in transformation
    return ("S" in transformation and not isVal), ("I" in transformation), ("N" in transformation and not isVal)


def resample_design(p, q, N=10, beta=5.0):
    """Filter of y = resample(x, p, q) [EXT: MATLAB Signal Processing Toolbox, called at getBatchEmoVoxCeleb.m:108;
    restated from its documented recipe]: p, q reduced by their gcd; h = firls(2 N max(p, q), [0 2fc 2fc 1], [1 1 0 0])
    .* kaiser(L, 5) with fc = 1 / (2 max(p, q)) -- with a zero-width transition band the least-squares design IS the
    truncated ideal low-pass 2 fc sinc(2 fc (n - (L-1)/2)) -- scaled to p * h / sum(h); zeros are put in front so that
    the delay is a whole number of OUTPUT samples, which is then dropped.  Returns (h float64, p, q, delay); the output
    has ceil(Lx p / q) samples."""
    g = math.gcd(int(p), int(q))
    p, q = int(p) // g, int(q) // g
    pqmax = max(p, q)
    fc = 0.5 / pqmax
    L = 2 * N * pqmax + 1
    n = np.arange(L, dtype=np.float64) - (L - 1) / 2
    h = 2 * fc * np.sinc(2 * fc * n) * np.kaiser(L, beta)
    h = p * h / h.sum()
    Lhalf = (L - 1) / 2
    nz = int(math.floor(q - (Lhalf % q)))
    h = np.concatenate([np.zeros(nz), h])
    delay = int(math.floor(math.ceil(Lhalf + nz) / q))
    return h, p, q, delay


def resample(x, p, q):
    """z = resample(zo, p, q) on the device (one clip, 1-D tensor)."""
    h, p, q, delay = resample_design(p, q)
    Ly = -(-int(x.numel()) * p // q)
    hd = torch.from_numpy(h.astype(np.float32)).to(x.device)
    return vl.resample(x.contiguous(), hd, p, q, delay, Ly)


class SyntheticEmoVoxImdb:
    """Stand-in for the imdb of fetch_emovoxceleb_imdb: per-track wav length (samples) and the
    cached teacher logits imdb.wavLogits{i} (F_i x 8 single, one row per sampled face frame)."""

    def __init__(self, num_tracks=64, seed=0, min_seconds=4.5, max_seconds=9.0, num_emotions=8, fs=16000,
                 val_fraction=0.0, heard_fraction=0.0):
        rng = np.random.default_rng(seed)
        self.fs = fs
        self.num_samples = rng.integers(int(min_seconds * fs), int(max_seconds * fs), num_tracks)
        self.wavLogits = []
        for n in self.num_samples:
            frames = time2idx(n / fs)
            self.wavLogits.append(np.asfortranarray(rng.standard_normal((frames, num_emotions)).astype(np.float32) * 3))
        self.set = np.ones(num_tracks, int)       # imdb.images.set: 1 = train, 2 = val (unheardVal), 3 = heardVal
        if val_fraction > 0:
            self.set[rng.permutation(num_tracks)[:int(round(num_tracks * val_fraction))]] = 2
        if heard_fraction > 0:   # 3 = heardVal (student_stats.m:79-81), drawn after everything else from the other tracks
            rest = np.nonzero(self.set == 1)[0]
            self.set[rng.permutation(rest)[:int(round(num_tracks * heard_fraction))]] = 3
        self.seed = seed
        self._dev = None

    def device_wav(self, ii, device):
        """synthetic waveform of track ii (seeded noise, num_samples[ii] samples) on the device."""
        cache = self.__dict__.setdefault("_wav", {})
        if ii not in cache:
            g = torch.Generator(device=device)
            g.manual_seed(self.seed * 100003 + int(ii))
            cache[ii] = torch.randn(int(self.num_samples[ii]), generator=g, device=device, dtype=torch.float32) * 0.1
        return cache[ii]

    # meta.noise of the reference (noisedir with `noisenum` wav files of `noiselen` samples, mixing volume `noisevol`,
    # getBatchEmoVoxCeleb.m:125-133): a seeded synthetic bank
    noisenum, noiselen, noisevol = 4, 20 * 16000, 0.3

    def device_noise(self, ir, device):
        cache = self.__dict__.setdefault("_noise", {})
        if ir not in cache:
            g = torch.Generator(device=device)
            g.manual_seed(self.seed * 7919 + 1000003 + int(ir))
            cache[ir] = torch.randn(self.noiselen, generator=g, device=device, dtype=torch.float32) * 0.05
        return cache[ir]

    def wav_offsets(self):
        """first sample of every track in the waveform bank (num_tracks + 1 values; host only)."""
        return np.concatenate([[0], np.cumsum(np.asarray(self.num_samples, np.int64))]).astype(np.int64)

    def noise_offsets(self):
        return np.arange(self.noisenum + 1, dtype=np.int64) * self.noiselen

    def logit_offsets(self):
        """row offsets of device_logits (host only)."""
        return np.cumsum([0] + [l.shape[0] for l in self.wavLogits])

    def device_wav_bank(self, device):
        """(bank, offsets): every track's device_wav concatenated, built once -- the samples the per-clip path reads."""
        if "_wav_bank" not in self.__dict__:
            self._wav_bank = torch.cat([self.device_wav(ii, device) for ii in range(len(self.num_samples))])
        return self._wav_bank, self.wav_offsets()

    def device_noise_bank(self, device):
        """(bank, offsets): the noise files device_noise(1 .. noisenum) concatenated, built once."""
        if "_noise_bank" not in self.__dict__:
            self._noise_bank = torch.cat([self.device_noise(ir, device) for ir in range(1, self.noisenum + 1)])
        return self._noise_bank, self.noise_offsets()

    def device_logits(self, device):
        """all tracks' logits concatenated (F_total x E) on the device + row offsets."""
        if self._dev is None:
            offs = np.cumsum([0] + [l.shape[0] for l in self.wavLogits])
            cat = np.asfortranarray(np.concatenate(self.wavLogits, 0))
            self._dev = (vl.from_numpy(cat, device), offs)
        return self._dev


class WavFileEmoVoxImdb(SyntheticEmoVoxImdb):
    """The interface of SyntheticEmoVoxImdb over WAV files: what cnn_get_batch_wav_emo reads through audioinfo /
    audioread (getBatchEmoVoxCeleb.m:79,97-117) and the noise files of meta.noise.noisedir (:126), decoded on the device
    by vl.audioread.  `files` is a {name: bytes} table or a callable read(names) -> list of bytes, `names` the tracks in
    imdb order (default: the table's keys); `noise` likewise with `noiseNames`.  wavLogits (one F_i x E single array per
    track) and `set` come from the caller.
      fs, num_samples      from vl.audioinfo alone (no device); a file at another rate or with more than one channel
                           raises ValueError naming it -- cnn_get_batch_wav_emo pads with zeros(n, 1) and fails there too
      device_wav_bank      the bank is allocated once from the planned total and filled in chunks of at most
                           `chunkBytes` of file bytes (out_base), so the staging buffer stays small next to the dataset
      device_wav(ii)       a view of the bank
      noisenum, noiselen   the number of noise files and the shortest of them (the reference has one `noiselen`);
                           noise_offsets() are the real cumulative offsets
      resample=True        tracks and noise files of any rate vl.audioread(fs=) accepts are brought to `fs` while they
                           are decoded (upstream converted such datasets with ffmpeg, :149); num_samples, noise_samples
                           and noiselen are then the resampled lengths, from the plan alone
      channel=c            files with several channels are read by that channel (compute_audio_feats.m:175 takes the
                           left stream, c = 0); None keeps the refusal"""

    def __init__(self, files, wavLogits, set=None, names=None, fs=16000, noise=None, noiseNames=None, noisevol=0.3,
                 chunkBytes=64 << 20, seed=0, resample=False, channel=None):
        self.fs, self.seed, self.noisevol, self.chunkBytes = int(fs), seed, noisevol, int(chunkBytes)
        self.resample, self.channel = bool(resample), None if channel is None else int(channel)
        self._read, self.names = self._source(files, names)
        self.num_samples = self._lengths(self._read, self.names, "track")
        self.wavLogits = [np.asfortranarray(l, dtype=np.float32) for l in wavLogits]
        if len(self.wavLogits) != len(self.names):
            raise ValueError("WavFileEmoVoxImdb: %d tracks, %d wavLogits" % (len(self.names), len(self.wavLogits)))
        self.set = np.ones(len(self.names), int) if set is None else np.asarray(set, int)
        self._read_noise, self.noise_names = self._source(noise, noiseNames) if noise is not None else (None, [])
        self.noise_samples = self._lengths(self._read_noise, self.noise_names, "noise file")
        self.noisenum = len(self.noise_names)
        self.noiselen = int(self.noise_samples.min()) if self.noisenum else 0
        self._dev = None
        self._banks = {}

    @classmethod
    def from_dir(cls, wavDir, names, wavLogits, set=None, noiseDir=None, **kw):
        """tracks wavDir/<name> read from disk chunk by chunk; noise files noiseDir/01.wav, 02.wav, ... (:126)"""
        import os

        def reader(root):
            def read(ns):
                out = []
                for n in ns:
                    with open(os.path.join(root, n), "rb") as fh:
                        out.append(fh.read())
                return out
            return read

        noise = noiseNames = None
        if noiseDir is not None:
            noiseNames = []
            while os.path.exists(os.path.join(noiseDir, "%02d.wav" % (len(noiseNames) + 1))):
                noiseNames.append("%02d.wav" % (len(noiseNames) + 1))
            noise = reader(noiseDir)
        return cls(reader(wavDir), wavLogits, set=set, names=list(names), noise=noise, noiseNames=noiseNames, **kw)

    @staticmethod
    def _source(files, names):
        if callable(files):
            if names is None:
                raise ValueError("WavFileEmoVoxImdb: a read(names) callable needs the list of names")
            return files, list(names)
        if isinstance(files, dict):
            names = list(files) if names is None else list(names)
            return (lambda ns: [files[n] for n in ns]), names
        files = list(files)
        return (lambda ns: [files[n] for n in ns]), list(range(len(files)))

    def _lengths(self, read, names, what):
        total = np.zeros(len(names), np.int64)
        for s in range(0, len(names), 256):
            info = vl.audioinfo(read(names[s:s + 256]), fs=self.fs if self.resample else None)
            for n, i in zip(names[s:s + 256], info):
                if i["SampleRate"] != self.fs and not self.resample:
                    raise ValueError("WavFileEmoVoxImdb: %s %r is sampled at %d Hz, the imdb at %d" % (what, n, i["SampleRate"], self.fs))
                if i["NumChannels"] != 1 and self.channel is None:
                    raise ValueError("WavFileEmoVoxImdb: %s %r has %d channels, one is required" % (what, n, i["NumChannels"]))
                if self.channel is not None and self.channel >= i["NumChannels"]:
                    raise ValueError("WavFileEmoVoxImdb: %s %r has %d channels, channel %d was asked for" %
                                     (what, n, i["NumChannels"], self.channel))
            total[s:s + 256] = [i["ResampledSamples" if self.resample else "TotalSamples"] for i in info]
        return total

    def _bank(self, key, read, names, lengths, device):
        if key not in self._banks:
            offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
            bank = torch.empty(int(offs[-1]), dtype=torch.float32, device=device)
            s = 0
            while s < len(names):                       # chunks of at most chunkBytes of file bytes, one file at least
                datas, used = [], 0
                while s + len(datas) < len(names):
                    d = read(names[s + len(datas):s + len(datas) + 1])[0]
                    if datas and used + len(d) > self.chunkBytes:
                        break
                    datas.append(d)
                    used += len(d)
                _, got = vl.audioread(datas, out=bank, out_base=int(offs[s]), channel=self.channel,
                                      fs=self.fs if self.resample else None)
                if int(got[-1]) != int(offs[s + len(datas)]):
                    raise RuntimeError("WavFileEmoVoxImdb: the files changed since their lengths were read")
                s += len(datas)
            self._banks[key] = (bank, offs)
        return self._banks[key]

    def wav_offsets(self):
        return np.concatenate([[0], np.cumsum(self.num_samples)]).astype(np.int64)

    def noise_offsets(self):
        return np.concatenate([[0], np.cumsum(self.noise_samples)]).astype(np.int64)

    def device_wav_bank(self, device):
        return self._bank("wav", self._read, self.names, self.num_samples, device)

    def device_noise_bank(self, device):
        if not self.noisenum:
            raise ValueError("WavFileEmoVoxImdb: no noise files were given")
        return self._bank("noise", self._read_noise, self.noise_names, self.noise_samples, device)

    def device_wav(self, ii, device):
        bank, offs = self.device_wav_bank(device)
        return bank[int(offs[ii]):int(offs[ii + 1])]

    def device_noise(self, ir, device):
        bank, offs = self.device_noise_bank(device)
        return bank[int(offs[ir - 1]):int(offs[ir])]


class SyntheticDenseFrames:
    """Stand-in for the unpacked dense face frames (opts.faceDir of fetch_emovoxceleb_imdb.m:69,127,246-247): which
    frame files each track has, what `find` reports, and the decoded pixels of a list of frames.
      lister(track)   the relative frame paths of one track, <celeb>/1.6/<video>/<track>/<00001..>.jpg (:246-247);
                      `track` is a dict with at least 'name', 'video', 'track' and 'id'.  A track has the frame count
                      SyntheticEmoVoxImdb assumes, time2idx(seconds), except the ids in `frameless`, which have none
                      (the 134 tracks of :231,264);
      find()          every frame file under faceDir (:209-222): the listed ones and `unclaimed` more that belong to no
                      track (the 1217 frames of :232-233);
      frames(paths, device)  the decoded frames, Hin x Win x 3 x n single with values 0..255.  The pixels of a frame are
                      a hash of (seed, its path, the pixel position): they do not depend on what else is in the batch, on
                      the batch size or on the order of the calls."""

    def __init__(self, imdb, seed=0, frameSize=(96, 96), frameless=(), unclaimed=0):
        ids = np.asarray(imdb.images["id"] if hasattr(imdb, "images") else np.arange(1, len(imdb.num_samples) + 1))
        self.counts = {int(i): time2idx(int(n) / imdb.fs) for i, n in zip(ids, imdb.num_samples)}
        for i in frameless:
            self.counts[int(i)] = 0
        self.seed, self.frameSize, self.unclaimed = int(seed), (int(frameSize[0]), int(frameSize[1])), int(unclaimed)
        self._tracks = {}

    def lister(self, track):
        celeb = str(track["name"]).split("/")[0]                                        # :244-246
        d = "%s/1.6/%s/%d" % (celeb, track["video"], int(track["track"]))
        paths = ["%s/%05d.jpg" % (d, j + 1) for j in range(self.counts.get(int(track["id"]), 0))]
        self._tracks[int(track["id"])] = paths
        return paths

    def find(self):
        """needs the tracks to have been listed once; the unclaimed files come last"""
        return [p for t in self._tracks.values() for p in t] + ["unclaimed/1.6/none/0/%05d.jpg" % (j + 1)
                                                       for j in range(self.unclaimed)]

    def frame_key(self, path):
        import zlib
        return zlib.crc32(str(path).encode())

    def __call__(self, paths, device=None):
        device = device or torch.device("cuda", torch.cuda.current_device())
        Hin, Win = self.frameSize
        # the keys go up through pinned memory without blocking: a pageable upload would make the host wait for the
        # device once per batch (buildImdb's loop only enqueues)
        k = torch.tensor([self.frame_key(p) for p in paths], dtype=torch.int64).pin_memory()
        k = k.to(device, non_blocking=True)[:, None]
        i = torch.arange(3 * Win * Hin, dtype=torch.int64, device=device)[None, :]
        M = 0xFFFFFFFF
        x = (k * 0x9E3779B1 + i * 0x85EBCA77 + (self.seed & M) * 0xC2B2AE3D) & M       # 32-bit integer hash, in int64
        x = ((x ^ (x >> 15)) * 0x2C1B3C6D) & M
        x = ((x ^ (x >> 12)) * 0x297A2D39) & M
        x = x ^ (x >> 15)
        raw = (x & 255).to(torch.float32).reshape(len(paths), 3, Win, Hin)
        return raw.permute(3, 2, 1, 0)


class JpegDenseFrames(SyntheticDenseFrames):
    """The dense face frames as JPEG files held in memory: the `lister` / `find` interface of SyntheticDenseFrames over a
    {path: bytes} table, and read(paths) -> list of bytes for buildImdb(read=...) / getImageBatch.  `files` is a list of
    JPEG files (bytes); frame j of the track with id i is files[(7 i + j) mod len(files)], so the frames of one track and
    of one batch differ in size when the files do.  index(path) names the file behind a listed path.  progressive=True
    says that some of the files are progressive: buildImdb(read=frames.read, progressive=frames.progressive)."""

    def __init__(self, imdb, files, frameless=(), unclaimed=0, progressive=False):
        super().__init__(imdb, frameless=frameless, unclaimed=unclaimed)
        self.progressive = bool(progressive)
        self.files = [bytes(f) for f in files]
        if not self.files:
            raise ValueError("JpegDenseFrames: no files")
        self.table, self._index = {}, {}

    def lister(self, track):
        paths = super().lister(track)
        for j, p in enumerate(paths):
            self._index[p] = (7 * int(track["id"]) + j) % len(self.files)
            self.table[p] = self.files[self._index[p]]
        return paths

    def index(self, path):
        return self._index[path]

    def read(self, paths):
        return [self.table[p] for p in paths]

    def __call__(self, paths, device=None):
        raise RuntimeError("JpegDenseFrames holds files, not pixels: use buildImdb(read=frames.read)")


def crop_window(total_samples, audSamp, fs, num_logit_rows, rng, fixedSegments=False, timeOffset=None):
    """(wr, startIdx, endIdx) of one clip, all 1-based as in cnn_get_batch_wav_emo (getBatchEmoVoxCeleb.m:81-152):
    wr is the first sample audioread takes, [startIdx, endIdx] the rows of the cached logits that are aggregated.
      random crop (:109-119):  total = min(19.9 fs, total) (:81-89);  wd = total - audSamp;
                               wd >= 1: wr = randi(wd) in [1, wd];  else wr = 1 (short clip, zero padded)
                               starttime = wr / fs, endtime = (wr + audSamp - 1) / fs (:141-142) -- wr enters 1-BASED --
                               rows time2idx(starttime) .. min(time2idx(endtime), #rows) (:145-152)
      fixedSegments (:91-101): wr = timeOffset * fs + 1, every row of the clip's logits (:136-137)."""
    if fixedSegments:
        if timeOffset is None:
            raise IndexError("fixedSegments: timeOffsets is empty (Index exceeds matrix dimensions upstream, :92)")
        return int(round(timeOffset * fs)) + 1, 1, int(num_logit_rows)
    total = min(int(total_samples), int(19.9 * fs))
    wd = total - int(round(audSamp))
    wr = int(rng.integers(1, wd + 1)) if wd >= 1 else 1
    s, e = time2idx(wr / fs), time2idx((wr + audSamp - 1) / fs)
    return wr, s, min(e, int(num_logit_rows))


def frame_index(imdb):
    """(counts, order) of the frame lists of an imdb that went through addFramesToImdb: counts[ii] frames belong to
    track ii (denseFramesWavIds == images.id[ii]) and order holds their positions in images.denseFrames, track after
    track in imdb order, each track in list order -- the grouping buildImdb gets from vl.group_rows.  Host only; kept
    with the imdb for as long as it holds the same `images`."""
    images = imdb.images
    held = imdb.__dict__.get("_frame_index")
    if held is None or held[0] is not images:
        ids = np.asarray(images["id"], np.int64)
        wav = np.asarray(images["denseFramesWavIds"], np.int64)
        by_id = np.argsort(wav, kind="stable")                  # frames grouped by wav id, list order inside a group
        lo, hi = np.searchsorted(wav[by_id], ids, "left"), np.searchsorted(wav[by_id], ids, "right")
        order = np.concatenate([by_id[a:b] for a, b in zip(lo, hi)] or [np.zeros(0, np.int64)])
        held = imdb.__dict__["_frame_index"] = (images, (hi - lo).astype(np.int64), order.astype(np.int64))
    return held[1], held[2]


def logit_rows(imdb):
    """(rows, offsets): the row count of every track's teacher logits and the row offsets of their concatenation
    (num_tracks + 1 values).  From the cached imdb.wavLogits when there are any, else from the frame lists: a track has
    one row per listed frame (frame_index).  Host only."""
    if getattr(imdb, "wavLogits", None) is not None:
        return np.array([l.shape[0] for l in imdb.wavLogits], np.int64), np.asarray(imdb.logit_offsets())
    rows, _ = frame_index(imdb)
    return rows, np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


def online_frame_plan(imdb, first, last, framesPerPair="all", frame_rng=None):
    """Which frame files the windows [first[k], last[k]] of wav_batch_plan name (1-based inclusive rows of the
    concatenated per-track logits), for an imdb that went through addFramesToImdb; it needs no wavLogits.  Row r of
    track ii is the r-th entry of images.denseFrames whose denseFramesWavIds equals images.id[ii], in list order.
    Returns (paths, wfirst, wlast): the frames to decode, pair after pair, each window in ascending row order, and the
    windows as 1-based inclusive int32 ranges into that compact list.
      framesPerPair = k   keeps k rows of a window longer than k, drawn without replacement from `frame_rng` (a generator
                          of its own: the audio crops of a run do not depend on it) and sorted; a window of at most k
                          rows keeps them all and draws nothing
      an empty window     (first > last) contributes no frames and keeps its length last - first + 1 <= 0, so that the
                          mean over it is the cached mode's 0 / (last - first + 1).
    Touches no device."""
    if framesPerPair != "all" and (isinstance(framesPerPair, str) or int(framesPerPair) < 1):
        raise ValueError("framesPerPair: 'all' or a positive number of frames, got %r" % (framesPerPair,))
    first, last = np.asarray(first, np.int64).reshape(-1), np.asarray(last, np.int64).reshape(-1)
    if first.shape != last.shape:
        raise ValueError("online_frame_plan: first and last differ in length")
    _, offs = logit_rows(imdb)
    counts, order = frame_index(imdb)
    foffs = np.concatenate([[0], np.cumsum(counts)])
    frames = imdb.images["denseFrames"]
    frame_rng = frame_rng if frame_rng is not None else np.random.default_rng(0)
    paths = []
    wfirst, wlast = np.zeros(len(first), np.int32), np.zeros(len(first), np.int32)
    for k, (a, b) in enumerate(zip(first, last)):
        wfirst[k] = len(paths) + 1
        if a > b:
            wlast[k] = len(paths) + (b - a + 1)
            continue
        if a < 1 or b > offs[-1]:
            raise ValueError("online_frame_plan: window %d = [%d, %d] leaves the %d rows of the imdb" % (k, a, b, offs[-1]))
        rows = np.arange(a - 1, b)                                      # 0-based rows of the concatenated logits
        if framesPerPair != "all" and len(rows) > int(framesPerPair):
            rows = rows[np.sort(frame_rng.choice(len(rows), int(framesPerPair), replace=False))]
        ii = np.searchsorted(offs, rows, "right") - 1                   # the track of every row
        r = rows - offs[ii]
        if (r >= counts[ii]).any():
            raise ValueError("online_frame_plan: window %d asks for a row its track lists no frame for" % k)
        paths += [frames[j] for j in order[foffs[ii] + r]]
        wlast[k] = len(paths)
    return paths, wfirst, wlast


class BatchInputs(list):
    """the inputs list of a getBatch whose tensors are produced on another stream: `input_events` {input name:
    torch.cuda.Event} goes to net.eval(..., input_events=...); a plain list has none"""
    input_events = None


class OnlineTeacher:
    """The frozen teacher run inside the batch provider: the targets of a batch come from the face frames its windows
    name instead of from imdb.wavLogits (fetch_emovoxceleb_imdb.m:98-136 per batch, not over the whole dataset).
      teacher   a ferPlusZoo network (losses stripped, test mode, one input, wrapped in FrozenTeacher(lanes)) or any
                object with .logits(faces) -> 1 x 1 x E x n
      imdb      has been through addFramesToImdb; needs no wavLogits
      read(paths) -> JPEG bytes (fetch_emovoxceleb_imdb.getImageBatch; `split`, `progressive` go there), or
      frames(paths, device) -> decoded pixels (vl.crop_resize_face); exactly one of the two
      chunk     at most that many faces per teacher call
      framesPerPair, seed   online_frame_plan's option and the seed of its generator
      precision zoo.FrozenTeacher's (None | 'fp32' | 'bf16x3'); .precision is what the teacher runs at
      overlap   the whole of targets() is enqueued on a stream of the object's own that first waits for the calling
                stream; the returned event is recorded behind the targets.  False: the calling stream, event None.
    Nothing synchronises the host."""

    def __init__(self, teacher, imdb, *, read=None, frames=None, lanes=2, chunk=128, framesPerPair="all", overlap=True,
                 split=None, progressive=False, seed=0, precision=None):
        from . import fetch_emovoxceleb_imdb as fe
        fe.check_precision(precision, "OnlineTeacher")
        if progressive and split is not None:
            raise ValueError("OnlineTeacher: progressive=True and split= exclude each other (vl.imreadjpeg)")
        if (frames is None) == (read is None):
            raise ValueError("OnlineTeacher: give either `frames` (decoded pixels) or `read` (JPEG bytes)")
        if (split is not None or progressive) and read is None:
            raise ValueError("OnlineTeacher: `split` and `progressive` belong to the device JPEG decode, which needs `read`")
        if int(chunk) < 1:
            raise ValueError("OnlineTeacher: chunk must be at least one face")
        online_frame_plan(imdb, [], [], framesPerPair)                   # refuses a bad framesPerPair before any device work
        if not torch.cuda.is_available():
            raise RuntimeError("OnlineTeacher needs a GPU; this build has no CPU path")
        self.model, self.imageSize, self.averageImage = fe._as_teacher(teacher, lanes, precision)
        self.precision = getattr(self.model, "precision", "fp32")
        self._norm = fe._Norm(self.imageSize, self.averageImage)
        self._getImageBatch = fe.getImageBatch
        self.imdb, self.read, self.frames = imdb, read, frames
        self.chunk, self.framesPerPair, self.split, self.progressive = int(chunk), framesPerPair, split, bool(progressive)
        self.frame_rng = np.random.default_rng(seed)
        self.device = getattr(teacher, "device", None) or torch.device("cuda", torch.cuda.current_device())
        self.overlap = bool(overlap)
        self.stream = torch.cuda.Stream(device=self.device) if self.overlap else None

    def faces(self, paths):
        """the normalised faces of a list of frames, imageSize x 3 x n"""
        if self.read is not None:
            return self._getImageBatch(paths, self._norm, read=self.read, device=self.device, split=self.split,
                                       progressive=self.progressive)
        return vl.crop_resize_face(self.frames(paths, self.device), self.averageImage, self.imageSize)

    def logits(self, paths):
        """1 x 1 x E x n teacher logits of the frames, evaluated `chunk` faces at a time"""
        n, out = len(paths), None
        for a in range(0, n, self.chunk):
            lg = self.model.logits(self.faces(paths[a:a + self.chunk]))
            if n <= self.chunk:
                return lg
            if out is None:
                out = vl.mat_empty(1, 1, int(lg.shape[2]), n, device=self.device)
            out[..., a:a + self.chunk].copy_(lg)
        return out

    def _targets(self, paths, wfirst, wlast, numPredEmotions, agg):
        up = torch.from_numpy(np.stack([wfirst, wlast])).pin_memory().to(self.device, non_blocking=True)
        # a batch of empty windows only: there is no frame to evaluate, the targets are those of empty ranges
        lg = self.logits(paths) if paths else vl.mat_zeros(1, 1, int(numPredEmotions), 1, device=self.device)
        if numPredEmotions > lg.shape[2]:
            raise ValueError("numPredEmotions exceeds the number of the teacher's logits")
        return vl.window_targets(lg, up[0], up[1], agg, numPredEmotions)

    def targets(self, first, last, numPredEmotions=8, agg="max"):
        """(lgo 1 x 1 x P x N, maxLabel 1 x 1 x 1 x N, event) of the windows [first, last] of wav_batch_plan"""
        if agg not in ("max", "mean"):
            raise ValueError("unreccognised aggregator %s" % agg)
        paths, wfirst, wlast = online_frame_plan(self.imdb, first, last, self.framesPerPair, self.frame_rng)
        if not self.overlap:
            return self._targets(paths, wfirst, wlast, int(numPredEmotions), agg) + (None,)
        main = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(main)
        with torch.cuda.stream(self.stream):
            lgo, lab = self._targets(paths, wfirst, wlast, int(numPredEmotions), agg)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        lgo.record_stream(main)        # made on the teacher stream, read (and freed) by the caller's
        lab.record_stream(main)
        return lgo, lab, ev


def wav_batch_plan(imdb, batch, W, transformation, rng, fixedSegments=False, timeOffsets=None):
    """The host side of one batch of cnn_get_batch_wav_emo (getBatchEmoVoxCeleb.m:76-158): every random draw, in the
    reference's order per clip -- speedR (:103), the crop offset wr (:106 | :111), then Nir, Nwr, Nratio (:125-133) --
    turned into the descriptor table of vl.wav_batch.  Touches no device.  Returns (desc, ratio, first, last):
      desc   N x 6 int64 {src, len, p, q, nsrc, nlen}: src / nsrc index the banks of imdb.device_wav_bank /
             device_noise_bank; a plain crop has p == q == fs and len = the samples the track has in [wr, wr + L);
             'S' has len = audSampR, p = round(fs / speedR), q = fs, and noise over its resampled length cut to L
             (nlen = min(ceil(len p / q), L)); a zero-padded crop gets noise over all L samples (:117 pads before :134)
      ratio  N float32, Nratio
      first, last  rows of imdb.device_logits that are aggregated (1-based, inclusive)."""
    batch = list(batch)
    N, fs = len(batch), int(imdb.fs)
    audSamp = aud_samples(W)
    L = int(round(audSamp))
    chspeed, _, noisy = findSettings(transformation)
    woffs, noffs = imdb.wav_offsets(), imdb.noise_offsets()
    nrows, loffs = logit_rows(imdb)          # from the frame lists when the imdb has no cached logits (OnlineTeacher)
    desc = np.zeros((N, 6), np.int64)
    ratio = np.zeros(N, np.float32)
    first = np.zeros(N, np.int32)
    last = np.zeros(N, np.int32)
    for k, ii in enumerate(batch):
        total, rows = int(imdb.num_samples[ii]), int(nrows[ii])
        p = q = fs
        if chspeed and not fixedSegments:
            # :102-108 -- draw order as upstream: speed first, then the crop offset; the window read is audSampR long
            # while the logit rows still follow [wr, wr + audSamp) (:141-142 use audSamp)
            total = min(total, int(19.9 * fs))
            speedR = 0.95 + float(rng.random()) * 0.1
            audSampR = int(round(audSamp * speedR))
            wd = total - audSampR
            if wd < 1:
                raise ValueError("clip %d is shorter than the speed-perturbed window (randi(wd) fails upstream, :106)" % ii)
            wr = int(rng.integers(1, wd + 1))
            s = time2idx(wr / fs)
            e = min(time2idx((wr + audSamp - 1) / fs), int(rows))
            p, ln = int(round(fs / speedR)), audSampR        # z = resample(zo, round(fs / speedR), fs)
            nz = -(-ln * p // q)
            if abs(nz - L) > 160:
                raise RuntimeError("resample produced %d samples for a window of %d" % (nz, L))
        else:
            # getBatchEmoVoxCeleb.m:81-89: no clip of the dataset is longer than DATASET_LIMIT = 19.9 s; the sample
            # count is thresholded accordingly (the cached teacher logits end there too)
            wr, s, e = crop_window(total, audSamp, fs, rows, rng, fixedSegments,
                                   None if timeOffsets is None else timeOffsets[k])
            ln = max(0, min(L, int(imdb.num_samples[ii]) - (wr - 1)))
            nz = L
        start = min(wr - 1, int(imdb.num_samples[ii]))      # 0-based slice start of audioread(audfile, [wr ...])
        desc[k, :4] = woffs[ii] + start, ln, p, q
        if noisy:                                                       # :123-135, draw order Nir, Nwr, Nratio
            nir, nwr = int(rng.integers(1, imdb.noisenum + 1)), int(rng.integers(1, imdb.noiselen - nz + 1))
            ratio[k] = float(rng.random()) * imdb.noisevol
            # z + y .* Nratio runs over numel(z) (:128-134): a short clip was zero-padded to audSamp BEFORE the mix, so
            # its padded tail receives noise too; the resampled window of 'S' is not padded (its own length, cut to L)
            desc[k, 4:] = noffs[nir - 1] + nwr - 1, min(nz, L)
        first[k], last[k] = loffs[ii] + s, loffs[ii] + e
    return desc, ratio, first, last


def wav_clips(imdb, batch, desc, ratio, L, device):
    """The L x N sample matrix of a planned batch, clip by clip: a slice of the track, for 'S' a float64 filter design on
    the host + xm_resample, for 'N' xm_scale_axpy on a one-clip view.  What vl.wav_batch does in one call."""
    woffs, noffs = imdb.wav_offsets(), imdb.noise_offsets()
    z = torch.zeros((len(batch), L), dtype=torch.float32, device=device)      # storage of the L x N mat
    for k, ii in enumerate(batch):
        src, ln, p, q, nsrc, nlen = (int(v) for v in desc[k])
        zo = imdb.device_wav(ii, device)[src - woffs[ii]:src - woffs[ii] + ln]
        # (the spectrogram width only depends on floor((len - 400) / 160): +-1 sample of 'S' is immaterial)
        w = resample(zo, p, q)[:L] if p != q else zo
        z[k, :w.numel()].copy_(w)                                    # zero padding when short (:117)
        if nlen:
            nir = int(np.searchsorted(noffs, nsrc, side="right"))    # 1-based noise file
            y = imdb.device_noise(nir, device)[nsrc - noffs[nir - 1]:nsrc - noffs[nir - 1] + nlen]
            a = vl.mat_empty(1, 1, 1, 1, device=device)
            a.fill_(float(ratio[k]))
            zk = z[k, :nlen]
            col = lambda t: t.reshape(1, 1, 1, -1).permute(3, 2, 1, 0)     # noqa: E731  (L x 1 x 1 x 1 mat view)
            zk.copy_(vl.scale_axpy(col(y), a, col(zk)).permute(3, 2, 1, 0).reshape(-1))   # z = z + y .* Nratio (:134)
    return z.t()


def getBatchEmoVoxCeleb(imdb, batch, imageSize=(512, 300), numPredEmotions=8, logitAggregator="max",
                        lossType="hot-cross-ent", transformation="I", rng=None, spec_source=None,
                        device=None, use_wav=False, fixedSegments=False, timeOffsets=None, wavBatch=False,
                        onlineTeacher=None):
    """inputs = getBatchEmoVoxCeleb(imdb, batch, ...) -> ['data', im, 'logitTarget', lgo,
    'maxLabel', maxLabel] (getBatchEmoVoxCeleb.m:31-43).  Spectrogram magnitudes come from
    `spec_source` (H x W x 1 x N device tensor), from the imdb's waveforms through the device
    front-end (`use_wav`: crop [wr, wr+audSamp) with zero padding of short clips :109-119, runSpec
    :162), or from a seeded half-normal generator.
    `wavBatch` (with `use_wav`): the L x N sample matrix comes from ONE vl.wav_batch call on the imdb's device banks
    instead of the per-clip loop (slice, host-designed filter + xm_resample, xm_scale_axpy); the draws, and
    everything behind the matrix, are the same.
    `fixedSegments` (:91-101, :136-137; off upstream, run_distillation.m:86): the crop of clip k starts at
    timeOffsets[k] seconds, clips are not thresholded to DATASET_LIMIT, and ALL cached logit rows of the clip are
    aggregated.  (Upstream always passes timeOffsets = [] (:15), so the branch cannot run there; an offset list is
    required here.)
    `onlineTeacher` (an OnlineTeacher over this imdb): the same draws and the same spectrogram path, but logitTarget and
    maxLabel come from onlineTeacher.targets -- the teacher evaluated on the frames the windows name -- and the imdb needs
    no wavLogits.  The returned list is a BatchInputs whose input_events {'logitTarget': ev, 'maxLabel': ev} belong to
    net.eval(..., input_events=...) (None when the teacher ran on the calling stream)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    rng = rng or np.random.default_rng(0)
    batch = list(batch)
    N = len(batch)
    H, W = imageSize
    audSamp = aud_samples(W)
    chspeed, _, noisy = findSettings(transformation)
    if (chspeed or noisy) and not (use_wav and spec_source is None):
        raise ValueError("transformations 'S' / 'N' act on the waveform: they need use_wav=True")
    if onlineTeacher is None:
        logits, _ = imdb.device_logits(device)
    from_wav = spec_source is None and use_wav
    desc, ratio, first, last = wav_batch_plan(imdb, batch, W, transformation, rng, fixedSegments, timeOffsets)
    events = None
    if onlineTeacher is not None:
        # first of all, so that the teacher's stream works while this one makes the spectrograms
        lgo, maxLabel, ev = onlineTeacher.targets(first, last, numPredEmotions, logitAggregator)
        events = {"logitTarget": ev, "maxLabel": ev} if ev is not None else None
    if from_wav and wavBatch:
        wav, _ = imdb.device_wav_bank(device)
        noise = imdb.device_noise_bank(device)[0] if noisy else None
        spec_source = runSpec(vl.wav_batch(wav, noise, desc, ratio, int(round(audSamp))), {"fs": imdb.fs})
    elif from_wav:
        spec_source = runSpec(wav_clips(imdb, batch, desc, ratio, int(round(audSamp)), device), {"fs": imdb.fs})
    if from_wav and int(spec_source.shape[1]) != W:
        raise RuntimeError("runSpec produced %d frames, expected %d" % (int(spec_source.shape[1]), W))
    if spec_source is None:
        g = torch.Generator(device=device)
        g.manual_seed(int(rng.integers(0, 2 ** 31)))
        raw = torch.randn((N, 1, W, H), generator=g, device=device, dtype=torch.float32).abs_()
        spec_source = raw.permute(3, 2, 1, 0)
    im = vl.spec_rownorm(spec_source) if "I" in transformation else spec_source
    if onlineTeacher is None:
        lgo, maxLabel = vl.aggregate_logits(logits, torch.from_numpy(first).to(device),
                                            torch.from_numpy(last).to(device), logitAggregator)
        if numPredEmotions > lgo.shape[2]:
            raise ValueError("numPredEmotions exceeds the number of cached logits")
        if numPredEmotions != lgo.shape[2]:
            # lgo = lgo(:,:,1:opts.numPredEmotions,:) ; [~, maxLabel] = max(lgo, [], 3)  (:30-32)
            lgo = lgo[:, :, :numPredEmotions, :].permute(3, 2, 1, 0).contiguous().permute(3, 2, 1, 0)
            maxLabel = vl.max_label(lgo)
    inputs = BatchInputs(["data", im]) if onlineTeacher is not None else ["data", im]
    if events is not None:
        inputs.input_events = events
    if lossType == "softmaxlog":
        inputs += ["maxLabel", maxLabel]
    elif lossType == "euclidean":
        weights = vl.mat_empty(1, 1, 1, N, device=device)   # "no re-weighting required" (:36)
        weights.fill_(1.0)
        inputs += ["logitTarget", lgo, "instanceWeights", weights, "maxLabel", maxLabel]
    elif lossType == "hot-cross-ent":
        inputs += ["logitTarget", lgo, "maxLabel", maxLabel]
    else:
        raise ValueError("unrecognised loss type: %s" % lossType)   # 'huber' included, as upstream (:41)
    return inputs


def getImageBatch(num, imageSize=(224, 224), averageImage=(131.0912, 103.8827, 91.4953), seed=1,
                  device=None, frameSize=None):
    """fetch_emovoxceleb_imdb.m:152-193 on synthetic frames: uint8-valued RGB -> rgb2gray ->
    replicate x3 -> minus the per-channel averageImage.  With `frameSize` = (Hin, Win) the frames are
    "decoded" at that size and go through the fused centre-crop(1/1.6) + bilinear-resize kernel first
    (the vl_imreadjpeg arguments of :161-167)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    if frameSize is not None:
        raw = torch.randint(0, 256, (num, 3, frameSize[1], frameSize[0]), generator=g, device=device)
        return vl.crop_resize_face(raw.to(torch.float32).permute(3, 2, 1, 0), averageImage, imageSize)
    rgb = torch.randint(0, 256, (num, 3, imageSize[1], imageSize[0]), generator=g, device=device)
    rgb = rgb.to(torch.float32).permute(3, 2, 1, 0)
    return vl.normalize_face(rgb, averageImage)


class SyntheticBenchmarkImdb:
    """Stand-in for the imdb of an external benchmark (RML, eNTERFACE, AFEW: getRmlImdb & co. are not in the reference
    and the media cannot be decoded here) as external/run_cross_val.m reads it: tracks.set (1 = train, 2 = val, the
    split the AFEW branch uses), tracks.labels (1-based, the classes dealt out evenly in seeded order) and tracks.id
    (1..N); per track a 512 x T spectrogram magnitude (audio, T in [min_frames, max_frames]) or F_i normalised face
    frames of face_size x face_size x 3 (visual, F_i in [min_faces, max_faces]), made on the device from seeded noise
    when first asked for.  Every size is a parameter; the defaults make no claim about the real datasets."""

    def __init__(self, num_tracks=120, num_classes=6, modality="audio", seed=0, val_fraction=0.0, min_frames=100,
                 max_frames=400, min_faces=1, max_faces=6, face_size=224, averageImage=(131.0912, 103.8827, 91.4953)):
        if modality not in ("audio", "visual"):
            raise ValueError("unknown modality %s" % modality)
        rng = np.random.default_rng(seed)
        N = int(num_tracks)
        self.modality, self.seed, self.face_size, self.averageImage = modality, int(seed), int(face_size), averageImage
        labels = rng.permutation(np.arange(N) % int(num_classes)) + 1
        sets = np.ones(N, int)
        sets[rng.permutation(N)[:int(round(N * val_fraction))]] = 2
        self.tracks = {"set": sets, "labels": labels.astype(int), "id": np.arange(1, N + 1)}
        if modality == "audio":
            self.frames = rng.integers(int(min_frames), int(max_frames) + 1, N)
        else:
            self.frames = rng.integers(int(min_faces), int(max_faces) + 1, N)
        self._dev = {}

    def __len__(self):
        return len(self.tracks["set"])

    def device_spec(self, ii, device):
        """512 x T spectrogram magnitude of track ii (MATLAB layout)."""
        g = torch.Generator(device=device)
        g.manual_seed(self.seed * 100003 + 17 + int(ii))
        T = int(self.frames[ii])
        return torch.randn(T, 512, generator=g, device=device, dtype=torch.float32).abs_().t()

    def device_faces(self, ii, device):
        """face_size x face_size x 3 x F_i normalised face frames of track ii (getImageBatch's arithmetic)."""
        return getImageBatch(int(self.frames[ii]), imageSize=(self.face_size, self.face_size),
                             averageImage=self.averageImage, seed=self.seed * 100003 + 29 + int(ii), device=device)


# ---------------------------------------------------------------------------------------------
# FER+ (teacher training): getBatchFerPlus / computeAugs of teacher/ferplus_baselines.m
# ---------------------------------------------------------------------------------------------
FERPLUS_CLASSES = ["neutral", "happiness", "surprise", "sadness", "anger", "disgust", "fear", "contempt", "unknown",
                   "NF"]


def ferplus_num_classes(dataType):
    """ferplus_baselines.m:88-93,160-165: 'CNTK' / 'clean' -> 8, 'full' -> 10."""
    if dataType in ("CNTK", "clean"):
        return 8
    if dataType == "full":
        return 10
    raise ValueError("%s uknown number of classes" % dataType)


class SyntheticFerPlusImdb:
    """Stand-in for the FER+ imdb (getFerPlusImdb is not part of the reference and the FER2013 / FER+ CSVs cannot be
    read here): seeded 48 x 48 greyscale faces (single, integer values 0..255, smooth blobs on a noisy background),
    ten vote columns per image in the FER+ order (the eight emotions, 'unknown', 'NF'; ten annotators, at least one
    vote among the first eight), hardLabels = 1-based argmax over the eight emotions, set 1 / 2 / 3 = train / val / test.
    Fields as the reference reads them: images.data (H x W x 1 x N), images.votes (N x 10), images.hardLabels (1 x N),
    images.set (N), meta.classes."""

    def __init__(self, num_images=256, seed=0, size=48, val_fraction=0.25, test_fraction=0.0):
        rng = np.random.default_rng(seed)
        N = int(num_images)
        yy, xx = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
        data = np.zeros((size, size, 1, N), np.float32, order="F")
        for n in range(N):
            cy, cx = rng.uniform(0.3, 0.7, 2) * size
            r = rng.uniform(0.15, 0.35) * size
            face = 200 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r)) + rng.normal(40, 15, (size, size))
            data[:, :, 0, n] = np.clip(np.round(face), 0, 255)
        votes = np.zeros((N, 10))
        for n in range(N):
            votes[n] = rng.multinomial(10, rng.dirichlet(np.full(10, 0.3)))
            if votes[n, :8].sum() == 0:
                votes[n, rng.integers(0, 8)] += 1
        sets = np.ones(N, int)
        perm = rng.permutation(N)
        nv, nt = int(round(N * val_fraction)), int(round(N * test_fraction))
        sets[perm[:nv]] = 2
        sets[perm[nv:nv + nt]] = 3
        self.images = {"data": data, "votes": votes, "set": sets,
                       "hardLabels": (votes[:, :8].argmax(1) + 1).reshape(1, N).astype(np.float64)}
        self.meta = {"classes": list(FERPLUS_CLASSES)}
        self._dev = {}

    @property
    def set(self):
        return self.images["set"]

    def device_arrays(self, numClasses, device):
        """device-resident copies, made once: the images (storage N x 1 x W x H: the MATLAB array H x W x 1 x N),
        the vote distributions over the first numClasses columns (N x numClasses) and the hard labels (N)."""
        key = (int(numClasses), str(device))
        if key not in self._dev:
            d = self.images["data"]
            data = torch.from_numpy(np.ascontiguousarray(d.transpose(3, 2, 1, 0))).to(device)
            v = self.images["votes"][:, :numClasses]
            probs = torch.from_numpy((v / v.sum(1, keepdims=True)).astype(np.float32)).to(device)   # :167-168
            hard = torch.from_numpy(self.images["hardLabels"].reshape(-1).astype(np.float32)).to(device)
            self._dev[key] = (data, probs, hard)
        return self._dev[key]


class FerPlusImdb:
    """The FER+ imdb built by getFerPlusImdb from fer2013.csv and fer2013new.csv.  The fields the reference reads
    (ferplus_baselines.m:139,167-181): images.data (H x W x 1 x N, a DEVICE tensor in MATLAB layout -- the images are
    never on the host), images.votes (N x 10), images.hardLabels (1 x N, 1-based first argmax over the eight
    emotions, as SyntheticFerPlusImdb), images.set (N: 1 / 2 / 3 from Training / PublicTest / PrivateTest),
    meta.classes; and two more: images.ferLabels (the `emotion` column of fer2013.csv) and images.row (the CSV line of
    every kept image)."""

    def __init__(self, data, votes, sets, ferLabels, rows):
        N = len(votes)
        self.images = {"data": data, "votes": votes, "set": sets,
                       "hardLabels": (votes[:, :8].argmax(1) + 1).reshape(1, N).astype(np.float64),
                       "ferLabels": ferLabels, "row": rows}
        self.meta = {"classes": list(FERPLUS_CLASSES)}
        self._dev = {}

    @property
    def set(self):
        return self.images["set"]

    def device_arrays(self, numClasses, device):
        """the contract of SyntheticFerPlusImdb.device_arrays: (images N x 1 x W x H, vote distributions N x numClasses,
        hard labels N), made once per (numClasses, device).  The images are the storage of images.data itself."""
        key = (int(numClasses), str(device))
        if key not in self._dev:
            data = self.images["data"].permute(3, 2, 1, 0)
            assert data.is_contiguous()
            data = data.to(device)
            v = self.images["votes"][:, :numClasses]
            with np.errstate(invalid="ignore", divide="ignore"):
                probs = torch.from_numpy((v / v.sum(1, keepdims=True)).astype(np.float32)).to(device)   # :167-168
            hard = torch.from_numpy(self.images["hardLabels"].reshape(-1).astype(np.float32)).to(device)
            self._dev[key] = (data, probs, hard)
        return self._dev[key]


FERPLUS_SETS = ("Training", "PublicTest", "PrivateTest")


def readFerPlusVotes(path):
    """fer2013new.csv on the host (36 k short rows, the csv module): header `Usage,Image name,neutral,...,NF` with the ten
    vote columns in the FERPLUS_CLASSES order.  Returns (usage: list of str, names: list of str, votes: n x 10 float64,
    lines: the CSV line of every row)."""
    import csv
    usage, names, votes, lines = [], [], [], []
    with open(path, newline="", encoding="utf-8-sig") as fh:
        reader = csv.reader(fh)
        header = None
        for rec in reader:
            if not rec or not any(f.strip() for f in rec):
                continue
            if header is None:
                header = [f.strip() for f in rec]
                want = ["Usage", "Image name"] + FERPLUS_CLASSES
                if header[:12] != want:
                    raise ValueError("%s: line %d: the header must be %s" % (path, reader.line_num, ",".join(want)))
                continue
            if len(rec) < 12:
                raise ValueError("%s: line %d: %d fields, the header has 12" % (path, reader.line_num, len(rec)))
            try:
                votes.append([float(f) for f in rec[2:12]])
            except ValueError:
                raise ValueError("%s: line %d: a vote is not a number" % (path, reader.line_num)) from None
            usage.append(rec[0].strip())
            names.append(rec[1].strip())
            lines.append(reader.line_num)
    if header is None:
        raise ValueError("%s: no header" % path)
    return usage, names, np.array(votes, np.float64).reshape(len(votes), 10), np.array(lines, np.int64)


def ferPlusKeep(names, votes, dataType="CNTK"):
    """Which rows of the FER2013 / FER+ pair become images.  A PROJECT RULE, not the reference's: getFerPlusImdb is not
    part of the reference.  Rows with an empty `Image name` (those FER+ removed from FER2013) are dropped; for 'CNTK' and
    'clean' -- the eight-class problems -- rows without a vote among the eight emotions are dropped too, because
    votes ./ sum(votes, 2) of ferplus_baselines.m:168-169 would be NaN for them.  'full' keeps those."""
    ferplus_num_classes(dataType)
    keep = np.array([bool(n) for n in names], bool)
    if dataType in ("CNTK", "clean"):
        keep &= np.asarray(votes)[:, :8].sum(1) > 0
    return keep


def ferPlusPlan(dataDir, dataType="CNTK"):
    """The host side of getFerPlusImdb (no device call): reads the vote file, plans the pixel file, checks that the two
    correspond and applies ferPlusKeep.  Returns dict(data: the pixel file's bytes, plan: vl.pixcsv_plan's with the
    output index of every kept row set and -1 for the others, keep, votes, sets, ferLabels, row -- the last four for the
    kept rows only)."""
    pix_path, vote_path = os.path.join(dataDir, "fer2013.csv"), os.path.join(dataDir, "fer2013new.csv")
    usage, names, votes, vlines = readFerPlusVotes(vote_path)
    data = np.fromfile(pix_path, np.uint8)
    plan = vl.pixcsv_plan(data)
    rows = plan["rows"]
    if plan["N"] != len(usage):
        raise ValueError("%s has %d rows and %s has %d: they must correspond 1 : 1" % (pix_path, plan["N"], vote_path, len(usage)))
    sets = np.array([FERPLUS_SETS.index(u) + 1 if u in FERPLUS_SETS else 0 for u in usage], int)
    for i in np.nonzero((sets == 0) | ((rows[:, 3] >= 0) & (rows[:, 3] != sets - 1)))[0][:1]:
        theirs = FERPLUS_SETS[rows[i, 3]] if rows[i, 3] >= 0 else "no known Usage"
        raise ValueError("%s: line %d: Usage %r, but %s has %s on its line %d"
                         % (vote_path, vlines[i], usage[i], pix_path, theirs, rows[i, 4]))
    keep = ferPlusKeep(names, votes, dataType)
    rows = rows.copy()
    rows[:, 5] = np.where(keep, np.cumsum(keep) - 1, -1)
    return dict(data=data, plan=dict(plan, rows=rows), keep=keep, votes=votes[keep], sets=sets[keep],
                ferLabels=rows[keep, 2].astype(np.float64), row=rows[keep, 4].copy())


def getFerPlusImdb(dataDir, dataType="CNTK", *, chunk_bytes=64 << 20, device=None, size=(48, 48)):
    """imdb = getFerPlusImdb(opts.dataDir) (ferplus_baselines.m:106; the function itself is not in the reference): reads
    fer2013.csv (emotion,pixels,Usage -- 35,887 rows of 2,304 numbers, about 290 MB of text) and fer2013new.csv (the
    FER+ votes, row for row) from dataDir and returns a FerPlusImdb.  The vote file is read on the host; the pixel file
    is planned on the host (where the fields lie, the two small columns) and its numbers are parsed on the device in
    chunks of about chunk_bytes cut at row boundaries, straight into the layout getBatchFerPlus gathers from -- the
    images are never on the host.  Rows kept: ferPlusKeep.  ValueError: a different row count in the two files, or a
    Usage that is unknown or disagrees with the pixel file's, with the line; a pixel field that is not size[0] * size[1]
    numbers in 0 .. 255 raises _lib.XmError with the line."""
    h = ferPlusPlan(dataDir, dataType)
    N, (H, W) = len(h["votes"]), size
    device = device or torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(N * H * W, dtype=torch.float32, device=device)
    images, _ = vl.pixcsv_decode(h["data"], h["plan"], size=(H, W), transpose=True, out=out, chunk_bytes=chunk_bytes)
    return FerPlusImdb(images, h["votes"], h["sets"], h["ferLabels"], h["row"])


def zoomOut(zoomScale, minYX):
    """ferplus_baselines.m:271-278 (the whole 3 x 3 matrix is scaled, its last row included)."""
    zs = (zoomScale - 1) / zoomScale
    tx = zs - 2 * zs * minYX[1]
    ty = zs - 2 * zs * minYX[0]
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64) * zoomScale


def rotate(theta):
    """ferplus_baselines.m:281-286."""
    return np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]])


def skew(s1, s2):
    """ferplus_baselines.m:289-294."""
    return np.array([[1, s1, 0], [s2, 1, 0], [0, 0, 1]], np.float64)


def _randi(rng, imax, shape):
    """randi(imax, shape...) drawn in MATLAB's column-major order from `rng`."""
    return rng.integers(1, int(imax) + 1, size=int(np.prod(shape))).reshape(shape, order="F")


def computeAugs(batchSize, rng):
    """affs = computeAugs(batchSize) -- ferplus_baselines.m:224-268: 3 x 3 x B affine matrices acting on (x, y, 1),
    zoom * rotate * skew, then about half of them replaced by eye(3).  Draw order as the reference: minXY =
    randi(maxOffset, B, 2) (maxOffset = round(224 / 25) = 9), zoomSc = 0.96 + 0.08 rand(1, B), thetas = randi(3, B) --
    a B x B matrix of which the first B values (column-major) are used, the rest only advances the stream --,
    skews = randi(3, B, 2), drop = rand(1, B) > 0.5.  `rng` is a numpy Generator standing in for MATLAB's."""
    B = int(batchSize)
    ratio = 1 / 25
    maxOffset = int(np.floor(ratio * 224 + 0.5))                     # round(): 8.96 -> 9
    minXY = _randi(rng, maxOffset, (B, 2))
    zoomSc = (1 - ratio) + (ratio * 2) * rng.random(B)
    vals = [-np.pi / 18, 0, np.pi / 18]
    thetas = _randi(rng, 3, (B, B)).reshape(-1, order="F")[:B]       # randi(3, batchSize): B x B
    svals = [-0.1, 0, 0.1]
    skews = _randi(rng, 3, (B, 2))
    affs = np.zeros((3, 3, B))
    for ii in range(B):
        affs[:, :, ii] = (zoomOut(zoomSc[ii], minXY[ii]) @ rotate(vals[thetas[ii] - 1]) @
                          skew(svals[skews[ii, 0] - 1], svals[skews[ii, 1] - 1]))
    drop = np.nonzero(rng.random(B) > 0.5)[0]
    for ii in drop:
        affs[:, :, ii] = np.eye(3)
    return affs


# tmp([5 4 2 1 8 7]) of ferplus_baselines.m:207, 0-based column-major positions of the 3 x 3 matrix
AFFINE_REORDER = [4, 3, 1, 0, 7, 6]


def affine_params(aff):
    """the six vl_nnaffinegrid parameters of a 3 x 3 matrix acting on (x, y, 1): tmp([5 4 2 1 8 7])
    = [a22 a12 a21 a11 a23 a13] -> grid Y = a22 y + a21 x + a23 = y', grid X = a12 y + a11 x + a13 = x'."""
    return np.asarray(aff, np.float64).reshape(-1, order="F")[AFFINE_REORDER]


def getBatchFerPlus(imdb, batch, dataType="CNTK", lossType="distributions", dataAug=True, imageSize=(224, 224),
                    averageImage=(131.0912, 103.8827, 91.4953), rng=None, device=None):
    """inputs = getBatchFerPlus(imdb, batch, opts, dag) -- ferplus_baselines.m:153-221.  Vote distributions over the
    first numClasses columns (1 x 1 x C x N), the single-set assertion, a flip draw per sample in train mode BEFORE
    computeAugs (which is always called: it advances the stream in validation too), identity transforms when dataAug
    is off or outside the training set, the [5 4 2 1 8 7] reorder, and the whole image path -- grey -> flip -> x3 minus
    averageImage -> affine grid -> bilinear sampler at imageSize -- in ONE xm_ferplus_batch launch.  The host draws the
    numbers and uploads two small arrays (int32 [batch indices | flips], float transforms); images, vote
    distributions and hard labels are gathered from the imdb's device-resident copies.
    Returns ['data', data, 'label', votes, 'hardlabel', hardlabel] ('distributions') or ['data', data, 'label',
    hardlabel] ('softmaxlog')."""
    rng = rng or np.random.default_rng(0)
    batch = [int(b) for b in batch]
    N = len(batch)
    numClasses = ferplus_num_classes(dataType)
    setIdx = np.unique(np.asarray(imdb.images["set"])[batch])
    assert setIdx.size == 1, "training/val/test sets have gotten mixed together!"     # :173-174
    device = device or torch.device("cuda", torch.cuda.current_device())
    trainMode = bool(setIdx[0] == 1)
    flips = (rng.random(N) > 0.5).astype(np.int32) if trainMode else np.zeros(N, np.int32)   # :180-186
    augs = computeAugs(N, rng)                                                                # :189
    transforms = np.zeros((6, N), np.float32)
    for i in range(N):
        transforms[:, i] = affine_params(augs[:, :, i] if (dataAug and trainMode) else np.eye(3))   # :190-207
    data_all, probs_all, hard_all = imdb.device_arrays(numClasses, device)
    ints = torch.from_numpy(np.concatenate([np.asarray(batch, np.int32), flips])).to(device)
    tr = torch.from_numpy(transforms.reshape(-1, order="F").copy()).to(device)
    idx = ints[:N].long()
    grey = data_all.index_select(0, idx).permute(3, 2, 1, 0)                     # H x W x 1 x N
    data = vl.ferplus_batch(grey, tr.reshape(N, 6, 1, 1).permute(3, 2, 1, 0), ints[N:], averageImage, imageSize)
    hardlabel = hard_all.index_select(0, idx).reshape(N, 1, 1, 1).permute(3, 2, 1, 0)
    if lossType == "distributions":
        votes = probs_all.index_select(0, idx).reshape(N, numClasses, 1, 1).permute(3, 2, 1, 0)
        return ["data", data, "label", votes, "hardlabel", hardlabel]
    if lossType == "softmaxlog":
        return ["data", data, "label", hardlabel]
    raise ValueError("unknown loss type: %s" % lossType)


def getBatchJpegFaces(files, labels, batch, dag, train, rng, *, read=None, interpolation="bilinear", antialias=False,
                      device=None, split=None, progressive=False, **aug):
    """inputs = getBatch(imdb, batch) over a folder of JPEG faces, the way every MatConvNet getBatch builds one (random
    crop, flip and colour jitter through vl_imreadjpeg's options [EXT]): bind it for train.cnn_train_dag as
        lambda imdb, batch: getBatchJpegFaces(files, labels, batch, dag, imdb.images["set"][batch[0]] == 1, rng, **aug)
    `files`: bytes or paths (with `read(paths) -> list of bytes`, names), `labels`: one class index per file (1-based, as
    vl_nnloss takes them), `batch`: indices into both.  `aug`: vl_imreadjpeg options by name -- CropSize=[0.35, 1],
    CropAnisotropy=[3 / 4, 4 / 3], Flip=True, Brightness=..., Contrast=..., Saturation=....  In train mode they apply
    with CropLocation 'random' and draws from `rng`; otherwise the crop is centred, of the largest CropSize, and nothing is
    drawn.  Both modes resize to meta.normalization.imageSize and, unless meta.normalization says grey=False, go through
    vl.normalize_face (grey -> x3 -> minus averageImage, the FER+ teachers' input); with grey=False averageImage is
    subtracted from the colour image instead.  Returns ['data', Ho x Wo x 3 x N, 'label', 1 x 1 x 1 x N]; no
    synchronisation."""
    norm = dag.meta["normalization"]
    imageSize, avg = [int(v) for v in norm["imageSize"][:2]], norm["averageImage"]
    grey = bool(norm.get("grey", True))
    batch = [int(b) for b in batch]
    datas = [files[b] for b in batch]
    if read is not None:
        datas = read(datas)
    aug = {str(k).lower(): v for k, v in aug.items()}
    unknown = sorted(set(aug) - {"cropsize", "cropanisotropy", "flip", "brightness", "contrast", "saturation"})
    if unknown:
        raise ValueError("getBatchJpegFaces: unknown augmentation %r" % (unknown[0],))
    options = ["Pack", "Resize", imageSize, "Interpolation", interpolation]
    if train:
        options += ["CropLocation", "random"]
        for k, v in aug.items():
            options += [k, bool(v)] if k == "flip" else [k, v]
    else:
        options += ["CropLocation", "center", "CropSize", float(np.max(aug.get("cropsize", 1.0)))]
    if not grey:
        options += ["SubtractAverage", avg]
    data = vl.vl_imreadjpeg(datas, *options, rng=rng if train else None, antialias=antialias, device=device, split=split,
                            progressive=progressive)
    if grey:
        data = vl.normalize_face(data, avg)
    lab = np.asarray(labels, np.float32)[batch]
    label = torch.from_numpy(lab).to(data.device).reshape(len(batch), 1, 1, 1).permute(3, 2, 1, 0)
    return ["data", data, "label", label]
