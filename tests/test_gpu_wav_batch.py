"""GPU: xm_wav_batch / vl.wav_batch -- the batched waveform front-end (crop | resample, zero padding, noise mix;
getBatchEmoVoxCeleb.m:102-135) -- against the float64 oracle, and the provider / run_distillation paths built on it.
L = 16384 (the W = 100 window); banks of 40,000-sample seeded noise tracks.

Resampling allowance: 1e-5 * max|ref| per clip.  The taps are evaluated in fp32 with an exact integer range reduction
of the sine's argument and a power series for I0; a CPU emulation of that arithmetic gave 3e-7 .. 4e-7 * max|y| at the
ratios below, and twenty-one fp32 multiply-adds account for about 1e-6."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

L, TRACK = 16384, 40000
# (p, q, len): small after gcd | coprime, 340,000-tap designs, p > q | p < q | unreduced (gcd 8)
RATIOS = [(1973, 2000, 15000),      # ceil(len p / q) = 14798 < L: exact zeros behind
          (1677, 1600, 15500),
          (16377, 16000, 16000),
          (16813, 16000, 17500),    # ceil(len p / q) = 18390 > L: cut
          (15366, 16000, 17000),
          (15784, 16000, 16500)]


@pytest.fixture(scope="module")
def banks():
    rng = np.random.default_rng(1234)
    wav = (rng.standard_normal(4 * TRACK) * 0.1).astype(np.float32)
    noise = (rng.standard_normal(2 * TRACK) * 0.05).astype(np.float32)
    return wav, noise


@pytest.fixture(scope="module")
def dev_banks(gpu, banks):
    import torch
    return torch.from_numpy(banks[0]).to(gpu), torch.from_numpy(banks[1]).to(gpu)


@pytest.fixture(scope="module")
def resample_case(banks):
    """descriptors of RATIOS (clip k starts 1000 k + 37 samples into track k mod 4) and their float64 references"""
    wav = banks[0].astype(np.float64)
    desc = np.zeros((len(RATIOS), 6), np.int64)
    refs = []
    for k, (p, q, ln) in enumerate(RATIOS):
        src = (k % 4) * TRACK + 1000 * k + 37
        desc[k, :4] = src, ln, p, q
        y = O.resample(wav[src:src + ln], p, q)
        assert y.size == -(-ln * p // q)
        refs.append(y)
    return desc, refs


def _run(dev_banks, desc, ratio=None):
    from mcncrossmodalemotions_amd import vl
    desc = np.asarray(desc, np.int64).reshape(-1, 6)
    ratio = np.zeros(desc.shape[0], np.float32) if ratio is None else ratio
    z = vl.wav_batch(dev_banks[0], dev_banks[1], desc, ratio, L)
    assert tuple(z.shape) == (L, desc.shape[0]) and vl.is_mat(z)
    return vl.to_numpy(z)


def test_resample_against_float64_oracle(dev_banks, resample_case, banks):
    import torch
    from mcncrossmodalemotions_amd import batch
    desc, refs = resample_case
    z = _run(dev_banks, desc)
    worst = worst_host = 0.0
    for k, ref in enumerate(refs):
        n = min(ref.size, L)
        err = np.abs(z[:n, k] - ref[:n]).max() / np.abs(ref).max()
        # xm_resample with the host-designed filter on the same clip (the figure DESIGN 11 quotes next to ours)
        src, ln, p, q = (int(v) for v in desc[k, :4])
        yh = batch.resample(dev_banks[0][src:src + ln], p, q).cpu().numpy()
        err_host = np.abs(yh[:n] - ref[:n]).max() / np.abs(ref).max()
        print("resample %d/%d len %d: wav_batch %.3e  xm_resample %.3e  (of max|ref|)" % (*RATIOS[k][:2], ln, err, err_host))
        worst, worst_host = max(worst, err), max(worst_host, err_host)
        assert err <= 1e-5, (RATIOS[k], err)
        assert (z[n:, k] == 0).all(), RATIOS[k]                 # exact zeros behind ceil(len p / q)
    print("resample worst: wav_batch %.3e  xm_resample %.3e" % (worst, worst_host))
    assert RATIOS[0][2] * RATIOS[0][0] < L * RATIOS[0][1] and refs[3].size > L      # the two length cases are present
    # the unreduced descriptor computes what its reduced form does, to the bit
    d2 = desc[5:6].copy()
    d2[0, 2:4] //= 8
    assert np.array_equal(_run(dev_banks, d2)[:, 0], z[:, 5])


def test_crops_are_bit_equal(dev_banks, banks):
    wav = banks[0]
    cases = [(5, L), (TRACK + 11, 9000), (2 * TRACK, 0), (4 * TRACK - 300, 300), (3 * TRACK + 1, 1)]
    desc = np.array([[s, n, 16000, 16000, 0, 0] for s, n in cases], np.int64)
    desc[1, 2:4] = 7, 7                                          # any p == q is a crop
    z = _run(dev_banks, desc)
    for k, (s, n) in enumerate(cases):
        ref = np.concatenate([wav[s:s + n], np.zeros(L - n, np.float32)])
        assert np.array_equal(z[:, k], ref), cases[k]


def test_noise_mix(dev_banks, banks):
    wav, noise = banks
    cases = [(100, L, 40, L, 0.3), (TRACK + 7, 5000, TRACK + 3, L, 0.125), (77, L, 2 * TRACK - 6000, 6000, 0.2999),
             (9, 0, 555, 1, 1.0)]
    desc = np.array([[s, n, 16000, 16000, ns, nl] for s, n, ns, nl, _ in cases], np.int64)
    ratio = np.array([c[4] for c in cases], np.float32)
    z = _run(dev_banks, desc, ratio)
    plain = _run(dev_banks, np.concatenate([desc[:, :4], np.zeros((len(cases), 2), np.int64)], 1))
    for k, (s, n, ns, nl, _) in enumerate(cases):
        ref = np.concatenate([wav[s:s + n], np.zeros(L - n, np.float32)]).astype(np.float64)
        ref[:nl] += float(ratio[k]) * noise[ns:ns + nl].astype(np.float64)
        err = np.abs(z[:, k] - ref).max()
        print("noise mix case %d: err %.3e, allowance %.3e" % (k, err, 1e-6 * np.abs(ref).max()))
        assert err <= 1e-6 * np.abs(ref).max(), cases[k]
        assert np.array_equal(z[nl:, k], plain[nl:, k]), cases[k]           # untouched behind nlen
    # on a resampled clip the noise covers min(ceil(len p / q), L) samples when the plan says so; the rest stays 0
    p, q, ln = RATIOS[0]
    nl = -(-ln * p // q)
    d = np.array([[37, ln, p, q, 1000, nl]], np.int64)
    zr, z0 = _run(dev_banks, d, np.array([0.25], np.float32))[:, 0], _run(dev_banks, np.array([[37, ln, p, q, 0, 0]]))[:, 0]
    ref = z0.astype(np.float64)
    ref[:nl] += 0.25 * noise[1000:1000 + nl].astype(np.float64)
    assert np.abs(zr - ref).max() <= 1e-6 * np.abs(ref).max() and (zr[nl:] == 0).all()


def test_clips_do_not_depend_on_their_batch(dev_banks, resample_case):
    desc = np.concatenate([resample_case[0][[0, 3, 4]], np.array([[TRACK + 3, 9000, 16000, 16000, 17, L],
                                                                  [3 * TRACK, 12345, 5, 5, 0, 0]], np.int64)])
    desc[1, 4:] = 4000, 7000
    ratio = np.array([0.0, 0.21, 0.0, 0.07, 0.0], np.float32)
    z = _run(dev_banks, desc, ratio)
    for k in range(5):
        alone = _run(dev_banks, desc[k:k + 1], ratio[k:k + 1])
        assert np.array_equal(alone[:, 0], z[:, k]), k
    perm = [3, 0, 4, 2, 1]
    zp = _run(dev_banks, desc[perm], ratio[perm])
    for pos, k in enumerate(perm):
        assert np.array_equal(zp[:, pos], z[:, k]), (pos, k)


def test_descriptors_outside_the_banks(gpu, dev_banks, banks):
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    good = np.array([[0, 100, 16000, 16000, 0, 0]], np.int64)
    r = np.zeros(1, np.float32)
    for field, value in [(0, 4 * TRACK - 50), (0, -1), (1, -1), (2, 0), (3, (1 << 20) + 1), (5, L + 1), (5, -1)]:
        bad = good.copy()
        bad[0, field] = value
        with pytest.raises(ValueError):
            vl.wav_batch(dev_banks[0], dev_banks[1], bad, r, L)
    bad = good.copy()
    bad[0, 4:] = 2 * TRACK - 10, 11
    with pytest.raises(ValueError):
        vl.wav_batch(dev_banks[0], dev_banks[1], bad, r, L)
    with pytest.raises(ValueError):
        vl.wav_batch(dev_banks[0], None, bad, r, L)
    with pytest.raises(ValueError):
        vl.wav_batch(dev_banks[0], dev_banks[1], good[:, :5], r, L)
    # the C entry point itself: the bank lies inside a larger buffer filled with 7 (slack on both sides), so a kernel
    # that read outside [0, wav_len) would show it and still touch memory that exists
    FRONT, BACK = 4096, 3 * L
    wav, noise = banks[0][:TRACK], banks[1][:TRACK]
    buf = torch.full((FRONT + TRACK + BACK,), 7.0, dtype=torch.float32, device=gpu)
    buf[FRONT:FRONT + TRACK].copy_(torch.from_numpy(wav))
    nbuf = torch.full((FRONT + TRACK + BACK,), 7.0, dtype=torch.float32, device=gpu)
    nbuf[FRONT:FRONT + TRACK].copy_(torch.from_numpy(noise))
    p, q = 16377, 16000
    desc = np.array([[TRACK - 5000, L, 16000, 16000, 0, 0],             # crop running off the end
                     [-300, 2000, 16000, 16000, 0, 0],                  # crop starting in front of the bank
                     [TRACK - 9000, 16000, p, q, 0, 0],                 # resample running off the end
                     [100, 1000, 16000, 16000, TRACK - 700, 1500],      # noise running off the end
                     [TRACK + 10, 5000, p, q, -(1 << 40), L],           # everything outside
                     [0, 16000, 0, 16000, 0, 0]], np.int64)             # unusable ratio: zeros
    ratio = np.full(len(desc), 0.5, np.float32)
    dd, dr = torch.from_numpy(desc).to(gpu), torch.from_numpy(ratio).to(gpu)
    z = torch.full((len(desc), L), 3.0, dtype=torch.float32, device=gpu)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)       # noqa: E731
    rc = _lib.load().xm_wav_batch(ptr(buf, FRONT), TRACK, ptr(nbuf, FRONT), TRACK, ptr(dd), ptr(dr), len(desc), ptr(z), L,
                                  vl._stream())
    assert rc == 0
    z = z.cpu().numpy()
    pad = lambda x, n: np.concatenate([x, np.zeros(n - x.size, x.dtype)])     # noqa: E731
    assert np.array_equal(z[0], pad(wav[TRACK - 5000:], L))
    assert np.array_equal(z[1], pad(np.concatenate([np.zeros(300, np.float32), wav[:1700]]), L))
    ref = O.resample(pad(wav[TRACK - 9000:].astype(np.float64), 16000), p, q)
    assert np.abs(z[2, :ref.size] - ref).max() <= 1e-5 * np.abs(ref).max() and (z[2, ref.size:] == 0).all()
    ref = pad(wav[100:1100], L).astype(np.float64)
    ref[:700] += 0.5 * noise[TRACK - 700:].astype(np.float64)
    assert np.abs(z[3] - ref).max() <= 1e-6 * np.abs(ref).max()
    assert (z[4] == 0).all() and (z[5] == 0).all()


def test_argument_errors(gpu, dev_banks):
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    Lb = _lib.load()
    w, nz = dev_banks
    d = torch.zeros(6, dtype=torch.int64, device=gpu)
    r = torch.zeros(1, dtype=torch.float32, device=gpu)
    z = torch.zeros(L, dtype=torch.float32, device=gpu)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    call = lambda wav, noise, desc, ratio, N, out, Lv: Lb.xm_wav_batch(   # noqa: E731
        P(wav), 0 if wav is None else wav.numel(), P(noise), 0 if noise is None else noise.numel(), P(desc), P(ratio), N,
        P(out), Lv, vl._stream())
    assert Lb.xm_version() >= 111
    assert call(w, nz, d, r, 1, z, L) == 0
    assert call(w, None, d, r, 1, z, L) == 0                      # no noise bank: fine while noise_len == 0
    for args in [(None, nz, d, r, 1, z, L), (w, nz, None, r, 1, z, L), (w, nz, d, None, 1, z, L),
                 (w, nz, d, r, 1, None, L), (w, nz, d, r, 1, z, 0), (w, nz, d, r, 1, z, -5), (w, nz, d, r, -1, z, L)]:
        assert call(*args) == 1, args                             # XM_EINVAL
    assert Lb.xm_wav_batch(P(w), w.numel(), None, 5, P(d), P(r), 1, P(z), L, vl._stream()) == 1
    assert call(None, None, None, None, 0, None, L) == 0          # N == 0: XM_OK, nothing is touched
    assert call(w, nz, d, r, 65536, z, L) == 4                    # XM_ETOOBIG, before any launch
    assert tuple(vl.wav_batch(w, nz, np.zeros((0, 6), np.int64), np.zeros(0, np.float32), L).shape) == (L, 0)


# ---- the provider on the fixture of tests/test_wav_batch_cpu.py ------------------------------------------------------
TRACKS, W = [1, 4, 5], 100


@pytest.fixture(scope="module")
def imdb():
    from mcncrossmodalemotions_amd import batch
    return batch.SyntheticEmoVoxImdb(num_tracks=6, seed=9, min_seconds=2.5, max_seconds=6.0)


def _provider(imdb, transformation, wavBatch, idx=TRACKS, seed=77):
    from mcncrossmodalemotions_amd import batch, vl
    inp = batch.getBatchEmoVoxCeleb(imdb, idx, imageSize=(512, W), rng=np.random.default_rng(seed), use_wav=True,
                                    transformation=transformation, wavBatch=wavBatch)
    return {inp[i]: vl.to_numpy(inp[i + 1]) for i in range(0, len(inp), 2)}


@pytest.mark.parametrize("transformation", ["I", "IS", "IN", "ISN", "ISNv"])
def test_provider_batched_front_end(gpu, imdb, transformation):
    from mcncrossmodalemotions_amd import batch
    got, per_clip = _provider(imdb, transformation, True), _provider(imdb, transformation, False)
    assert np.array_equal(got["logitTarget"], per_clip["logitTarget"])
    assert np.array_equal(got["maxLabel"], per_clip["maxLabel"])
    # the oracle's float64 composition of the planned batch (the plan itself: tests/test_wav_batch_cpu.py)
    desc, ratio, _, _ = batch.wav_batch_plan(imdb, TRACKS, W, transformation, np.random.default_rng(77))
    wav = imdb.device_wav_bank(gpu)[0].cpu().numpy().astype(np.float64)
    noise = imdb.device_noise_bank(gpu)[0].cpu().numpy().astype(np.float64)
    for k in range(len(TRACKS)):
        src, ln, p, q, nsrc, nlen = (int(v) for v in desc[k])
        z = wav[src:src + ln] if p == q else O.resample(wav[src:src + ln], p, q)
        z = np.concatenate([z, np.zeros(max(0, L - z.size))])[:L]
        z[:nlen] += float(ratio[k]) * noise[nsrc:nsrc + nlen]
        ref = O.spec_rownorm(O.run_spec(z.astype(np.float32)))[:, :, 0, 0]
        err = np.abs(got["data"][:, :, 0, k] - ref).max() / max(1.0, np.abs(ref).max())
        print("%s clip %d: data err %.3e" % (transformation, k, err))
        assert err <= 2e-3, (transformation, k, err)
    if transformation in ("I", "ISNv"):          # plain crops of whole windows: the same samples reach runSpec
        assert (desc[:, 1] == L).all() and np.array_equal(got["data"], per_clip["data"])


def test_bank_is_the_per_clip_waveform(gpu, imdb):
    import torch
    wav, offs = imdb.device_wav_bank(gpu)
    noise, noffs = imdb.device_noise_bank(gpu)
    assert int(wav.numel()) == offs[-1] == int(np.sum(imdb.num_samples)) and int(noise.numel()) == noffs[-1]
    for ii in (0, 3, 5):
        assert torch.equal(wav[offs[ii]:offs[ii + 1]], imdb.device_wav(ii, gpu))
    for ir in (1, imdb.noisenum):
        assert torch.equal(noise[noffs[ir - 1]:noffs[ir]], imdb.device_noise(ir, gpu))
    assert imdb.device_wav_bank(gpu)[0] is wav                    # built once


def test_run_distillation_on_waveforms(gpu, tmp_path, monkeypatch):
    """run_distillation(useWav, transformation='ISN'): finite objectives, and 'v' in front of the transformation of
    every validation batch and of no training batch (getBatchEmoVoxCeleb.m:14-25)."""
    from mcncrossmodalemotions_amd import batch
    from mcncrossmodalemotions_amd.run_distillation import run_distillation
    seen = []
    inner = batch.getBatchEmoVoxCeleb

    def spy(imdb_, b, **kw):
        seen.append((int(imdb_.set[b[0]]), kw["transformation"], kw.get("use_wav"), kw.get("wavBatch")))
        return inner(imdb_, b, **kw)

    monkeypatch.setattr(batch, "getBatchEmoVoxCeleb", spy)
    net, info = run_distillation(gpus=[0], numSeconds=1, batchSize=4, numEpochs=1, miniEpochRatio=1.0, miniVal=0.5,
                                 numTracks=16, widthMult=0.125, dataDir=str(tmp_path), learningRate=[1e-3],
                                 useWav=True, transformation="ISN")
    assert net.meta["augmentation"]["transformation"] == "ISN"
    assert np.isfinite(info["train"][0]["objective"]) and np.isfinite(info["val"][0]["objective"])
    train_tr = {t for s, t, _, _ in seen if s == 1}
    val_tr = {t for s, t, _, _ in seen if s != 1}
    assert train_tr == {"ISN"} and val_tr == {"vISN"}, seen
    assert all(u and b for _, _, u, b in seen)
    assert info["train"][0]["num"] == 12 and info["val"][0]["num"] == 2
