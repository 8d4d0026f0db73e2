"""GPU: vl.audioread / xm_wav_decode_batch against the samples stored in tests/golden/wav_small.npz and the numpy
restatement of tests/test_wav_read_cpu.py -- bit for bit, as uint32, every conversion is exact or a defined rounding --
alone and in ragged batches with guard words around the bank, with ranges, channels and out_base, the launch count, and
batch.WavFileEmoVoxImdb / external.compute_audio_feats_files against the same functions fed numpy-decoded floats."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_wav_read_cpu import (F32, F64, GOLDEN, S16, S24, S32, U8, bits, files_of, np_decode, np_parse, random_values,
                               wav_bytes)

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, 0xDEADBEEF - (1 << 32)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def names(golden):
    return [str(n) for n in golden["names"]]


def decode_guarded(gpu, files, ranges=None, channel=None, shift=0, out_base=0, bank=None):
    """xm_wav_decode_batch into a bank with guard words on both sides (`shift` moves the bank's address by that many
    floats) -> (uint32 numpy bank, rows); the guards are checked"""
    from mcncrossmodalemotions_amd import _lib, vl
    buf, plan = vl.wav_plan(files, ranges, channel, out_base)
    n = out_base + plan["floats"]
    if bank is None:
        bank = torch.full((GUARD + shift + n + GUARD,), SENTINEL, dtype=torch.int32, device=gpu)
    assert bank.numel() == GUARD + shift + n + GUARD
    dev = torch.from_numpy(buf).to(gpu)
    p = dev.data_ptr()
    _lib.check(_lib.load().xm_wav_decode_batch(C.c_void_p(p), plan["nbytes"], C.c_void_p(p + plan["desc"][0]), plan["N"],
                                               C.c_void_p(bank.data_ptr() + 4 * (GUARD + shift)), n,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    host = bank.cpu().numpy().view(np.uint32)
    guard = np.uint32(SENTINEL & 0xFFFFFFFF)
    assert (host[:GUARD + shift + out_base] == guard).all() and (host[GUARD + shift + n:] == guard).all()
    return host[GUARD + shift:GUARD + shift + n], plan["rows"].copy(), bank


@pytest.fixture(scope="module")
def singles(gpu, golden, names):
    """every fixture decoded alone through vl.audioread: name -> (uint32 samples, info)"""
    from mcncrossmodalemotions_amd import vl
    out = {}
    for n in names:
        bank, offs, info = vl.audioread([golden["bytes_" + n].tobytes()], return_info=True)
        assert list(offs) == [0, bank.numel()]
        out[n] = (bank.cpu().numpy().view(np.uint32), info[0])
    return out


@pytest.mark.parametrize("k", range(42))
def test_every_fixture_alone_equals_its_bits(singles, golden, names, k):
    assert len(names) == 42
    got, info = singles[names[k]]
    want, meta = golden["exp_" + names[k]], golden["meta_" + names[k]]
    assert (info["SampleRate"], info["NumChannels"], info["BitsPerSample"], info["TotalSamples"], int(info["Truncated"])) == \
        (meta[0], meta[1], meta[2], meta[4], meta[5])
    assert got.shape == want.shape and np.array_equal(got, want), (names[k], np.nonzero(got != want)[0][:8])


def ragged_order(names, seed):
    s = names.index("streamed_s16_m30")
    order = [int(i) for i in np.random.default_rng(seed).permutation(len(names)) if i != s]
    order.insert(len(order) // 2, s)          # the odd-length file in the middle: odd file starts behind it
    return order


@pytest.mark.parametrize("seed,shift", [(7, 0), (21, 3)])
def test_one_ragged_batch_of_all_fixtures(gpu, golden, names, seed, shift):
    order = ragged_order(names, seed)
    files = files_of(golden, [names[i] for i in order])
    starts = np.concatenate([[0], np.cumsum([len(f) for f in files])])[:-1]
    assert {int(s) % 16 for s in starts} == set(range(16))
    got, rows, _ = decode_guarded(gpu, files, shift=shift)
    want = np.concatenate([golden["exp_" + names[i]] for i in order])
    assert got.shape == want.shape
    for j, i in enumerate(order):
        a, b = int(rows[j, 11]), int(rows[j, 11] + rows[j, 8] * rows[j, 9])
        assert np.array_equal(got[a:b], golden["exp_" + names[i]]), (j, names[i])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt", [U8, S16, S24, S32, F32, F64])
def test_ranges_equal_slices_of_the_whole_decode(gpu, fmt):
    T = 1100
    data = wav_bytes(fmt, random_values(np.random.default_rng(50 + fmt), fmt, T))
    whole, _, _ = decode_guarded(gpu, [data])
    assert np.array_equal(whole, bits(np_decode(data)))
    ranges = [(1, T), (2, T - 1), (T, T), (60, 70), (250, 260), (1020, 1030), (1, 1), (64, 65), (1024, -1)]
    got, rows, _ = decode_guarded(gpu, [data] * len(ranges), ranges, shift=1)
    for (a, b), r in zip(ranges, rows):
        b = T if b == -1 else b
        assert int(r[8]) == b - a + 1
        assert np.array_equal(got[int(r[11]):int(r[11] + r[8])], whole[a - 1:b]), (a, b)


def test_channels(gpu, golden, names):
    st = [n for n in names if golden["meta_" + n][1] >= 2]
    assert len(st) == 5
    files = files_of(golden, st)
    allc, rows, _ = decode_guarded(gpu, files)
    for n, r in zip(st, rows):
        assert np.array_equal(allc[int(r[11]):int(r[11] + r[8] * r[9])], golden["exp_" + n]), n      # column-major matrix
    for c in (0, 1):
        one, rows1, _ = decode_guarded(gpu, files, channel=c, shift=2)
        for n, r in zip(st, rows1):
            frames = int(r[8])
            assert int(r[9]) == 1 and np.array_equal(one[int(r[11]):int(r[11]) + frames], golden["exp_" + n][c * frames:(c + 1) * frames]), (n, c)
    # ranges and a channel together, a longer interleaved file of every format (windows across frames 64 and 256)
    rng = np.random.default_rng(9)
    for fmt in (U8, S16, S24, S32, F32, F64):
        v = random_values(rng, fmt, 300, 3)
        data = wav_bytes(fmt, v)
        ref = bits(np_decode(data)).reshape(3, 300)
        ranges = [(1, 300), (60, 70), (250, 260), (2, 299)]
        got, rows, _ = decode_guarded(gpu, [data] * 4, ranges, channel=2, shift=1)
        for (a, b), r in zip(ranges, rows):
            assert np.array_equal(got[int(r[11]):int(r[11] + r[8])], ref[2, a - 1:b]), (fmt, a, b)
        got, rows, _ = decode_guarded(gpu, [data] * 4, ranges)
        for (a, b), r in zip(ranges, rows):
            assert np.array_equal(got[int(r[11]):int(r[11] + 3 * r[8])], ref[:, a - 1:b].reshape(-1)), (fmt, a, b)


def test_chunked_decode_through_out_base_equals_the_single_call(gpu, golden, names):
    from mcncrossmodalemotions_amd import vl
    files = files_of(golden, names)
    single, rows, _ = decode_guarded(gpu, files)
    n = single.size
    bank = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=gpu)
    view = bank[GUARD:GUARD + n].view(torch.float32)
    cuts, offs = [0, 5, 6, 17, 30, len(files)], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out, o = vl.audioread(files[a:b], out=view, out_base=int(rows[a, 11]))
        assert out.data_ptr() == view.data_ptr() and int(o[0]) == int(rows[a, 11])
        offs.append(o)
    torch.cuda.synchronize()
    host = bank.cpu().numpy().view(np.uint32)
    assert (host[:GUARD] == host[0]).all() and (host[-GUARD:] == host[0]).all() and host[0] == np.uint32(SENTINEL & 0xFFFFFFFF)
    assert np.array_equal(host[GUARD:GUARD + n], single)
    assert int(offs[-1][-1]) == n
    with pytest.raises(ValueError, match="do not fit"):
        vl.audioread(files[:3], out=view[:10])
    with pytest.raises(ValueError, match="out_base needs out"):
        vl.audioread(files[:3], out_base=4)


def test_out_base_past_2_31(gpu, golden):
    """output indices are 64-bit: a small batch decoded behind float 2^31 of a bank of 8.6 GB"""
    from mcncrossmodalemotions_amd import vl
    if torch.cuda.mem_get_info()[0] < 12 << 30:
        pytest.skip("needs 12 GB of free device memory")
    base = (1 << 31) + 5
    files = files_of(golden, ["s16_m257", "s24_st21", "f64_m64"])
    want = np.concatenate([golden["exp_" + n] for n in ("s16_m257", "s24_st21", "f64_m64")])
    bank = torch.empty(base + want.size + 8, dtype=torch.float32, device=gpu)
    edge = bank[base - 8:].view(torch.int32)
    edge.fill_(SENTINEL)
    _, offs = vl.audioread(files, out=bank, out_base=base)
    got = edge.cpu().numpy().view(np.uint32)
    guard = np.uint32(SENTINEL & 0xFFFFFFFF)
    assert int(offs[0]) == base and int(offs[-1]) == base + want.size
    assert (got[:8] == guard).all() and (got[-8:] == guard).all() and np.array_equal(got[8:-8], want)


def _launches(L, fn):
    from mcncrossmodalemotions_amd import prof
    return {r.name: r.launches for r in prof.kernels_run(fn, L)[1]}


def test_one_launch_whatever_n(gpu, golden, names):
    from mcncrossmodalemotions_amd import _lib, vl
    L = _lib.load()
    files = files_of(golden, names)
    one = _launches(L, lambda: vl.audioread(files[7:8]))
    every = _launches(L, lambda: vl.audioread(files))
    print("launches:", every)
    assert one == every == {"wav_decode_kernel": 1}
    empty = files_of(golden, ["empty_s16"])
    bank, offs = vl.audioread(empty * 2)
    assert bank.numel() == 0 and list(offs) == [0, 0, 0]
    assert vl.audioread([])[0].numel() == 0


# ------------------------------------------------------------------------------------------------ WavFileEmoVoxImdb
FS = 16000


def pcm16_track(rng, seconds):
    v = (rng.standard_normal((int(seconds * FS), 1)) * 3000).clip(-32768, 32767).astype(np.int16)
    return wav_bytes(S16, v)


@pytest.fixture(scope="module")
def wav_imdb(gpu):
    """8 PCM16 tracks of 1.3 - 2.5 s, a ninth of 0.7 s, 3 noise files; the file-backed imdb next to a stand-in that
    holds the numpy-decoded floats"""
    from mcncrossmodalemotions_amd import batch as xbatch
    rng = np.random.default_rng(77)
    secs = list(np.linspace(1.3, 2.5, 8) + rng.random(8) * 0.01) + [0.7]
    tracks = {"id%05d/clip%d.wav" % (k, k): pcm16_track(rng, s) for k, s in enumerate(secs)}
    noise = [pcm16_track(rng, s) for s in (2.2, 1.9, 2.6)]
    logits = [np.asfortranarray(rng.standard_normal((xbatch.time2idx(np_parse(t)["total"] / FS), 8)).astype(np.float32) * 3)
              for t in tracks.values()]
    imdb = xbatch.WavFileEmoVoxImdb(tracks, logits, noise=noise)

    class StandIn(xbatch.SyntheticEmoVoxImdb):
        def __init__(self):
            self.fs, self.seed, self._dev = FS, 0, None
            self.wavs = [np_decode(t) for t in tracks.values()]
            self.noises = [np_decode(t) for t in noise]
            self.num_samples = np.array([w.size for w in self.wavs], np.int64)
            self.wavLogits = logits
            self.set = np.ones(len(self.wavs), int)
            self.noisenum, self.noiselen, self.noisevol = 3, min(w.size for w in self.noises), 0.3

        def noise_offsets(self):
            return np.concatenate([[0], np.cumsum([w.size for w in self.noises])]).astype(np.int64)

        def device_wav_bank(self, device):
            if "_wb" not in self.__dict__:
                self._wb = torch.from_numpy(np.concatenate(self.wavs)).to(device)
            return self._wb, self.wav_offsets()

        def device_noise_bank(self, device):
            if "_nb" not in self.__dict__:
                self._nb = torch.from_numpy(np.concatenate(self.noises)).to(device)
            return self._nb, self.noise_offsets()

    return imdb, StandIn(), tracks, noise


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_wav_file_imdb_bank_and_batches(gpu, wav_imdb):
    from mcncrossmodalemotions_amd import batch as xbatch
    imdb, ref, tracks, noise = wav_imdb
    assert imdb.fs == FS and np.array_equal(imdb.num_samples, ref.num_samples) and imdb.noisenum == 3
    assert imdb.noiselen == ref.noiselen == int(1.9 * FS) and np.array_equal(imdb.noise_offsets(), ref.noise_offsets())
    bank, offs = imdb.device_wav_bank(gpu)
    assert np.array_equal(offs, ref.wav_offsets())
    assert np.array_equal(bank.cpu().numpy().view(np.uint32), bits(np.concatenate(ref.wavs)))
    nb, _ = imdb.device_noise_bank(gpu)
    assert np.array_equal(nb.cpu().numpy().view(np.uint32), bits(np.concatenate(ref.noises)))
    assert imdb.device_wav(3, gpu).data_ptr() == bank.data_ptr() + 4 * int(offs[3])                    # a view of the bank
    assert np.array_equal(imdb.device_wav(3, gpu).cpu().numpy(), ref.wavs[3])
    assert np.array_equal(imdb.device_noise(2, gpu).cpu().numpy(), ref.noises[1])
    # 'ISN' at width 100: equal draws, equal banks -> equal bits
    out = []
    for im in (imdb, ref):
        out.append(xbatch.getBatchEmoVoxCeleb(im, range(8), imageSize=(512, 100), transformation="ISN", rng=np.random.default_rng(5),
                                              device=gpu, use_wav=True, wavBatch=True))
    assert out[0][0::2] == out[1][0::2] == ["data", "logitTarget", "maxLabel"]
    assert tuple(out[0][1].shape) == (512, 100, 1, 8)
    for a, b in zip(out[0][1::2], out[1][1::2]):
        assert same_bits(a, b)
    # 'I' with the 0.7 s track: the zero-padded path
    L = int(round(xbatch.aud_samples(100)))
    desc, _, _, _ = xbatch.wav_batch_plan(imdb, [1, 8, 3], 100, "I", np.random.default_rng(6))
    assert int(desc[1, 1]) == int(imdb.num_samples[8]) < L and int(desc[0, 1]) == L
    out = [xbatch.getBatchEmoVoxCeleb(im, [1, 8, 3], imageSize=(512, 100), transformation="I", rng=np.random.default_rng(6),
                                      device=gpu, use_wav=True, wavBatch=True) for im in (imdb, ref)]
    for a, b in zip(out[0][1::2], out[1][1::2]):
        assert same_bits(a, b)
    assert bool(torch.isfinite(out[0][1]).all())


def test_wav_file_imdb_chunks_and_refusals(gpu, wav_imdb, tmp_path):
    from mcncrossmodalemotions_amd import batch as xbatch
    imdb, ref, tracks, noise = wav_imdb
    want = bits(np.concatenate(ref.wavs))
    small = xbatch.WavFileEmoVoxImdb(tracks, ref.wavLogits, chunkBytes=1000)          # smaller than any file
    assert np.array_equal(small.device_wav_bank(gpu)[0].cpu().numpy().view(np.uint32), want)
    calls = []
    names = list(tracks)

    def read(ns):
        calls.append(list(ns))
        return [tracks[n] for n in ns]

    some = xbatch.WavFileEmoVoxImdb(read, ref.wavLogits, names=names, chunkBytes=150000)
    assert np.array_equal(some.device_wav_bank(gpu)[0].cpu().numpy().view(np.uint32), want)
    for n in names:
        p = tmp_path / n
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(tracks[n])
    nd = tmp_path / "noise"
    nd.mkdir()
    for k, f in enumerate(noise):
        (nd / ("%02d.wav" % (k + 1))).write_bytes(f)
    disk = xbatch.WavFileEmoVoxImdb.from_dir(str(tmp_path), names, ref.wavLogits, noiseDir=str(nd))
    assert disk.noisenum == 3 and np.array_equal(disk.device_wav_bank(gpu)[0].cpu().numpy().view(np.uint32), want)
    rng = np.random.default_rng(1)
    stereo = wav_bytes(S16, random_values(rng, S16, 30000, 2))
    slow = wav_bytes(S16, random_values(rng, S16, 30000, 1), rate=8000)
    for bad, what in ((stereo, "channels"), (slow, "8000 Hz")):
        with pytest.raises(ValueError, match=what) as e:
            xbatch.WavFileEmoVoxImdb({"a.wav": tracks[names[0]], "b.wav": bad}, ref.wavLogits[:2])
        assert "b.wav" in str(e.value)
    with pytest.raises(ValueError, match="8000 Hz"):
        xbatch.WavFileEmoVoxImdb(tracks, ref.wavLogits, noise=[noise[0], slow])


# ------------------------------------------------------------------------------------------------ compute_audio_feats_files
def test_compute_audio_feats_files(gpu, tmp_path):
    from mcncrossmodalemotions_amd import external, zoo
    rng = np.random.default_rng(12)
    lens = [16247, 20000, 30001, 32245, 40000, 47000]                      # 100, 123, 186 | 200, 248, 292 frames
    files = [wav_bytes(S16, (rng.standard_normal((n, 2)) * 2500).clip(-32768, 32767).astype(np.int16), rate=r)
             for n, r in zip(lens, (16000, 16000, 44100, 16000, 8000, 16000))]   # no rate check, as upstream
    T, rsize, _, _ = external.audio_feats_plan(lens, np.concatenate([[0], np.cumsum(lens)])[:-1])
    assert sorted(set(rsize)) == [100, 200] and list(T) == [100, 123, 186, 200, 248, 292]
    left = [np_decode(f, channel=0) for f in files]
    net = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=9)
    bank = torch.from_numpy(np.concatenate(left)).to(gpu)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    want = external.compute_audio_feats_wav(net, bank, offs)
    got = external.compute_audio_feats_files(net, files)
    assert got.shape == want.shape == (6, 8) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    paths = []
    for k, f in enumerate(files):
        paths.append(str(tmp_path / ("%d.wav" % k)))
        open(paths[-1], "wb").write(f)
    few = external.compute_audio_feats_files(net, paths, limit=3, maxBatch=2)
    assert few.shape == (4, 8) and np.array_equal(few.view(np.uint32), external.compute_audio_feats_wav(net, bank, offs, limit=3, maxBatch=2).view(np.uint32))
    three = wav_bytes(S16, random_values(rng, S16, 20000, 3))
    with pytest.raises(ValueError, match="unexpected number of streams"):
        external.compute_audio_feats_files(net, files[:2] + [three])
