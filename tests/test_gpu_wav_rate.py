"""GPU: vl.audioread(fs=) / xm_wav_decode_resample_batch -- WAV files of 48000, 44100, 22050, 11025, 8000, 32000, 192000
and 16000 Hz decoded and resampled to 16000 Hz in one pass.
  * against oracle.resample(np_decode(file).astype(float64), fs, rate), the float64 restatement of MATLAB's resample, within
    1e-5 * max|ref| (the allowance tests/test_gpu_wav_batch.py uses for this resampler; fp32 accumulation over the at most
    241 taps of a 192 kHz file stays some 30 times below it);
  * bit for bit against vl.wav_batch on the natively decoded bank (one resampler in the library), against vl.audioread
    without fs for the 16 kHz files, between a file alone and among others, and between one call and chunked calls;
  * at the edges: files of 1, 2 and 3 frames, an empty file between two others, several files inside one tile, outputs that
    end at, one before and one after a tile boundary (xm_wav_resample_geometry), ranges, interleaved channels;
  * through batch.WavFileEmoVoxImdb(resample=True, channel=0) and external.compute_audio_feats_files(fs=16000).
Guard words around the bank show that nothing outside the batch is written."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from test_wav_read_cpu import F32, F64, S16, S24, S32, U8, bits, np_decode, np_parse, random_values, wav_bytes

pytestmark = pytest.mark.gpu
FS = 16000
RATES = [48000, 44100, 22050, 11025, 8000, 32000, 192000, 16000]
FORMATS = [U8, S16, S24, S32, F32, F64]
GUARD, SENTINEL = 64, 0xDEADBEEF - (1 << 32)
TOL = 1e-5


def ceil_div(a, b):
    return -(-a // b)


def make(fmt, frames, rate, nch=1, seed=0, odd=False):
    """a WAV file; odd=True drops the pad byte of an odd data chunk so that the next file of a batch starts at an odd byte"""
    if frames == 0:
        one = wav_bytes(fmt, random_values(np.random.default_rng(seed), fmt, 1, nch), rate)
        return one[:4] + struct.pack("<I", 36) + one[8:40] + struct.pack("<I", 0)
    data = wav_bytes(fmt, random_values(np.random.default_rng(seed), fmt, frames, nch), rate)
    if odd:
        assert len(data) % 2 == 0 and np_parse(data)["total"] * np_parse(data)["align"] % 2 == 1
        data = data[:-1]
    return data


def oracle_file(data, fs=FS, rng=None, channel=None):
    """float64: resample(audioread(file, rng)(:, channels), fs, rate) column by column, flattened in MATLAB layout"""
    from oracle import oracle as O
    w = np_parse(data)
    x = np_decode(data, rng, channel).astype(np.float64)
    cw = 1 if channel is not None else w["nch"]
    if x.size == 0:
        return np.zeros(0)
    return np.concatenate([O.resample(c, fs, w["rate"]) for c in x.reshape(cw, -1)])


def read_guarded(gpu, files, ranges=None, channel=None, shift=0, fs=FS):
    """xm_wav_decode_resample_batch into a bank with guard words on both sides (`shift` moves the bank's address by that
    many floats) -> (float32 numpy bank, rows); the guards are checked"""
    from mcncrossmodalemotions_amd import _lib, vl
    buf, plan = vl.wav_plan(files, ranges, channel, 0, fs=fs)
    n = plan["floats"]
    bank = torch.full((GUARD + shift + n + GUARD,), SENTINEL, dtype=torch.int32, device=gpu)
    dev = torch.from_numpy(buf).to(gpu)
    p = dev.data_ptr()
    _lib.check(_lib.load().xm_wav_decode_resample_batch(C.c_void_p(p), plan["nbytes"], C.c_void_p(p + plan["desc"][0]), plan["N"],
                                                        C.c_void_p(bank.data_ptr() + 4 * (GUARD + shift)), n,
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    host = bank.cpu().numpy().view(np.uint32)
    guard = np.uint32(SENTINEL & 0xFFFFFFFF)
    assert (host[:GUARD + shift] == guard).all() and (host[GUARD + shift + n:] == guard).all()
    return host[GUARD + shift:GUARD + shift + n].view(np.float32), plan["rows"].copy()


def check_close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    scale = np.abs(ref).max()
    if scale == 0:
        assert not got.any(), what
        return 0.0
    err = np.abs(got.astype(np.float64) - ref).max() / scale
    assert err <= TOL, (what, err)
    return err


def pieces(bank, rows):
    out = []
    for r in rows:
        n = ceil_div(int(r[8]) * int(r[14]), int(r[15])) * int(r[9])
        out.append(bank[int(r[11]):int(r[11]) + n])
    return out


# ------------------------------------------------------------------------------------------------ one mixed batch
@pytest.fixture(scope="module")
def mixed():
    """every rate in every format once and more: 16 files, the formats walking against the rates, lengths of 700 .. 5200
    frames with every remainder class, 24-bit and 8-bit files of odd length so that later files start at odd bytes, one
    stereo file; with their float64 references"""
    rng = np.random.default_rng(2024)
    files, meta = [], []
    for k in range(16):
        rate, fmt = RATES[k % 8], FORMATS[(k + k // 8 * 3) % 6]
        frames = int(rng.integers(700, 5200)) | 1                       # odd counts: U8 and S24 mono bodies are odd
        nch = 2 if k == 9 else 1
        odd = fmt in (U8, S24) and nch == 1
        files.append(make(fmt, frames, rate, nch, seed=100 + k, odd=odd))
        meta.append((rate, fmt, frames, nch))
    assert {m[1] for m in meta} == set(FORMATS) and {(m[0], m[1]) for m in meta if m[1] == S24} >= {(22050, S24)}
    starts = np.concatenate([[0], np.cumsum([len(f) for f in files])])[:-1]
    assert any(int(s) & 1 for s in starts)
    return files, meta, [oracle_file(f) for f in files]


@pytest.mark.parametrize("shift", [0, 3])
def test_mixed_batch_equals_the_oracle(gpu, mixed, shift):
    from mcncrossmodalemotions_amd import vl
    files, meta, refs = mixed
    bank, rows = read_guarded(gpu, files, shift=shift)
    worst = 0.0
    for k, (got, ref) in enumerate(zip(pieces(bank, rows), refs)):
        assert got.size == ceil_div(meta[k][2] * FS, meta[k][0]) * meta[k][3]
        worst = max(worst, check_close(got, ref, (k, meta[k])))
    print("worst error over max|ref|: %.3g" % worst)
    # the 16 kHz files: a copy, bit for bit what audioread without fs gives
    same = [k for k, m in enumerate(meta) if m[0] == FS]
    assert len(same) == 2
    plain, offs = vl.audioread([files[k] for k in same])
    plain = plain.cpu().numpy()
    for j, k in enumerate(same):
        assert np.array_equal(bits(pieces(bank, rows)[k]), bits(plain[int(offs[j]):int(offs[j + 1])])), k
    # through vl.audioread: the same bits, offsets in output floats, the info dicts
    got, offs, info = vl.audioread(files, fs=FS, return_info=True)
    assert np.array_equal(bits(got.cpu().numpy()), bits(bank)) and list(offs[:-1]) == list(rows[:, 11]) and offs[-1] == bank.size
    for i, m in zip(info, meta):
        assert (i["SampleRate"], i["TotalSamples"], i["NumChannels"], i["ResampledSamples"]) == (m[0], m[2], m[3], ceil_div(m[2] * FS, m[0]))


def test_two_launches_whatever_the_batch(gpu, mixed):
    from mcncrossmodalemotions_amd import _lib, prof, vl
    L = _lib.load()
    files = mixed[0]
    run = lambda fn: {r.name: r.launches for r in prof.kernels_run(fn, L)[1]}   # noqa: E731
    one, every = run(lambda: vl.audioread(files[1:2], fs=FS)), run(lambda: vl.audioread(files, fs=FS))
    assert one == every == {"wav_rate_gain_kernel": 1, "wav_resample_kernel": 1}
    assert vl.wav_resample_geometry()[1] == 2
    assert run(lambda: vl.audioread(files)) == {"wav_decode_kernel": 1}          # the default path is the old kernel
    bank, offs = vl.audioread([make(S16, 0, 48000)] * 2, fs=FS)
    assert bank.numel() == 0 and list(offs) == [0, 0, 0] and vl.audioread([], fs=FS)[0].numel() == 0


# ------------------------------------------------------------------------------------------------ one resampler
def test_bit_equal_to_wav_batch_on_the_decoded_bank(gpu):
    """every rate at a few thousand frames: vl.wav_batch of {src, frames, fs, rate, 0, 0} on the natively decoded bank"""
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(31)
    frames = [int(rng.integers(3000, 6000)) for _ in RATES]
    frames[6] = 9001                                                     # 192 kHz: the longest tap loop the plan accepts
    files = [make(FORMATS[k % 6], n, r, seed=300 + k) for k, (n, r) in enumerate(zip(frames, RATES))]
    native, noffs = vl.audioread(files)
    want = [ceil_div(n * FS, r) for n, r in zip(frames, RATES)]
    L = max(want) + 5
    desc = np.array([[noffs[k], frames[k], FS, RATES[k], 0, 0] for k in range(8)], np.int64)
    z = vl.wav_batch(native, None, desc, np.zeros(8, np.float32), L).cpu().numpy()        # L x N
    got, offs = vl.audioread(files, fs=FS)
    got = got.cpu().numpy()
    assert list(np.diff(offs)) == want
    for k in range(8):
        a = got[int(offs[k]):int(offs[k + 1])]
        assert np.array_equal(bits(a), bits(z[:want[k], k])), (RATES[k], np.nonzero(bits(a) != bits(z[:want[k], k]))[0][:8])
        assert not z[want[k]:, k].any()
    check_close(got[int(offs[6]):int(offs[7])], oracle_file(files[6]), "192 kHz")


# ------------------------------------------------------------------------------------------------ edges
def test_files_shorter_than_the_filter_and_an_empty_file(gpu):
    """1, 2 and 3 frames at every rate -- shorter than the filter on both sides, many files inside one tile --, with an
    empty file between two others"""
    files = []
    for k, rate in enumerate(RATES):
        for n in (1, 2, 3):
            files.append(make(FORMATS[(k + n) % 6], n, rate, seed=500 + 3 * k + n))
        if k % 3 == 0:
            files.append(make(S16, 0, rate))
    bank, rows = read_guarded(gpu, files, shift=1)
    from mcncrossmodalemotions_amd import vl
    assert bank.size < vl.wav_resample_geometry()[0]
    empties = [k for k, r in enumerate(rows) if r[8] == 0]
    assert len(empties) == 3 and all(rows[k, 11] == rows[k + 1, 11] for k in empties)
    for k, (got, f) in enumerate(zip(pieces(bank, rows), files)):
        check_close(got, oracle_file(f), k)


def test_outputs_ending_around_a_tile_boundary(gpu):
    from mcncrossmodalemotions_amd import vl
    tile, _ = vl.wav_resample_geometry()
    tail = make(S24, 1001, 44100, seed=7, odd=True)
    after = make(S16, 3 * tile + 1501, 48000, seed=8)                   # more than one whole tile of its own
    ref_tail, ref_after = oracle_file(tail), oracle_file(after)
    alone = None
    for d in (-1, 0, 1):
        n = 2 * tile + d                                                 # outputs of the first file
        head = make(S16, 3 * n - 1, 48000, seed=9)                       # ceil((3 n - 1) / 3) = n
        bank, rows = read_guarded(gpu, [head, tail, after], shift=2 + d)
        assert list(rows[:, 11]) == [0, n, n + ref_tail.size]
        a, b, c = pieces(bank, rows)
        ref_head = oracle_file(head)
        check_close(a, ref_head, ("head", d))
        check_close(b, ref_tail, ("tail", d))
        check_close(c, ref_after, ("after", d))
        # wherever the tiles fall, the same bits
        if alone is None:
            alone = (bits(read_guarded(gpu, [tail])[0]), bits(read_guarded(gpu, [after])[0]))
        assert np.array_equal(bits(b), alone[0]) and np.array_equal(bits(c), alone[1])


def test_a_range_is_cut_before_resampling(gpu):
    T = 3000
    data = make(S16, T, 44100, seed=11)
    ranges = [(1, T), (500, 2000), (2, T - 1), (T, T), (1000, 1002), (1, 441)]
    bank, rows = read_guarded(gpu, [data] * len(ranges), ranges)
    for (a, b), got in zip(ranges, pieces(bank, rows)):
        ref = oracle_file(data, rng=(a, b))                              # the cut vector: zero outside, not the neighbours
        assert got.size == ceil_div((b - a + 1) * 160, 441)
        check_close(got, ref, (a, b))
    stereo = make(S24, 1500, 22050, nch=2, seed=12)
    bank, rows = read_guarded(gpu, [stereo, stereo], [(100, 1200), (1, -1)], channel=1)
    check_close(pieces(bank, rows)[0], oracle_file(stereo, rng=(100, 1200), channel=1), "stereo range")
    check_close(pieces(bank, rows)[1], oracle_file(stereo, channel=1), "stereo whole")


@pytest.mark.parametrize("fmt", [S24, F64])
def test_interleaved_three_channels(gpu, fmt):
    from mcncrossmodalemotions_amd import vl
    tile, _ = vl.wav_resample_geometry()
    data = make(fmt, 2 * tile + 123, 22050, nch=3, seed=13)              # every channel crosses tile boundaries
    lead = make(U8, 77, 8000, seed=14, odd=True)
    bank, rows = read_guarded(gpu, [lead, data])
    n = ceil_div((2 * tile + 123) * 320, 441)
    got = pieces(bank, rows)[1]
    ref = oracle_file(data)
    assert got.size == 3 * n
    check_close(got, ref, "all channels")
    one, rows1 = read_guarded(gpu, [lead, data], channel=0, shift=1)
    assert np.array_equal(bits(pieces(one, rows1)[1]), bits(got[:n]))
    with pytest.raises(Exception, match="channel 1"):
        read_guarded(gpu, [lead, data], channel=1)                       # the lead file is mono
    mid, rowsm = read_guarded(gpu, [data], channel=1)
    assert np.array_equal(bits(mid), bits(got[n:2 * n]))
    check_close(mid, ref[n:2 * n], "channel 1")


def test_alone_and_among_nine_others_the_same_bits(gpu, mixed):
    from mcncrossmodalemotions_amd import vl
    files = mixed[0]
    for k in (1, 6, 9):                                                  # 44100 Hz, 192000 Hz, the stereo file
        alone, _ = vl.audioread([files[k]], fs=FS)
        others = [f for j, f in enumerate(files) if j != k][:9]
        among, offs = vl.audioread(others[:4] + [files[k]] + others[4:], fs=FS)
        assert torch.equal(alone.view(torch.int32), among[int(offs[4]):int(offs[5])].view(torch.int32)), k


def test_chunked_calls_equal_one_call(gpu, mixed):
    from mcncrossmodalemotions_amd import vl
    files = mixed[0]
    single, offs = vl.audioread(files, fs=FS)
    n = single.numel()
    bank = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=gpu)
    view = bank[GUARD:GUARD + n].view(torch.float32)
    cuts = [0, 3, 4, 9, 15, len(files)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        out, o = vl.audioread(files[a:b], out=view, out_base=int(offs[a]), fs=FS)
        assert out.data_ptr() == view.data_ptr() and list(o) == list(offs[a:b + 1])
    torch.cuda.synchronize()
    host = bank.cpu().numpy().view(np.uint32)
    guard = np.uint32(SENTINEL & 0xFFFFFFFF)
    assert (host[:GUARD] == guard).all() and (host[-GUARD:] == guard).all()
    assert np.array_equal(host[GUARD:GUARD + n], bits(single.cpu().numpy()))
    with pytest.raises(ValueError, match="do not fit"):
        vl.audioread(files[:3], out=view[:10], fs=FS)


# ------------------------------------------------------------------------------------------------ the users
def test_wav_file_imdb_resamples_tracks_and_noise(gpu):
    from mcncrossmodalemotions_amd import batch as xbatch, vl
    rng = np.random.default_rng(77)

    def track(seconds, rate, nch):
        v = (rng.standard_normal((int(seconds * rate), nch)) * 3000).clip(-32768, 32767).astype(np.int16)
        return wav_bytes(S16, v, rate)

    tracks = {"a.wav": track(1.5, 44100, 2), "b.wav": track(1.4, 16000, 1), "c.wav": track(1.7, 44100, 2), "d.wav": track(1.6, 16000, 1)}
    noise = [track(2.3, 48000, 1)]
    lens = [ceil_div(np_parse(t)["total"] * FS, np_parse(t)["rate"]) for t in tracks.values()]
    logits = [np.asfortranarray(rng.standard_normal((xbatch.time2idx(n / FS), 8)).astype(np.float32) * 3) for n in lens]
    imdb = xbatch.WavFileEmoVoxImdb(tracks, logits, noise=noise, resample=True, channel=0, chunkBytes=200000)
    assert list(imdb.num_samples) == lens and imdb.noiselen == ceil_div(int(2.3 * 48000) * FS, 48000)
    bank, offs = imdb.device_wav_bank(gpu)
    want, woffs = vl.audioread(list(tracks.values()), fs=FS, channel=0)
    assert np.array_equal(offs, woffs) and torch.equal(bank.view(torch.int32), want.view(torch.int32))
    nb, _ = imdb.device_noise_bank(gpu)
    assert torch.equal(nb.view(torch.int32), vl.audioread(noise, fs=FS, channel=0)[0].view(torch.int32))
    check_close(imdb.device_wav(2, gpu).cpu().numpy(), oracle_file(tracks["c.wav"], channel=0), "track c")
    out = xbatch.getBatchEmoVoxCeleb(imdb, range(4), imageSize=(512, 100), transformation="SN", rng=np.random.default_rng(5),
                                     device=gpu, use_wav=True, wavBatch=True)
    assert out[0::2] == ["data", "logitTarget", "maxLabel"] and tuple(out[1].shape) == (512, 100, 1, 4)
    assert bool(torch.isfinite(out[1]).all())
    with pytest.raises(ValueError) as e:
        xbatch.WavFileEmoVoxImdb(tracks, logits)
    assert str(e.value) == "WavFileEmoVoxImdb: track 'a.wav' is sampled at 44100 Hz, the imdb at 16000"
    with pytest.raises(ValueError) as e:
        xbatch.WavFileEmoVoxImdb({"b.wav": tracks["b.wav"], "s.wav": track(1.0, 16000, 2)}, logits[:2])
    assert str(e.value) == "WavFileEmoVoxImdb: track 's.wav' has 2 channels, one is required"


def test_compute_audio_feats_files_at_fs(gpu):
    from mcncrossmodalemotions_amd import external, vl, zoo
    rng = np.random.default_rng(12)
    spec = [(50000, 44100, 2), (20000, 16000, 1), (60000, 48000, 1), (30000, 22050, 2)]
    files = [wav_bytes(S16, (rng.standard_normal((n, c)) * 2500).clip(-32768, 32767).astype(np.int16), rate=r) for n, r, c in spec]
    net = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=9)
    bank, offs = vl.audioread(files, fs=FS, channel=0)
    assert list(np.diff(offs)) == [ceil_div(n * FS, r) for n, r, _ in spec]
    want = external.compute_audio_feats_wav(net, bank, offs)
    got = external.compute_audio_feats_files(net, files, fs=FS)
    assert got.shape == want.shape == (4, 8) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # fs=None keeps upstream's absent rate check: the 44.1 kHz file is read as if it were at the student's rate
    raw, roffs = vl.audioread(files, channel=0)
    plain = external.compute_audio_feats_files(net, files)
    assert np.array_equal(plain.view(np.uint32), external.compute_audio_feats_wav(net, raw, roffs).view(np.uint32))
    assert not np.array_equal(plain[0], got[0])
