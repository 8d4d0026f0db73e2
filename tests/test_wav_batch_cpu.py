"""CPU: batch.wav_batch_plan, the host side of the batched waveform front-end (getBatchEmoVoxCeleb.m:76-158), against a
replay of the reference's draws -- speedR, then the crop offset, then Nir, Nwr, Nratio per clip -- written out here the way
tests/test_gpu_nets.py replays them for the per-clip path.  No device is touched."""
import numpy as np
import pytest

FS, W = 16000, 100
TRACKS = [1, 4, 5]


@pytest.fixture(scope="module")
def imdb():
    from mcncrossmodalemotions_amd import batch
    return batch.SyntheticEmoVoxImdb(num_tracks=6, seed=9, min_seconds=2.5, max_seconds=6.0)


def _replay(imdb, idx, transformation, rng):
    """(desc, ratio, first, last) from the draws of cnn_get_batch_wav_emo, independent of wav_batch_plan's code"""
    from mcncrossmodalemotions_amd import batch
    aud = batch.aud_samples(W)
    L = int(round(aud))
    isVal = "v" in transformation
    chspeed, noisy = "S" in transformation and not isVal, "N" in transformation and not isVal
    woffs = np.concatenate([[0], np.cumsum(imdb.num_samples)])
    loffs = np.cumsum([0] + [l.shape[0] for l in imdb.wavLogits])
    desc, ratio, first, last = [], [], [], []
    for ii in idx:
        total = min(int(imdb.num_samples[ii]), int(19.9 * FS))
        rows = imdb.wavLogits[ii].shape[0]
        if chspeed:
            speedR = 0.95 + float(rng.random()) * 0.1
            ln = int(round(aud * speedR))
            wr = int(rng.integers(1, total - ln + 1))
            p = int(round(FS / speedR))
            nz = -(-ln * p // FS)
            s, e = batch.time2idx(wr / FS), min(batch.time2idx((wr + aud - 1) / FS), rows)
        else:
            wr, s, e = batch.crop_window(total, aud, FS, rows, rng)
            ln, p, nz = min(L, int(imdb.num_samples[ii]) - (wr - 1)), FS, L
        row = [woffs[ii] + wr - 1, ln, p, FS, 0, 0]
        r = 0.0
        if noisy:
            nir, nwr = int(rng.integers(1, imdb.noisenum + 1)), int(rng.integers(1, imdb.noiselen - nz + 1))
            r = float(rng.random()) * imdb.noisevol
            row[4:] = [(nir - 1) * imdb.noiselen + nwr - 1, min(nz, L)]
        desc.append(row)
        ratio.append(r)
        first.append(loffs[ii] + s)
        last.append(loffs[ii] + e)
    return np.array(desc, np.int64), np.array(ratio, np.float32), np.array(first), np.array(last)


@pytest.mark.parametrize("transformation", ["I", "IS", "IN", "ISN", "ISNv"])
def test_plan_matches_replayed_draws(imdb, transformation):
    from mcncrossmodalemotions_amd import batch
    rng, rng2 = np.random.default_rng(77), np.random.default_rng(77)
    desc, ratio, first, last = batch.wav_batch_plan(imdb, TRACKS, W, transformation, rng)
    rdesc, rratio, rfirst, rlast = _replay(imdb, TRACKS, transformation, rng2)
    assert desc.dtype == np.int64 and desc.shape == (3, 6) and ratio.dtype == np.float32 and ratio.shape == (3,)
    for f, name in enumerate(["src", "len", "p", "q", "nsrc", "nlen"]):
        assert (desc[:, f] == rdesc[:, f]).all(), (name, desc[:, f], rdesc[:, f])
    assert (ratio == rratio).all()
    assert (first == rfirst).all() and (last == rlast).all()
    # the same number of draws, of the same kinds, in the same order: the generators end in the same state
    assert rng.bit_generator.state == rng2.bit_generator.state
    L = int(round(batch.aud_samples(W)))
    if "S" in transformation and "v" not in transformation:
        assert (desc[:, 2] != desc[:, 3]).all() and (np.abs(desc[:, 1] - L) <= 0.05 * L + 1).all()
    if "N" in transformation and "v" not in transformation:
        assert (desc[:, 5] > 0).all() and (desc[:, 5] <= L).all() and (ratio > 0).all()
    # every range lies in its bank
    assert (desc[:, 0] >= 0).all() and (desc[:, 0] + desc[:, 1] <= imdb.wav_offsets()[-1]).all()
    assert (desc[:, 4] >= 0).all() and (desc[:, 4] + desc[:, 5] <= imdb.noise_offsets()[-1]).all()


def test_validation_switches_speed_and_noise_off(imdb):
    from mcncrossmodalemotions_amd import batch
    desc, ratio, first, last = batch.wav_batch_plan(imdb, TRACKS, W, "ISNv", np.random.default_rng(3))
    assert (desc[:, 5] == 0).all() and (desc[:, 2] == desc[:, 3]).all() and (ratio == 0).all()
    plain = batch.wav_batch_plan(imdb, TRACKS, W, "I", np.random.default_rng(3))
    assert all((a == b).all() for a, b in zip((desc, ratio, first, last), plain))
    desc2 = batch.wav_batch_plan(imdb, TRACKS, W, "vISN", np.random.default_rng(3))[0]    # 'v' in front, as upstream
    assert (desc2 == desc).all()


def test_first_last_follow_crop_window(imdb):
    from mcncrossmodalemotions_amd import batch
    rng, rng2 = np.random.default_rng(5), np.random.default_rng(5)
    desc, _, first, last = batch.wav_batch_plan(imdb, TRACKS, W, "I", rng)
    loffs = imdb.logit_offsets()
    for k, ii in enumerate(TRACKS):
        wr, s, e = batch.crop_window(int(imdb.num_samples[ii]), batch.aud_samples(W), FS, imdb.wavLogits[ii].shape[0], rng2)
        assert (first[k], last[k]) == (loffs[ii] + s, loffs[ii] + e)
        assert desc[k, 0] == imdb.wav_offsets()[ii] + wr - 1


def test_short_clip_is_padded_or_refused():
    from mcncrossmodalemotions_amd import batch
    short = batch.SyntheticEmoVoxImdb(num_tracks=3, seed=2, min_seconds=0.9, max_seconds=0.95)
    L = int(round(batch.aud_samples(W)))
    # plain crop: wr = 1, the track's samples, the rest is padding -- and noise runs over the whole padded window
    desc, ratio, _, _ = batch.wav_batch_plan(short, [0, 2], W, "IN", np.random.default_rng(1))
    assert (desc[:, 1] == short.num_samples[[0, 2]]).all() and (desc[:, 1] < L).all()
    assert (desc[:, 0] == short.wav_offsets()[[0, 2]]).all() and (desc[:, 5] == L).all()
    # 'S': randi(wd) with wd < 1 fails upstream (:106)
    with pytest.raises(ValueError, match="shorter than the speed-perturbed window"):
        batch.wav_batch_plan(short, [0, 2], W, "IS", np.random.default_rng(1))


def test_fixed_segments_need_offsets(imdb):
    from mcncrossmodalemotions_amd import batch
    with pytest.raises(IndexError):
        batch.wav_batch_plan(imdb, TRACKS, W, "I", np.random.default_rng(0), fixedSegments=True)
    desc, _, first, last = batch.wav_batch_plan(imdb, TRACKS, W, "IS", np.random.default_rng(0), fixedSegments=True,
                                                timeOffsets=[0.5, 1.0, 400.0])
    woffs, loffs = imdb.wav_offsets(), imdb.logit_offsets()
    assert (desc[:2, 0] == woffs[TRACKS[:2]] + [8000, 16000]).all() and (desc[:, 2] == desc[:, 3]).all()
    assert desc[2, 1] == 0 and desc[2, 0] == woffs[TRACKS[2] + 1]          # an offset behind the track: nothing to read
    assert (first == loffs[TRACKS] + 1).all() and (last == loffs[np.array(TRACKS) + 1]).all()
