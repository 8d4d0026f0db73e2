"""CPU: external.audio_feats_plan, the host side of the batched whole-clip front-end (compute_audio_feats.m:160-185):
frames, width bucket and first frame of the centre crop per clip, grouping by bucket.  Touches no device."""
import numpy as np
import pytest

NW, NS = 400, 160
FRAMES = [100, 101, 102, 103, 199, 200, 257, 999, 1000, 1099, 1100, 1500]
F0 = [0, 0, 0, 1, 49, 0, 28, 49, 0, 49, 49, 249]


def _len(T, r=0):
    return NW + NS * (T - 1) + r


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def test_frames_bucket_and_crop_start():
    from mcncrossmodalemotions_amd import external
    lengths = [_len(T) for T in FRAMES]
    T, rsize, f0, _ = external.audio_feats_plan(lengths, _offsets(lengths)[:-1])
    assert T.tolist() == FRAMES
    assert rsize.tolist() == [max(w for w in external.BUCKETS_WIDTH if w <= t) for t in FRAMES]
    assert f0.tolist() == F0
    # compute_audio_feats.m:182-183 spelled out: round() away from zero, 0 -> 1, 1-based
    for t, w, s in zip(T, rsize, f0):
        rstart = int(np.floor((t - w) / 2.0 + 0.5)) or 1
        assert s == rstart - 1 and s + w <= t


def test_short_clip_raises():
    from mcncrossmodalemotions_amd import external
    assert (16239 - NW) // NS + 1 == 99
    with pytest.raises(ValueError, match="empty audio clip"):
        external.audio_feats_plan([_len(150), 16239], [0, _len(150)])


def test_residual_samples_do_not_change_the_frame_count():
    from mcncrossmodalemotions_amd import external
    for T in (100, 157, 1000):
        lengths = [_len(T, r) for r in (0, 1, 159)]
        got, _, f0, _ = external.audio_feats_plan(lengths, _offsets(lengths)[:-1])
        assert got.tolist() == [T] * 3 and len(set(f0.tolist())) == 1
    assert external.audio_feats_plan([_len(100, 160)], [0])[0].tolist() == [101]


def test_grouping_keeps_clip_order():
    from mcncrossmodalemotions_amd import external
    frames = [250, 100, 205, 1012, 137, 299, 199]
    lengths = [_len(T, 7 * i) for i, T in enumerate(frames)]
    offs = _offsets(lengths)
    T, rsize, f0, groups = external.audio_feats_plan(lengths, offs[:-1])
    assert [g[0] for g in groups] == [100, 200, 1000]
    assert [g[1].tolist() for g in groups] == [[1, 4, 6], [0, 2, 5], [3]]
    for w, idx, desc in groups:
        assert desc.dtype == np.int64 and desc.shape == (len(idx), 3)
        assert desc[:, 0].tolist() == offs[idx].tolist() and desc[:, 1].tolist() == [lengths[i] for i in idx]
        assert desc[:, 2].tolist() == f0[idx].tolist() and (rsize[idx] == w).all()
    # an extra trailing offset (the bank's length, as imdb.wav_offsets gives it) is accepted
    assert external.audio_feats_plan(lengths, offs)[3][0][1].tolist() == [1, 4, 6]
    assert external.audio_feats_plan([], [])[3] == []
