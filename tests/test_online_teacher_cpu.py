"""CPU: the host side of teacherMode='online' -- xm_window_targets in the ABI, and batch.online_frame_plan against the
cached mode: the frames it names are the rows of imdb.wavLogits that getBatchEmoVoxCeleb aggregates.  The cached logits
of the test carry their own address (row r of track ii holds 1000 ii + r in column 1), the frame paths carry theirs
(<celeb of the track>/.../<frame number>.jpg), so both sides are aggregated here in numpy from what each names."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 8


# ------------------------------------------------------------------------------------------------ ABI
def test_window_targets_abi_declared_typed_and_exported():
    from mcncrossmodalemotions_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    L = _lib.load()
    assert L.xm_version() >= 121
    name = "xm_window_targets"
    assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SIGNATURES
    assert getattr(L, name).argtypes == _lib.SIGNATURES[name]
    proto = re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == 11
    assert "getBatchEmoVoxCeleb.m:30-32,145-158,179-188" in hdr
    assert "121 = + xm_window_targets" in hdr


def test_window_targets_refuses_bad_arguments_without_a_device():
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    one = C.c_void_p(4096)
    g = lambda **k: [k.get("lg", one), k.get("E", 8), k.get("n", 5), k.get("first", one), k.get("last", one), k.get("N", 3),
                     k.get("agg", 0), k.get("P", 8), k.get("out", one), k.get("lab", one), None]
    for bad, msg in [(dict(E=0), b"E = 0"), (dict(E=65, P=8), b"E = 65"), (dict(P=0), b"numPredEmotions"),
                     (dict(P=9), b"numPredEmotions"), (dict(E=7, P=8), b"numPredEmotions"), (dict(n=-1), b"negative"),
                     (dict(N=-1), b"negative"), (dict(agg=2), b"aggregator"), (dict(agg=7), b"aggregator"),
                     (dict(agg=-1), b"aggregator"), (dict(out=None), b"NULL"), (dict(lab=None), b"NULL"),
                     (dict(first=None), b"NULL"), (dict(last=None), b"NULL"), (dict(lg=None), b"NULL")]:
        assert L.xm_window_targets(*g(**bad)) == 1 and msg in L.xm_last_error(), bad
    assert L.xm_window_targets(*g(N=0)) == 0
    assert L.xm_window_targets(*g(N=0, lg=None, out=None, lab=None, first=None, last=None, n=0)) == 0


def test_wrappers_refuse_before_any_device_work():
    import torch
    from mcncrossmodalemotions_amd import batch, run_distillation as rd, vl
    with pytest.raises(RuntimeError, match="no CPU path"):
        vl.window_targets(torch.zeros(4, 8, 1, 1).permute(3, 2, 1, 0), torch.ones(1, dtype=torch.int32),
                          torch.ones(1, dtype=torch.int32))
    imdb = frame_imdb()[0]
    with pytest.raises(ValueError, match="either"):
        batch.OnlineTeacher(None, imdb)
    with pytest.raises(ValueError, match="either"):
        batch.OnlineTeacher(None, imdb, read=lambda p: [], frames=lambda p, d: None)
    with pytest.raises(ValueError, match="progressive=True and split="):
        batch.OnlineTeacher(None, imdb, read=lambda p: [], split=64, progressive=True)
    with pytest.raises(ValueError, match="need"):
        batch.OnlineTeacher(None, imdb, frames=lambda p, d: None, split=64)
    with pytest.raises(ValueError, match="framesPerPair"):
        batch.OnlineTeacher(None, imdb, frames=lambda p, d: None, framesPerPair=0)
    with pytest.raises(ValueError, match="teacherMode"):
        rd.run_distillation(teacherMode="live")
    with pytest.raises(ValueError, match="belong to teacherMode='online'"):
        rd.run_distillation(framesPerPair=1)
    with pytest.raises(ValueError, match="needs an imdb"):
        rd.run_distillation(teacherMode="online", frames=lambda p, d: None)
    with pytest.raises(ValueError, match="either"):
        rd.run_distillation(teacherMode="online", imdb=imdb)


# ------------------------------------------------------------------------------------------------ imdbs
def frame_imdb(lost=None, single=None, frameless=(), num_tracks=6, seed=3):
    """(imdb with frame lists and no wavLogits, the same imdb with the cached logits of the module docstring).
    `lost`: id of a track that keeps only its first 40 % of frames; `single`: id of a track with one frame; `frameless`:
    ids addFramesToImdb removes."""
    import copy
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe
    syn = batch.SyntheticEmoVoxImdb(num_tracks=num_tracks, seed=seed, min_seconds=4.5, max_seconds=9.0)
    src = fe.src_imdb(syn)
    dense = batch.SyntheticDenseFrames(src, frameless=frameless)

    def lister(track):
        paths = dense.lister(track)
        if lost is not None and int(track["id"]) == lost:
            paths = paths[:max(2, int(len(paths) * 0.4))]
        if single is not None and int(track["id"]) == single:
            paths = paths[:1]
        return paths

    imdb = fe.addFramesToImdb(src, lister)
    assert imdb.wavLogits is None
    wavIds, ids = np.asarray(imdb.images["denseFramesWavIds"]), np.asarray(imdb.images["id"])
    cached = copy.copy(imdb)
    cached.wavLogits = [np.asfortranarray(np.stack([value(ii, r) for r in range(1, int((wavIds == i).sum()) + 1)]))
                        for ii, i in enumerate(ids)]
    return imdb, cached


def value(ii, r):
    """the 8 logits of row r (1-based) of track ii (0-based position): its address in column 1, then columns that
    move the label around"""
    a = 1000 * ii + r
    return np.array([a] + [(a * (e + 3) * 7919) % 2003 for e in range(1, E)], np.float32)


def path_value(imdb, path):
    """the logits of the frame a path names: <celeb>/1.6/<video>/<track>/<frame>.jpg, celeb id<id>"""
    ids = [int(i) for i in imdb.images["id"]]
    celeb, _, _, _, frame = path.split("/")
    return value(ids.index(int(celeb[2:])), int(frame[:-4]))


def aggregate(rows, span, agg):
    """numpy float32 max / mean of E-column rows; an empty window: -Inf, or 0 / span as the kernels do"""
    rows = np.asarray(rows, np.float32).reshape(-1, E)
    if agg == "max":
        return rows.max(0) if len(rows) else np.full(E, -np.inf, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return rows.sum(0, dtype=np.float64).astype(np.float32) / np.float32(span if not len(rows) else len(rows))


def label(v):
    best, arg = -np.inf, 0
    for c, x in enumerate(v):
        if x > best:
            best, arg = x, c
    return arg + 1


def check_plan(imdb, cached, first, last, k, frame_rng=None):
    """the frames named for windows [first, last] are the cached rows; returns the number of frames named"""
    from mcncrossmodalemotions_amd import batch
    paths, wfirst, wlast = batch.online_frame_plan(imdb, first, last, k, frame_rng)
    assert wfirst.dtype == wlast.dtype == np.int32 and len(wfirst) == len(wlast) == len(first)
    cat = np.concatenate(cached.wavLogits, 0)
    pos = 0
    for j, (a, b) in enumerate(zip(first, last)):
        rows = cat[a - 1:b] if a <= b else cat[:0]
        assert wfirst[j] == pos + 1                                           # pair after pair, nothing between them
        if a > b:
            assert wlast[j] - wfirst[j] == b - a and wlast[j] < wfirst[j]
            got = cat[:0]
        else:
            want = len(rows) if k == "all" else min(int(k), len(rows))
            assert wlast[j] == pos + want
            got = np.stack([path_value(imdb, p) for p in paths[pos:pos + want]])
            addr = got[:, 0]
            assert (np.diff(addr) > 0).all()                                  # ascending row order, no frame twice
            assert np.isin(addr, rows[:, 0]).all()                            # rows of this very window
            sel = rows[np.isin(rows[:, 0], addr)]
            assert np.array_equal(sel, got)
            if want == len(rows):
                assert np.array_equal(got, rows)
            pos += want
        span = wlast[j] - wfirst[j] + 1
        for agg in ("max", "mean"):
            ours, theirs = aggregate(got, span, agg), aggregate(rows if (k == "all" or len(got) == len(rows)) else got, b - a + 1, agg)
            assert np.array_equal(ours, theirs, equal_nan=True), (j, agg)
            assert label(ours) == label(theirs)
    assert pos == len(paths)
    return len(paths)


VARIANTS = {"plain": {}, "lost": dict(lost=2), "single": dict(single=4), "frameless": dict(frameless=(3,)),
            "all-at-once": dict(lost=5, single=1, frameless=(2,))}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("W", [300, 400])
def test_frame_plan_names_the_rows_the_cached_mode_aggregates(variant, W):
    from mcncrossmodalemotions_amd import batch
    imdb, cached = frame_imdb(**VARIANTS[variant])
    T = len(imdb.images["id"])
    assert T == 6 - len(VARIANTS[variant].get("frameless", ()))
    tracks = list(range(T)) + [0, T - 1]
    p_online = batch.wav_batch_plan(imdb, tracks, W, "I", np.random.default_rng(11))
    p_cached = batch.wav_batch_plan(cached, tracks, W, "I", np.random.default_rng(11))
    for a, b in zip(p_online, p_cached):                     # the row counts from the frame lists = those of the cache
        assert np.array_equal(a, b)
    first, last = p_cached[2], p_cached[3]
    lengths = last - first + 1
    if variant == "plain":
        assert lengths.min() >= 8 and len(set(lengths)) > 1              # ragged time2idx windows
    if variant in ("lost", "all-at-once"):
        assert (lengths < 0.04 * W).any()         # endIdx was clamped to the frames left (a whole window: W / 24 rows)
    for k in ("all", 1, 4, 100):
        n = check_plan(imdb, cached, first, last, k, np.random.default_rng(5))
        assert n == (np.maximum(lengths, 0).sum() if k in ("all", 100) else np.minimum(np.maximum(lengths, 0), k).sum())


def test_frame_plan_empty_and_clamped_windows():
    """the track that lost frames: crops late in the clip start past its last row -- first > last, an empty window that
    names no frame and keeps its (non-positive) length"""
    from mcncrossmodalemotions_amd import batch
    plain = frame_imdb()[0]
    longest = int(np.argmax(plain.num_samples))                # the longest clip: most of its crops start past 40 % of it
    assert plain.num_samples[longest] > 7.5 * 16000
    imdb, cached = frame_imdb(lost=int(plain.images["id"][longest]))
    rng = np.random.default_rng(0)
    empties = 0
    for _ in range(40):
        _, _, first, last = batch.wav_batch_plan(cached, [longest, longest, 0], 300, "I", rng)
        empties += int((first > last).sum())
        check_plan(imdb, cached, first, last, "all")
        check_plan(imdb, cached, first, last, 2, np.random.default_rng(1))
    assert empties > 5
    paths, wf, wl = batch.online_frame_plan(imdb, [7, 3], [4, 2], "all")
    assert paths == [] and list(wf) == [1, 1] and list(wl) == [-2, 0]
    with pytest.raises(ValueError, match="leaves"):
        batch.online_frame_plan(imdb, [1], [10 ** 6])
    with pytest.raises(ValueError, match="framesPerPair"):
        batch.online_frame_plan(imdb, [1], [2], "some")


def test_frame_plan_fixed_segments_and_speed_perturbation():
    from mcncrossmodalemotions_amd import batch
    imdb, cached = frame_imdb(single=4, frameless=(3,))
    T = len(imdb.images["id"])
    tracks = list(range(T))
    offs = [0.25 * k for k in range(T)]
    a = batch.wav_batch_plan(imdb, tracks, 300, "I", np.random.default_rng(2), fixedSegments=True, timeOffsets=offs)
    b = batch.wav_batch_plan(cached, tracks, 300, "I", np.random.default_rng(2), fixedSegments=True, timeOffsets=offs)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    rows = np.array([l.shape[0] for l in cached.wavLogits])
    assert np.array_equal(b[3] - b[2] + 1, rows) and rows.min() == 1          # every row of every clip, the single frame too
    for k in ("all", 1, 4, 100):
        check_plan(imdb, cached, b[2], b[3], k, np.random.default_rng(9))
    a = batch.wav_batch_plan(imdb, tracks, 300, "IS", np.random.default_rng(2))
    b = batch.wav_batch_plan(cached, tracks, 300, "IS", np.random.default_rng(2))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (b[0][:, 2] != b[0][:, 3]).all()   # resampled crops
    for k in ("all", 1, 4, 100):
        check_plan(imdb, cached, b[2], b[3], k, np.random.default_rng(9))


def test_rows_follow_list_order_not_frame_names():
    """row r of a track is the r-th entry of denseFrames with the track's wav id IN LIST ORDER, also when the list is
    neither sorted by name nor contiguous per track (the grouping of vl.group_rows)"""
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe
    images = {"name": ["a", "b", "c"], "video": ["v"] * 3, "track": np.ones(3, int), "id": np.array([7, 3, 9]),
              "set": np.ones(3, int), "numSamples": np.full(3, 80000),
              "denseFrames": ["x3", "p9", "x1", "q3", "x2", "p3", "r9"],
              "denseFramesWavIds": np.array([7, 9, 7, 3, 7, 3, 9])}
    imdb = fe.EmoVoxImdb(images)
    rows, offs = batch.logit_rows(imdb)
    assert list(rows) == [3, 2, 2] and list(offs) == [0, 3, 5, 7]
    paths, wf, wl = batch.online_frame_plan(imdb, [1, 4, 6, 2], [3, 5, 7, 6])
    assert paths == ["x3", "x1", "x2", "q3", "p3", "p9", "r9", "x1", "x2", "q3", "p3", "p9"]
    assert list(wf) == [1, 4, 6, 8] and list(wl) == [3, 5, 7, 12]
    images["denseFrames"].append("late")                      # another `images`: the index is made again
    imdb2 = fe.EmoVoxImdb(dict(images, denseFramesWavIds=np.append(images["denseFramesWavIds"], 3)))
    assert list(batch.logit_rows(imdb2)[0]) == [3, 3, 2]


def test_crops_do_not_depend_on_frames_per_pair():
    from mcncrossmodalemotions_amd import batch
    imdb, _ = frame_imdb()
    runs = {}
    for k in ("all", 1, 4):
        rng, frng, out = np.random.default_rng(21), np.random.default_rng(0), []
        for _ in range(3):
            desc, ratio, first, last = batch.wav_batch_plan(imdb, [0, 1, 2, 3, 4, 5], 300, "IS", rng)
            paths, wf, wl = batch.online_frame_plan(imdb, first, last, k, frng)
            out.append((desc, ratio, first, last))
        runs[k] = (out, rng.random())
    for k in (1, 4):
        assert runs[k][1] == runs["all"][1]                                    # the audio generator stands where it stood
        for x, y in zip(runs[k][0], runs["all"][0]):
            assert all(np.array_equal(p, q) for p, q in zip(x, y))
    # frames drawn for k differ from call to call (the generator advances), and never touch the default generator's state
    a = batch.online_frame_plan(imdb, [1], [20], 3, np.random.default_rng(4))[0]
    assert a == batch.online_frame_plan(imdb, [1], [20], 3, np.random.default_rng(4))[0]
    frng = np.random.default_rng(4)
    draws = {tuple(batch.online_frame_plan(imdb, [1], [20], 3, frng)[0]) for _ in range(6)}
    assert len(draws) > 1


# ------------------------------------------------------------------------------------------------ wav_batch_plan as it was
def test_wav_batch_plan_on_cached_logits_follows_its_rules():
    """an imdb with wavLogits: the plan of a plain crop restated from the docstrings of wav_batch_plan / crop_window
    (getBatchEmoVoxCeleb.m:67-68,81-89,109-119,141-152,210-214), drawn from a generator in the same state"""
    import math
    from mcncrossmodalemotions_amd import batch
    imdb = batch.SyntheticEmoVoxImdb(num_tracks=9, seed=6)
    fs = 16000
    t2i = lambda t: int(math.floor(max(t * 25 - 1, 0) / 6)) + 1
    imdb.num_samples = np.array([int(s * fs) for s in (2.2, 3.5, 4.1, 6.0, 9.3, 12.0, 19.95, 23.9, 5.5)])
    imdb.wavLogits = [np.zeros((t2i(n / fs), 8), np.float32, order="F") for n in imdb.num_samples]
    woffs = np.concatenate([[0], np.cumsum(imdb.num_samples)])
    loffs = np.concatenate([[0], np.cumsum([l.shape[0] for l in imdb.wavLogits])])
    tracks = [8, 0, 3, 3, 5, 1, 2, 4, 6, 7]
    for W in (300, 400):
        audSamp = (0.01 * W + 0.001 * 25 - 0.001) * fs
        L = int(round(audSamp))
        assert (imdb.num_samples < L).any() and (imdb.num_samples > 19.9 * fs).any()     # padded clips and thresholded ones
        rng, mine = np.random.default_rng(77), np.random.default_rng(77)
        for _ in range(2):
            desc, ratio, first, last = batch.wav_batch_plan(imdb, tracks, W, "I", rng)
            for k, ii in enumerate(tracks):
                num, rows = int(imdb.num_samples[ii]), imdb.wavLogits[ii].shape[0]
                wd = min(num, int(19.9 * fs)) - L
                wr = int(mine.integers(1, wd + 1)) if wd >= 1 else 1
                s, e = t2i(wr / fs), min(t2i((wr + audSamp - 1) / fs), rows)
                assert list(desc[k]) == [woffs[ii] + min(wr - 1, num), max(0, min(L, num - (wr - 1))), fs, fs, 0, 0]
                assert (first[k], last[k]) == (loffs[ii] + s, loffs[ii] + e) and ratio[k] == 0
            assert desc.dtype == np.int64 and first.dtype == last.dtype == np.int32 and ratio.dtype == np.float32
        assert rng.random() == mine.random()
