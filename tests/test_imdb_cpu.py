"""CPU: the host side of emoVoxCeleb/fetch_emovoxceleb_imdb.m and emoVoxCeleb/sample_audio.m -- the ABI of xm_group_rows /
xm_gather_rows / xm_scatter_rows / xm_track_peaks (declared, typed, exported, arguments rejected without a device),
addFramesToImdb, the `limit` asymmetry, the bytes of meta.txt -- and the numpy restatements (stable group-by,
column-major-first peak) that the GPU tests compare against."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ABI = ["xm_group_rows", "xm_gather_rows", "xm_scatter_rows", "xm_track_peaks"]


# ------------------------------------------------------------------------------------------------ numpy restatements
def np_group_rows(ids, keys):
    """wavLogits{ii} = logits(denseFramesWavIds == images.id(ii), :) as index sets: group t = the 1-based rows with
    ids == keys[t], ascending.  Returns (offsets T + 1, rows nnz)."""
    ids = np.asarray(ids).reshape(-1)
    groups = [np.nonzero(ids == k)[0] + 1 for k in keys]
    offsets = np.concatenate([[0], np.cumsum([g.size for g in groups])]).astype(np.int64)
    rows = np.concatenate(groups).astype(np.int64) if groups else np.zeros(0, np.int64)
    return offsets, rows


def np_track_peaks(x):
    """[~, m] = max(x(:)); [frameIdx, tag] = ind2sub(size(x), m); maxed = max(x, [], 1) for one F_i x E block, with the
    NaN rule of xm_aggregate_logits (a NaN never wins, a column without an entry above -Inf gives -Inf) and the first
    maximum in column-major order.  An empty block gives 0, 0, -Inf."""
    x = np.asarray(x, dtype=np.float32)
    F, E = x.shape
    if F == 0:
        return 0, 0, np.full(E, -np.inf, np.float32)
    best, fi, tg = -np.inf, 1, 1
    for e in range(E):
        for r in range(F):
            if x[r, e] > best:
                best, fi, tg = x[r, e], r + 1, e + 1
    maxed = np.full(E, -np.inf, np.float32)
    for e in range(E):
        col = x[:, e][~np.isnan(x[:, e])]
        if col.size:
            maxed[e] = col.max()
    return fi, tg, maxed


def test_group_restatement_on_hand_cases():
    # unsorted ids, an id in no key (7, 0, -1), an absent key (5), an empty result
    ids = [3, 1, 3, 0, 7, 2, 1, -1, 3]
    off, rows = np_group_rows(ids, [1, 3, 5, 2])
    assert list(off) == [0, 2, 5, 5, 6] and list(rows) == [2, 7, 1, 3, 9, 6]
    off, rows = np_group_rows(ids, [9])
    assert list(off) == [0, 0] and rows.size == 0
    off, rows = np_group_rows([], [1, 2])
    assert list(off) == [0, 0, 0]
    off, rows = np_group_rows([2, 2, 1, 1], [2, 1])            # key order decides the group order, not the id order
    assert list(off) == [0, 2, 4] and list(rows) == [1, 2, 3, 4]
    # on what addFramesToImdb leaves: group ii = the frames the lister gave track images.id(ii), in order
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    im = fe.addFramesToImdb(hand_imdb(), hand_lister, find=lambda: ["x"] * 12).images
    off, rows = np_group_rows(im["denseFramesWavIds"], im["id"])
    for ii in range(len(im["id"])):
        track = {k: im[k][ii] for k in ("name", "video", "track", "id")}
        assert [im["denseFrames"][r - 1] for r in rows[off[ii]:off[ii + 1]]] == hand_lister(track)
    assert off[-1] == len(im["denseFrames"]) == 9


def test_peak_restatement_on_hand_cases():
    x = np.array([[1, 5, 2], [5, 0, 5], [3, 5, 1]], np.float32)       # 5 at (2,1), (1,2), (3,2), (2,3): column 1 first
    assert np_track_peaks(x)[:2] == (2, 1) and list(np_track_peaks(x)[2]) == [5, 5, 5]
    x = np.array([[0, 9], [0, 9]], np.float32)                       # tie across rows of one column: the lower row
    assert np_track_peaks(x)[:2] == (1, 2)
    x = np.array([[4, 4], [4, 4]], np.float32)                       # everything tied: first entry
    assert np_track_peaks(x)[:2] == (1, 1)
    fi, tg, mx = np_track_peaks(np.zeros((0, 3), np.float32))        # an empty group
    assert (fi, tg) == (0, 0) and np.all(np.isneginf(mx))
    x = np.array([[np.nan, 1], [2, np.nan]], np.float32)             # NaN never wins and is dropped from the maxima
    fi, tg, mx = np_track_peaks(x)
    assert (fi, tg) == (2, 1) and list(mx) == [2, 1]
    x = np.array([[np.nan, -np.inf]], np.float32)                    # nothing above -Inf: index 1 of max(x(:))
    fi, tg, mx = np_track_peaks(x)
    assert (fi, tg) == (1, 1) and np.all(np.isneginf(mx))
    # it is ind2sub of the first maximum of x(:)
    rng = np.random.default_rng(0)
    for _ in range(50):
        x = rng.integers(0, 4, (rng.integers(1, 9), 8)).astype(np.float32)
        m = int(np.argmax(x.reshape(-1, order="F")))
        assert np_track_peaks(x)[:2] == (m % x.shape[0] + 1, m // x.shape[0] + 1)
        assert np.array_equal(np_track_peaks(x)[2], x.max(0))
    # its maxima are what sample_audio writes into meta.txt
    from mcncrossmodalemotions_amd import sample_audio as sa
    x = np.array([[1, -2, 3, 4, 5, 6, 7, np.nan], [0.5, 2, -np.inf, 4, 9, 6, 7.25, np.nan]], np.float32)
    assert sa.format_meta("a.avi", np_track_peaks(x)[2]) == ("aviPath: a.avi\n1.0000 2.0000 3.0000 4.0000 9.0000 6.0000 "
                                                             "7.2500 \n-Inf ")


# ------------------------------------------------------------------------------------------------ ABI
def test_imdb_abi_declared_typed_and_exported():
    from mcncrossmodalemotions_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    L = _lib.load()
    assert L.xm_version() >= 110
    for name in NEW_ABI:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name]
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
    for cite in ("fetch_emovoxceleb_imdb.m:140-148", "fetch_emovoxceleb_imdb.m:130-131", "sample_audio.m:69-74"):
        assert cite in hdr, cite


def test_imdb_arguments_are_rejected_without_a_device():
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    one = C.c_void_p(16)     # never dereferenced: every call below fails its checks first
    g = lambda **k: [k.get("ids", one), k.get("n", 10), k.get("keys", one), k.get("T", 3), k.get("key_max", 9),
                     k.get("offsets", one), k.get("rows", one), k.get("nnz", one), None]
    for bad, msg in [(dict(n=-1), b"n >= 0"), (dict(T=-1), b"T >= 0"), (dict(key_max=-1), b"key_max >= 0"),
                     (dict(ids=None), b"NULL"), (dict(keys=None), b"NULL"), (dict(offsets=None), b"NULL"),
                     (dict(rows=None), b"NULL"), (dict(nnz=None), b"NULL")]:
        assert L.xm_group_rows(*g(**bad)) == 1 and msg in L.xm_last_error(), bad
    assert L.xm_group_rows(*g(key_max=2 ** 28)) == 5 and b"2^28" in L.xm_last_error()           # XM_ENOTSUP
    for fn, a in [(L.xm_gather_rows, lambda **k: [k.get("mat", one), k.get("F", 100), k.get("E", 8), k.get("row0", 0),
                                                  k.get("rows", None), k.get("n", 10), k.get("packed", one), None]),
                  (L.xm_scatter_rows, lambda **k: [k.get("packed", one), k.get("n", 10), k.get("E", 8), k.get("mat", one),
                                                   k.get("F", 100), k.get("row0", 0), k.get("rows", None), None])]:
        for bad, msg in [(dict(n=-1), b"n >= 0"), (dict(E=0), b"E >= 1"), (dict(F=0), b"F >= 1"), (dict(row0=-1), b"row0 >= 0"),
                         (dict(mat=None), b"NULL"), (dict(packed=None), b"NULL"), (dict(row0=95), b"do not fit")]:
            assert fn(*a(**bad)) == 1 and msg in L.xm_last_error(), (fn, bad)
        assert fn(*a(F=2 ** 28, E=8)) == 5 and b"2^31" in L.xm_last_error()
        assert fn(*a(n=2 ** 28, E=8, rows=one, F=10)) == 5 and b"2^31" in L.xm_last_error()
        assert fn(*a(n=0, mat=None, packed=None)) == 0                                           # nothing to do
    p = lambda **k: [k.get("logits", one), k.get("F", 100), k.get("E", 8), k.get("offsets", one), k.get("rows", None),
                     k.get("T", 4), k.get("frame_idx", one), k.get("tag", one), k.get("maxed", one), None]
    for bad, msg in [(dict(F=0), b"F >= 1"), (dict(E=0), b"E >= 1"), (dict(T=-1), b"T >= 0"), (dict(logits=None), b"NULL"),
                     (dict(offsets=None), b"NULL"), (dict(frame_idx=None), b"NULL"), (dict(tag=None), b"NULL"),
                     (dict(maxed=None), b"NULL")]:
        assert L.xm_track_peaks(*p(**bad)) == 1 and msg in L.xm_last_error(), bad
    assert L.xm_track_peaks(*p(F=2 ** 28)) == 5 and b"2^31" in L.xm_last_error()
    assert L.xm_track_peaks(*p(T=2 ** 28)) == 5 and b"2^31" in L.xm_last_error()
    assert L.xm_track_peaks(*p(T=0, logits=None)) == 0


def test_host_wrappers_refuse_host_tensors_and_duplicate_keys():
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    mat = torch.zeros(8, 10).t()
    packed = torch.zeros(4, 8, 1, 1).permute(3, 2, 1, 0)
    i32 = torch.ones(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        vl.group_rows(i32, [1, 2])
    with pytest.raises(RuntimeError, match="not on the GPU"):
        vl.gather_rows(mat, n=4)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        vl.scatter_rows(packed, mat)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        vl.track_peaks(mat, i32)
    # duplicate / out-of-range keys: XM_EINVAL from the wrapper, before anything else is looked at
    for keys in ([1, 2, 1], [0, 1], [3]):
        with pytest.raises(_lib.XmError) as e:
            vl.group_rows(i32, keys, key_max=2)
        assert e.value.code == 1


# ------------------------------------------------------------------------------------------------ addFramesToImdb
def hand_imdb():
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    images = {"name": ["a/v1/1.wav", "a/v1/2.wav", "b/v2/1.wav", "c/v3/1.wav", "c/v3/2.wav"],
              "video": ["v1", "v1", "v2", "v3", "v3"], "track": np.array([1, 2, 1, 1, 2]), "id": np.arange(1, 6),
              "set": np.array([1, 1, 2, 3, 1]), "numSamples": np.array([80000, 90000, 100000, 110000, 120000])}
    return fe.EmoVoxImdb(images)


FRAME_COUNTS = {1: 3, 2: 0, 3: 2, 4: 0, 5: 4}


def hand_lister(track):
    celeb = track["name"].split("/")[0]
    return ["%s/1.6/%s/%d/%05d.jpg" % (celeb, track["video"], track["track"], j + 1)
            for j in range(FRAME_COUNTS[int(track["id"])])]


def test_add_frames_drops_frameless_tracks_and_unclaimed_frames():
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    src = hand_imdb()
    found = lambda: ["x"] * (9 + 4)                                  # `find` sees 4 frames no track claims
    imdb = fe.addFramesToImdb(src, hand_lister, find=found, expectFrames=13)
    im = imdb.images
    # frameless tracks 2 and 4 are gone from EVERY field, the ids of the others are kept
    assert list(im["id"]) == [1, 3, 5] and im["name"] == ["a/v1/1.wav", "b/v2/1.wav", "c/v3/2.wav"]
    assert im["video"] == ["v1", "v2", "v3"] and list(im["track"]) == [1, 1, 2] and list(im["set"]) == [1, 2, 1]
    assert list(im["numSamples"]) == [80000, 100000, 120000] and list(imdb.set) == [1, 2, 1]
    # frames in track order, wavIds = the track's index, the unclaimed slots (id 0) dropped
    assert list(im["denseFramesWavIds"]) == [1, 1, 1, 3, 3, 5, 5, 5, 5] and len(im["denseFrames"]) == 9
    assert im["denseFrames"][0] == "a/1.6/v1/1/00001.jpg" and im["denseFrames"][-1] == "c/1.6/v3/2/00004.jpg"
    assert im["denseFrames"][3] == "b/1.6/v2/1/00001.jpg"
    # the argument is untouched; a wrong count trips the assertion of :223
    assert list(src.images["id"]) == [1, 2, 3, 4, 5] and "denseFrames" not in src.images
    with pytest.raises(AssertionError, match="unexpected number of face images"):
        fe.addFramesToImdb(src, hand_lister, find=found, expectFrames=5078961)
    assert len(fe.addFramesToImdb(src, hand_lister).images["denseFrames"]) == 9


def test_synthetic_dense_frames_lister():
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe
    syn = batch.SyntheticEmoVoxImdb(num_tracks=10, seed=3)
    src = fe.src_imdb(syn)
    fr = batch.SyntheticDenseFrames(src, frameless=(4, 9), unclaimed=5)
    imdb = fe.addFramesToImdb(src, fr.lister, find=fr.find)
    assert list(imdb.images["id"]) == [1, 2, 3, 5, 6, 7, 8, 10]
    want = [syn.wavLogits[i - 1].shape[0] for i in imdb.images["id"]]      # the frame count the synthetic imdb assumes
    got = [int((imdb.images["denseFramesWavIds"] == i).sum()) for i in imdb.images["id"]]
    assert got == want and len(fr.find()) == sum(want) + 5
    assert len(set(fr.frame_key(p) for p in imdb.images["denseFrames"])) == sum(want)


def limit_counts(wavIds, ids, limit):
    """fetch_emovoxceleb_imdb.m:112-115,140-142 on the host"""
    numKeep = int((np.asarray(wavIds) <= ids[0] + limit).sum())
    return min(len(wavIds), numKeep), int(min(len(ids), limit))


def test_limit_asymmetry():
    """the reference evaluates the frames of the tracks with id <= firstId + limit (limit + 1 tracks) and fills `limit`
    cells: the rows of the extra track are computed and belong to no cell"""
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    imdb = fe.addFramesToImdb(hand_imdb(), hand_lister)
    ids, wavIds = imdb.images["id"], imdb.images["denseFramesWavIds"]
    assert limit_counts(wavIds, ids, math.inf) == (9, 3)
    assert limit_counts(wavIds, ids, 1) == (3, 1)          # ids <= 2: track 1 only (2 was dropped)
    assert limit_counts(wavIds, ids, 2) == (5, 2)          # ids <= 3: tracks 1 and 3, two cells
    numIms, numLogits = limit_counts(wavIds, ids, 2)
    off, rows = np_group_rows(wavIds[:numIms], ids[:numLogits])
    assert list(off) == [0, 3, 5]
    # consecutive ids show the asymmetry itself: 3 tracks of frames, 2 cells
    wav = np.repeat(np.arange(1, 6), 2)
    numIms, numLogits = limit_counts(wav, np.arange(1, 6), 2)
    assert (numIms, numLogits) == (6, 2)
    off, rows = np_group_rows(wav[:numIms], np.arange(1, 6)[:numLogits])
    assert list(off) == [0, 2, 4] and list(rows) == [1, 2, 3, 4]    # rows 5, 6 (track 3) were evaluated and are dropped


# ------------------------------------------------------------------------------------------------ sample_audio
def test_meta_txt_bytes():
    from mcncrossmodalemotions_amd import sample_audio as sa
    v = [1.23456, -0.5, 10, 0.00004, -3.14159, 2.5, 7.77777, -12.000049]
    want = ("aviPath: id00001/video00001/00001.avi\n"
            "1.2346 -0.5000 10.0000 0.0000 -3.1416 2.5000 7.7778 \n"
            "-12.0000 ")
    assert sa.format_meta("id00001/video00001/00001.avi", v) == want
    assert sa.format_meta("p", np.arange(7)).endswith("6.0000 \n") and sa.format_meta("p", np.arange(7)).count("\n") == 2
    assert sa.format_meta("p", [np.inf, -np.inf, np.nan]) == "aviPath: p\nInf -Inf NaN "
    assert sa.EMOTIONS[:3] == ["neutral", "happiness", "surprise"] and len(sa.COLORS) == 8 and sa.SAMPLES_PER_EMO == 20


def test_imdb_file_round_trip_and_cache_key(tmp_path):
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    imdb = fe.addFramesToImdb(hand_imdb(), hand_lister)
    rng = np.random.default_rng(0)
    imdb.wavLogits = [rng.standard_normal((3, 8)).astype(np.float32), rng.standard_normal((2, 8)).astype(np.float32),
                      np.zeros((0, 8), np.float32)]
    path = fe.getImdbPath(str(tmp_path), "senet50-ferplus")
    assert path.endswith(os.path.join(str(tmp_path), "senet50-ferplus-logits.mat"))
    fe.save_imdb(path, imdb)
    back = fe.load_imdb(path)
    assert back.images["name"] == imdb.images["name"] and back.images["denseFrames"] == imdb.images["denseFrames"]
    for k in ("id", "set", "track", "numSamples", "denseFramesWavIds"):
        assert np.array_equal(back.images[k], imdb.images[k]), k
    assert all(np.array_equal(a, b) and a.shape == b.shape for a, b in zip(back.wavLogits, imdb.wavLogits))
    # an existing file is loaded, not rebuilt (no teacher is touched); the cache key holds the teacher
    fe._CACHE.clear()
    a = fe.fetch_emovoxceleb_imdb("senet50-ferplus", str(tmp_path), verbose=False)
    assert fe.fetch_emovoxceleb_imdb("senet50-ferplus", str(tmp_path), verbose=False) is a
    fe.save_imdb(fe.getImdbPath(str(tmp_path), "resnet50-ferplus"), imdb)
    b = fe.fetch_emovoxceleb_imdb("resnet50-ferplus", str(tmp_path), verbose=False)
    assert b is not a and len(fe._CACHE) == 2
    fe._CACHE.clear()


def test_sample_audio_returns_before_sampling_when_the_destination_exists(tmp_path):
    """the answer 'n' of confirmSamplingProcess: no imdb is fetched, no device is touched, nothing is written"""
    from mcncrossmodalemotions_amd import sample_audio as sa
    dest = tmp_path / "samples"
    dest.mkdir()
    (dest / "kept.txt").write_text("x")
    assert sa.sample_audio(dest=str(dest), imdb=object(), verbose=False) is None
    assert sorted(os.listdir(dest)) == ["kept.txt"]
