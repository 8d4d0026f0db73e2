"""GPU: xm_group_rows / xm_gather_rows / xm_scatter_rows / xm_track_peaks against the numpy restatements of
tests/test_imdb_cpu.py (exactly), buildImdb's bookkeeping end to end, the built logits against the oracle, and the built
imdb driving getBatchEmoVoxCeleb, run_distillation, student_stats and sample_audio."""
import json
import math
import os

import numpy as np
import pytest
import torch

from test_imdb_cpu import np_group_rows, np_track_peaks

pytestmark = pytest.mark.gpu


def fast_group_rows(ids, keys):
    """the restatement for large cases: a stable argsort by group number (checked against np_group_rows below)"""
    ids, keys = np.asarray(ids, np.int64), np.asarray(keys, np.int64)
    slot = {int(k): t for t, k in enumerate(keys)}
    g = np.array([slot.get(int(i), -1) for i in ids], np.int64) if ids.size < 4096 else None
    if g is None:
        table = np.full(int(max(ids.max(), keys.max())) + 2, -1, np.int64)
        table[keys] = np.arange(keys.size)
        g = np.where(ids > 0, table[np.clip(ids, 0, table.size - 1)], -1)
    kept = np.nonzero(g >= 0)[0]
    order = kept[np.argsort(g[kept], kind="stable")]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(g[kept], minlength=keys.size))])
    return offsets.astype(np.int64), order + 1


def run_group(gpu, ids, keys, key_max=None):
    from mcncrossmodalemotions_amd import vl
    d = torch.from_numpy(np.asarray(ids, np.int32)).to(gpu)
    off, rows, nnz = vl.group_rows(d, keys, key_max)
    return off.cpu().numpy().astype(np.int64), rows.cpu().numpy().astype(np.int64), int(nnz.cpu()[0])


@pytest.mark.parametrize("n,T,key_max,seed", [(1, 1, 1, 0), (9, 4, 9, 1), (500, 7, 12, 2), (2048, 1, 3, 3), (2049, 300, 400, 4),
                                              (70000, 3000, 3500, 5), (33333, 4097, 70000, 6)])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_group_rows_equals_the_restatement(gpu, n, T, key_max, seed, order):
    rng = np.random.default_rng(seed)
    ids = rng.integers(-1, key_max + 3, n)                      # holds 0 ("unclaimed"), -1 and ids past key_max
    if order == "sorted":
        ids = np.sort(ids)
    keys = rng.permutation(np.arange(1, key_max + 1))[:T]       # a subset: absent keys and dropped ids both occur
    off, rows, nnz = run_group(gpu, ids, keys, key_max)
    ref_off, ref_rows = np_group_rows(ids, keys)
    f_off, f_rows = fast_group_rows(ids, keys)
    assert np.array_equal(f_off, ref_off) and np.array_equal(f_rows, ref_rows)
    assert nnz == ref_off[-1] and np.array_equal(off, ref_off), (n, T)
    assert np.array_equal(rows[:nnz], ref_rows) and not rows[nnz:].any()
    assert nnz < n or n < 9                                      # rows were dropped in every case of any size


def test_group_rows_on_a_million_rows_and_degenerate_calls(gpu):
    rng = np.random.default_rng(7)
    n, key_max = 2 ** 20 + 12345, 40000
    keys = rng.permutation(np.arange(1, key_max + 1))[:31000]
    for ids in (np.sort(rng.integers(0, key_max + 1, n)), rng.integers(0, key_max + 1, n)):
        off, rows, nnz = run_group(gpu, ids, keys, key_max)
        ref_off, ref_rows = fast_group_rows(ids, keys)
        assert nnz == ref_off[-1] and np.array_equal(off, ref_off) and np.array_equal(rows[:nnz], ref_rows)
        assert not rows[nnz:].any() and 0 < nnz < n
    # no keys, no rows, nothing claimed
    off, rows, nnz = run_group(gpu, [3, 4, 5], [], 9)
    assert list(off) == [0] and nnz == 0 and not rows.any()
    off, rows, nnz = run_group(gpu, [], [2, 1], 9)
    assert list(off) == [0, 0, 0] and nnz == 0 and rows.size == 0
    off, rows, nnz = run_group(gpu, [3, 4, 5], [1, 2], 9)
    assert list(off) == [0, 0, 0] and nnz == 0 and not rows.any()


def planted(rng, F, E):
    """logits with ties planted across emotions and rows, a few NaN and -Inf"""
    x = (rng.standard_normal((F, E)) * 3).astype(np.float32)
    x[rng.random((F, E)) < 0.15] = np.float32(2.5)
    x[rng.random((F, E)) < 0.05] = np.float32(7.25)              # the usual maximum, several times per track
    x[rng.random((F, E)) < 0.01] = np.nan
    x[rng.random((F, E)) < 0.01] = -np.inf
    return np.asfortranarray(x)


def check_peaks(got, x, groups):
    fi, tg, mx = got
    for t, r in enumerate(groups):
        rfi, rtg, rmx = np_track_peaks(x[np.asarray(r, int) - 1] if len(r) else np.zeros((0, x.shape[1]), np.float32))
        assert (fi[t], tg[t]) == (rfi, rtg), (t, len(r), fi[t], tg[t], rfi, rtg)
        assert np.array_equal(mx[:, t].view(np.uint32), rmx.view(np.uint32)), t


@pytest.mark.parametrize("E", [8, 3, 70])
def test_track_peaks_equals_the_restatement(gpu, E):
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(E)
    lens = np.concatenate([[0, 1, 2, 63, 64, 65, 129, 0, 300], rng.integers(1, 90, 60), [0]])
    F = int(lens.sum())
    x = planted(rng, F, E)
    x[3:66, :] = np.float32(1.5)                                 # a whole track tied: first entry
    x[66] = np.nan                                               # ... and the head of the next one all NaN
    offs = np.concatenate([[0], np.cumsum(lens)])
    dx = vl.from_numpy(x, gpu)
    doff = torch.from_numpy(offs.astype(np.int32)).to(gpu)
    fi, tg, mx = vl.track_peaks(dx, doff)
    got = (fi.cpu().numpy(), tg.cpu().numpy(), vl.to_numpy(mx).reshape(E, -1, order="F"))
    check_peaks(got, x, [np.arange(offs[t], offs[t + 1]) + 1 for t in range(len(lens))])
    assert got[0][0] == 0 and got[1][0] == 0 and np.isneginf(got[2][:, 0]).all()        # the empty group
    assert (got[0][3], got[1][3]) == (1, 1)
    # through a row list: shuffled rows, rows shared between groups
    groups = [rng.permutation(F)[:l] + 1 for l in lens]
    roff = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    rows = torch.from_numpy(np.concatenate(groups).astype(np.int32)).to(gpu)
    fi, tg, mx = vl.track_peaks(dx, torch.from_numpy(roff).to(gpu), rows)
    check_peaks((fi.cpu().numpy(), tg.cpu().numpy(), vl.to_numpy(mx).reshape(E, -1, order="F")), x, groups)
    with pytest.raises(ValueError, match="reach past"):
        vl.track_peaks(dx, torch.from_numpy(roff + 1).to(gpu), rows)


def test_track_peaks_equals_aggregate_logits_bit_for_bit(gpu):
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(11)
    lens = rng.integers(1, 120, 500)
    x = planted(rng, int(lens.sum()), 8)
    offs = np.concatenate([[0], np.cumsum(lens)])
    dx = vl.from_numpy(x, gpu)
    fi, tg, mx = vl.track_peaks(dx, torch.from_numpy(offs.astype(np.int32)).to(gpu))
    first = torch.from_numpy((offs[:-1] + 1).astype(np.int32)).to(gpu)
    last = torch.from_numpy(offs[1:].astype(np.int32)).to(gpu)
    amax, _ = vl.aggregate_logits(dx, first, last, "max")
    apeak, _ = vl.aggregate_logits(dx, first, last, "peak")
    assert torch.equal(mx.contiguous().view(torch.int32), amax.contiguous().view(torch.int32))
    # the row XM_AGG_PEAK picked = the frame_idx-th row of the track
    prow = vl.gather_rows(dx, (first + fi - 1).to(torch.int32).contiguous())
    assert torch.equal(prow.contiguous().view(torch.int32), apeak.contiguous().view(torch.int32))


def test_gather_then_scatter_round_trips(gpu):
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(5)
    F, E = 1000, 8
    x = planted(rng, F, E)
    dx = vl.from_numpy(x, gpu)
    bits = lambda t: vl.to_numpy(t).view(np.uint32)
    # contiguous block
    p = vl.gather_rows(dx, row0=100, n=300)
    assert np.array_equal(bits(p).reshape(E, 300, order="F"), x[100:400].T.view(np.uint32))
    y = vl.mat_zeros(F, E, device=gpu)
    vl.scatter_rows(p, y, row0=100)
    got = vl.to_numpy(y)
    assert np.array_equal(got[100:400].view(np.uint32), x[100:400].view(np.uint32))
    assert not got[:100].any() and not got[400:].any()           # the other rows are left as they were
    # a permutation of all rows through a list, and back
    perm = torch.from_numpy((rng.permutation(F) + 1).astype(np.int32)).to(gpu)
    p = vl.gather_rows(dx, perm)
    z = vl.mat_zeros(F, E, device=gpu)
    vl.scatter_rows(p, z, perm)
    assert np.array_equal(bits(z), x.view(np.uint32))
    # the whole matrix without a list
    z2 = vl.mat_zeros(F, E, device=gpu)
    vl.scatter_rows(vl.gather_rows(dx), z2)
    assert np.array_equal(bits(z2), x.view(np.uint32))


# ------------------------------------------------------------------------------------------------ buildImdb
class CountingTeacher:
    """.logits(faces): logit e of the k-th frame it has ever been shown is 8 k + e -- exact in fp32 below 2^24"""
    imageSize, averageImage = (8, 8), (0.0, 0.0, 0.0)

    def __init__(self, device):
        self.seen, self.device, self.batches = 0, device, []

    def logits(self, faces):
        from mcncrossmodalemotions_amd import vl
        n = int(faces.shape[3])
        assert tuple(faces.shape[:3]) == (8, 8, 3)
        self.batches.append(n)
        k = torch.arange(self.seen, self.seen + n, device=self.device, dtype=torch.float32)
        out = (k[:, None] * 8 + torch.arange(8, device=self.device, dtype=torch.float32)[None, :])
        self.seen += n
        return out.reshape(n, 8, 1, 1).permute(3, 2, 1, 0)


def framed_imdb(num_tracks, seed, frameless=(), unclaimed=0, frameSize=(16, 16), **kw):
    from mcncrossmodalemotions_amd import batch, fetch_emovoxceleb_imdb as fe
    syn = batch.SyntheticEmoVoxImdb(num_tracks=num_tracks, seed=seed, **kw)
    src = fe.src_imdb(syn)
    frames = batch.SyntheticDenseFrames(src, seed=seed, frameSize=frameSize, frameless=frameless, unclaimed=unclaimed)
    return fe.addFramesToImdb(src, frames.lister, find=frames.find), frames


@pytest.mark.parametrize("batchSize", [1, 7, 128, 1000])
@pytest.mark.parametrize("limit", [math.inf, 5])
def test_build_bookkeeping_with_a_counting_teacher(gpu, batchSize, limit):
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    imdb, frames = framed_imdb(12, 3, frameless=(8, 11), unclaimed=4, min_seconds=1.0, max_seconds=4.0)
    asked = []

    def source(paths, device):
        asked.append(list(paths))
        return frames(paths, device)

    teacher = CountingTeacher(gpu)
    built = fe.buildImdb(teacher, imdb, source, limit=limit, batchSize=batchSize)
    wavIds, ids = imdb.images["denseFramesWavIds"], imdb.images["id"]
    numIms = int((wavIds <= ids[0] + limit).sum())
    numLogits = int(min(len(ids), limit))
    assert teacher.seen == numIms and sum(asked, []) == imdb.images["denseFrames"][:numIms]
    assert teacher.batches == [min(batchSize, numIms - s) for s in range(0, numIms, batchSize)]
    assert numIms % batchSize or batchSize == 1                  # a ragged last batch in every other case
    assert len(built.wavLogits) == len(ids) == 10
    for i, cell in enumerate(built.wavLogits):
        f = np.nonzero(wavIds[:numIms] == ids[i])[0] if i < numLogits else np.zeros(0, int)
        want = f[:, None] * 8.0 + np.arange(8)[None, :]
        assert cell.dtype == np.float32 and cell.shape == (len(f), 8) and np.array_equal(cell, want), i
    if limit == 5:      # ids 1 .. 6 are <= firstId + 5: six tracks of frames, five cells
        assert numIms == int(np.isin(wavIds, [1, 2, 3, 4, 5, 6]).sum()) and numLogits == 5
        assert sum(c.shape[0] for c in built.wavLogits) == int(np.isin(wavIds, [1, 2, 3, 4, 5]).sum()) < numIms
    # the device copy is the concatenation of the cells, with the offsets of every track
    dev, offs = built.device_logits(gpu)
    from mcncrossmodalemotions_amd import vl
    cat = np.concatenate(built.wavLogits, 0)
    assert np.array_equal(vl.to_numpy(dev)[:cat.shape[0]], cat)
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum([c.shape[0] for c in built.wavLogits])]))
    assert built.images is imdb.images and imdb.wavLogits is None


def test_frames_do_not_depend_on_the_batch(gpu):
    imdb, frames = framed_imdb(4, 1, min_seconds=1.0, max_seconds=2.0)
    paths = imdb.images["denseFrames"][:9]
    whole = frames(paths, gpu)
    assert tuple(whole.shape) == (16, 16, 3, 9) and float(whole.min()) >= 0 and float(whole.max()) <= 255
    for i in (0, 4, 8):
        assert torch.equal(frames([paths[i]], gpu)[..., 0], whole[..., i])
    assert torch.equal(frames(paths[::-1], gpu), whole.flip(3))
    assert not torch.equal(whole[..., 0], whole[..., 1])


def small_teacher(seed=1):
    """a ferPlusZoo teacher as loaded (its loss layers still attached), narrow and for 64 x 64 faces"""
    from mcncrossmodalemotions_amd import zoo
    net = zoo.ferPlusZoo("resnet50-ferplus", seed=seed, width_mult=0.125, blocks=(1, 1, 1, 1))
    net.getLayer("pool5").block.poolSize = [2, 2]
    net.meta["normalization"]["imageSize"] = [64, 64, 3]
    return net


def test_built_logits_match_the_oracle_forward(gpu):
    """the real test-mode teacher (ResNet-50 topology at a quarter of the width, 224 x 224 faces) over 36 distinct
    synthetic frames in ragged batches of 12: the allowance of tests/test_gpu_nets_full.py for the teacher's logits
    (1e-4 of max(1, max|ref|))"""
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe, vl, zoo
    from oracle import oracle_net
    imdb, frames = framed_imdb(3, 21, frameSize=(300, 280), min_seconds=2.0, max_seconds=3.5)
    numIms = len(imdb.images["denseFrames"])
    assert 24 <= numIms <= 48
    net = zoo.ferPlusZoo("resnet50-ferplus", seed=5, width_mult=0.25, blocks=(1, 1, 1, 1))
    built = fe.buildImdb(net, imdb, frames, batchSize=12)
    assert net.mode == "test" and len(net.getInputs()) == 1
    faces = vl.crop_resize_face(frames(imdb.images["denseFrames"], gpu), net.meta["normalization"]["averageImage"],
                                (224, 224))
    ref = oracle_net.forward(net, {"data": vl.to_numpy(faces)}, mode="test")["prediction"].reshape(8, numIms, order="F").T
    got = np.concatenate(built.wavLogits, 0)
    err, scale = float(np.abs(got - ref).max()), max(1.0, float(np.abs(ref).max()))
    print("built logits vs oracle: max err %.3e, allowance %.3e" % (err, 1e-4 * scale))
    assert got.shape == ref.shape and err <= 1e-4 * scale
    assert np.unique(ref, axis=0).shape[0] == numIms        # distinct frames gave distinct logits


@pytest.fixture(scope="module")
def built(gpu):
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    imdb, frames = framed_imdb(40, 8, frameless=(7,), unclaimed=3, frameSize=(96, 96), min_seconds=1.6, max_seconds=4.0,
                               val_fraction=0.3, heard_fraction=0.2)
    return fe.buildImdb(small_teacher(), imdb, frames, batchSize=50)


def test_built_imdb_drives_get_batch(gpu, built):
    from mcncrossmodalemotions_amd import batch, vl
    assert all(np.isfinite(c).all() and c.shape[0] > 0 for c in built.wavLogits)
    assert np.std(np.concatenate(built.wavLogits, 0), 0).min() > 0          # a teacher's logits, not a constant
    sel = [0, 5, 11, 38]
    inputs = batch.getBatchEmoVoxCeleb(built, sel, imageSize=(512, 100), rng=np.random.default_rng(3), device=gpu)
    d = dict(zip(inputs[::2], inputs[1::2]))
    lgo = vl.to_numpy(d["logitTarget"]).reshape(8, -1, order="F")
    rng = np.random.default_rng(3)
    for k, ii in enumerate(sel):
        _, s, e = batch.crop_window(int(built.num_samples[ii]), batch.aud_samples(100), built.fs,
                                    built.wavLogits[ii].shape[0], rng)
        want = built.wavLogits[ii][s - 1:e].max(0)
        assert np.array_equal(lgo[:, k], want), (k, ii)
        assert int(vl.to_numpy(d["maxLabel"]).ravel()[k]) == int(want.argmax()) + 1


def test_built_imdb_drives_distillation_and_student_stats(gpu, built, tmp_path):
    from mcncrossmodalemotions_amd import student_stats as ss, zoo
    from mcncrossmodalemotions_amd.run_distillation import run_distillation
    net, info = run_distillation(gpus=[0], numSeconds=1, batchSize=4, miniEpochRatio=0.5, miniVal=0.5, widthMult=0.125,
                                 dataDir=str(tmp_path), learningRate=[1e-3], numEpochs=1, imdb=built)
    assert len(info["train"]) == 1 and np.isfinite(info["train"][0]["objective"]) and info["train"][0]["num"] > 0
    student = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=9)
    res = ss.student_stats(partition="train", student="reduced", figDir=str(tmp_path / "figs"), imdb=built, net=student,
                           root=str(tmp_path), verbose=False)
    r = res["train"]
    lab = np.stack([c.max(0) for c in built.wavLogits]).argmax(1) + 1
    keep = built.set == 1
    assert np.array_equal(r["counts"]["p"], np.bincount(lab[keep], minlength=9)[1:])
    assert np.array_equal(r["counts"]["p"] + r["counts"]["n"], np.full(8, keep.sum())) and not r["status"].any()
    assert np.isfinite(r["auc"]).all()
    res = ss.teacher_stats(figurePath=str(tmp_path / "fig.pdf"), imdb=built, verbose=False)
    assert np.array_equal(res["emoCeleb"], np.bincount(np.concatenate(built.wavLogits, 0).argmax(1), minlength=8))


def test_sample_audio_on_the_built_imdb(gpu, built, tmp_path):
    from mcncrossmodalemotions_amd import sample_audio as sa
    dest = str(tmp_path / "samples")
    # logits with enough tracks per emotion: the built rows with one entry per track raised above everything else
    # (25 tracks tagged 2)
    import copy
    imdb = copy.copy(built)
    cells = [c.copy() for c in built.wavLogits]
    for i, c in enumerate(cells):
        c[i % c.shape[0], (1 if i < 25 else i % 8)] = np.float32(2 * np.abs(c).max() + 50)
    imdb.wavLogits, imdb._dev = cells, None
    out = sa.sample_audio(sampleFrameSeq=True, imdb=imdb, dest=dest, verbose=False)
    ref = [np_track_peaks(c) for c in cells]
    assert np.array_equal(out["frameIdx"], [r[0] for r in ref]) and np.array_equal(out["tags"], [r[1] for r in ref])
    assert np.array_equal(out["maxedLogits"], np.stack([r[2] for r in ref]))
    assert sorted(out["samples"]) == sorted(["neutral", "happiness", "surprise", "sadness", "anger"])
    assert sorted(os.listdir(dest)) == sorted(e for e in out["samples"] if out["samples"][e])
    assert len(out["samples"]["happiness"]) == 20 and (out["tags"] == 2).sum() >= 25
    wavIds = np.asarray(imdb.images["denseFramesWavIds"])
    seen = 0
    for emo, recs in out["samples"].items():
        emoIdx = sa.EMOTIONS.index(emo) + 1
        assert len(recs) == min(20, int((out["tags"] == emoIdx).sum()))
        assert len(set(r["track"] for r in recs)) == len(recs)
        for jj, r in enumerate(recs, 1):
            ti = r["track"]
            seen += 1
            assert out["tags"][ti] == emoIdx and r["dir"] == os.path.join(dest, emo, str(jj))
            trackFrames = [p for p, w in zip(imdb.images["denseFrames"], wavIds) if w == imdb.images["id"][ti]]
            with open(os.path.join(r["dir"], "manifest.json")) as f:
                man = json.load(f)
            assert man["peakFrame"]["path"] == trackFrames[out["frameIdx"][ti] - 1]
            assert [x["src"].split("unzippedIntervalFaces/")[1] for x in man["frames"]] == sorted(trackFrames)
            assert man["frames"][0]["dest"] == os.path.join("frames", "00001.jpg")
            with open(os.path.join(r["dir"], "meta.txt"), newline="") as f:
                meta = f.read()
            assert meta == sa.format_meta(imdb.images["name"][ti][:-4] + ".avi", out["maxedLogits"][ti])
            assert meta.startswith("aviPath: id") and meta.count("\n") == 2 and meta.endswith(" ")
            with open(os.path.join(r["dir"], "distribution.json")) as f:
                dj = json.load(f)
            assert dj["values"] == [float(v) for v in out["maxedLogits"][ti]] and dj["colors"] == sa.COLORS
            assert dj["ylim"] == [min(-3.0, min(dj["values"])), max(10.0, max(dj["values"]))]
            assert dj["xticklabels"][:2] == ["Neu", "Hap"]
    assert seen > 20
    for emo in ("disgust", "contempt", "fear"):
        assert not os.path.exists(os.path.join(dest, emo))
    # a second run without clobber changes nothing; with clobber only <dest> is rebuilt
    stamp = {os.path.join(d, p): os.path.getmtime(os.path.join(d, p)) for d, _, fs in os.walk(dest) for p in fs}
    keepme = tmp_path / "other.txt"
    keepme.write_text("x")
    assert sa.sample_audio(sampleFrameSeq=True, imdb=imdb, dest=dest, verbose=False) is None
    assert stamp == {os.path.join(d, p): os.path.getmtime(os.path.join(d, p)) for d, _, fs in os.walk(dest) for p in fs}
    again = sa.sample_audio(clobber=True, samplePeaks=False, imdb=imdb, dest=dest, verbose=False)
    assert [r["track"] for r in again["samples"]["happiness"]] == [r["track"] for r in out["samples"]["happiness"]]
    assert again["samples"]["happiness"][0]["peakFrame"] is None and again["samples"]["happiness"][0]["frames"] is None
    assert keepme.read_text() == "x"
