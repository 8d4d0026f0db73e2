"""GPU: xm_spec_bucket_batch / vl.spec_bucket_batch / external.compute_audio_feats_wav -- the batched whole-clip audio
front-end (compute_audio_feats.m:160-185: runSpec of the whole clip, rows normalised by mean / std over ALL its frames,
centre crop to the bucket width) -- against the float64 restatement O.spec_rownorm(O.run_spec(clip))[:, f0:f0 + rsize].

Clips are seeded 0.1 * randn laid back to back in one bank: the first starts at 0, the last ends at the bank's end, and
no other start is a multiple of the hop.  Allowance: `close` of tests/test_gpu_ops.py at 1e-3, what
test_run_spec_front_end gives rownorm(runSpec) on the existing path."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

NW, NS, TOL = 400, 160, 1e-3


def err_of(a, b):
    """the quantity `close` of tests/test_gpu_ops.py bounds: max |a - b| / max(1, max |b|)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


def close(a, b, tol, what):
    err = err_of(a, b)
    print("%s: err %.3e (allowed %.1e)" % (what, err, tol))
    assert err <= tol, "%s: err %.3e > %.1e" % (what, err, tol)


def _len(T, r=0):
    return NW + NS * (T - 1) + r


def _bank(frames_r, seed):
    """(bank float32, offsets) of seeded clips with T frames and r residual samples each, back to back"""
    rng = np.random.default_rng(seed)
    lengths = [_len(T, r) for T, r in frames_r]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    assert all(int(o) % NS for o in offs[1:-1]), offs
    return (rng.standard_normal(int(offs[-1])) * 0.1).astype(np.float32), offs


def _reference(bank, offs, f0, rsize):
    return [O.spec_rownorm(O.run_spec(bank[offs[k]:offs[k + 1]]))[:, int(f0[k]):int(f0[k]) + rsize, 0, 0]
            for k in range(len(offs) - 1)]


def _run(gpu, bank, desc, rsize):
    import torch
    from mcncrossmodalemotions_amd import vl
    return vl.to_numpy(vl.spec_bucket_batch(torch.from_numpy(bank).to(gpu), desc, rsize))


# T in {100, 101, 103, 157, 199} x r in {0, 1, 159}
NINE = [(100, 159), (199, 0), (103, 159), (101, 1), (157, 0), (100, 0), (199, 1), (157, 159), (101, 0)]


@pytest.fixture(scope="module")
def nine():
    from mcncrossmodalemotions_amd import external
    bank, offs = _bank(NINE, 2024)
    T, rsize, f0, groups = external.audio_feats_plan(np.diff(offs), offs[:-1])
    assert T.tolist() == [t for t, _ in NINE] and (rsize == 100).all() and len(groups) == 1
    return bank, offs, groups[0][2], _reference(bank, offs, f0, 100)


def test_parity_bucket_100(gpu, nine):
    bank, offs, desc, ref = nine
    got = _run(gpu, bank, desc, 100)
    assert got.shape == (512, 100, 1, 9)
    worst = max(err_of(got[:, :, 0, k], ref[k]) for k in range(9))
    print("bucket 100, nine clips: worst err %.3e" % worst)
    for k in range(9):
        close(got[:, :, 0, k], ref[k], TOL, "clip %d (T = %d, r = %d)" % (k, *NINE[k]))


@pytest.mark.parametrize("k", [0, 4, 8])
def test_a_clip_is_its_own(gpu, nine, k):
    """everything outside clip k made 100 times louder: neither the pre-emphasis predecessor of its first sample nor a
    frame running past its end may see it"""
    bank, offs, desc, _ = nine
    loud = bank * np.float32(100)
    loud[offs[k]:offs[k + 1]] = bank[offs[k]:offs[k + 1]]
    a, b = _run(gpu, bank, desc, 100), _run(gpu, loud, desc, 100)
    assert np.array_equal(a[:, :, 0, k], b[:, :, 0, k])
    assert not np.array_equal(a[:, :, 0, (k + 1) % 9], b[:, :, 0, (k + 1) % 9])


def test_statistics_over_the_whole_clip(gpu):
    """T = 157 with the samples of the first 20 frames 30 times louder; the window at the start, the centre and the end"""
    rng = np.random.default_rng(7)
    clip = (rng.standard_normal(_len(157, 3)) * 0.1).astype(np.float32)
    clip[:20 * NS] *= np.float32(30)
    full = O.spec_rownorm(O.run_spec(clip))[:, :, 0, 0]
    desc = np.array([[0, clip.size, f0] for f0 in (0, 28, 57)], np.int64)
    got = _run(gpu, clip, desc, 100)
    for i, f0 in enumerate((0, 28, 57)):
        close(got[:, :, 0, i], full[:, f0:f0 + 100], TOL, "window at %d" % f0)
    # statistics over the crop alone would be far off: the reference of the last window normalised by itself
    alone = O.spec_rownorm(O.run_spec(clip)[:, 57:157])[:, :, 0, 0]
    assert err_of(alone, full[:, 57:157]) > 100 * TOL


@pytest.mark.parametrize("rsize,frames_r", [(200, [(200, 1), (257, 1), (299, 159)]), (1000, [(1012, 5)])])
def test_other_buckets(gpu, rsize, frames_r):
    from mcncrossmodalemotions_amd import external
    bank, offs = _bank(frames_r, 100 + rsize)
    _, rs, f0, groups = external.audio_feats_plan(np.diff(offs), offs[:-1])
    assert (rs == rsize).all()
    got = _run(gpu, bank, groups[0][2], rsize)
    for k, ref in enumerate(_reference(bank, offs, f0, rsize)):
        close(got[:, :, 0, k], ref, TOL, "bucket %d, T = %d" % (rsize, frames_r[k][0]))


def test_conditioning(gpu):
    """A tone on bin 100 exactly (1562.5 Hz) over a 1e-3 noise floor, T = 120: the rows near the tone have a mean far
    above their std.  The new path may miss the float64 reference by the larger of TOL and twice what the parent path
    (runSpec -> test_getinput) misses it by: only the summation order of the 401-term products and of the statistics
    differs between the two."""
    import torch
    from mcncrossmodalemotions_amd import batch as xbatch, external, vl
    rng = np.random.default_rng(11)
    L = _len(120)
    clip = (np.sin(2 * np.pi * 1562.5 * np.arange(L) / 16000.0) + 1e-3 * rng.standard_normal(L)).astype(np.float32)
    ref = O.spec_rownorm(O.run_spec(clip))[:, :, 0, 0]
    assert np.isfinite(ref).all()
    T, rsize, f0, groups = external.audio_feats_plan([L], [0])
    ref = ref[:, int(f0[0]):int(f0[0]) + 100]
    dev = torch.from_numpy(clip).to(gpu)
    parent, w = external.test_getinput(xbatch.runSpec(dev)[:, :, 0, 0])
    assert w == 100
    e_parent = err_of(vl.to_numpy(parent)[:, :, 0, 0], ref)
    e_new = err_of(vl.to_numpy(vl.spec_bucket_batch(dev, groups[0][2], 100))[:, :, 0, 0], ref)
    print("conditioning: parent path err %.3e, spec_bucket_batch err %.3e" % (e_parent, e_new))
    assert e_new <= max(TOL, 2 * e_parent)


def test_driver_bookkeeping(gpu):
    """compute_audio_feats_wav against compute_audio_feats on runSpec of every clip, on the network of
    test_compute_audio_feats_variable_width; allowance: what that test gives batched against per-clip (1e-5)"""
    import torch
    from mcncrossmodalemotions_amd import batch as xbatch, external, zoo
    frames_r = [(100, 0), (205, 1), (137, 159), (250, 3), (199, 0), (299, 77), (157, 1)]
    bank, offs = _bank(frames_r, 41)
    net = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=9)
    dev = torch.from_numpy(bank).to(gpu)
    specs = [xbatch.runSpec(dev[offs[k]:offs[k + 1]])[:, :, 0, 0] for k in range(7)]
    ref = external.compute_audio_feats(net, specs, batch_by_bucket=True)
    got = external.compute_audio_feats_wav(net, dev, offs)
    assert got.shape == ref.shape == (7, 8)
    close(got, ref, 1e-5, "compute_audio_feats_wav vs compute_audio_feats")
    few = external.compute_audio_feats_wav(net, dev, offs, limit=3)      # ids <= firstId + 3: four clips
    assert few.shape == (4, 8)
    close(few, got[:4], 1e-5, "limit = 3")
    close(external.compute_audio_feats_wav(net, dev, offs, maxBatch=2), got, 1e-5, "maxBatch 2 vs 64")
    assert external.compute_audio_feats_wav(net, dev, offs, limit=0).shape == (1, 8)


def _launches(L, fn):
    from mcncrossmodalemotions_amd import prof
    out, rows = prof.kernels_run(fn, L)
    return out, {r.name: r.launches for r in rows}


def test_fixed_launch_count_no_tuning(gpu, nine):
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    L = _lib.load()
    bank, offs, desc, _ = nine
    dev = torch.from_numpy(bank).to(gpu)
    vl.spec_bucket_batch(dev, desc, 100)                               # the filter bank and the workspace exist
    tot0, new0 = C.c_int(0), C.c_int(0)
    L.xm_tune_entries(C.byref(tot0), C.byref(new0))
    a, two = _launches(L, lambda: vl.spec_bucket_batch(dev, desc[:2], 100))
    b, all9 = _launches(L, lambda: vl.spec_bucket_batch(dev, desc, 100))
    print("launches:", all9)
    assert two == all9 and sum(all9.values()) == 4 and all(k.startswith("spec_") for k in all9)
    tot1, new1 = C.c_int(0), C.c_int(0)
    L.xm_tune_entries(C.byref(tot1), C.byref(new1))
    assert (tot0.value, new0.value) == (tot1.value, new1.value)
    assert torch.equal(b, vl.spec_bucket_batch(dev, desc, 100))
    assert torch.equal(a, b[:, :, :, :2])                             # the first two clips do not see the others


def test_status_codes(gpu, nine):
    import torch
    from mcncrossmodalemotions_amd import _lib, batch as xbatch, vl
    Lb = _lib.load()
    bank, offs, desc, _ = nine
    w = torch.from_numpy(bank).to(gpu)
    d = torch.from_numpy(desc[:1].copy()).to(gpu)
    fb = xbatch._spec_filter_bank(16000, 25, 10, 0.97, 1024, gpu)
    out = vl.mat_empty(512, 100, 1, 1, device=gpu)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    call = lambda wav, dd, N, rsize, f, o, wav_len=None: Lb.xm_spec_bucket_batch(   # noqa: E731
        P(wav), (0 if wav is None else wav.numel()) if wav_len is None else wav_len, P(dd), N, rsize, P(f), NW + 1, NS, 512,
        P(o), vl._stream())
    assert Lb.xm_version() >= 112
    assert call(w, d, 1, 100, fb, out) == 0
    for args in [(w, d, -1, 100, fb, out), (w, d, 1, 0, fb, out), (w, d, 1, -3, fb, out), (None, d, 1, 100, fb, out),
                 (w, None, 1, 100, fb, out), (w, d, 1, 100, None, out), (w, d, 1, 100, fb, None),
                 (w, d, 1, 100, fb, out, -1)]:
        assert call(*args) == 1, args                                  # XM_EINVAL
    assert call(None, None, 0, 100, None, None) == 0                   # N == 0: XM_OK, nothing is touched
    assert call(w, d, 65536, 100, fb, out) == 4                        # XM_ETOOBIG, before any launch
    assert tuple(vl.spec_bucket_batch(w, np.zeros((0, 3), np.int64), 100).shape) == (512, 100, 1, 0)
    bad = desc.copy()
    bad[8, 1] += 1                                                     # the last clip ends at the bank's end
    with pytest.raises(ValueError, match="leaves the waveform bank"):
        vl.spec_bucket_batch(w, bad, 100)
    bad = desc.copy()
    bad[0, 0] = -1
    with pytest.raises(ValueError, match="leaves the waveform bank"):
        vl.spec_bucket_batch(w, bad, 100)
    bad = desc.copy()
    bad[4, 2] = 58                                                     # T = 157: 58 + 100 > T
    with pytest.raises(ValueError, match="leave its spectrogram"):
        vl.spec_bucket_batch(w, bad, 100)
    with pytest.raises(ValueError):
        vl.spec_bucket_batch(w, desc[:, :2], 100)


def test_student_stats_wav_batch(gpu, tmp_path):
    from mcncrossmodalemotions_amd import batch, student_stats as ss, zoo
    imdb = batch.SyntheticEmoVoxImdb(num_tracks=12, seed=3, val_fraction=0.25, heard_fraction=0.25, min_seconds=1.2,
                                     max_seconds=3.5)
    net = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=9)
    logits = {}
    for wavBatch in (False, True):
        root = str(tmp_path / ("wav" if wavBatch else "clip"))
        res = ss.student_stats(student="reduced", figDir=root + "/figs", imdb=imdb, net=net, root=root, verbose=False,
                               wavBatch=wavBatch)
        path = res["train"]["featPath"]
        assert path.startswith(root)
        logits[wavBatch] = ss.load_student_feats(path)[1]
    assert logits[True].shape == (12, 8)
    close(logits[True], logits[False], 1e-5, "student_stats(wavBatch=True) logits")
