"""GPU: the cross-validation step of external/run_cross_val.m and external/emo_benchmarks.m -- the 'peak' aggregator,
the fold-batched fp64 mnrfit (xm_mnrfit) and mnrval (xm_mnrval), and the two entry points end to end."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ numpy restatements
def np_peak(lg, first, last):
    """selectPeakLogit per track: the row of the F_i x E block holding max(logits(:)), column-major first."""
    out = []
    for f, l in zip(first, last):
        blk = lg[f - 1:l]
        idx = int(np.argmax(blk.ravel(order="F")))          # first maximum in column-major order
        out.append(blk[idx % blk.shape[0]])
    return np.stack(out, 1)


def _probs(Xt, B):
    eta = np.hstack([Xt @ B, np.zeros((Xt.shape[0], 1))])
    m = eta.max(1, keepdims=True)
    e = np.exp(eta - m)
    return e / e.sum(1, keepdims=True), eta, m, e


def np_loglik_grad(X, y, B):
    """fp64 log-likelihood and its gradient (p+1) x (k-1) of the nominal model at B; X is n x p, y 1-based."""
    n = X.shape[0]
    Xt = np.hstack([np.ones((n, 1)), X.astype(np.float64)])
    P, eta, m, e = _probs(Xt, B)
    k = P.shape[1]
    Y = np.zeros((n, k))
    Y[np.arange(n), y - 1] = 1
    L = float((eta[np.arange(n), y - 1] - m[:, 0] - np.log(e.sum(1))).sum())
    return L, Xt.T @ (Y - P)[:, :k - 1]


def np_mnrfit(X, y, k, maxIter=100, tolX=1e-6):
    """Newton-Raphson from B = 0 with step halving and statset('mnrfit')'s stopping rule, fp64."""
    n, p = X.shape
    Xt = np.hstack([np.ones((n, 1)), X.astype(np.float64)])
    D = (p + 1) * (k - 1)

    def ev(B):
        L, g = np_loglik_grad(X, y, B)
        P = _probs(Xt, B)[0][:, :k - 1]
        W = np.einsum("ij,jl->ijl", P, np.eye(k - 1)) - np.einsum("ij,il->ijl", P, P)
        H = np.einsum("ia,ib,ijl->jalb", Xt, Xt, W).reshape(D, D)      # index a + (p+1) j
        return L, g.reshape(-1, order="F"), H

    B = np.zeros(D)
    L, g, H = ev(B.reshape(p + 1, k - 1, order="F"))
    it = 0
    for it in range(1, maxIter + 1):
        delta = np.linalg.solve(H, g)
        t = 1.0
        for h in range(31):
            Bn = B + t * delta
            Ln, gn, Hn = ev(Bn.reshape(p + 1, k - 1, order="F"))
            if Ln >= L or h == 30:
                break
            t /= 2
        step, B, L, g, H = np.abs(Bn - B).max(), Bn, Ln, gn, Hn
        if step <= tolX * max(1.0, np.abs(B).max()):
            break
    return B.reshape(p + 1, k - 1, order="F"), -2 * L, it


def np_mnrval(B, X):
    n = X.shape[0]
    return _probs(np.hstack([np.ones((n, 1)), X.astype(np.float64)]), B)[0]


def planted(n, p, k, seed, scale=1.2):
    """non-separable data: Gaussian class means + unit noise, labels dealt out evenly."""
    rng = np.random.default_rng(seed)
    y = rng.permutation(np.arange(n) % k) + 1
    mu = rng.standard_normal((k, p)) * scale
    X = (mu[y - 1] + rng.standard_normal((n, p))).astype(np.float32)
    return X, y


def folds(n, K, seed):
    from mcncrossmodalemotions_amd.emo_benchmarks import cross_val_folds
    return cross_val_folds(np.random.default_rng(seed).permutation(n) + 1, K)


def _dev(X, y):
    """X n x p host -> p x n device features, y -> int32 device labels."""
    import torch
    from mcncrossmodalemotions_amd import vl
    return vl.from_numpy(np.asarray(X, np.float32).T), torch.from_numpy(np.asarray(y, np.int32)).cuda()


def _fit(X, y, sets, k, **kw):
    from mcncrossmodalemotions_amd import vl
    dX, dy = _dev(X, y)
    B, st, it, dv = vl.mnrfit(dX, dy, sets, k, **kw)
    return vl.to_numpy(B), st.cpu().numpy(), it.cpu().numpy(), dv.cpu().numpy()


# ------------------------------------------------------------------------------------------------ peak aggregator
def test_peak_aggregator_bit_exact_with_ties(gpu):
    import torch
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(3)
    counts = [1, 4, 7, 1, 3, 5, 2, 6]
    E = 8
    lg = np.round(rng.standard_normal((sum(counts), E)) * 4) / 4          # coarse values: many natural ties
    last = np.cumsum(counts)
    first = last - np.array(counts) + 1
    # planted ties: track 1 -- the maximum twice in one column (rows 2 and 4): the lower row wins
    b = first[1] - 1
    lg[b:b + 4] = -1
    lg[b + 1, 3] = lg[b + 3, 3] = 9
    # track 2 -- the maximum in two columns on different rows: the lower column wins even on the later row
    b = first[2] - 1
    lg[b:b + 7] = 0
    lg[b + 5, 1] = 7
    lg[b + 2, 6] = 7
    # track 5 -- the same maximum everywhere: the first row
    b = first[5] - 1
    lg[b:b + 5] = 2.5
    lg = lg.astype(np.float32)
    ref = np_peak(lg, first, last)
    assert ref[3, 1] == 9 and np.array_equal(ref[:, 2], lg[first[2] - 1 + 5])
    dfirst = torch.from_numpy(first.astype(np.int32)).cuda()
    dlast = torch.from_numpy(last.astype(np.int32)).cuda()
    dlg = vl.from_numpy(np.asfortranarray(lg))
    out, lab = vl.aggregate_logits(dlg, dfirst, dlast, "peak")
    got = vl.to_numpy(out).reshape(E, -1, order="F")
    assert np.array_equal(got, ref)
    assert np.array_equal(vl.to_numpy(lab).ravel(), ref.argmax(0) + 1)
    # max / mean: unchanged by the new mode on the same input
    for agg in ("max", "mean"):
        o, l2 = vl.aggregate_logits(dlg, dfirst, dlast, agg)
        g2 = vl.to_numpy(o).reshape(E, -1, order="F")
        if agg == "max":
            assert np.array_equal(g2, np.stack([lg[f - 1:l].max(0) for f, l in zip(first, last)], 1))
        else:
            ref_m = np.stack([lg[f - 1:l].sum(0, dtype=np.float32) / np.float32(l - f + 1)
                              for f, l in zip(first, last)], 1)
            assert np.abs(g2 - ref_m).max() < 1e-6
    with pytest.raises(ValueError):
        vl.aggregate_logits(dlg, dfirst, dlast, "median")


# ------------------------------------------------------------------------------------------------ mnrfit
@pytest.mark.parametrize("n,p,k,K,scale", [(700, 8, 6, 10, 1.2), (380, 8, 7, 1, 0.5)])
def test_mnrfit_gradient_vanishes(gpu, n, p, k, K, scale):
    """At the returned B the fp64 gradient of the log-likelihood, recomputed here, is <= 1e-6 n (RML-like 10 folds,
    AFEW-like one fold)."""
    from mcncrossmodalemotions_amd import vl
    X, y = planted(n, p, k, seed=n + k, scale=scale)
    train = folds(n, K, 1)[0] if K > 1 else [np.arange(1, int(n * 0.6) + 1)]
    B, st, it, dv = _fit(X, y, train, k)
    assert B.shape == (p + 1, k - 1, len(train))
    assert (st == vl.MNR_CONVERGED).all(), st
    assert (it > 2).all() and (it < 30).all(), it
    for g, tr in enumerate(train):
        L, grad = np_loglik_grad(X[tr - 1], y[tr - 1], B[:, :, g])
        assert np.abs(grad).max() <= 1e-6 * len(tr), (g, np.abs(grad).max())
        assert abs(dv[g] - (-2 * L)) <= 1e-9 * abs(L)


def test_mnrfit_matches_newton_restatement(gpu):
    X, y = planted(700, 8, 6, seed=11)
    train = folds(700, 10, 2)[0][:3]
    B, st, it, dv = _fit(X, y, train, 6)
    for g, tr in enumerate(train):
        Bref, dref, itref = np_mnrfit(X[tr - 1], y[tr - 1], 6)
        assert np.abs(B[:, :, g] - Bref).max() <= 1e-6 * np.abs(Bref).max()
        assert abs(dv[g] - dref) <= 1e-9 * dref
        assert abs(int(it[g]) - itref) <= 1


def test_mnrfit_batching_is_bit_identical(gpu):
    X, y = planted(700, 8, 6, seed=12)
    train = folds(700, 10, 3)[0]
    B, st, it, dv = _fit(X, y, train, 6)
    B2, st2, it2, dv2 = _fit(X, y, train, 6)
    assert np.array_equal(B, B2) and np.array_equal(dv, dv2) and np.array_equal(it, it2)
    for g, tr in enumerate(train):
        b1, s1, i1, d1 = _fit(X, y, [tr], 6)
        assert np.array_equal(b1[:, :, 0], B[:, :, g]) and d1[0] == dv[g] and i1[0] == it[g] and s1[0] == st[g]


def test_mnrfit_bad_input(gpu):
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    # separable: two classes either side of 0 in the first feature -- the iteration limit, finite coefficients
    rng = np.random.default_rng(5)
    X = rng.standard_normal((60, 2)).astype(np.float32)
    X[:30, 0] = -np.abs(X[:30, 0]) - 0.5
    X[30:, 0] = np.abs(X[30:, 0]) + 0.5
    y = np.r_[np.ones(30, int), np.full(30, 2)]
    B, st, it, dv = _fit(X, y, [np.arange(1, 61)], 2)
    assert st[0] == vl.MNR_ITERLIMIT and it[0] == 100 and np.isfinite(B).all() and np.isfinite(dv).all()
    assert np.abs(B).max() > 10
    # a class absent from one fold's training rows (and only that fold) is flagged
    X, y = planted(60, 3, 3, seed=6)
    no3 = np.nonzero(y != 3)[0] + 1
    B, st, it, dv = _fit(X, y, [np.arange(1, 61), no3], 3)
    assert st[0] == vl.MNR_CONVERGED and st[1] == vl.MNR_BADINPUT and np.isnan(dv[1]) and (B[:, :, 1] == 0).all()
    # a label outside 1..k
    B, st, it, dv = _fit(X, np.where(y == 3, 4, y), [np.arange(1, 61)], 3)
    assert st[0] == vl.MNR_BADINPUT
    # D = (p + 1)(k - 1) > 64: XM_EINVAL before any launch
    X, y = planted(40, 8, 9, seed=7)       # 9 x 8 = 72
    dX, dy = _dev(X, y)
    with pytest.raises(_lib.XmError) as ei:
        vl.mnrfit(dX, dy, [np.arange(1, 41)], 9)
    assert ei.value.code == 1
    with pytest.raises(_lib.XmError):
        vl.mnrval(torch.zeros(1, 8, 9, dtype=torch.float64, device="cuda").permute(2, 1, 0), dX,
                  [np.arange(1, 41)])


# ------------------------------------------------------------------------------------------------ mnrval
def test_mnrval_probs_preds_confusion(gpu):
    import torch
    from mcncrossmodalemotions_amd import vl
    X, y = planted(300, 8, 6, seed=21)
    tr, va = folds(300, 4, 4)
    B, st, it, dv = _fit(X, y, tr, 6)
    # planted ties: fold 2 gets coefficients with equal columns 2 and 4 (classes 2 and 4 tie wherever they lead), fold
    # 3 all zeros (every class ties: class 1)
    B[:, 3, 2] = B[:, 1, 2]
    B[:, :, 3] = 0
    dB = torch.from_numpy(np.ascontiguousarray(B.transpose(2, 1, 0))).cuda().permute(2, 1, 0)
    dX, dy = _dev(X, y)
    probs, preds, conf = vl.mnrval(dB, dX, va, dy)
    conf = conf.cpu().numpy()
    for g, v in enumerate(va):
        P = np_mnrval(B[:, :, g], X[v - 1])
        got = probs[g].cpu().numpy()
        assert got.shape == (len(v), 6)
        assert np.abs(got - P).max() <= 1e-12
        cls = preds[g].cpu().numpy()
        # the first maximum of the kernel's own probabilities (the ties are exact there)
        assert np.array_equal(cls, got.argmax(1) + 1)
        assert np.array_equal(cls, P.argmax(1) + 1) or g == 2
        ref = np.zeros((6, 6), int)
        np.add.at(ref, (y[v - 1] - 1, cls - 1), 1)
        assert np.array_equal(conf[g], ref)
    assert (preds[3].cpu().numpy() == 1).all()
    c2 = preds[2].cpu().numpy()
    assert (c2 != 4).all() and (c2 == 2).any()
    # without labels: no counts
    _, preds2, conf2 = vl.mnrval(dB, dX, va)
    assert conf2 is None and all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(preds, preds2))


# ------------------------------------------------------------------------------------------------ entry points
def test_run_cross_val_planted_features(gpu, tmp_path):
    from scipy.io import loadmat
    from mcncrossmodalemotions_amd import batch, emo_benchmarks as eb
    n, k = 240, 6
    X, y = planted(n, 8, k, seed=31, scale=0.5)
    imdb = batch.SyntheticBenchmarkImdb(num_tracks=n, num_classes=k, seed=3)
    imdb.tracks["labels"] = y
    path = eb.cached_feats_path(str(tmp_path), "audio", "planted", "rml")
    eb.save_feats(path, imdb.tracks, [X[i:i + 1] for i in range(n)])
    mini, expDirs, valIdxSets = eb.run_cross_val(numFolds=5, targetDataset="rml", modality="audio",
                                                 modelName="planted", root=str(tmp_path))
    # no features were drawn: rng(0) -> randperm directly
    order = np.random.default_rng(0).permutation(n) + 1
    tr, va = eb.cross_val_folds(order, 5)
    assert all(np.array_equal(a, b) for a, b in zip(va, valIdxSets))
    assert np.array_equal(mini["fusedLogits"], X) and np.array_equal(mini["labels"], y)
    for f, (t, v) in enumerate(zip(tr, va)):
        coef = loadmat(os.path.join(expDirs[f], "mnr-params.mat"))["coefficients"]
        Bref = np_mnrfit(X[t - 1], y[t - 1], k)[0]
        assert coef.shape == (9, 5) and np.abs(coef - Bref).max() <= 1e-6 * np.abs(Bref).max()
        assert np.array_equal(np_mnrval(coef, X[v - 1]).argmax(1), np_mnrval(Bref, X[v - 1]).argmax(1))
    # emo_benchmarks on the same cache: the fold predictions are the restatement's
    res = eb.emo_benchmarks(modality="audio", datasets=["rml"], modelName="planted", figDir=str(tmp_path / "figs"),
                            root=str(tmp_path), verbose=False)["rml"]
    for f, v in enumerate(res["valIdxSets"]):
        coef = loadmat(os.path.join(res["expDirs"][f], "mnr-params.mat"))["coefficients"]
        assert np.array_equal(res["preds"][f], np_mnrval(coef, X[v - 1]).argmax(1) + 1)
    # a class absent from a training fold raises with the fold number
    y2 = y.copy()
    y2[y2 == 6] = 5
    y2[valIdxSets[0][0] - 1] = 6           # the only class-6 track validates in fold 1 -> fold 1 trains without it
    imdb.tracks["labels"] = y2
    path2 = eb.cached_feats_path(str(tmp_path), "audio", "absent", "rml")
    eb.save_feats(path2, imdb.tracks, [X[i:i + 1] for i in range(n)])
    with pytest.raises(ValueError, match="fold 1:"):
        eb.run_cross_val(numFolds=5, targetDataset="rml", modality="audio", modelName="absent", root=str(tmp_path))


def test_random_model_sanity_figure(gpu, tmp_path):
    """emo_benchmarks.m:21-24: a 'random' model scores about 1/6 on a 6-class set.  Asserted within 1/6 +- 0.05
    (~3.5 binomial sigma at 720 tracks); the fixed-seed run is reported, not tuned."""
    from mcncrossmodalemotions_amd import batch, emo_benchmarks as eb
    imdb = batch.SyntheticBenchmarkImdb(num_tracks=720, num_classes=6, seed=0)
    res = eb.emo_benchmarks(modality="audio", datasets=["rml"], modelName="random", figDir=str(tmp_path / "f"),
                            imdbs={"rml": imdb}, root=str(tmp_path), verbose=False)["rml"]
    print("random model on the 720-track stand-in: mean fold accuracy %.4f, std %.4f" % (res["mean"], res["std"]))
    assert abs(res["mean"] - 1 / 6) <= 0.05
    assert res["confSum"].sum() == 720 and len(res["foldAccs"]) == 10
    # the cache was written after drawing the logits from the rng(0) stream, column-major
    path = eb.cached_feats_path(str(tmp_path), "audio", "random", "rml")
    tracks, fl = eb.load_feats(path)
    r = np.random.default_rng(0)
    want = r.standard_normal(720 * 8).reshape((720, 8), order="F").astype(np.float32)
    assert np.array_equal(np.concatenate(fl, 0), want)
    order = r.permutation(720) + 1
    assert np.array_equal(np.concatenate(res["valIdxSets"]), order)
    with open(res["confPath"]) as f:
        js = json.load(f)
    assert js["labels"] == ["Anger", "Disgust", "Fear", "Happiness", "Sadness", "Surprise"]
    assert os.path.exists(os.path.join(str(tmp_path / "f"), "confmat", "rml-random.txt"))


def test_end_to_end_audio_student_and_cache(gpu, tmp_path):
    from mcncrossmodalemotions_amd import batch, emo_benchmarks as eb, zoo
    net = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=9)
    imdb = batch.SyntheticBenchmarkImdb(num_tracks=120, num_classes=6, seed=4, min_frames=100, max_frames=260)
    res = eb.emo_benchmarks(modality="audio", datasets=["enterface"], modelName="emovoxceleb-student",
                            figDir=str(tmp_path / "f"), net=net, imdbs={"enterface": imdb}, root=str(tmp_path),
                            verbose=False)["enterface"]
    assert res["confSum"].sum() == 120
    conf = res["confSum"]
    accs = []
    for f, v in enumerate(res["valIdxSets"]):
        lab = imdb.tracks["labels"][v - 1]
        accs.append((res["preds"][f] == lab).sum() / len(v))
    assert np.allclose(res["foldAccs"], accs)
    assert np.trace(conf) == sum(round(a * len(v)) for a, v in zip(accs, res["valIdxSets"]))
    # a second call reuses the cache: the network is not run again (a broken one would raise)
    path = eb.cached_feats_path(str(tmp_path), "audio", "emovoxceleb-student", "enterface")
    mtime = os.path.getmtime(path)

    class Broken:
        def __getattr__(self, name):
            raise AssertionError("the network was used although the features are cached")
    mini, expDirs, _ = eb.run_cross_val(targetDataset="enterface", modality="audio",
                                        modelName="emovoxceleb-student", net=Broken(), root=str(tmp_path))
    assert os.path.getmtime(path) == mtime and len(expDirs) == 10


def test_end_to_end_afew_branch(gpu, tmp_path):
    from mcncrossmodalemotions_amd import batch, emo_benchmarks as eb
    imdb = batch.SyntheticBenchmarkImdb(num_tracks=140, num_classes=7, seed=5, val_fraction=0.4)
    res = eb.emo_benchmarks(modality="audio", datasets=["afew"], modelName="random", figDir=str(tmp_path / "f"),
                            imdbs={"afew": imdb}, root=str(tmp_path), verbose=False)["afew"]
    v = res["valIdxSets"][0]
    assert np.array_equal(v, np.nonzero(imdb.tracks["set"] == 2)[0] + 1) and len(res["foldAccs"]) == 1
    raw = (res["preds"][0] == imdb.tracks["labels"][v - 1]).mean()
    assert res["adjustmentFactor"] == 381 / 383 and res["foldAccs"][0] == raw * 381 / 383
    assert res["std"] == 0 and res["confSum"].shape == (7, 7) and res["confSum"].sum() == len(v)
    assert res["labels"][-1] == "Neutral"


def test_visual_path_peak_aggregator(gpu, tmp_path):
    from mcncrossmodalemotions_amd import batch, emo_benchmarks as eb, external, vl, zoo
    import torch
    net = zoo.ferPlusZoo("resnet50-ferplus", seed=7, width_mult=0.125, blocks=(1, 1, 1, 1))
    net.getLayer("pool5").block.poolSize = [2, 2]
    imdb = batch.SyntheticBenchmarkImdb(num_tracks=36, num_classes=6, modality="visual", seed=6, min_faces=1,
                                        max_faces=4, face_size=64)
    mini, expDirs, valIdxSets = eb.run_cross_val(numFolds=3, aggregator="peak", targetDataset="rml",
                                                 modality="visual", modelName="reduced-teacher", imdb=imdb, net=net,
                                                 root=str(tmp_path))
    tracks, fl = eb.load_feats(eb.cached_feats_path(str(tmp_path), "visual", "reduced-teacher", "rml"))
    assert [f.shape[0] for f in fl] == list(imdb.frames)
    counts = np.array([f.shape[0] for f in fl])
    last = np.cumsum(counts)
    assert np.array_equal(mini["fusedLogits"], np_peak(np.concatenate(fl, 0), last - counts + 1, last).T)
    assert len(expDirs) == 3 and sum(len(v) for v in valIdxSets) == 36
    assert all(os.path.exists(os.path.join(e, "mnr-params.mat")) for e in expDirs)
