"""CPU: the host side of emoVoxCeleb/student_stats.m and teacher_stats.m -- the ABI of xm_roc / xm_label_hist (declared,
typed, exported, arguments rejected without a device), meanAuc over the represented emotions, the AUC cache, the
partition map, the curve thinning -- and the numpy restatement of vlfeat's vl_roc that the GPU tests compare against."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ABI = ["xm_roc", "xm_label_hist"]


# ------------------------------------------------------------------------------------------------ numpy restatement
def np_roc(labels, scores):
    """vl_roc / vl_tpfp of vlfeat with default options, restated from its documentation.  labels in {-1, 0, +1},
    scores single.  Rows labelled 0 are dropped first.  Stable descending sort (argsort of the negated score:
    -0.0 == +0.0, ties keep their order, -Inf last), cumulative sums, rows scoring -Inf are never retrieved.
    Returns order (indices into the INPUT, the 0-labelled rows left out), tp (positives among the first i + 1 ranked
    rows, over all of them), p, n, retrieved, S (the integer area), auc_int = S / (p n) and auc_float (the
    floating trapezoid of the documentation)."""
    labels = np.asarray(labels).reshape(-1)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    kept = np.nonzero(labels != 0)[0]
    lab, sc = labels[kept], scores[kept]
    perm = np.argsort(-sc, kind="stable")
    pos = lab[perm] > 0
    tp = np.cumsum(pos).astype(np.int64)
    p, n = int((lab > 0).sum()), int((lab < 0).sum())
    retrieved = int((sc > -np.inf).sum())
    tpv = np.concatenate([[0], tp[:retrieved]]).astype(np.float64)
    fpv = np.arange(retrieved + 1, dtype=np.float64) - tpv
    tpr, fpr = tpv / max(p, 1e-10), fpv / max(n, 1e-10)
    auc_float = float(0.5 * np.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1])))
    S = int(tp[:retrieved][~pos[:retrieved]].sum())
    auc_int = float(S) / (float(p) * float(n)) if p and n else 0.0
    return {"order": kept[perm], "tp": tp, "p": p, "n": n, "retrieved": retrieved, "S": S, "auc_int": auc_int,
            "auc_float": auc_float, "tpr": tpr, "tnr": 1.0 - fpr}


def softmax32(x):
    x = x.astype(np.float32)
    e = np.exp(x - x.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (65, 2), (4505, 3), (30496, 4)])
def test_integer_area_equals_the_floating_trapezoid(n, seed):
    rng = np.random.default_rng(seed)
    sc = softmax32(rng.standard_normal((n, 8)) * 3)
    sc[rng.random((n, 8)) < 0.05] = np.float32(0.25)          # planted ties
    cls = rng.integers(1, 9, n)
    for c in range(8):
        r = np_roc(np.where(cls == c + 1, 1, -1), sc[:, c])
        assert abs(r["auc_int"] - r["auc_float"]) <= 1e-15, (c, r["auc_int"], r["auc_float"])
        assert r["p"] + r["n"] == n and r["retrieved"] == n
        # the rank-sum form: S counts (positive, negative) pairs with the positive ranked first
        assert 0 <= r["S"] <= r["p"] * r["n"]


def test_restatement_on_hand_cases():
    # perfect separation, its negation, all tied (positives first / last), -Inf never retrieved, 0 labels ignored
    lab = np.array([1, 1, -1, -1, -1])
    assert np_roc(lab, [5, 4, 3, 2, 1])["auc_int"] == 1.0 and np_roc(lab, [-5, -4, -3, -2, -1])["auc_int"] == 0.0
    assert np_roc(lab, np.zeros(5))["auc_int"] == 1.0 and np_roc(lab[::-1], np.zeros(5))["auc_int"] == 0.0
    r = np_roc([1, -1, 1, -1], [0.9, -np.inf, 0.1, 0.5])
    assert (r["p"], r["n"], r["retrieved"], r["S"]) == (2, 2, 3, 1) and r["auc_int"] == 0.25
    assert list(r["order"]) == [0, 3, 2, 1] and list(r["tp"]) == [1, 1, 2, 2]
    r = np_roc([1, 0, -1, 0, 1], [0.5, 9.0, 0.4, -9.0, 0.3])
    assert (r["p"], r["n"], r["S"]) == (2, 1, 1) and list(r["order"]) == [0, 2, 4] and r["auc_int"] == 0.5
    r = np_roc([1, -1], [-0.0, 0.0])                           # equal: the listed order stays
    assert list(r["order"]) == [0, 1] and r["auc_int"] == 1.0
    assert np_roc([1, 1], [1, 2])["auc_int"] == 0.0 and np_roc([], [])["auc_int"] == 0.0


# ------------------------------------------------------------------------------------------------ ABI
def test_roc_abi_declared_typed_and_exported():
    from mcncrossmodalemotions_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    L = _lib.load()
    assert L.xm_version() >= 109
    for name in NEW_ABI:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name]
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
    assert re.search(r"XM_ROC_OK = 0, XM_ROC_NAN = 1, XM_ROC_BADINPUT = 2", hdr)
    assert L.xm_roc_launches() > 0


def test_roc_geometry_is_host_only_and_matches_the_case_table():
    """xm_roc_geometry (ABI 126): declared, typed, exported, NULL pointers skipped; its numbers are the literals the edge
    cases of tests/roc_cases.py stand on, and the class limit is the one xm_label_hist enforces"""
    import roc_cases
    from mcncrossmodalemotions_amd import _lib, vl
    hdr = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    L = _lib.load()
    assert L.xm_version() >= 126 and "126 = + xm_roc_geometry" in hdr
    proto = re.search(r"\bint xm_roc_geometry\(([^;]*)\);", hdr).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["xm_roc_geometry"]) == 4
    assert L.xm_roc_geometry.argtypes == _lib.SIGNATURES["xm_roc_geometry"]
    assert L.xm_roc_geometry(None, None, None, None) == 0
    tile, span, threads, classes = vl.roc_geometry()
    assert (tile, span, threads, classes) == roc_cases.GEOMETRY
    assert tile == threads * (span // 64) and tile % span == 0
    assert L.xm_label_hist(None, 0, classes, 0, None, None) == 0
    assert L.xm_label_hist(None, 0, classes + 1, 0, None, None) == 5 and b"more than %d classes" % classes in L.xm_last_error()


def test_roc_arguments_are_rejected_without_a_device():
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    one = C.c_void_p(16)     # never dereferenced: every call below fails its checks first
    args = lambda **k: [k.get("scores", one), k.get("n", 10), k.get("E", 8), k.get("cls", one), k.get("offsets", one),
                        k.get("rows", one), k.get("nnz", 4), k.get("G", 1), k.get("auc", one), k.get("area", one),
                        k.get("counts", one), k.get("status", one), k.get("perm", None), k.get("tp", None), None]
    for bad, msg in [(dict(E=0), b"E >= 1"), (dict(G=-1), b"G >= 0"), (dict(n=0), b"n >= 1"), (dict(nnz=-1), b"nnz >= 0"),
                     (dict(scores=None), b"NULL"), (dict(cls=None), b"NULL"), (dict(offsets=None), b"NULL"),
                     (dict(rows=None), b"NULL"), (dict(auc=None), b"NULL"), (dict(area=None), b"NULL"),
                     (dict(counts=None), b"NULL"), (dict(status=None), b"NULL"), (dict(perm=one), b"both or neither")]:
        assert L.xm_roc(*args(**bad)) == 1 and msg in L.xm_last_error(), bad
    assert L.xm_roc(*args(nnz=2 ** 29, E=8)) == 5 and b"2^31" in L.xm_last_error()      # XM_ENOTSUP
    assert L.xm_roc(*args(G=0)) == 0                                                       # nothing to do
    assert L.xm_label_hist(one, 10, 0, 0, one, None) == 1 and b"E >= 1" in L.xm_last_error()
    assert L.xm_label_hist(one, -1, 8, 0, one, None) == 1
    assert L.xm_label_hist(None, 10, 8, 0, one, None) == 1 and b"NULL" in L.xm_last_error()
    assert L.xm_label_hist(one, 10, 5000, 0, one, None) == 5
    assert L.xm_label_hist(None, 0, 8, 0, None, None) == 0


def test_host_wrappers_refuse_host_tensors_and_bad_rows():
    import torch
    from mcncrossmodalemotions_amd import vl
    sc = torch.zeros(8, 10).t()
    with pytest.raises(RuntimeError, match="not on the GPU"):
        vl.roc(sc, torch.ones(10, dtype=torch.int32), [np.arange(1, 11)])
    with pytest.raises(RuntimeError, match="not on the GPU"):
        vl.vl_roc(np.ones(10), torch.zeros(10))
    with pytest.raises(RuntimeError, match="not on the GPU"):
        vl.label_hist(sc)


# ------------------------------------------------------------------------------------------------ host arithmetic
def test_mean_auc_ignores_and_skips_unrepresented():
    from mcncrossmodalemotions_amd import student_stats as ss
    emo = ss.EMOTIONS
    assert emo == ["neutral", "happiness", "surprise", "sadness", "anger", "disgust", "fear", "contempt"]
    auc = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2])
    labels = np.array([1, 1, 2, 3, 4, 5, 6, 7, 8, 8])
    m, rep = ss.mean_auc(auc, labels, emo, ("fear", "contempt", "disgust"))
    assert list(rep) == [1, 2, 3, 4, 5] and m == pytest.approx(np.mean([0.9, 0.8, 0.7, 0.6, 0.5]))
    m, rep = ss.mean_auc(auc, np.array([2, 2, 5, 7]), emo, ("fear", "contempt", "disgust"))   # 1, 3, 4 unrepresented
    assert list(rep) == [2, 5] and m == pytest.approx(0.65)
    m, rep = ss.mean_auc(auc, labels, emo, ())
    assert list(rep) == list(range(1, 9)) and m == pytest.approx(auc.mean())
    m, rep = ss.mean_auc(auc, np.array([7]), emo, ("fear",))
    assert rep.size == 0 and np.isnan(m)


def test_cache_keeps_an_existing_partition_row(tmp_path):
    from scipy.io import loadmat
    from mcncrossmodalemotions_amd import student_stats as ss
    path = str(tmp_path / "cache" / ss.CACHE_NAME)
    a, b = np.linspace(0.1, 0.8, 8), np.linspace(0.2, 0.9, 8)
    ss.update_cache(path, ss.EMOTIONS, "train", a)
    ss.update_cache(path, ss.EMOTIONS, "heardVal", b)
    ss.update_cache(path, ss.EMOTIONS, "train", b)            # :146-148: the row that is there stays
    m = loadmat(path)
    assert m["train"].shape == (1, 8) and np.array_equal(m["train"][0], a) and np.array_equal(m["heardVal"][0], b)
    assert [str(e[0]) for e in m["emotions"].reshape(-1)] == ss.EMOTIONS and "unheardVal" not in m


def test_partition_map():
    from mcncrossmodalemotions_amd import batch, student_stats as ss
    assert ss.PARTITIONS == {"train": 1, "unheardVal": 2, "heardVal": 3}
    assert ss.partition_list("all") == ["train", "unheardVal", "heardVal"] and ss.partition_list("heardVal") == ["heardVal"]
    with pytest.raises(ValueError, match="unknown partition"):
        ss.partition_list("unheardTest")
    # the synthetic imdb: the new keyword adds set 3 and leaves everything drawn before it as it was
    a = batch.SyntheticEmoVoxImdb(num_tracks=40, seed=5, val_fraction=0.25)
    b = batch.SyntheticEmoVoxImdb(num_tracks=40, seed=5, val_fraction=0.25, heard_fraction=0.1)
    assert set(a.set) == {1, 2} and np.array_equal(np.bincount(b.set)[1:], [26, 10, 4])
    assert np.array_equal(a.set == 2, b.set == 2) and np.array_equal(a.num_samples, b.num_samples)
    assert all(np.array_equal(x, y) for x, y in zip(a.wavLogits, b.wavLogits))


@pytest.mark.parametrize("retrieved", [0, 1, 5, 257, 258, 259, 4505, 118485])
def test_curve_thinning_keeps_the_end_points_and_is_monotone(retrieved):
    from mcncrossmodalemotions_amd import student_stats as ss
    idx = ss.thin_curve(retrieved)
    assert idx[0] == 0 and idx[-1] == retrieved and np.all(np.diff(idx) > 0) and len(idx) <= ss.CURVE_POINTS + 2
    rng = np.random.default_rng(retrieved)
    lab = np.where(rng.random(retrieved + 3) < 0.3, 1, -1)
    sc = rng.standard_normal(retrieved + 3).astype(np.float32)
    sc[:3] = -np.inf
    r = np_roc(lab, sc)
    i2, tpr, tnr = ss.curve_points(r["tp"], r["p"], r["n"], r["retrieved"])
    assert np.array_equal(i2, idx) and np.array_equal(tpr, r["tpr"][idx]) and np.array_equal(tnr, r["tnr"][idx])
    assert np.all(np.diff(tpr) >= 0) and np.all(np.diff(tnr) <= 0) and tpr[0] == 0 and tnr[0] == 1
