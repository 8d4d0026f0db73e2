"""GPU: xm_roc (vlfeat's vl_roc for G x E problems per call) and xm_label_hist against the numpy restatement of
test_student_stats_cpu.py, on the same score bits: integers (area, p, n, retrieved, the ranking, the cumulative
positives) equal exactly, the AUC equals S / (p n) bit for bit."""
import numpy as np
import pytest

from test_student_stats_cpu import np_roc

pytestmark = pytest.mark.gpu


def run(gpu, scores, cls, sets, want_curve=True):
    import torch
    from mcncrossmodalemotions_amd import vl
    d = scores if isinstance(scores, torch.Tensor) else vl.from_numpy(np.asfortranarray(scores), gpu)
    r = vl.roc(d, torch.from_numpy(np.asarray(cls, np.int32)).to(gpu), sets, want_curve=want_curve)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def check(scores, cls, sets, out):
    """every problem of the call against the restatement; returns the number of tied pairs with different labels"""
    from mcncrossmodalemotions_amd import vl
    E = scores.shape[1]
    offs = out["offsets"]
    mixed_ties = 0
    for g, rows in enumerate(sets):
        rows = np.asarray(rows, np.int64)
        for c in range(E):
            sc = scores[rows - 1, c]
            lab = np.where(cls[rows - 1] == c + 1, 1, -1)
            where = "set %d emotion %d" % (g, c + 1)
            if np.isnan(sc).any():
                assert out["status"][g, c] == vl.ROC_NAN and np.isnan(out["auc"][g, c]), where
                continue
            ref = np_roc(lab, sc)
            assert out["status"][g, c] == vl.ROC_OK, where
            assert (out["p"][g, c], out["n"][g, c], out["retrieved"][g, c]) == (ref["p"], ref["n"], ref["retrieved"]), where
            assert out["area"][g, c] == ref["S"], where
            assert bits(out["auc"][g, c]) == bits(ref["auc_int"]), (where, out["auc"][g, c], ref["auc_int"])
            assert abs(ref["auc_float"] - ref["auc_int"]) <= 1e-15, where
            if "perm" in out:
                sl = slice(int(offs[g]), int(offs[g + 1]))
                assert np.array_equal(out["perm"][c, sl], rows[ref["order"]]), where
                assert np.array_equal(out["tp"][c, sl], ref["tp"]), where
            s2, l2 = sc[ref["order"]], lab[ref["order"]]
            mixed_ties += int(np.sum((s2[1:] == s2[:-1]) & (l2[1:] != l2[:-1])))
    return mixed_ties


def device_softmax(gpu, logits):
    """fp32 softmax over dim 2 on the device, downloaded: the restatement sees the bits the kernel sees"""
    from mcncrossmodalemotions_amd import vl
    d = vl.vl_nnsoftmaxt(vl.from_numpy(np.asfortranarray(logits.astype(np.float32)), gpu), dim=2)
    return d, vl.to_numpy(d)


def test_softmax_scores_with_natural_ties(gpu):
    rng = np.random.default_rng(7)
    n = 60000
    logits = (rng.standard_normal((n, 8)) * 3).astype(np.float32)
    d, sc = device_softmax(gpu, logits)
    cls = np.where(rng.random(n) < 0.3, rng.integers(1, 9, n), logits.argmax(1) + 1)
    sets = [np.arange(1, n + 1), rng.permutation(n)[:20000] + 1]
    out = run(gpu, d, cls, sets)
    ties = check(sc, cls, sets, out)
    print("tied neighbouring pairs with different labels: %d" % ties)
    assert ties >= 1          # stability is exercised: saturated softmax outputs tie across labels


def edge_cases():
    """(name, labels +1/-1, scores, expected AUC or None)"""
    rng = np.random.default_rng(11)
    m = 300
    lab_pf = np.r_[np.ones(100), -np.ones(200)].astype(int)
    sep = np.r_[rng.random(100) + 2, rng.random(200)].astype(np.float32)
    mixed_lab = np.where(rng.random(m) < 0.4, 1, -1)
    zeros = np.where(rng.random(m) < 0.5, np.float32(0.0), np.float32(-0.0))
    zeros[::7] = rng.standard_normal(len(zeros[::7])).astype(np.float32) * np.float32(1e-3)
    inf = rng.standard_normal(m).astype(np.float32)
    inf[rng.random(m) < 0.2] = -np.inf
    inf[5] = np.inf
    den = (rng.standard_normal(m) * 1e-41).astype(np.float32)          # denormals of both signs, some flushed to +-0
    neg = -np.abs(rng.standard_normal(m)).astype(np.float32) * 1e3
    return [("all tied, positives first", lab_pf, np.full(m, 0.5, np.float32), 1.0),
            ("all tied, positives last", lab_pf[::-1].copy(), np.full(m, 0.5, np.float32), 0.0),
            ("separated", lab_pf, sep, 1.0), ("separated, negated", lab_pf, -sep, 0.0),
            ("signed zeros", mixed_lab, zeros, None), ("some -Inf", mixed_lab, inf, None),
            ("denormal", mixed_lab, den, None), ("negative", mixed_lab, neg, None),
            ("no positive", -np.ones(m, int), inf, 0.0), ("no negative", np.ones(m, int), neg, 0.0),
            ("empty", np.zeros(0, int), np.zeros(0, np.float32), 0.0),
            ("one row", np.ones(1, int), np.ones(1, np.float32), 0.0)]


def test_edge_cases_in_one_call(gpu):
    cases = edge_cases()
    # each case is a set of its own over one column; cls 1 = positive, 2 = negative; column 2 holds the negated scores
    sc = np.concatenate([c[2] for c in cases]).astype(np.float32)
    scores = np.stack([sc, -sc], 1)
    cls = np.concatenate([np.where(c[1] > 0, 1, 2) for c in cases])
    ends = np.cumsum([len(c[1]) for c in cases])
    sets = [np.arange(e - len(c[1]) + 1, e + 1) for c, e in zip(cases, ends)]
    out = run(gpu, scores, cls, sets)
    check(scores, cls, sets, out)
    for g, (name, _, _, want) in enumerate(cases):
        if want is not None:
            assert out["auc"][g, 0] == want, name
    g = [c[0] for c in cases].index("empty")
    assert (out["p"][g, 0], out["n"][g, 0], out["retrieved"][g, 0], out["status"][g, 0]) == (0, 0, 0, 0)
    g = [c[0] for c in cases].index("some -Inf")
    assert out["retrieved"][g, 0] < len(cases[g][1]) and out["retrieved"][g, 1] < len(cases[g][1])


def test_nan_flags_its_problem_only(gpu):
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(3)
    n = 5000
    scores = rng.standard_normal((n, 4)).astype(np.float32)
    cls = rng.integers(1, 5, n)
    scores[1234, 2] = np.nan
    sets = [np.arange(1, 2001), np.arange(1001, n + 1), np.arange(1, 1001)]
    out = run(gpu, scores, cls, sets)
    check(scores, cls, sets, out)
    want = np.zeros((3, 4), int)
    want[0, 2] = want[1, 2] = vl.ROC_NAN
    assert np.array_equal(out["status"], want)


def partition_problem(seed, sizes, n=None):
    rng = np.random.default_rng(seed)
    n = n or int(sum(sizes))
    logits = (rng.standard_normal((n, 8)) * 3).astype(np.float32)
    cls = np.where(rng.random(n) < 0.5, rng.integers(1, 9, n), logits.argmax(1) + 1)
    order = rng.permutation(n) + 1
    ends = np.cumsum(sizes)
    sets = [order[e - s:e] for s, e in zip(sizes, ends)]
    return logits, cls, sets


@pytest.mark.parametrize("sizes", [(118485, 30496, 4505), (1, 63, 64, 65, 4505, 30496, 118485)])
def test_reference_partition_sizes(gpu, sizes):
    logits, cls, sets = partition_problem(5, sizes)
    d, sc = device_softmax(gpu, logits)
    out = run(gpu, d, cls, sets)
    check(sc, cls, sets, out)
    nocurve = run(gpu, d, cls, sets, want_curve=False)
    for k in ("auc", "area", "p", "n", "retrieved", "status"):
        assert nocurve[k].tobytes() == out[k].tobytes(), k


def test_independent_of_G_order_and_run(gpu):
    logits, cls, sets = partition_problem(9, (70001, 30496, 4505))
    d, _ = device_softmax(gpu, logits)
    keys = ("auc", "area", "p", "n", "retrieved", "status")
    a = run(gpu, d, cls, sets)
    b = run(gpu, d, cls, sets)
    for k in keys + ("perm", "tp"):
        assert a[k].tobytes() == b[k].tobytes(), k                       # two runs
    for g in range(3):
        one = run(gpu, d, cls, [sets[g]])
        sl = slice(int(a["offsets"][g]), int(a["offsets"][g + 1]))
        for k in keys:
            assert one[k][0].tobytes() == a[k][g].tobytes(), (g, k)      # G = 1 against G = 3
        assert one["perm"].tobytes() == np.ascontiguousarray(a["perm"][:, sl]).tobytes()
        assert one["tp"].tobytes() == np.ascontiguousarray(a["tp"][:, sl]).tobytes()
    order = [2, 0, 1]
    c = run(gpu, d, cls, [sets[g] for g in order])
    for i, g in enumerate(order):
        for k in keys:
            assert c[k][i].tobytes() == a[k][g].tobytes(), (g, k)        # the sets in another order
        sa = slice(int(a["offsets"][g]), int(a["offsets"][g + 1]))
        sc_ = slice(int(c["offsets"][i]), int(c["offsets"][i + 1]))
        assert np.array_equal(c["perm"][:, sc_], a["perm"][:, sa]) and np.array_equal(c["tp"][:, sc_], a["tp"][:, sa])


def test_bad_rows_and_offsets_are_flagged_not_read(gpu):
    """the C entry takes device index arrays: a row outside 1..n flags its problem, offsets that do not ascend flag the
    call; vl.roc, which has the sets on the host, refuses them before the call"""
    import ctypes as C
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    n, E = 100, 2
    scores = vl.from_numpy(np.asfortranarray(np.random.default_rng(0).standard_normal((n, E)).astype(np.float32)), gpu)
    cls = torch.ones(n, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match="outside 1..100"):
        vl.roc(scores, cls, [np.array([1, 101])])
    L = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(offsets, rows, G):
        offs = torch.tensor(offsets, dtype=torch.int32, device=gpu)
        r = torch.tensor(rows, dtype=torch.int32, device=gpu)
        auc = torch.zeros(G, E, dtype=torch.float64, device=gpu)
        area = torch.zeros(G, E, dtype=torch.int64, device=gpu)
        cnt = torch.zeros(G, E, 3, dtype=torch.int32, device=gpu)
        st = torch.zeros(G, E, dtype=torch.int32, device=gpu)
        _lib.check(L.xm_roc(p(scores), n, E, p(cls), p(offs), p(r), len(rows), G, p(auc), p(area), p(cnt), p(st), None,
                            None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return auc.cpu().numpy(), st.cpu().numpy()

    auc, st = call([0, 3, 6], [1, 2, 3, 4, 0, 101], 2)
    assert np.array_equal(st, [[0, 0], [2, 2]]) and np.isnan(auc[1]).all() and not np.isnan(auc[0]).any()
    auc, st = call([0, 4, 2], [1, 2, 3, 4], 2)
    assert np.array_equal(st, [[2, 2], [2, 2]]) and np.isnan(auc).all()


def test_vl_roc_ignores_zero_labels(gpu):
    import torch
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(21)
    n = 7000
    lab = rng.choice([-1, 0, 1], n, p=[0.5, 0.2, 0.3])
    sc = np.round(rng.standard_normal(n), 2).astype(np.float32)      # rounded: ties
    sc[rng.random(n) < 0.01] = -np.inf
    tpr, tnr, info = vl.vl_roc(lab, torch.from_numpy(sc).to(gpu))
    ref = np_roc(lab, sc)
    assert (info["p"], info["n"]) == (ref["p"], ref["n"]) and bits(info["auc"]) == bits(ref["auc_int"])
    assert np.array_equal(tpr, ref["tpr"]) and np.array_equal(tnr, ref["tnr"]) and len(tpr) == ref["retrieved"] + 1
    assert abs(info["auc"] - ref["auc_float"]) <= 1e-15


def test_label_hist_at_the_reference_frame_count(gpu):
    import torch
    from mcncrossmodalemotions_amd import vl
    N, E = 5078961, 8
    g = torch.Generator(device=gpu)
    g.manual_seed(4)
    x = torch.randn(E, N, generator=g, device=gpu, dtype=torch.float32).t()          # N x E, column-major
    x = torch.round(x * 2) / 2                                                        # halves: most rows have tied maxima
    host = x.cpu().numpy()
    assert (np.sort(host, 1)[:, -1] == np.sort(host, 1)[:, -2]).mean() > 0.1
    want = np.bincount(host.argmax(1), minlength=E)                                   # argmax: the first maximum
    h = vl.label_hist(x)
    assert h.dtype == torch.int64 and np.array_equal(h.cpu().numpy(), want) and int(h.sum()) == N
    # the other layout (1 x 1 x E x N) and accumulation into given bins
    xt = vl.from_numpy(host[:100003].T.reshape(1, 1, E, -1), gpu)
    h2 = vl.label_hist(xt, dim=3, bins=h.clone())
    assert np.array_equal(h2.cpu().numpy(), want + np.bincount(host[:100003].argmax(1), minlength=E))
    lab = vl.to_numpy(vl.max_label(xt)).reshape(-1).astype(int)
    assert np.array_equal(np.bincount(lab - 1, minlength=E), np.bincount(host[:100003].argmax(1), minlength=E))
