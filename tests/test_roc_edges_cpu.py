"""CPU: the cases of tests/test_gpu_roc_edges.py (tests/roc_cases.py) on the numpy restatement alone -- no library is
loaded.  A case stands in the GPU file because of a property of its input (every entry tied in three radix passes, an
area past 2^33, a set length on a tile or wave edge, a set that starts past the first trip of the set loop); this file
asserts that property, so a generator that drifts off its edge fails here, where it can be seen without a GPU."""
import numpy as np
import pytest

import roc_cases as rc
from test_student_stats_cpu import np_roc

TILE, SPAN, THREADS, HIST_MAX = rc.GEOMETRY


def labels(cls, rows, c):
    return np.where(cls[np.asarray(rows) - 1] == c + 1, 1, -1)


def mixed_ties(ref, lab, sc):
    s2, l2 = sc[ref["order"]], lab[ref["order"]]
    return int(np.sum((s2[1:] == s2[:-1]) & (l2[1:] != l2[:-1])))


def test_geometry_literals_are_consistent():
    assert TILE % SPAN == 0 and SPAN % 64 == 0 and TILE == THREADS * (SPAN // 64) and THREADS == 256
    assert 4 * HIST_MAX <= 64 * 1024          # one 32-bit LDS counter per class within a workgroup's 64 KiB


@pytest.mark.parametrize("b", [0, 1, 2, 3])
def test_one_byte_varies_ties_every_other_pass(b):
    n = 2 * TILE + 1
    scores, cls, sets = rc.one_byte_varies(b, n)
    sc = scores[:, 0]
    bits = sc.view(np.uint32)
    assert np.isfinite(sc).all() and len(np.unique(bits)) == 256 and len(np.unique(sc)) == 256
    for other in range(4):
        digits = np.unique((bits >> np.uint32(8 * other)) & np.uint32(255))
        assert len(digits) == (256 if other == b else 1), (b, other)
    lab = labels(cls, sets[0], 0)
    ref = np_roc(lab, sc)
    ties = mixed_ties(ref, lab, sc)
    print("byte %d: %d neighbouring tied pairs with different labels" % (b, ties))
    assert ties >= 1000
    assert len(sets) == 1 and np.array_equal(sets[0], np.arange(1, n + 1))


@pytest.mark.parametrize("positives,auc", [("first", 1.0), ("last", 0.0)])
def test_one_value_keeps_the_input_order(positives, auc):
    n = 2 * TILE + 1
    scores, cls, sets = rc.few_values(n, 1, positives)
    assert len(np.unique(scores)) == 1
    ref = np_roc(labels(cls, sets[0], 0), scores[:, 0])
    assert np.array_equal(ref["order"], np.arange(n)) and ref["auc_int"] == auc
    assert ref["p"] == n // 3 and ref["n"] == n - n // 3 and ref["S"] == (ref["p"] * ref["n"] if auc else 0)


def test_three_values_tie_across_tiles():
    n = 3 * TILE + 5
    scores, cls, sets = rc.few_values(n, 3)
    sc = scores[:, 0]
    assert len(np.unique(sc)) == 3 and min(np.bincount(np.unique(sc, return_inverse=True)[1])) > TILE // 4
    lab = labels(cls, sets[0], 0)
    ref = np_roc(lab, sc)
    assert mixed_ties(ref, lab, sc) >= 1000
    # every value occurs in every tile and every wave span of the input: the order of a run is decided across all of them
    for v in np.unique(sc):
        assert all((sc[a:a + SPAN] == v).any() for a in range(0, n - 5, SPAN))


def test_big_set_has_more_tiles_than_scan_threads_and_an_area_past_2_33():
    scores, cls, sets = rc.big_case()
    n = scores.shape[0]
    assert n == 257 * TILE + 1 == 526337 and -(-n // TILE) > THREADS and n % TILE == 1
    ref = np_roc(labels(cls, sets[0], 0), scores[:, 0])
    print("big set: n = %d, p = %d, S = %d" % (n, ref["p"], ref["S"]))
    assert ref["S"] >= 2 ** 33 and ref["tp"][-1] < 2 ** 31 and ref["retrieved"] == n
    # the positives are spread so that the tile prefix differs from tile to tile (a scan that drops a tile shows in tp)
    per_tile = np.add.reduceat((labels(cls, sets[0], 0)[ref["order"]] > 0).astype(np.int64), np.arange(0, n, TILE))
    assert (per_tile[:-1] > 0).all()


def test_lattice_lengths_sit_on_every_tile_and_wave_edge():
    lengths = rc.lattice_lengths()
    for want in (TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, SPAN - 1, SPAN, SPAN + 1):
        assert want in lengths
    # the figures of the GPU file's table: 15,873 entries, Tc = floor(nnz / tile) + G = 15 blocks per column for 12 tiles
    assert sum(lengths) == 15873 and sum(lengths) // TILE + len(lengths) == 15 and sum(-(-m // TILE) for m in lengths) == 12
    scores, cls, sets = rc.lattice_case(lengths)
    assert [len(s) for s in sets] == lengths and scores.shape == (sum(lengths), 2)
    assert np.array_equal(scores[:, 1], -scores[:, 0])
    allrows = np.concatenate(sets)
    assert len(np.unique(allrows)) == len(allrows) and allrows.min() == 1 and allrows.max() == scores.shape[0]
    for rows in sets:
        for c in range(2):
            sc, lab = scores[rows - 1, c], labels(cls, rows, c)
            ref = np_roc(lab, sc)
            assert 0 < ref["retrieved"] < len(rows) and ref["p"] > 0 and ref["n"] > 0
            assert mixed_ties(ref, lab, sc) >= 10
            assert (sc == 0).any() and np.signbit(sc[sc == 0]).any() and not np.signbit(sc[sc == 0]).all()
            assert np.isposinf(sc).any() and ((sc != 0) & (np.abs(sc) < 1e-38)).any()
    # the second call: exact multiples of the tile, so floor(nnz / tile) + G over-counts the tiles by G
    mult = rc.multiple_lengths()
    assert all(m % TILE == 0 and m > 0 for m in mult)
    assert sum(mult) // TILE + len(mult) - sum(-(-m // TILE) for m in mult) == len(mult)


@pytest.mark.parametrize("G", [257, 513])
def test_many_sets_pass_the_first_trip_of_the_set_loop(G):
    scores, cls, sets = rc.many_sets_case(G)
    assert len(sets) == G > THREADS and -(-G // THREADS) > 1 and scores.shape[1] == 3
    lens = np.array([len(s) for s in sets])
    assert np.array_equal(lens == 0, np.arange(G) % 5 == 4) and lens.max() == 3 and set(lens) == {0, 1, 2, 3}
    assert lens[THREADS:].sum() > 0 and sum(lens) == scores.shape[0] < 10000


def test_empty_set_cases():
    scores, cls, sets = rc.empties_case()
    lens = [len(s) for s in sets]
    assert lens[:2] == [0, 0] and lens[-2:] == [0, 0] and lens[4:7] == [0, 0, 0] and lens.count(300) == 3
    r = np_roc([], [])
    assert (r["p"], r["n"], r["retrieved"], r["S"], r["auc_int"]) == (0, 0, 0, 0, 0.0)
    scores, cls, sets = rc.only_empties_case()
    assert len(sets) == 3 and sum(len(s) for s in sets) == 0 and scores.shape[0] >= 1


@pytest.mark.parametrize("E", rc.HIST_E)
def test_label_hist_reference_and_inputs(E):
    assert rc.HIST_E == [1, 8, 257, HIST_MAX] and rc.HIST_N == [1, 255, 256, 257, 1000]
    for N in rc.HIST_N:
        x = rc.hist_input(N, E)
        finite = np.nan_to_num(x, nan=0.25, neginf=-7.0)
        assert np.array_equal(rc.first_max_labels(finite), finite.argmax(1)), (N, E)     # argmax: the first maximum
        lab = rc.first_max_labels(x)
        assert np.array_equal(rc.label_hist_ref(x), np.bincount(lab, minlength=E)) and rc.label_hist_ref(x).sum() == N
        if N >= 8:
            assert np.isnan(x[2]).all() and np.isnan(x[N - 1]).all() and np.isneginf(x[5]).all()
            assert lab[2] == lab[N - 1] == lab[5] == lab[N // 2] == 0
        if N >= 255 and E >= 8:
            srt = np.sort(np.where(np.isnan(x), -np.inf, x), 1)
            tied = srt[:, -1] == srt[:, -2]
            assert tied.mean() > 0.1                                           # a last-maximum rule lands elsewhere
            assert np.isnan(x).mean() > 0.01 and np.isneginf(x).mean() > 0.01
            # a NaN stands before the winner in some row: a rule that lets NaN win, or stops at it, lands elsewhere
            before = np.isnan(x) & (np.arange(E)[None, :] < lab[:, None])
            assert before.any()
    # hand rows
    x = np.array([[np.nan, 1, 1], [-np.inf, -np.inf, -np.inf], [np.nan, np.nan, np.nan], [2, np.nan, 2], [-np.inf, np.nan, -3]],
                 np.float32)
    assert list(rc.first_max_labels(x)) == [1, 0, 0, 0, 2]
