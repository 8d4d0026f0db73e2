"""GPU: xm_roc and xm_label_hist (csrc/roc.hip) at the edges of their tiles, waves and grids.  tests/test_gpu_roc.py runs the
unit at the workload's sizes; the cases here stand on the kernels' own constants, which vl.roc_geometry() reports and the
`geometry` fixture holds against the literals of tests/roc_cases.py: tile = 2048 entries per workgroup, wave span = 512
consecutive entries per wave (4 waves), threads = 256, at most 4096 classes in xm_label_hist.  Every comparison is against
the numpy restatement of tests/test_student_stats_cpu.py (np_roc) or the first-maximum restatement of tests/roc_cases.py,
on the same score bits, and every one is exact: integers, the ranking, and the AUC bit for bit.  No tolerance appears in
this file.  tests/test_roc_edges_cpu.py asserts, without a GPU, the property of each input that makes it a case (ties,
area, lengths); the derived quantities below are recomputed from the launch code of csrc/roc.hip.

Kernel / branch -> the case that reaches it, and through which condition:
  roc_setup_kernel, chunk > 1, part[] prefix       test_many_sets G = 257: chunk = ceil(257 / 256) = 2, threads 0 .. 127 number two
                                                   sets each and thread 128 one; G = 513: chunk = 3, threads 0 .. 170.  Every
                                                   thread past 0 starts from part[tid] != 0 (4 of 5 sets are one tile); G = 300
                                                   in the bad-row call: chunk = 2
  roc_scanpos_kernel, chunk > 1                    test_more_tiles_than_scan_threads: 257 * 2048 + 1 = 526,337 rows = 258 tiles >
                                                   256: chunk = 2, thread t scans tiles 2 t, 2 t + 1, thread 128 the last two
                                                   (tile 257 holds one entry); every full tile holds positives, so tp shows it
  64-bit atomicAdd of S, high word                 the same set: S >= 2^33 (asserted on the device's area; tp[-1] < 2^31), so each
                                                   of the 258 * 4 wave sums lands in a total whose high word is 1 or more
  tile boundary, last tile of 1 entry, idle tail   test_tile_and_wave_lattice[lattice]: lengths 2047, 2048, 2049 (second tile of
                                                   one entry), 4096, 4097 (third tile of one entry); Tc = 15,873 / 2048 + 8 = 15
                                                   blocks per column for 12 tiles: 3 idle.  [multiples]: lengths 2048, 4096,
                                                   2048: Tc = 4 + 3 = 7 for 4 tiles, G = 3 idle blocks that return from roc_locate
  roc_scatter / roc_curve, wave hand-over          [lattice]: lengths 511 (lane 63 of wave 0's last round is invalid), 512 (wave 0
                                                   full, waves 1 .. 3 empty), 513 (wave 1 owns one entry: cnt[1][d] and wtot[0]
                                                   carry wave 0's 512); the full tiles run all four waves
  stability across tiles and waves, all tied       test_each_radix_pass_alone[b], 4097 rows = 3 tiles: one digit value in the
                                                   three other passes (b = 3: two, the sign's), 256 in pass b, about 1800 tied
                                                   neighbours with different labels: the hist offsets alone order the rest.
                                                   test_one_value_keeps_the_input_order: one key, 3 tiles, perm must be the
                                                   identity and the AUC exactly 1 / 0; test_three_values: 6149 rows = 4 tiles
  roc_locate over runs of equal tile_start         test_empty_sets_around_full_ones: tile_start = 0 0 0 1 2 2 2 2 3 3 3 (two leading,
                                                   three in the middle, two trailing empties); test_only_empty_sets: nnz = 0, no
                                                   sort scratch (M = 0), tile_start all 0, Tc = 3 blocks per column, all idle
  offsets check, g strided over the threads        test_bad_offsets_past_the_first_trip: G = 300, the only descent is at
                                                   g = 299 = 256 + 43: thread 43's second trip of `for g = tid; g < G; g += 256`
  label_hist_kernel                                test_label_hist[E-N]: E = 257: second trip of `for c = threadIdx.x; c < E;
                                                   c += 256` (clear and write-back); E = 4096: 16 trips and 16 KiB of dynamic
                                                   LDS, the limit; E = 4097 refused; N = 1, 255, 256 (one block, partial / full),
                                                   257 (second block of one sample), 1000 (4 blocks); halves: ties of the maximum;
                                                   NaN before the winner, rows of NaN only and of -Inf only -> class 1"""
import ctypes as C

import numpy as np
import pytest

import roc_cases as rc
from test_gpu_roc import bits, check, run
from test_student_stats_cpu import np_roc

pytestmark = pytest.mark.gpu

SCALARS = ("auc", "area", "p", "n", "retrieved", "status")


@pytest.fixture(scope="module", autouse=True)
def geometry(gpu):
    from mcncrossmodalemotions_amd import vl
    assert vl.roc_geometry() == rc.GEOMETRY, "tests/roc_cases.py restates other constants than csrc/roc.hip has"
    assert _launches() == 18
    return rc.GEOMETRY


def _launches():
    from mcncrossmodalemotions_amd import _lib
    return _lib.load().xm_roc_launches()


def same_scalars(a, b, where=""):
    for k in SCALARS:
        assert a[k].tobytes() == b[k].tobytes(), (where, k)


# ------------------------------------------------------------------------------------------------ tile and wave lattice
@pytest.mark.parametrize("which", ["lattice", "multiples"])
def test_tile_and_wave_lattice(gpu, which):
    lengths = rc.lattice_lengths() if which == "lattice" else rc.multiple_lengths()
    scores, cls, sets = rc.lattice_case(lengths)
    out = run(gpu, scores, cls, sets, want_curve=True)
    assert list(np.diff(out["offsets"])) == lengths
    ties = check(scores, cls, sets, out)
    print("%s: %d tied neighbouring pairs with different labels" % (which, ties))
    nocurve = run(gpu, scores, cls, sets, want_curve=False)
    assert "perm" not in nocurve
    same_scalars(nocurve, out, which)


# ------------------------------------------------------------------------------------------------ each radix pass alone
@pytest.mark.parametrize("b", [0, 1, 2, 3])
def test_each_radix_pass_alone(gpu, b):
    scores, cls, sets = rc.one_byte_varies(b, 2 * rc.TILE + 1)
    out = run(gpu, scores, cls, sets)
    ties = check(scores, cls, sets, out)                    # perm == the stable order of np_roc, tp, S, the AUC's bits
    print("byte %d: %d tied neighbouring pairs with different labels" % (b, ties))
    assert ties >= 1000


@pytest.mark.parametrize("positives,auc", [("first", 1.0), ("last", 0.0)])
def test_one_value_keeps_the_input_order(gpu, positives, auc):
    n = 2 * rc.TILE + 1
    scores, cls, sets = rc.few_values(n, 1, positives)
    out = run(gpu, scores, cls, sets)
    check(scores, cls, sets, out)
    assert np.array_equal(out["perm"][0], np.arange(1, n + 1))
    assert bits(out["auc"][0, 0]) == bits(auc)
    assert out["area"][0, 0] == (out["p"][0, 0].astype(np.int64) * out["n"][0, 0] if auc else 0)


def test_three_values(gpu):
    scores, cls, sets = rc.few_values(3 * rc.TILE + 5, 3)
    out = run(gpu, scores, cls, sets)
    assert check(scores, cls, sets, out) >= 1000


# ------------------------------------------------------------------------------------------------ many sets
@pytest.mark.parametrize("G", [257, 513])
def test_many_sets(gpu, G):
    scores, cls, sets = rc.many_sets_case(G)
    assert len(sets) == G
    out = run(gpu, scores, cls, sets)
    check(scores, cls, sets, out)
    for g in range(4, G, 5):                                # the empty sets
        for k in ("p", "n", "retrieved", "area", "status"):
            assert not out[k][g].any(), (g, k)
        assert bits(out["auc"][g]).tolist() == [0, 0, 0], g
    # the same bits from a call of the set alone: G-independence past the 256-set boundary
    for g in [0, 128, 255, 256, G - 1 if G > 257 else 253]:
        assert len(sets[g]) > 0
        one = run(gpu, scores, cls, [sets[g]])
        sl = slice(int(out["offsets"][g]), int(out["offsets"][g + 1]))
        for k in SCALARS:
            assert one[k][0].tobytes() == out[k][g].tobytes(), (g, k)
        assert one["perm"].tobytes() == np.ascontiguousarray(out["perm"][:, sl]).tobytes(), g
        assert one["tp"].tobytes() == np.ascontiguousarray(out["tp"][:, sl]).tobytes(), g


# ------------------------------------------------------------------------------------------------ empty sets
def test_empty_sets_around_full_ones(gpu):
    scores, cls, sets = rc.empties_case()
    out = run(gpu, scores, cls, sets)
    check(scores, cls, sets, out)                           # the neighbours, and the empties through np_roc([], [])
    for g, rows in enumerate(sets):
        if len(rows) == 0:
            for k in ("p", "n", "retrieved", "area", "status"):
                assert not out[k][g].any(), (g, k)
            assert bits(out["auc"][g]).tolist() == [0, 0], g            # +0.0, not -0.0 and not NaN
    nocurve = run(gpu, scores, cls, sets, want_curve=False)
    same_scalars(nocurve, out)


@pytest.mark.parametrize("want_curve", [True, False])
def test_only_empty_sets(gpu, want_curve):
    scores, cls, sets = rc.only_empties_case()
    out = run(gpu, scores, cls, sets, want_curve=want_curve)
    for k in SCALARS:
        assert out[k].shape == (3, 2) and not np.ascontiguousarray(out[k]).view(np.uint8).any(), k   # AUC +0.0, status OK
    assert list(out["offsets"]) == [0, 0, 0, 0]
    if want_curve:
        assert out["perm"].shape == (2, 0) and out["tp"].shape == (2, 0)


# ------------------------------------------------------------------------------------------------ more than 256 tiles in one set
def test_more_tiles_than_scan_threads(gpu):
    scores, cls, sets = rc.big_case()
    assert scores.shape[0] == (rc.THREADS + 1) * rc.TILE + 1
    out = run(gpu, scores, cls, sets)
    print("S = %d, p = %d, n = %d" % (out["area"][0, 0], out["p"][0, 0], out["n"][0, 0]))
    ref = np_roc(np.where(cls == 1, 1, -1), scores[:, 0])
    first_bad = np.nonzero(out["tp"][0] != ref["tp"])[0][:1]
    assert first_bad.size == 0, "tp differs from rank %d (tile %d) on" % (first_bad[0], first_bad[0] // rc.TILE)
    assert np.array_equal(out["perm"][0], ref["order"] + 1)
    assert out["area"][0, 0] >= 2 ** 33 and out["area"][0, 0] == ref["S"]
    check(scores, cls, sets, out)                           # the counts, the status and the AUC's bits as well


# ------------------------------------------------------------------------------------------------ bad offsets / rows, raw entry
def raw_roc(gpu, scores, cls, offsets, rows, nnz):
    """xm_roc itself on device index arrays that vl.roc would refuse; outputs start from a sentinel: all are overwritten"""
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    n, E = scores.shape
    G = len(offsets) - 1
    d = vl.from_numpy(np.asfortranarray(scores), gpu)
    p = lambda t: C.c_void_p(t.data_ptr())
    lab = torch.from_numpy(np.asarray(cls, np.int32)).to(gpu)
    offs = torch.from_numpy(np.asarray(offsets, np.int32)).to(gpu)
    r = torch.from_numpy(np.asarray(rows, np.int32)).to(gpu)
    auc = torch.full((G, E), 7.25, dtype=torch.float64, device=gpu)
    area = torch.full((G, E), -5, dtype=torch.int64, device=gpu)
    cnt = torch.full((G, E, 3), -5, dtype=torch.int32, device=gpu)
    st = torch.full((G, E), -5, dtype=torch.int32, device=gpu)
    _lib.check(_lib.load().xm_roc(p(d), n, E, p(lab), p(offs), p(r), nnz, G, p(auc), p(area), p(cnt), p(st), None, None,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy()
    return {"auc": auc.cpu().numpy(), "area": area.cpu().numpy(), "p": cnt[:, :, 0], "n": cnt[:, :, 1],
            "retrieved": cnt[:, :, 2], "status": st.cpu().numpy(), "offsets": np.asarray(offsets)}


def test_bad_offsets_past_the_first_trip(gpu):
    from mcncrossmodalemotions_amd import vl
    G = 300
    scores, cls, sets = rc.many_sets_case(G)
    n = scores.shape[0]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    rows = np.concatenate(sets)
    # every offset valid and ascending but the last: offsets[299] > offsets[300] (set 299 is empty, so the step down is by one)
    bad = offsets.copy()
    assert bad[G - 1] == bad[G] and bad[G - 1] >= 1
    bad[G] = bad[G - 1] - 1
    assert (np.diff(bad[:G]) >= 0).all() and bad.min() >= 0 and bad.max() <= len(rows) and G - 1 >= rc.THREADS
    out = raw_roc(gpu, scores, cls, bad, rows, len(rows))
    assert (out["status"] == vl.ROC_BADINPUT).all() and np.isnan(out["auc"]).all()
    # second call: the only defect is a row n + 1 in set 280; that set is flagged, every other problem is right
    g_bad = 280
    assert len(sets[g_bad]) > 0
    rows2 = rows.copy()
    rows2[offsets[g_bad]] = n + 1
    out = raw_roc(gpu, scores, cls, offsets, rows2, len(rows2))
    assert (out["status"][g_bad] == vl.ROC_BADINPUT).all() and np.isnan(out["auc"][g_bad]).all()
    keep = [g for g in range(G) if g != g_bad]
    assert not out["status"][keep].any() and not np.isnan(out["auc"][keep]).any()
    rest = {k: (v[keep] if k in SCALARS else v) for k, v in out.items()}
    check(scores, cls, [sets[g] for g in keep], rest)


# ------------------------------------------------------------------------------------------------ xm_label_hist
@pytest.mark.parametrize("N", rc.HIST_N)
@pytest.mark.parametrize("E", rc.HIST_E)
def test_label_hist(gpu, E, N):
    import torch
    from mcncrossmodalemotions_amd import vl
    x = rc.hist_input(N, E)
    want = rc.label_hist_ref(x)
    assert want.sum() == N
    d2 = vl.from_numpy(x, gpu)                                          # N x E, column-major
    d3 = vl.from_numpy(x.T.reshape(1, 1, E, N), gpu)                     # 1 x 1 x E x N: a sample's values contiguous
    assert np.array_equal(vl.to_numpy(d3)[0, 0].T, x, equal_nan=True)
    h = vl.label_hist(d2)
    assert h.dtype == torch.int64 and np.array_equal(h.cpu().numpy(), want)
    assert np.array_equal(vl.label_hist(d3, dim=3).cpu().numpy(), want)
    # accumulation into given bins, twice, from a start past 2^32
    start = (np.arange(E, dtype=np.int64) * 7919) % 1000 + (np.int64(1) << 33)
    given = torch.from_numpy(start.copy()).to(gpu)
    back = vl.label_hist(d3, dim=3, bins=given)
    assert back is given and np.array_equal(given.cpu().numpy(), start + want)
    vl.label_hist(d2, dim=2, bins=given)
    assert np.array_equal(given.cpu().numpy(), start + 2 * want)
    # vl.max_label on the same samples: the same rule
    lab = vl.to_numpy(vl.max_label(d3)).reshape(-1).astype(np.int64)
    assert np.array_equal(lab - 1, rc.first_max_labels(x))
    assert np.array_equal(np.bincount(lab - 1, minlength=E), want)


def test_label_hist_refusal_and_no_samples(gpu):
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    E = rc.HIST_CLASSES_MAX + 1
    start = np.arange(E, dtype=np.int64) + 11
    given = torch.from_numpy(start.copy()).to(gpu)
    with pytest.raises(_lib.XmError, match="more than %d classes" % rc.HIST_CLASSES_MAX):
        vl.label_hist(vl.from_numpy(np.zeros((2, E), np.float32), gpu), bins=given)
    with pytest.raises(_lib.XmError):
        vl.label_hist(vl.from_numpy(np.zeros((1, 1, E, 2), np.float32), gpu), dim=3, bins=given)
    torch.cuda.synchronize()
    assert np.array_equal(given.cpu().numpy(), start)
    # N = 0: the bins come back unchanged, in either layout
    start = np.arange(8, dtype=np.int64) * 3 + 1
    given = torch.from_numpy(start.copy()).to(gpu)
    assert vl.label_hist(torch.empty(8, 0, dtype=torch.float32, device=gpu).t(), bins=given) is given
    vl.label_hist(torch.empty(0, 8, 1, 1, dtype=torch.float32, device=gpu).permute(3, 2, 1, 0), dim=3, bins=given)
    torch.cuda.synchronize()
    assert np.array_equal(given.cpu().numpy(), start)
    assert not vl.label_hist(torch.empty(8, 0, dtype=torch.float32, device=gpu).t()).cpu().numpy().any()
