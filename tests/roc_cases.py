"""The inputs of tests/test_gpu_roc_edges.py, as pure numpy: importable without a GPU and without the library, so that
tests/test_roc_edges_cpu.py checks, on the restatement, exactly the arrays the GPU file runs.

The geometry below restates the constants of csrc/roc.hip; the GPU file asserts it against vl.roc_geometry() before it
uses a case, so a kernel whose tile changes fails there instead of silently testing beside its edges.

Every generator returns (scores n x E float32, cls n int, sets): cls is 1-based as vl.roc takes it (problem (g, c) labels a
row +1 where cls == c + 1), sets is a list of 1-based row arrays."""
import numpy as np

TILE, WAVE_SPAN, THREADS, HIST_CLASSES_MAX = 2048, 512, 256, 4096
GEOMETRY = (TILE, WAVE_SPAN, THREADS, HIST_CLASSES_MAX)


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def one_byte_varies(b, n, seed=0):
    """finite scores whose bit patterns differ in byte b only (so three of the four radix passes see one digit value, or,
    for b = 3, the two the sign leaves in the low bytes), digit d uniform in 0..255; positives with probability 0.4.  The
    four bytes draw in turn from one generator, so each pass is tested on digits and labels of its own"""
    rng = np.random.default_rng(seed)
    for _ in range(b + 1):
        d = rng.integers(0, 256, n).astype(np.uint32)
        cls = np.where(rng.random(n) < 0.4, 1, 2)
    bits = (np.uint32(0x3F800000) ^ (d << np.uint32(8 * b))) if b < 3 else ((d << np.uint32(24)) | np.uint32(0x00400000))
    return _f32(bits).reshape(n, 1).copy(), cls, [np.arange(1, n + 1)]


FEW_VALUES = np.array([0.5, -1.25, 3.0], np.float32)


def few_values(n, v, positives="random", seed=0):
    """v distinct scores over n rows.  positives: 'first' / 'last' put the n // 3 positives at that end of the set,
    'random' labels a row positive with probability 0.4"""
    rng = np.random.default_rng(seed)
    sc = FEW_VALUES[rng.integers(0, v, n)]
    if positives == "random":
        cls = np.where(rng.random(n) < 0.4, 1, 2)
    else:
        cls = np.full(n, 2)
        cls[:n // 3] = 1
        if positives == "last":
            cls = cls[::-1].copy()
    return sc.reshape(n, 1).copy(), cls, [np.arange(1, n + 1)]


def _mix_column(rng, n):
    u = rng.random(n)
    sc = rng.standard_normal(n).astype(np.float32)
    half = rng.random(n) < 0.5
    sc[half] = np.round(sc[half] * 2) / 2                                     # ties among the normals
    zero = (u >= 0.20) & (u < 0.30)
    sc[zero] = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0))[zero]
    den = (u >= 0.30) & (u < 0.40)
    sc[den] = (rng.standard_normal(n) * 1e-41).astype(np.float32)[den]       # denormals of both signs, some +-0
    sc[(u >= 0.40) & (u < 0.42)] = np.inf
    sc[u < 0.20] = -np.inf
    return sc


def signed_mix(n, E=1, seed=0):
    """normals (half of them rounded to halves), +-0, -Inf (about 20 %), +Inf, denormals: the content of the hand cases of
    test_gpu_roc.py at any length.  Column 2 is column 1 negated, further columns are drawn afresh; cls is uniform over
    1 .. max(E, 2).  All rows form one set"""
    rng = np.random.default_rng(seed)
    cols = []
    for c in range(E):
        cols.append(-cols[0] if c == 1 else _mix_column(rng, n))
    cls = rng.integers(1, max(E, 2) + 1, n)
    return np.stack(cols, 1), cls, [np.arange(1, n + 1)]


def deal(n, lengths, seed):
    """sets of the given lengths dealt, in turn, from one permutation of the rows 1..n"""
    assert sum(lengths) <= n
    order = np.random.default_rng(seed).permutation(n) + 1
    ends = np.cumsum(lengths)
    return [order[e - m:e] for m, e in zip(lengths, ends)]


def lattice_lengths(tile=TILE, span=WAVE_SPAN):
    return [span - 1, span, span + 1, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1]


def multiple_lengths(tile=TILE):
    return [tile, 2 * tile, tile]


def lattice_case(lengths, seed=0):
    """E = 2 (column 2 = the negated scores), sets of `lengths` dealt from a permutation of the rows"""
    n = int(sum(lengths))
    scores, cls, _ = signed_mix(n, 2, seed)
    return scores, cls, deal(n, lengths, seed + 1)


def many_sets_case(G, seed=0):
    """G sets of 1..3 rows, every fifth one (g % 5 == 4) empty, E = 3, signed_mix scores"""
    rng = np.random.default_rng(seed + 100)
    lengths = [0 if g % 5 == 4 else int(m) for g, m in enumerate(rng.integers(1, 4, G))]
    n = int(sum(lengths))
    scores, cls, _ = signed_mix(n, 3, seed)
    return scores, cls, deal(n, lengths, seed + 1)


EMPTY_LENGTHS = [0, 0, 300, 300, 0, 0, 0, 300, 0, 0]


def empties_case(seed=0):
    """two leading empty sets, three consecutive in the middle, two trailing, around 300-row sets; E = 2"""
    return lattice_case(EMPTY_LENGTHS, seed)


def only_empties_case(seed=0):
    """three empty sets over a 10-row score matrix: nnz = 0"""
    scores, cls, _ = signed_mix(10, 2, seed)
    return scores, cls, [np.zeros(0, np.int64)] * 3


def big_case(tile=TILE, threads=THREADS, seed=0):
    """one set of (threads + 1) tile + 1 rows: more tiles than the per-problem scan has threads, the last of one entry;
    scores round(randn, 1), 30 % positives: S >= 2^33"""
    n = (threads + 1) * tile + 1
    rng = np.random.default_rng(seed)
    sc = np.round(rng.standard_normal(n), 1).astype(np.float32)
    cls = np.where(rng.random(n) < 0.3, 1, 2)
    return sc.reshape(n, 1), cls, [np.arange(1, n + 1)]


# ------------------------------------------------------------------------------------------------ xm_label_hist
HIST_E = [1, 8, 257, HIST_CLASSES_MAX]
HIST_N = [1, 255, 256, 257, 1000]


def hist_input(N, E, seed=0):
    """N x E values in halves (ties of the maximum), 2 % NaN, 2 % -Inf, and from N >= 8 on two all-NaN rows and two
    all--Inf rows (rows 2, N - 1 and 5, N // 2)"""
    rng = np.random.default_rng(seed + 1000 * E + N)
    x = (np.round(rng.standard_normal((N, E)) * 2) / 2).astype(np.float32)
    u = rng.random((N, E))
    x[u < 0.02] = np.nan
    x[(u >= 0.02) & (u < 0.04)] = -np.inf
    if N >= 8:
        x[[2, N - 1]] = np.nan
        x[[5, N // 2]] = -np.inf
    return x


def first_max_labels(x):
    """0-based label per row of an N x E array as the header states it for xm_label_hist / xm_max_label: the first index
    whose value exceeds the running best, which starts at -Inf.  A NaN compares false and never wins; a row of NaN or
    -Inf only keeps index 0 (class 1)"""
    x = np.asarray(x, np.float32)
    best = np.full(x.shape[0], -np.inf, np.float32)
    arg = np.zeros(x.shape[0], np.int64)
    with np.errstate(invalid="ignore"):
        for c in range(x.shape[1]):
            win = x[:, c] > best
            best[win] = x[win, c]
            arg[win] = c
    return arg


def label_hist_ref(x):
    return np.bincount(first_max_labels(x), minlength=np.asarray(x).shape[1]).astype(np.int64)
