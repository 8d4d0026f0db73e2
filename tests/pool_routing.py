"""numpy restatement of the max-pooling routing table, and the shared geometries / inputs of
tests/test_pool_routing_cpu.py and tests/test_gpu_norm_pool_edges.py (a plain module, not a conftest).

The table holds, per output, the position of the FIRST maximum in column-major scan order (w outer, h inner) inside the
UN-clipped window: code = dh + ph * dw.  Taps outside the tensor are skipped.  A window without any value above -inf has
no maximum: the oracle routes its derivative nowhere, the table holds NO_MAX there."""
import numpy as np

NO_MAX = 255


def out_size(n, pa, pb, f, s):
    return (n + pa + pb - f) // s + 1


def _pair(v):
    if np.isscalar(v):
        return int(v), int(v)
    v = list(v)
    return int(v[0]), int(v[-1])


def _pad4(pad):
    if np.isscalar(pad):
        return (int(pad),) * 4
    pad = [int(v) for v in pad]
    if len(pad) == 1:
        return (pad[0],) * 4
    if len(pad) == 2:
        return pad[0], pad[0], pad[1], pad[1]
    return tuple(pad)


class Geo:
    def __init__(self, H, W, pool, stride=1, pad=0):
        self.H, self.W = int(H), int(W)
        self.ph, self.pw = _pair(pool)
        self.sy, self.sx = _pair(stride)
        self.pt, self.pb, self.pl, self.pr = _pad4(pad)
        self.Ho = out_size(self.H, self.pt, self.pb, self.ph, self.sy)
        self.Wo = out_size(self.W, self.pl, self.pr, self.pw, self.sx)
        assert self.Ho > 0 and self.Wo > 0
        # extents of the un-clipped windows, with the tensor at [pt, pt + H) x [pl, pl + W)
        self.Hp = max(self.pt + self.H, self.sy * (self.Ho - 1) + self.ph)
        self.Wp = max(self.pl + self.W, self.sx * (self.Wo - 1) + self.pw)

    def tap(self, dh, dw):
        """index of tap (dh, dw) of every window inside an array of the un-clipped extents"""
        return (slice(dh, dh + self.sy * (self.Ho - 1) + 1, self.sy), slice(dw, dw + self.sx * (self.Wo - 1) + 1, self.sx))

    def embed(self, x, fill):
        x = np.asarray(x)
        xp = np.full((self.Hp, self.Wp) + x.shape[2:], fill, x.dtype)
        xp[self.pt:self.pt + self.H, self.pl:self.pl + self.W] = x
        return xp


def _as4(x):
    x = np.asarray(x)
    return x.reshape(x.shape + (1,) * (4 - x.ndim))


def routing_table(x, pool, stride=1, pad=0):
    """code[Ho, Wo, C, N] (uint8) of max pooling over x[H, W, C, N]"""
    x = _as4(x)
    g = Geo(x.shape[0], x.shape[1], pool, stride, pad)
    assert g.ph * g.pw <= 255
    xp = g.embed(x, -np.inf)            # a skipped tap and a tap of -inf behave alike: neither is ever "> best"
    best = np.full((g.Ho, g.Wo) + x.shape[2:], -np.inf, x.dtype)
    code = np.full(best.shape, NO_MAX, np.uint8)
    for dw in range(g.pw):
        for dh in range(g.ph):
            v = xp[g.tap(dh, dw)]
            up = v > best
            best = np.where(up, v, best)
            code[up] = dh + g.ph * dw
    return code


def top2_gap(x, pool, stride=1, pad=0):
    """largest minus second largest value (by position, so equal maxima give 0) of every window; inf with one tap"""
    x = _as4(x)
    g = Geo(x.shape[0], x.shape[1], pool, stride, pad)
    xp = g.embed(x, -np.inf)
    best = np.full((g.Ho, g.Wo) + x.shape[2:], -np.inf, np.float64)
    second = best.copy()
    for dw in range(g.pw):
        for dh in range(g.ph):
            v = xp[g.tap(dh, dw)].astype(np.float64)
            second = np.maximum(second, np.minimum(best, v))
            best = np.maximum(best, v)
    with np.errstate(invalid="ignore"):
        gap = best - second
    return np.where(np.isnan(gap), 0.0, gap)


def scatter(code, dzdy, H, W, pool, stride=1, pad=0):
    """DX of max pooling from the table alone.  An input element sums the windows that route to it in the order the
    oracle (and the kernels) visit them -- wo outer, ho inner, i.e. dw and dh DEscending -- in fp32, so the result is
    comparable bit for bit."""
    code, dzdy = _as4(code), _as4(np.asarray(dzdy, np.float32))
    g = Geo(H, W, pool, stride, pad)
    assert code.shape == dzdy.shape == (g.Ho, g.Wo) + dzdy.shape[2:]
    dxp = np.zeros((g.Hp, g.Wp) + dzdy.shape[2:], np.float32)
    zero = np.float32(0)
    for dw in reversed(range(g.pw)):
        for dh in reversed(range(g.ph)):
            dxp[g.tap(dh, dw)] += np.where(code == dh + g.ph * dw, dzdy, zero)
    return np.asfortranarray(dxp[g.pt:g.pt + H, g.pl:g.pl + W])


# ---- the geometries of the LDS-staged 3 x 3 max pooling and of its gate (pool_lds_plan in csrc/norm_pool_plan.h) -------------
# The figures beside each case are asserted against that header by tests/norm_pool_plan_check.cpp (kLdsCases; run by
# tests/test_norm_pool_plan_cpu.py), which is the evidence that a case reaches the branch it is written for.
# maxcols = 4096 / H (integer); wob = min((maxcols - 3) / sx + 1, Wo) (0 if maxcols < 3); the LDS kernel runs iff
# Ho * Wo >= 256 and (wob >= 4 or wob == Wo); then groups = ceil(Wo / wob), wob = ceil(Wo / groups); a block's run starts at
# base = plane * H * W + wlo * H and lead = base % 4.
# name: (H, W, C, N, stride, pad)
LDS_CASES = {
    # Ho x Wo = 17 x 16 = 272; maxcols = 117, wob = min(58, 16) = 16 == Wo, 1 group; plane size 1155 = 4 * 288 + 3, so
    # lead = 0, 3, 2, 1, 0, 3 over the 6 planes; 6 * 1155 = 6930 = 4 * 1732 + 2: the last quad of the last plane (start 5772,
    # cnt 1158, i = 1156) ends past the tensor -> the three-scalar tail load
    "a": (35, 33, 3, 2, (2, 2), 0),
    # the teachers' Caffe-style pool1: Ho x Wo = 17 x 17 = 289; maxcols = 120, wob = min(59, 17) = 17 == Wo; lead 0; the
    # last window row / column hangs one element over the tensor
    "b": (34, 34, 2, 2, (2, 2), (0, 1, 0, 1)),
    # stride 1 with padding: Ho x Wo = 20 x 18 = 360; maxcols = 204, wob = min(202, 18) = 18 == Wo; lead 0; wlo clamps at 0
    "c": (20, 18, 4, 2, (1, 1), 1),
    # largest legal pad, mixed strides: Ho = (31 + 4 - 3) / 2 + 1 = 17, Wo = 15 + 4 - 3 + 1 = 17; maxcols = 132,
    # wob = min(130, 17) = 17; plane size 465 = 4 * 116 + 1: lead = 0, 1, 2, 3, 0, 1; 6 * 465 = 2790 = 4 * 697 + 2: tail load
    "d": (31, 15, 3, 2, (2, 1), 2),
    # Ho x Wo = 99 x 25; maxcols = 20, wob = (20 - 3) / 2 + 1 = 9, groups = ceil(25 / 9) = 3, evened wob = ceil(25 / 3) = 9:
    # groups of 9, 9 and 7 columns; wlo = 0, 18, 36 (runs of 19, 19 and 15 input columns); lead 0
    "e": (200, 52, 2, 2, (2, 2), 0),
    # a column stride wider than the window: Ho x Wo = 20 x 20; maxcols = 68, wob = (68 - 3) / 4 + 1 = 17, groups = 2, evened
    # wob = 10; ncols = 9 * 4 + 3 = 39 <= 68; wlo = 0, 40; lead 0
    "f": (60, 80, 2, 2, (3, 4), 0),
    # the tallest plane the LDS kernel accepts: maxcols = 4096 / 1365 = 3, wob = 1 == Wo (Ho x Wo = 682 x 1); plane size
    # 4095 = 4 * 1023 + 3: lead = 0, 3, 2, 1, 0, 3; 6 * 4095 = 24570 = 4 * 6142 + 2: tail load; LDS = (4095 + 8) floats
    "g1": (1365, 3, 3, 2, (2, 2), 0),
    # maxcols = 4096 / 1366 = 2 < 3: wob = 0 -> the one-thread-per-output kernel
    "g2": (1366, 3, 3, 2, (2, 2), 0),
    # Ho x Wo = 349 x 4; maxcols = 5, wob = (5 - 3) / 2 + 1 = 2: below 4 and not Wo -> the one-thread-per-output kernel
    "g3": (700, 9, 3, 2, (2, 2), 0),
}
POOL3 = (3, 3)


def planted_input(seed, H, W, C, N, pool, stride=1, pad=0):
    """post-ReLU style input (about half of it exact zeros, which tie) with planted maxima: on the first and the last row
    and column any window covers, in the first and in the last plane, and one 3 x 3 plateau of equal values"""
    g = Geo(H, W, pool, stride, pad)
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((H, W, C, N)), 0).astype(np.float32)
    big = np.float32(8.0)
    hl = min(H - 1, g.sy * (g.Ho - 1) - g.pt + g.ph - 1)      # last covered row / column
    wl = min(W - 1, g.sx * (g.Wo - 1) - g.pl + g.pw - 1)
    for (c, n) in ((0, 0), (C - 1, N - 1)):
        x[0, 0, c, n] = big
        x[hl, wl, c, n] = big
        x[hl, 0, c, n] = big
        x[0, wl, c, n] = big
        h0, w0 = min(5, H - 3), min(4, W - 3)
        x[h0:h0 + 3, w0:w0 + 3, c, n] = big * np.float32(0.5)     # plateau: the FIRST maximum of each window wins
    return np.asfortranarray(x)


def lds_case_input(name):
    H, W, C, N, stride, pad = LDS_CASES[name]
    seed = 1000 + sorted(LDS_CASES).index(name)
    x = planted_input(seed, H, W, C, N, POOL3, stride, pad)
    g = Geo(H, W, POOL3, stride, pad)
    dzdy = np.asfortranarray(np.random.default_rng(seed + 500).standard_normal((g.Ho, g.Wo, C, N)).astype(np.float32))
    return x, dzdy


# ---- fused bnorm + relu + pool over the same geometries: inputs and the near-tie exemption ----------------------------------
FUSED_TOL = 1e-4          # TOL of tests/test_gpu_ops.py
# seeds (train mode, given moments) per geometry for which the fp32 oracle's own table differs from the fp64-accumulate
# one only inside near-tie windows AND those are at most 0.1 % of the windows (tests/test_pool_routing_cpu.py checks it)
FUSED_SEEDS = {"a": (105, 200), "b": (101, 201), "c": (100, 202), "d": (109, 209), "e": (101, 203), "f": (100, 205),
               "g1": (112, 200), "g2": (102, 201), "g3": (102, 201)}


def fused_case_input(name, train):
    """x, g, b, moments (None in train mode) as in test_fused_bnorm_relu_pool, with a positive shift so that few windows
    are all zeros after the relu (such a window is an exact tie and counts as exempt)"""
    H, W, C, N, stride, pad = LDS_CASES[name]
    rng = np.random.default_rng(FUSED_SEEDS[name][0 if train else 1])
    x = np.asfortranarray((rng.standard_normal((H, W, C, N)) * 1.5 + 0.3).astype(np.float32))
    g = (rng.uniform(0.5, 1.5, C) * rng.choice([-1, 1], C)).astype(np.float32)      # negative gains too
    b = (np.abs(rng.standard_normal(C)) * 0.5 + 0.5).astype(np.float32)
    mom = None
    if not train:
        mom = np.asfortranarray(np.stack([rng.standard_normal(C) * 0.3 + 0.3, rng.uniform(1.0, 2.0, C)], 1).astype(np.float32))
    return x, g, b, mom


def near_tie_windows(yr, pool, stride=1, pad=0, tol=FUSED_TOL):
    """windows of yr whose two largest values differ by less than the bound tol * max(1, max |yr|)"""
    bound = tol * max(1.0, float(np.abs(yr).max()))
    return top2_gap(yr, pool, stride, pad) < bound
