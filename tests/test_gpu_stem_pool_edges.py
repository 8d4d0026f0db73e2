"""The fused stem chain (csrc/stem_pool_kernels.h: stem_gram_kernel, conv_stem_bnpool_fwd_kernel,
conv_stem_wgrad_pool_kernel) at the edges of its tilings, against the references of tests/test_gpu_stem_pool.py -- the
oracle's fp64-accumulated composition vl_nnconv -> vl_nnbnorm -> relu -> vl_nnpool, G.pool_argmax_codes, G.pool_route -- and
under that file's tolerances, unchanged: 1e-4 of the largest entry for the pooled output, df, dg, db; 2e-6 for the Gram
matrix; 1e-5 relative for sigma; the routing-table rule with its < 1e-3 cap.

Every case names the boundary it sits on; tests/stem_pool_plan_check.cpp pins those figures (CASE FIGURES there, same order)
against csrc/stem_pool_plan.h on the CPU, so this file and the plan cannot drift apart.  The shapes are the smallest that
reach the edge, not the workload's.

Destinations go through the C ABI into guarded buffers (aligned_views.Guarded; ByteGuard below for the routing table): the
fused forward stores through the scalar offset of its buffer stores, which the hardware does not range-check -- a store for a
filter row >= K or behind the last window row / column shows as a touched guard, a window the kernel forgot as a sentinel
left in place.

Routing tables of tiny tensors: the cap `differing codes < 1e-3 of all` allows NO differing code below 1000 windows, and a
near-tie that fp32 and fp64 accumulation decide differently would break it through the reference alone.  So each forward
case takes the first seed, counting up from its nominal one, for which the oracle's fp32-accumulated and fp64-accumulated
chains give the same table and the same closed windows everywhere (agreed_seed below; the search runs on the CPU, usually
one extra oracle pass)."""
import ctypes as C

import numpy as np
import pytest

from aligned_views import Guarded, misaligned
from oracle import oracle as O
from oracle import graphs as G
from test_gpu_stem_pool import _kernels_run, close, patches, rnd

pytestmark = pytest.mark.gpu

POOL = (3, 3, 2, 2, 0, 0, 0, 0)          # window, stride, pad of pool1: the only pooling the fused kernels are written for
BYTE_SENTINEL = 0xEE                      # not a routing code (0 .. 8, 255)
BYTE_GUARD = 256


class ByteGuard:
    """a uint8 destination of `n` bytes, `offset` bytes past a 16-byte boundary, with BYTE_GUARD sentinel bytes on either
    side; the destination itself starts out as sentinels too"""

    def __init__(self, n, offset, device):
        import torch
        self.n, self.lo = int(n), BYTE_GUARD + offset
        self.flat = torch.full((self.n + 2 * BYTE_GUARD + 16,), BYTE_SENTINEL, dtype=torch.uint8, device=device)
        self.view = self.flat[self.lo:self.lo + self.n]
        assert self.view.data_ptr() % 16 == offset

    def assert_guards_untouched(self, what=""):
        b = self.flat.cpu().numpy()
        assert not (b[:self.lo] != BYTE_SENTINEL).any(), "%s: wrote in front of the table" % what
        assert not (b[self.lo + self.n:] != BYTE_SENTINEL).any(), "%s: wrote behind the table" % what


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _geo(x, f, stride, pad):
    sy, sx = (stride, stride) if np.isscalar(stride) else stride
    pt, pb, pl, pr = (pad,) * 4 if np.isscalar(pad) else pad
    return tuple(int(v) for v in x.shape), tuple(int(v) for v in f.shape), (int(sy), int(sx), int(pt), int(pb), int(pl), int(pr))


def _rc(rc):
    """None for "not covered", True otherwise (errors raise)"""
    from mcncrossmodalemotions_amd import _lib, vl
    if rc == vl.XM_ENOTSUP:
        return None
    _lib.check(rc)
    return True


def gram_abi(x, fshape, stride, pad, gram):
    """xm_stem_gram into the caller's fp64 [64][64]"""
    from mcncrossmodalemotions_amd import _lib
    (H, W, _, N), (FH, FW, _, _), geo = _geo(x, np.empty(tuple(fshape) + (1, 1)), stride, pad)
    return _rc(_lib.load().xm_stem_gram(_p(x), H, W, N, FH, FW, *geo, _p(gram), _stream()))


def fwd_abi(x, f, b, g, bb, stride, pad, mom_in, gram, y, am, mom_out, pool=POOL):
    """xm_nnconv_bnorm_relu_pool_forward into the caller's y_pool / table / moments / Gram matrix"""
    from mcncrossmodalemotions_amd import _lib
    (H, W, Cc, N), (FH, FW, FC, K), geo = _geo(x, f, stride, pad)
    return _rc(_lib.load().xm_nnconv_bnorm_relu_pool_forward(
        _p(x), H, W, Cc, N, _p(f), FH, FW, FC, K, _p(b), *geo, 1, 1, _p(g), _p(bb), 1e-4, _p(mom_in), *pool, _p(gram), _p(y),
        _p(am), _p(mom_out), _stream()))


def bwd_abi(x, f, b, g, mom, train, am, yp, dz, gram, df, dbias, dg, db, stride, pad, pool=POOL):
    """xm_nnconv_backward_filter_bnrelupool_gram into the caller's df / dbias / dg / db"""
    from mcncrossmodalemotions_amd import _lib
    (H, W, Cc, N), (FH, FW, FC, K), geo = _geo(x, f, stride, pad)
    return _rc(_lib.load().xm_nnconv_backward_filter_bnrelupool_gram(
        _p(x), H, W, Cc, N, _p(f), FH, FW, FC, K, _p(b), *geo, 1, 1, _p(g), _p(mom), 1 if train else 0, *pool, _p(am), _p(yp),
        _p(dz), _p(gram), _p(df), _p(dbias), _p(dg), _p(db), _stream()))


def dev(a, offset=0):
    from mcncrossmodalemotions_amd import vl
    t = vl.from_numpy(a)
    return misaligned(t, offset) if offset else t


def col(v):
    return None if v is None else np.asarray(v).reshape(-1, 1)


def got(gd, what):
    """the guarded destination's content; every element written, no guard touched"""
    from mcncrossmodalemotions_amd import vl
    gd.assert_guards_untouched(what)
    out = vl.to_numpy(gd.view)
    assert not np.isnan(out).any(), "%s: elements left unwritten" % what
    return out


def table_bytes(code):
    import torch
    return torch.from_numpy(np.ascontiguousarray(code.ravel(order="F"))).cuda()


# ---- the oracle's chain ---------------------------------------------------------------------------------------------------
def draw(seed, H, W, N, K, FH, FW, train, has_bias, dead=None):
    rng = np.random.default_rng(seed)
    x, f = rnd(rng, H, W, 1, N), O.F(rng.standard_normal((FH, FW, 1, K)) * 0.2)
    b = rnd(rng, K) if has_bias else None
    g, bb = O.F(rng.uniform(0.5, 1.5, K) * rng.choice([-1, 1], K)), rnd(rng, K)
    mom = None if train else O.F(np.stack([rng.standard_normal(K) * 0.3, rng.uniform(0.5, 1.5, K)], 1))
    if dead is not None:                   # a filter whose every window is closed: bnorm's output far below zero
        g[dead], bb[dead] = 0.5, -50.0
    return rng, x, f, b, g, bb, mom


def chain(x, f, b, g, bb, mom, stride, pad, acc64=True):
    y = O.vl_nnconv(x, f, b, stride=stride, pad=pad, acc64=acc64)
    yb, mref = O.vl_nnbnorm(y, g, bb, moments=mom, acc64=acc64)
    yr = np.maximum(yb, 0)
    return y, yb, mref, yr, O.vl_nnpool(yr, [3, 3], stride=2, pad=0, method="max"), G.pool_argmax_codes(yr, [3, 3], 2, 0)


def agreed_seed(seed, stride, pad, *shape, **kw):
    """first seed >= `seed` for which fp32 and fp64 accumulation decide every window alike (module docstring)"""
    for s in range(seed, seed + 50):
        _, x, f, b, g, bb, mom = draw(s, *shape, **kw)
        yp32, c32 = chain(x, f, b, g, bb, mom, stride, pad, acc64=False)[4:]
        yp64, c64 = chain(x, f, b, g, bb, mom, stride, pad, acc64=True)[4:]
        if np.array_equal(c32, c64) and np.array_equal(yp32 == 0, yp64 == 0):
            return s
    raise AssertionError("no seed among 50 without a near-tie")


def plant_routes(code, yp):
    """tests/test_gpu_stem_pool.py's planted routes for any pooled size: all nine codes at the corners and in the middle of
    the first plane of the first sample and of the LAST filter of the LAST sample, the rows either side of every 16-row
    chunk boundary the tensor has (the row in front of a chunk pair travels by a load of its own), a dead window beside
    live ones"""
    pHo, pWo, K, N = yp.shape
    c1 = min(1, pWo - 1)
    for (c, n) in ((0, 0), (K - 1, N - 1)):
        for k, (hh, ww) in enumerate(((0, 0), (pHo - 1, pWo - 1), (pHo - 1, 0), (0, pWo - 1), (pHo // 2, pWo // 2),
                                      (min(15, pHo - 1), c1), (min(16, pHo - 1), c1), (pHo - 2, pWo - 1), (1, 0))):
            code[hh, ww, c, n] = (2 * k + 8) % 9
            yp[hh, ww, c, n] = 1.0
        cols = slice(min(2, pWo - 1), max(min(4, pWo), min(2, pWo - 1) + 1))
        for row in (15, 16, 31, 32, 63, 64, 95, 96):
            if row < pHo:
                code[row, cols, c, n] = 2
                yp[row, cols, c, n] = 1.0
        yp[3, min(3, pWo - 1), c, n] = 0.0


# ---- stem_gram_kernel -------------------------------------------------------------------------------------------------------
GRAM_CASES = [  # H, W, N, FH, FW, stride, pad [t b l r]
    (68, 9, 1, 7, 7, 2, 1),                      # Ho 32 (the gate's minimum: the wave's second chunk is absent), Wo 3, N 1
    (68, 18, 3, 7, 7, 2, [2, 2, 6, 1]),          # Ho 33: a second chunk of ONE row; pl 6: the first column sees one source column
    (132, 21, 2, 8, 7, 2, [0, 2, 1, 3]),         # Ho 64: both chunks full, no second wave; 56 taps; pt 0, pr > pl
    (132, 15, 1, 7, 7, 2, [4, 0, 1, 1]),         # Ho 65: a second wave with one row; pt 4
    (260, 8, 2, 5, 5, 1, 0),                     # stride 1, Ho 256: exactly one 256-row group per column pair
    (260, 7, 1, 5, 5, 1, [0, 1, 1, 1]),          # stride 1, Ho 257: a second group of one row (three idle waves), Wo 5
    (72, 10, 2, 4, 4, (2, 1), 0),                # stride (2, 1), 16 taps (the minimum), Wo 7
    (40, 25, 1, 4, 7, (1, 2), 0),                # stride (1, 2), 28 taps
    (76, 12, 2, 8, 4, 2, 1),                     # 32 taps: the ones column opens the second column tile
    (68, 9, 700, 7, 7, 2, 1),                    # 1400 block units on the grid's cap of 768: a block walks a SECOND unit
]


@pytest.mark.parametrize("case", GRAM_CASES)
def test_stem_gram_edges(gpu, case):
    from mcncrossmodalemotions_amd import vl, _lib
    L = _lib.load()
    H, W, N, FH, FW, stride, pad = case
    rng = np.random.default_rng(7 * H + W + N + FH)
    x = rnd(rng, H, W, 1, N) + np.float32(0.3)
    P, Ho, Wo = patches(x, FH, FW, stride, pad)
    ref = P.T @ P
    R = FH * FW
    gd = Guarded((2 * 64 * 64,), 0, gpu)                                   # fp64 [64][64] as pairs of floats
    ok, names = _kernels_run(L, lambda: gram_abi(dev(x), (FH, FW), stride, pad, gd.view))
    assert ok and any("stem_gram" in n for n in names), names
    gd.assert_guards_untouched("gram")
    import torch
    gram = gd.flat[gd.lo:gd.lo + gd.n].view(torch.float64)
    g = gram.cpu().numpy().reshape(64, 64)
    assert not np.isnan(g).any(), "gram: elements left unwritten"
    assert np.array_equal(g, g.T)
    close(g[:R + 1, :R + 1], ref, 2e-6, what="gram")
    assert g[R, R] == Ho * Wo * N
    assert not g[R + 1:].any() and not g[:, R + 1:].any()
    K = 24
    f, b = O.F(rng.standard_normal((FH, FW, 1, K)) * 0.2), rnd(rng, K)
    y = O.vl_nnconv(x, f, b, stride=stride, pad=pad, acc64=True)
    _, m_ref = O.vl_nnbnorm(y, O.F(np.ones(K)), O.F(np.zeros(K)), acc64=True)
    md = Guarded((K, 2), 0, gpu)
    vl.stem_gram_moments(gram, dev(f), dev(col(b)), moments_out=md.view)
    mo = got(md, "moments")
    close(mo[:, 0], m_ref[:, 0], what="mean from G")
    assert np.abs(mo[:, 1] / m_ref[:, 1] - 1).max() <= 1e-5, "sigma from G"


# ---- conv_stem_wgrad_pool_kernel --------------------------------------------------------------------------------------------
BWD_CASES = [  # H, W, N, K, FH, FW, stride, pad, train, conv bias, y_pool given (else the 255-marked table), dead filter
    (68, 9, 1, 1, 7, 7, 2, 1, True, True, True, None),                 # Ho 32 / pHo 15: quads reach two planes on; pWo 1; K 1
    (68, 18, 3, 15, 7, 7, 2, [2, 2, 6, 1], False, False, False, 7),    # Ho 33; K 15: a partly filled group, group 1 missing
    (132, 21, 1, 16, 8, 7, 2, [0, 2, 1, 3], True, True, True, 8),      # Ho 64: one chunk pair, both chunks full; K 16; 56 taps
    (132, 15, 3, 17, 7, 7, 2, [4, 0, 1, 1], True, False, False, None), # Ho 65: chunk pair 1 = one row + the row in front; K 17
    (260, 8, 1, 33, 5, 5, 1, 0, True, True, True, None),               # stride 1, Ho 256: four full chunk pairs; K 33; pWo 1
    (260, 7, 2, 47, 5, 5, 1, [0, 1, 1, 1], False, True, False, None),  # stride 1, Ho 257: a fifth chunk pair of one row; K 47
    (72, 10, 1, 65, 4, 4, (2, 1), 0, True, True, True, None),          # stride (2, 1), 16 taps; K 65: one filter in row tile 2
    (40, 25, 3, 95, 4, 7, (1, 2), 0, True, False, False, None),        # stride (1, 2), 28 taps; K 95: all groups, one lane short
    (76, 12, 2, 96, 8, 4, 2, 1, False, True, True, 40),                # 32 taps; all filters; a dead filter under the ReLU gate
    (132, 463, 3, 40, 7, 7, 2, [4, 0, 1, 1], True, True, False, None), # 690 units for 672 waves per row tile (the grid's cap): 18
                                                                       # waves walk a SECOND unit, operands in flight a unit ahead
                                                                       # -- no smaller tensor reaches that loop; K 40, last sample
]


@pytest.mark.parametrize("case", BWD_CASES)
def test_conv_stem_wgrad_pool_edges(gpu, case):
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    H, W, N, K, FH, FW, stride, pad, train, has_bias, with_yp, dead = case
    rng, x, f, b, g, bb, mom = draw(H + 5 * W + K + FH + int(train), H, W, N, K, FH, FW, train, has_bias)
    y, yb, mref, yr, yp, code = chain(x, f, b, g, bb, mom, stride, pad)
    yp = yp.copy()
    plant_routes(code, yp)
    if dead is not None:
        yp[:, :, dead, :] = 0.0
    dz = rnd(rng, *yp.shape)
    dyr = G.pool_route(dz * (yp > 0), code, yr.shape, [3, 3], 2, 0)
    dx_ref, dg_ref, db_ref, _ = O.vl_nnbnorm(y, g, bb, dyr, moments=mom, acc64=True)
    _, df_ref, _ = O.vl_nnconv(x, f, b, dx_ref, stride=stride, pad=pad, acc64=True, no_der_data=True)
    table = code if with_yp else np.where(yp > 0, code, 255).astype(np.uint8)

    xd, fd, bd, gd_, mo = dev(x), dev(f), None if b is None else dev(col(b)), dev(col(g)), dev(mref if mom is None else mom)
    am, ypd, dzd = table_bytes(table), dev(O.F(yp)) if with_yp else None, dev(dz)
    out = [Guarded((FH, FW, 1, K), 0, gpu), Guarded((K, 1), 0, gpu) if has_bias else None, Guarded((K, 1), 0, gpu),
           Guarded((K, 1), 0, gpu)]
    views = [None if o is None else o.view for o in out]
    ok, names = _kernels_run(L, lambda: bwd_abi(xd, fd, bd, gd_, mo, train, am, ypd, dzd, None, *views, stride, pad))
    assert ok, "the fused kernel must cover this geometry"
    assert any("stem_wgrad_pool" in n for n in names), names
    assert any("stem_gram" in n for n in names) == train, names
    df, dg, db = got(out[0], "df"), got(out[2], "dg"), got(out[3], "db")
    close(df, df_ref, what="filter derivative")
    close(dg.ravel(), dg_ref, what="dg")
    close(db.ravel(), db_ref, what="db")
    if dead is not None:
        assert not df[..., dead].any() and dg[dead, 0] == 0 and db[dead, 0] == 0, "a filter without an open window"
    if has_bias:
        ref = dx_ref.astype(np.float64).sum((0, 1, 3))
        mag = np.abs(dx_ref.astype(np.float64)).sum((0, 1, 3)).max()
        assert np.abs(got(out[1], "dbias").ravel() - ref).max() <= 2e-6 * max(1.0, mag), "conv bias derivative"
    # pooled tensors one float past a 16-byte boundary (the gate reads & 3 only): the same bits
    again = [Guarded((FH, FW, 1, K), 0, gpu), None, Guarded((K, 1), 0, gpu), Guarded((K, 1), 0, gpu)]
    assert bwd_abi(xd, fd, bd, gd_, mo, train, am, None if ypd is None else misaligned(ypd), misaligned(dzd), None,
                   *[None if o is None else o.view for o in again], stride, pad)
    assert np.array_equal(got(again[0], "df"), df) and np.array_equal(got(again[2], "dg"), dg)
    assert np.array_equal(got(again[3], "db"), db)


# ---- conv_stem_bnpool_fwd_kernel ----------------------------------------------------------------------------------------------
FWD_CASES = [  # H, W, N, K, FH, pad, train, conv bias, dead filter
    (68, 9, 1, 8, 7, 1, True, True, None),                  # pHo 15: one short strip; pWo 1 = SG 1; K 8: one group of a row tile
    (264, 8, 3, 24, 7, [1, 1, 6, 1], False, False, None),   # pHo 64: one row in the second strip; pWo 2, Wo 5; pl 6; K 24
    (512, 30, 1, 32, 7, [1, 3, 1, 2], True, True, None),    # pHo 127: one row in the third strip; pWo 6, Wo 14; K 32: one row tile
    (68, 33, 2, 40, 5, [0, 0, 1, 1], True, True, None),     # pWo 7: one ring period (15 output columns); FH 5; pt 0; K 40
    (72, 37, 1, 72, 3, [4, 0, 1, 1], False, True, None),    # pWo 8: a period and a column; FH 3; pt 4; K 72: row tile 2 = one group
    (68, 201, 1, 96, 7, 1, True, True, 50),                 # pWo 49 in SG 13 segments (13 does not divide 49) of 3 and 4 window
                                                            # columns = 7 and 9 output columns: one ring period, and one + 2 (up to
                                                            # 16 window columns SG = pWo: three output columns per unit); dead filter
    (68, 9, 700, 8, 7, 1, True, True, None),                # 2100 wave units for 2048 resident waves: a wave takes a SECOND unit
]


@pytest.mark.parametrize("case", FWD_CASES)
def test_conv_stem_bnpool_fwd_edges(gpu, case):
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    H, W, N, K, FH, pad, train, has_bias, dead = case
    shape = (H, W, N, K, FH, 7, train, has_bias)
    seed = agreed_seed(H + 3 * W + K + FH, 2, pad, *shape, dead=dead)
    rng, x, f, b, g, bb, mom = draw(seed, *shape, dead=dead)
    y, yb, mref, yr, yp_ref, code_ref = chain(x, f, b, g, bb, mom, 2, pad)
    pHo, pWo = yp_ref.shape[:2]
    xd, fd, bd, gd_, bbd = dev(x), dev(f), None if b is None else dev(col(b)), dev(col(g)), dev(col(bb))
    yg, ag = Guarded((pHo, pWo, K, N), 0, gpu), ByteGuard(pHo * pWo * K * N, 0, gpu)
    mg, gg = (Guarded((K, 2), 0, gpu), Guarded((2 * 64 * 64,), 0, gpu)) if train else (None, None)
    momd = None if train else dev(mom)
    ok, names = _kernels_run(L, lambda: fwd_abi(xd, fd, bd, gd_, bbd, 2, pad, momd, None if gg is None else gg.view, yg.view,
                                                ag.view, None if mg is None else mg.view))
    assert ok, "the fused kernel must cover this geometry"
    assert any("bnpool_fwd" in n for n in names), names
    assert any("stem_gram" in n for n in names) == train, names
    yp = got(yg, "pooled output")
    ag.assert_guards_untouched("routing table")
    code = ag.view.cpu().numpy().reshape(yp_ref.shape, order="F")
    close(yp, yp_ref, what="pooled output")
    m = got(mg, "moments") if train else mom
    if train:
        gg.assert_guards_untouched("gram")
        close(m[:, 0], mref[:, 0], what="mean")
        assert np.abs(m[:, 1] / mref[:, 1] - 1).max() <= 1e-5
    dead_w = yp == 0
    assert np.array_equal(code == 255, dead_w), "255 exactly at the closed windows (a sentinel left in place is neither)"
    assert not (dead_w & (yp_ref > 1e-4 * max(1.0, float(np.abs(yb).max())))).any()
    if dead is not None:
        assert dead_w[:, :, dead, :].all()
    diff = (code != code_ref) & ~dead_w
    if diff.any():
        pos = G.pool_positions(np.where(dead_w, code_ref, code), yr.shape, [3, 3], 2, 0)
        at = yr.ravel(order="F")[pos]
        assert np.abs(at - yp_ref)[diff].max() <= 1e-4 * max(1.0, float(np.abs(yb).max())), "routing differs away from a tie"
        assert diff.mean() < 1e-3
    # backward through this table, y_pool not given
    dz = rnd(rng, *yp_ref.shape)
    code_use = np.where(dead_w, 0, code).astype(np.uint8)
    dyr = G.pool_route(dz * ~dead_w, code_use, yr.shape, [3, 3], 2, 0)
    dx_ref, dg_ref, db_ref, _ = O.vl_nnbnorm(y, g, bb, dyr, moments=mom, acc64=True)
    _, df_ref, _ = O.vl_nnconv(x, f, b, dx_ref, stride=2, pad=pad, acc64=True, no_der_data=True)
    out = [Guarded((FH, 7, 1, K), 0, gpu), Guarded((K, 1), 0, gpu) if has_bias else None, Guarded((K, 1), 0, gpu),
           Guarded((K, 1), 0, gpu)]
    import torch
    gram = None if gg is None else gg.flat[gg.lo:gg.lo + gg.n].view(torch.float64)
    assert bwd_abi(xd, fd, bd, gd_, dev(m), train, ag.view, None, dev(dz), gram, *[None if o is None else o.view for o in out],
                   2, pad)
    close(got(out[0], "df"), df_ref, what="filter derivative through the fused forward's table")
    close(got(out[2], "dg").ravel(), dg_ref, what="dg")
    close(got(out[3], "db").ravel(), db_ref, what="db")


# ---- the gates --------------------------------------------------------------------------------------------------------------
def _gate_operands(H, W, N, K, seed=11):
    rng, x, f, b, g, bb, _ = draw(seed, H, W, N, K, 7, 7, True, True)
    return rng, x, f, b, g, bb


def test_gate_x_off_a_16_byte_boundary(gpu):
    """x one float past a 16-byte boundary: the three entry points answer "not covered" (16-byte loads of x), and the
    caller's composed path -- vl_nnconv, vl_nnbnorm, vl_nnrelu, vl_nnpool -- gives the oracle's result from the same x"""
    from mcncrossmodalemotions_amd import vl
    H, W, N, K, pad = 68, 20, 2, 16, 1
    rng, x, f, b, g, bb = _gate_operands(H, W, N, K)
    y, yb, mref, yr, yp_ref, code = chain(x, f, b, g, bb, None, 2, pad)
    xo, fd, bd, gd_, bbd = dev(x, 1), dev(f), dev(col(b)), dev(col(g)), dev(col(bb))
    assert xo.data_ptr() % 16 == 4
    assert vl.stem_gram(xo, (7, 7), stride=2, pad=pad) is None
    assert vl.conv_bnorm_relu_pool(xo, fd, bd, gd_, bbd, [3, 3], stride=2, pad=pad, pool_stride=2, pool_pad=0) is None
    dz = rnd(rng, *yp_ref.shape)
    assert vl.conv_backward_filter_bnrelupool_gram(xo, fd, bd, gd_, dev(mref), table_bytes(code), dev(yp_ref), dev(dz), [3, 3],
                                                   stride=2, pad=pad, pool_stride=2, pool_pad=0) is None
    assert vl.stem_gram(dev(x), (7, 7), stride=2, pad=pad) is not None      # ... and the aligned copy IS covered
    yc = vl.vl_nnconv(xo, fd, bd, stride=2, pad=pad)
    yn = vl.vl_nnbnorm(yc, gd_, bbd)[0]
    ypc = vl.vl_nnpool(vl.vl_nnrelu(yn), [3, 3], stride=2, pad=0)
    close(vl.to_numpy(ypc), yp_ref, what="composed path from the unaligned x")


def test_gate_pooled_destination_one_float_off(gpu):
    """the fused forward into a y_pool one float past a 16-byte boundary (4-byte stores: & 3 only) and a table one byte
    past: accepted, the same bits as into aligned destinations, guards untouched"""
    H, W, N, K, pad = 68, 20, 2, 16, 1
    rng, x, f, b, g, bb = _gate_operands(H, W, N, K)
    pHo, pWo = 15, 3
    xd, fd, bd, gd_, bbd = dev(x), dev(f), dev(col(b)), dev(col(g)), dev(col(bb))
    res = []
    for off in (0, 1):
        yg, ag = Guarded((pHo, pWo, K, N), off, gpu), ByteGuard(pHo * pWo * K * N, off, gpu)
        mg, gg = Guarded((K, 2), 0, gpu), Guarded((2 * 64 * 64,), 0, gpu)
        assert fwd_abi(xd, fd, bd, gd_, bbd, 2, pad, None, gg.view, yg.view, ag.view, mg.view)
        ag.assert_guards_untouched("routing table")
        res.append((got(yg, "pooled output"), ag.view.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert not (res[0][1] == BYTE_SENTINEL).any()


def test_gate_filter_count_height_and_padded_pooling(gpu):
    """K % 8 != 0: refused by the forward (stores in groups of 8 filters), accepted by the backward; Ho 31: refused by all
    three; a padded pooling: refused by both fused entry points"""
    from mcncrossmodalemotions_amd import vl
    H, W, N, pad = 68, 20, 1, 1
    for K, fwd_ok in ((12, False), (16, True)):
        rng, x, f, b, g, bb = _gate_operands(H, W, N, K)
        y, yb, mref, yr, yp_ref, code = chain(x, f, b, g, bb, None, 2, pad)
        xd, fd, bd, gd_, bbd = dev(x), dev(f), dev(col(b)), dev(col(g)), dev(col(bb))
        res = vl.conv_bnorm_relu_pool(xd, fd, bd, gd_, bbd, [3, 3], stride=2, pad=pad, pool_stride=2, pool_pad=0)
        assert (res is not None) == fwd_ok, K
        args = (xd, fd, bd, gd_, dev(mref), table_bytes(code), dev(yp_ref), dev(rnd(rng, *yp_ref.shape)), [3, 3])
        assert vl.conv_backward_filter_bnrelupool_gram(*args, stride=2, pad=pad, pool_stride=2, pool_pad=0) is not None, K
    # padded pooling (K = 16 from the loop): the pooled tensors have the padded pooling's own size
    ypp = O.vl_nnpool(yr, [3, 3], stride=2, pad=[0, 1, 0, 1], method="max")
    assert vl.conv_bnorm_relu_pool(xd, fd, bd, gd_, bbd, [3, 3], stride=2, pad=pad, pool_stride=2, pool_pad=[0, 1, 0, 1]) is None
    codep = G.pool_argmax_codes(yr, [3, 3], 2, [0, 1, 0, 1])
    assert vl.conv_backward_filter_bnrelupool_gram(xd, fd, bd, gd_, dev(mref), table_bytes(codep), dev(ypp),
                                                   dev(rnd(rng, *ypp.shape)), [3, 3], stride=2, pad=pad, pool_stride=2,
                                                   pool_pad=[0, 1, 0, 1]) is None
    # Ho = 31 (H 64, pad 2): below a wave's chunk of an output column
    H = 64
    rng, x, f, b, g, bb = _gate_operands(H, W, N, 16)
    y, yb, mref, yr, yp_ref, code = chain(x, f, b, g, bb, None, 2, 2)
    assert y.shape[0] == 31
    xd, fd, bd, gd_, bbd = dev(x), dev(f), dev(col(b)), dev(col(g)), dev(col(bb))
    assert vl.stem_gram(xd, (7, 7), stride=2, pad=2) is None
    assert vl.conv_bnorm_relu_pool(xd, fd, bd, gd_, bbd, [3, 3], stride=2, pad=2, pool_stride=2, pool_pad=0) is None
    assert vl.conv_backward_filter_bnrelupool_gram(xd, fd, bd, gd_, dev(mref), table_bytes(code), dev(yp_ref),
                                                   dev(rnd(rng, *yp_ref.shape)), [3, 3], stride=2, pad=2, pool_stride=2,
                                                   pool_pad=0) is None
