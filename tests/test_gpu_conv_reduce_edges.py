"""The reduction helpers behind vl_nnconv's backward and statistics paths at the edges of their launch arithmetic.  None of
them is profiled or has a force hook; their arms follow from sizes, and each case reads the split count it reached from the
library (xm_debug_get: "wgrad_last_splits", "bias_grad_last_splits", "stats_last_splits") before it compares with the
fp64-accumulate oracle under test_gpu_ops.TOL -- the dispatch policy is not restated here.

Kernel / arm -> the case that reaches it:
  reduce_splits_kernel<1>    (splits < 8)    5 slabs: one dependent chain per output; 189 outputs (a ragged block of 256), 256
  reduce_splits_kernel<4>    (8 .. 63)       37 slabs: lane 0 of an output takes z = 0, 4, 8, 12 / 16 .. 28 in the
                                             four-accumulator loop and 32, 36 in the tail, lane 1 only 33 there; 189 and 256
                                             outputs (64 per block); 10 and 12 slabs of the patch kernels (own slab stride)
  reduce_splits_kernel<16>   (>= 64)         64 slabs: the four-accumulator loop alone; 100 slabs: the tail runs twice for
                                             every z-lane and a third time for lanes 0 .. 3 only; 189 and 256 outputs (16 per block)
  bias_grad_partial_kernel                   S == N (one sample per split); N = 20 over S = 13 (seven splits of two samples, six
                                             of one); 33 x 33 (odd: 4-byte arm) with S > 1; Ho * Wo = 8 over 300 samples (S = 1, the
                                             flat (sample, position) index); dzdy = 1e4 + noise (fp64 partial sums)
  bias_grad_finalize_kernel                  S = 70 > 64 (a lane's second step); K = 3 and K = 5 (idle waves in the last block)
  conv_stats_reduce_kernel, S > 1 +
  conv_stats_finalize2_kernel                a 1 x 1 layer over 233,472 pixels in 64-pixel tiles: 3,648 partial rows per channel,
                                             four tile splits; K = 9 leaves seven idle channel lanes in the second block"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_ops import close, rnd
from test_gpu_conv_alignment import conv_bwd, conv_fwd, col, dbg, dev, forced, got, kernels
from aligned_views import Guarded

pytestmark = pytest.mark.gpu


# ---- reduce_splits_kernel behind conv_wgrad_kernel ----------------------------------------------------------------------------
# filter banks inside one 128 x 128 tile (configuration 0): K * R = 7 * 27 = 189 outputs -- no multiple of 16 -- and 16 * 16 =
# 256 -- a multiple of 256, 64 and 16, the outputs per block of the three arms.  (FH, C, K, pad)
BANKS = {"189": (3, 3, 7, 1), "256": (2, 4, 16, 0)}
# output pixels N * Ho * Wo as (Ho, Wo, N) -> the slab count the library reports for them
PIXELS = [((16, 10, 4), 5), ((16, 37, 8), 37), ((32, 32, 8), 64), ((40, 40, 8), 100)]


@pytest.mark.parametrize("bank", sorted(BANKS))
@pytest.mark.parametrize("pixels,splits", PIXELS)
def test_wgrad_split_reduction(gpu, pixels, splits, bank):
    FH, Cc, K, pad = BANKS[bank]
    (Ho, Wo, N) = pixels
    H, W = Ho + (FH - 1) - 2 * pad, Wo + (FH - 1) - 2 * pad
    rng = np.random.default_rng(Ho * 1000 + Wo * 10 + K)
    xh, fh = rnd(rng, H, W, Cc, N), rnd(rng, FH, FH, Cc, K)
    dh = rnd(rng, Ho, Wo, K, N)
    _, df_ref, _ = O.vl_nnconv(xh, fh, None, dh, pad=pad, acc64=True, no_der_data=True)
    x, dzdy, df = dev(xh), dev(dh), Guarded((FH, FH, Cc, K), 0, gpu)
    with forced(conv_cfg=0):
        names = kernels(lambda: conv_bwd((H, W, Cc, N), (FH, FH, Cc, K), dzdy, x=x, df=df.view, pad=pad))
        reached = dbg("wgrad_last_splits")
    assert names == ["conv_wgrad_kernel<2, 2, 2, 2, 4>"], names
    print("%d x %d x %d pixels, %d outputs: %d slabs" % (Ho, Wo, N, K * FH * FH * Cc, reached))
    assert reached == splits, (reached, splits)
    df.assert_guards_untouched("df")
    close(got(df), df_ref, what="wgrad over %d slabs, %s outputs" % (splits, bank))


def _patch_reduction(gpu, key, kernel, shape, fshape, stride, splits, seed):
    rng = np.random.default_rng(seed)
    xh, fh = rnd(rng, *shape), rnd(rng, *fshape)
    dh = rnd(rng, *O.vl_nnconv(xh, fh, None, stride=stride, pad=1).shape)
    _, df_ref, _ = O.vl_nnconv(xh, fh, None, dh, stride=stride, pad=1, acc64=True, no_der_data=True)
    x, dzdy, df = dev(xh), dev(dh), Guarded(fshape, 0, gpu)
    with forced(**{key: 1}):
        names = kernels(lambda: conv_bwd(shape, fshape, dzdy, x=x, df=df.view, stride=stride, pad=1))
        reached = dbg("wgrad_last_splits")          # (the patch launch is the last one: the generic candidates run before it)
    assert kernel in names, names
    print("%s: %d slabs" % (kernel, reached))
    assert reached == splits, (reached, splits)
    df.assert_guards_untouched("df")
    close(got(df), df_ref, what="%s over %d slabs" % (kernel, splits))


def test_wgrad_patch_split_reduction(gpu):
    """launch_wgrad_patch: 85 output columns in stages of 9 -> 10 slabs of 70 x 180"""
    _patch_reduction(gpu, "wgrad_patch", "conv_wgrad_patch_kernel<30>", (30, 17, 20, 5), (3, 3, 20, 70), 1, 10, 301705)


def test_wgrad_patch_s2_split_reduction(gpu):
    """launch_wgrad_patch_s2: 120 column segments in stages of 10 -> 12 slabs of 130 x 500"""
    _patch_reduction(gpu, "wgrad_patch_s2", "conv_wgrad_patch_s2_kernel<5, 2>", (30, 21, 20, 12), (5, 5, 20, 130), 2, 12, 302112)


# ---- bias derivative ----------------------------------------------------------------------------------------------------------
# (Ho, Wo, K, N, offset of dzdy's values) -> S
BIAS = [((32, 32, 5, 3, 0.0), 3),         # S == N: one sample per split; K = 5: three idle waves in the second finalize block
        ((32, 32, 150, 20, 0.0), 13),     # N no multiple of S: splits 0 .. 6 hold two samples, 7 .. 12 one
        ((32, 32, 3, 70, 0.0), 70),       # S > 64: the finalize wave's lanes 0 .. 5 take a second partial; K < 4: one idle wave
        ((33, 33, 5, 3, 0.0), 3),         # 1,089 positions (odd): the 4-byte arm with S > 1
        ((1, 8, 6, 300, 0.0), 1),         # FC-shaped, many samples: the flat (sample, position) index in one split
        ((32, 32, 5, 3, 1e4), 3)]         # mean >> spread: fp64 partial sums keep what an fp32 chain would lose


@pytest.mark.parametrize("case,S", BIAS)
def test_bias_derivative(gpu, case, S):
    Ho, Wo, K, N, offset = case
    rng = np.random.default_rng(Ho * 100 + K * 7 + N)
    dh = O.F(rng.standard_normal((Ho, Wo, K, N)) + offset)
    xh, fh, bh = rnd(rng, Ho, Wo, 1, N), rnd(rng, 1, 1, 1, K), rnd(rng, K)
    _, _, db_ref = O.vl_nnconv(xh, fh, bh, dh, acc64=True, no_der_data=True, no_der_filters=True)
    dzdy, db = dev(dh), Guarded((K, 1), 0, gpu)
    conv_bwd((Ho, Wo, 1, N), (1, 1, 1, K), dzdy, db=db.view)
    reached = dbg("bias_grad_last_splits")
    print("%r: S = %d" % (case, reached))
    assert reached == S, (reached, S)
    db.assert_guards_untouched("db")
    close(got(db).ravel(), db_ref.ravel(), what="dzdb %r" % (case,))


# ---- batch moments from split partial rows ------------------------------------------------------------------------------------
STATS = (64, 64, 16, 57, 9)   # H, W, C, N, K: 233,472 pixels -- above the skinny kernel's grid limit for K = 9


@functools.lru_cache(maxsize=None)
def stats_inputs():
    H, W, Cc, N, K = STATS
    rng = np.random.default_rng(646416)
    return rnd(rng, H, W, Cc, N), O.F(rng.standard_normal((1, 1, Cc, K)) * 0.25), rnd(rng, K)


@pytest.mark.parametrize("bias_offset", [0.0, 25.0])
def test_batch_moments_from_split_statistics(gpu, bias_offset):
    """conv_stats_reduce_kernel with S > 1 and conv_stats_finalize2_kernel, zero-mean and with a mean of 25 standard deviations
    (the cancellation in E[y^2] - mean^2); bounds of test_gpu_ops.test_conv_forward_with_batch_moments.  The reference
    moments are NumPy's, in fp64, over the oracle's y."""
    H, W, Cc, N, K = STATS
    xh, fh, bh = stats_inputs()
    bh = O.F(bh + bias_offset)
    y_ref = O.vl_nnconv(xh, fh, bh, acc64=True)
    y64 = y_ref.astype(np.float64).transpose(2, 0, 1, 3).reshape(K, -1)
    mean_ref, sigma_ref = y64.mean(1), np.sqrt(y64.var(1) + 1e-4)
    x, f, b = dev(xh), dev(fh), dev(col(bh))
    y, mo = Guarded((H, W, K, N), 0, gpu), Guarded((K, 2), 0, gpu)
    with forced(conv_cfg=4):                       # 64 x 64 tiles: one partial row per 64 pixels
        names = kernels(lambda: conv_fwd(x, f, b, y.view, moments=mo.view))
        reached = dbg("stats_last_splits")
    assert names == ["conv_gemm_kernel<1, 1, 2, 2, 0>"], names
    print("tile splits of the statistics: %d" % reached)
    assert reached == 4, reached
    y.assert_guards_untouched("y")
    mo.assert_guards_untouched("moments")
    close(got(y), y_ref, what="forward")
    m = got(mo)
    close(m[:, 0], mean_ref, what="mean")
    err = float(np.abs(m[:, 1] / sigma_ref - 1).max())
    assert err <= 1e-4, err
