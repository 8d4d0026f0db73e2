"""GPU parity of csrc/misc.hip at the edges of its launch arithmetic: tensors past one pass of the capped grids, operands that
are not 16-byte aligned, class counts at the limits of the per-thread arrays, logits that only the max-subtraction keeps
finite, labels outside 1..C, partial blocks and tiles of the batch-provider kernels.  Every comparison is against the CPU
oracle (oracle.oracle) or, where the oracle has no entry (softmax along dim != 3, the peak aggregator, the magnitude), against
a float64 numpy restatement written here -- never against another HIP path alone.  The bounds are those tests/test_gpu_ops.py
uses for the same operator (test_elementwise, test_losses, test_sgd_and_batch_math, test_se_tail_backward); the two new ones are
derived: vl.scale_ is one fp32 multiply (bit for bit), the magnitude is sqrtf(re * re + im * im), at most four roundings
(|got - ref| <= 1e-6 |ref| per element).

The derived quantities beside each case are recomputed from the launch code; the library's profiler hooks do not count these
kernels, so that derivation is the evidence of which branch a case reaches.  ew_grid(items) = min(ceil(items / 256), 2048) and
the 16-byte gate aligned16(...) of the launchers are csrc/norm_pool_plan.h's, checked without a GPU by
tests/norm_pool_plan_check.cpp.

Kernel / branch -> the case that reaches it, and through which condition:
  ew_kernel<OP> vec arm, second trip + tail        n = 2,100,003 aligned: n4 = 525,000 > 2,048 * 256 = 524,288 (blocks 0 .. 2 take a
                                                   second step); n % 4 = 3: the scalar tail on threads 0 .. 2; all six OPs
  ew_kernel<OP> vec arm, n4 == 0 / no tail         n = 3 (tail only), n = 4 (one quad, no tail)
  ew_kernel<OP> scalar arm (vec == 0)              the same n from a view one float past a 16-byte boundary -- x, dzdy (b), or both:
                                                   the launcher ORs the pointers; grid 2,048: ceil(2,100,003 / 524,288) = 5 trips
  scale_kernel                                     n = 1, 255, 256, 257, 4099 (block edge of 256), aligned and flat[1 : 1 + n]
  sgd_kernel vec arm, second trip + tail           n = 2,100,003 aligned (as ew_kernel)
  sgd_kernel scalar arm                            one of w, m, der one float off: 5 trips
  average_kernel                                   the same n and views (one thread per element: 8,204 blocks, the last partial)
  scale_axpy_kernel, eighth trip                   (7,7,1712,50): 4,194,400 elements / 524,288 = 8 trips; HW = 49: xm_div by a
                                                   non-power-of-two with numerators up to 4,194,399
  scale_axpy_bn_kernel scalar arm, several trips   (7,7,1712,50): HW % 4 = 1; grid = 1,048,600 / 256 + 1 + 1 = 4,098 blocks (sized for
                                                   quads) -> 4 trips over the elements
  scale_axpy_bn_kernel scalar arm, misalignment    (4,4,6,3), (8,8,5,2): HW % 4 == 0 with u, r or y one float off (vec == false)
  scale_axpy_bn_kernel vec arm                     the same two shapes aligned
  se_squeeze_bn_kernel scalar arm                  HW = 49, 3 (odd); HW % 4 == 0 with u one float off; vec arm: the same shapes aligned
  se_tail_reduce_kernel scalar arm                 HW = 49, 3; HW % 4 == 0 with y, dzdy or u one float off (the alignment gate)
  se_tail_reduce_kernel float4 arm                 (4,4,6,3), (8,8,5,2), (2,2,8,70) aligned
  se_tail_finalize_kernel, second lane step        N = 70 > 64: (2,2,8,70) (HW % 4 == 0), (1,3,5,70) (HW % 4 != 0): lanes 0 .. 5 add n + 64
  se_tail_apply_kernel<false>, second trip         (7,7,1712,50): 4,194,400 > 16,384 * 256 = 4,194,304: 96 threads of block 0 take a
                                                   second element
  se_tail_apply_kernel<false>, misalignment        HW % 4 == 0 with y, dzdy, u, dz_out or du_out one float off (the host's gate)
  se_tail_apply_kernel<true>                       the aligned HW % 4 == 0 shapes.  Its grid-stride loop is the SAME loop header as
                                                   <false> (cnt = total / 4), so its second trip (16.8 M elements) has no case
  softmaxt_kernel, softmaxt_bwd_kernel             (1,1,C,N), C = 1, 8, 64, N = 128, 129: cols = N: one full block of 128 / one thread
                                                   into a second block; (3,5,8,9): HW = 15, 135 columns; dim = 1, 2, 3, 4 of (6,8,5,4)
                                                   (HW, C, N) = (1,6,160), (6,8,20), (48,5,4), (240,4,1); T = 0.25, 2; logits 60 randn
                                                   and +-300: exp(x / T) overflows without the max-subtraction
  softmaxceloss_kernel, pt[64]                     C = 64 (the whole array), 63, 8, 1; N = 257, 513 (second / third step of the
                                                   thread-per-sample loop, one sample in it), 256, 3; logit and probability targets,
                                                   instanceWeights, dzdy = 1, 0.37; x[0] = 300, x[C - 1] = -300 in sample 0
  xm_nnsoftmaxceloss rejection                     C = 65: XM_ENOTSUP before any launch, the output keeps its fill
  nnloss_kernel                                    C = 1, 2, 8, 100 x N = 256, 257, 513; the same logits; ties of the maximum (two and
                                                   three equal, the label on the second of them); labels 0, C + 1, -3 at n = 0, N - 1 and
                                                   N / 2 (skipped: the range check)
  regloss_kernel backward, second trip             (1,1,4100,257): 1,053,700 > 4,096 * 256 = 1,048,576; forward: one block, 4,116
                                                   terms per thread; E = 4100 and (3,2,5,7): E = 30; Huber's knee at sigma = 0.5:
                                                   |d| = 4, nextafter(4, 5), nextafter(4, 3), both signs
  spec_rownorm_kernel, ok == false lanes           H = 1, 63, 65, 130 (H % 64 != 0; 130: three blocks, 2 rows in the last); W = 2, 3 (waves
                                                   2 / 3 without a column), 4, 5, 9 (a second / third column per wave)
  spec_magnitude_kernel, partial tiles             (Wo, B) = (1,1), (31,33), (33,31): b < B / j < Wo cut the 32 x 32 tile in either
                                                   direction; (32,32) exact; (300,512): 10 x 16 tiles, the last column tile 12 wide
  aggregate_logits_kernel, max_label_kernel        N = 130 segments: blocks of 64, 64, 2; max_label N = 1, 64, 65, 129
  class_stats_kernel                               C = 300: 2 C = 600 > 256 (three steps of the initialisation loop), C > 256 (two of
                                                   the write-back); N = 513: third step of the sample loop; labels 0 and C + 1"""
import ctypes as C_
import functools

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_ops import TOL, close, rnd
from test_gpu_norm_pool_edges import misaligned

pytestmark = pytest.mark.gpu

BIG_N = 2100003
FLAT_SIZES = [BIG_N, 3, 4]


def guarded(a, off):
    """device copy of the 1-D array `a` as the view flat[off : off + n] of a buffer filled with a sentinel (off = 4: 16-byte
    aligned; off = 1: one float past a boundary); returns (flat, view)"""
    import torch
    flat = torch.full((a.size + 8,), 7.25, dtype=torch.float32, device="cuda")
    v = flat[off:off + a.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a.ravel())))
    assert v.data_ptr() % 16 == (4 * off) % 16
    return flat, v


def guards_intact(flat, off, n):
    g = flat.cpu().numpy()
    return bool((g[:off] == 7.25).all() and (g[off + n:] == 7.25).all())


# ============================================ elementwise =====================================================================
@functools.lru_cache(maxsize=None)
def _ew_case(n):
    rng = np.random.default_rng(n)
    x, d, r = rnd(rng, n), rnd(rng, n), rnd(rng, n)
    xs = O.F(rng.standard_normal(n) * 30)          # both tails of the sigmoid saturate to exactly 0 and 1
    if n >= 4:
        x[0], x[n - 1], x[n - 2] = 0.0, -0.0, -1.5     # relu at +-0 and a negative in the scalar tail
    ref = {"relu": O.vl_nnrelu(x), "relu bwd": O.vl_nnrelu(x, d), "leaky": O.vl_nnrelu(x, leak=0.1),
           "leaky bwd": O.vl_nnrelu(x, d, leak=0.1), "sigmoid": O.vl_nnsigmoid(xs), "sigmoid bwd": O.vl_nnsigmoid(xs, d),
           "sum": O.sum2(x, r), "sum relu": O.sum2(x, r, relu=True)}
    if n == BIG_N:
        assert ref["sigmoid"].min() == 0.0 and ref["sigmoid"].max() == 1.0
    return x, d, r, xs, ref


@pytest.mark.parametrize("which", ["aligned", "x", "dzdy", "both"])
@pytest.mark.parametrize("n", FLAT_SIZES)
def test_elementwise_grid_stride_and_scalar_arm(gpu, n, which):
    """ew_kernel, all six operators: relu, relu backward, sum, sum + relu bit for bit; leaky relu 1e-7; sigmoid 1e-6"""
    from mcncrossmodalemotions_amd import vl
    x, d, r, xs, ref = _ew_case(n)
    mx = misaligned if which in ("x", "both") else (lambda t: t)
    md = misaligned if which in ("dzdy", "both") else (lambda t: t)
    xd, xsd, dd, rd = mx(vl.from_numpy(x)), mx(vl.from_numpy(xs)), md(vl.from_numpy(d)), md(vl.from_numpy(r))
    close(vl.to_numpy(vl.vl_nnrelu(xd)), ref["relu"], 0, "relu")
    close(vl.to_numpy(vl.vl_nnrelu(xd, dd)), ref["relu bwd"], 0, "relu bwd")
    close(vl.to_numpy(vl.vl_nnrelu(xd, leak=0.1)), ref["leaky"], 1e-7, "leaky")
    close(vl.to_numpy(vl.vl_nnrelu(xd, dd, leak=0.1)), ref["leaky bwd"], 1e-7, "leaky bwd")
    close(vl.to_numpy(vl.vl_nnsigmoid(xsd)), ref["sigmoid"], 1e-6, "sigmoid")
    close(vl.to_numpy(vl.vl_nnsigmoid(xsd, dd)), ref["sigmoid bwd"], 1e-6, "sigmoid bwd")
    close(vl.to_numpy(vl.sum2(xd, rd)), ref["sum"], 0, "sum")
    close(vl.to_numpy(vl.sum2(xd, rd, relu=True)), ref["sum relu"], 0, "sum relu")


@pytest.mark.parametrize("off", [4, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_scale_in_place(gpu, n, off):
    """vl.scale_ (xm_scale_f32) on an aligned tensor and on the slice flat[1 : 1 + n] (train.py scales parameter slices of the
    flat derivative buffer): one fp32 multiply, bit for bit np.float32(a) * x; the neighbours of the slice are untouched"""
    from mcncrossmodalemotions_amd import vl
    x = rnd(np.random.default_rng(n), n)
    flat, v = guarded(x, off)
    vl.scale_(v, 0.37)
    assert np.array_equal(v.cpu().numpy(), np.float32(0.37) * x)
    assert guards_intact(flat, off, n)


# 1e-7 * max(1, max |ref|) is below one ulp of a result in [1, 2) (1.19e-7), and the kernels' fused multiply-adds may differ from
# the oracle's separately rounded products by one ulp of the result: the inputs are drawn from (-0.95, 0.95), which keeps every
# result of both updates inside (-1, 1) (|m'| <= 0.9 * 0.95 + 5e-4 + 0.95 / 64, |w'| <= 0.95 + 1e-4, average: 0.9 * 0.95 +
# 0.1 * 0.95 / 2), where one ulp is at most 6e-8 and two are not
@functools.lru_cache(maxsize=None)
def _sgd_case():
    rng = np.random.default_rng(13)
    w, m, d = (O.F(rng.uniform(-0.95, 0.95, BIG_N)) for _ in range(3))
    w_ref, m_ref = O.sgd_update(w, m, d, 1e-4, 0.9, 5e-4, 64)
    return w, m, d, w_ref, m_ref, O.average_update(w, d, 0.1, 2)


@pytest.mark.parametrize("which", ["aligned", "w", "m", "der"])
def test_sgd_and_average_update_views(gpu, which):
    """sgd_kernel (vector arm with a second trip and a tail; scalar arm when ONE of w, m, der is one float off) and
    average_kernel, in place in views of larger buffers: results at test_sgd_and_batch_math's 1e-7, der and the elements on
    both sides of every view unchanged"""
    from mcncrossmodalemotions_amd import vl
    w, m, d, w_ref, m_ref, a_ref = _sgd_case()
    n = BIG_N
    off = {k: (1 if k == which else 4) for k in ("w", "m", "der")}
    fw, vw = guarded(w, off["w"])
    fm, vm = guarded(m, off["m"])
    fd, vd = guarded(d, off["der"])
    vl.sgd_update(vw, vm, vd, 1e-4, 0.9, 5e-4, 64)
    close(vw.cpu().numpy(), w_ref, 1e-7, "sgd w")
    close(vm.cpu().numpy(), m_ref, 1e-7, "sgd m")
    assert np.array_equal(vd.cpu().numpy(), d), "sgd changed der"
    assert guards_intact(fw, off["w"], n) and guards_intact(fm, off["m"], n) and guards_intact(fd, off["der"], n)
    fa, va = guarded(w, off["w"])
    vl.average_update(va, vd, 0.1, 2)
    close(va.cpu().numpy(), a_ref, 1e-7, "avg update")
    assert np.array_equal(vd.cpu().numpy(), d), "average update changed der"
    assert guards_intact(fa, off["w"], n) and guards_intact(fd, off["der"], n)


# ============================================ SE tail =========================================================================
SE_BIG = (7, 7, 1712, 50)
SE_LANE_SHAPES = [(2, 2, 8, 70), (1, 3, 5, 70)]
SE_GATE_SHAPES = [(4, 4, 6, 3), (8, 8, 5, 2)]


@functools.lru_cache(maxsize=None)
def _se_case(shape, train):
    """operands and oracle references exactly as test_se_tail_backward builds them"""
    H, W, C, N = shape
    rng = np.random.default_rng(H * 7 + C + int(train))
    u = O.F(rng.standard_normal(shape) * 1.3 + 0.4)
    g, b = O.F(rng.uniform(0.5, 1.5, C) * rng.choice([-1, 1], C)), rnd(rng, C)
    mom = None if train else O.F(np.stack([rng.standard_normal(C) * 0.3, rng.uniform(0.5, 1.5, C)], 1))
    x, mref = O.vl_nnbnorm(u, g, b, moments=mom, acc64=True)
    a = O.F(rng.uniform(0.05, 0.95, (1, 1, C, N)))
    s = rnd(rng, *shape)
    y = O.scale_axpy(x, a, s, relu=True)
    dzdy, dgp = rnd(rng, *shape), rnd(rng, 1, 1, C, N)
    dz_ref = O.vl_nnrelu(y, dzdy)                 # y > 0 <=> pre-activation > 0
    dx1, da_ref = O.scale_backward(x, a, dz_ref)
    dx = dx1 + O.vl_nnpool(x, (H, W), dgp, method="avg")
    du_ref, dg_ref, db_ref, _ = O.vl_nnbnorm(u, g, b, O.F(dx), moments=mom, acc64=True)
    inp = dict(u=u, g=g, b=b, mom=mref, a=a, s=s, y=y, dzdy=dzdy, dgp=dgp, x=x)
    ref = dict(gp=O.vl_nnpool(x, (H, W), method="avg"), y=y, ys=O.scale_axpy(x, a), da=da_ref, dz=dz_ref, du=du_ref, dg=dg_ref,
               db=db_ref)
    return inp, ref


def _se_check(shape, train, off=None):
    """the whole tail, forward halves and backward, with the operand named `off` one float past a 16-byte boundary ("y_out",
    "dz_out", "du_out": the outputs, through the C ABI), against the oracle at test_se_tail_backward's bounds"""
    from mcncrossmodalemotions_amd import vl, _lib
    L = _lib.load()
    H, W, C, N = shape
    inp, ref = _se_case(shape, train)

    def d(k):
        t = vl.from_numpy(inp[k])
        return misaligned(t) if k == off else t

    def out(k):
        t = vl.mat_empty(H, W, C, N)
        t.fill_(float("nan"))
        return misaligned(t) if k == off else t
    p = vl._ptr
    gd, bd, md = vl.from_numpy(inp["g"].reshape(C, 1)), vl.from_numpy(inp["b"].reshape(C, 1)), vl.from_numpy(inp["mom"])
    ud, ad, sd = d("u"), vl.from_numpy(inp["a"]), d("s")
    close(vl.to_numpy(vl.se_squeeze_bn(ud, gd, bd, md)), ref["gp"], 2e-5, "squeeze of bnorm(u)")
    yo = out("y_out")
    _lib.check(L.xm_scale_axpy_bn(p(ud), H, W, C, N, p(ad), p(sd), p(gd), p(bd), p(md), 1, p(yo), vl._stream()))
    close(vl.to_numpy(yo), ref["y"], 2e-5, "excite of bnorm(u)")
    close(vl.to_numpy(vl.scale_axpy_bn(ud, ad, None, gd, bd, md)), ref["ys"], 2e-5, "excite of bnorm(u), no shortcut")
    xd = d("x")
    close(vl.to_numpy(vl.scale_axpy(xd, ad, sd, relu=True)), ref["y"], 1e-6, "axpy")
    close(vl.to_numpy(vl.scale_axpy(xd, ad)), ref["ys"], 1e-6, "scale")
    yd, dd = d("y"), d("dzdy")
    da, sums = vl.se_tail_backward_reduce(yd, dd, ud, gd, bd, md)
    close(vl.to_numpy(da), ref["da"], TOL, "da")
    dz, du, dg, db = out("dz_out"), out("du_out"), vl.mat_empty(C, 1), vl.mat_empty(C, 1)
    _lib.check(L.xm_se_tail_backward_apply(p(yd), p(dd), p(ud), H, W, C, N, p(ad), p(vl.from_numpy(inp["dgp"])), p(gd), p(md),
                                           1 if train else 0, C_.c_void_p(sums.data_ptr()), p(dz), p(du), p(dg), p(db),
                                           vl._stream()))
    assert np.array_equal(vl.to_numpy(dz), ref["dz"])
    close(vl.to_numpy(du), ref["du"], TOL, "du")
    close(vl.to_numpy(dg).ravel(), ref["dg"], TOL, "dg")
    close(vl.to_numpy(db).ravel(), ref["db"], TOL, "db")


@pytest.mark.parametrize("train", [True, False])
def test_se_tail_past_one_pass_of_the_grid(gpu, train):
    """(7,7,1712,50): 4,194,400 elements -- scale_axpy_kernel's eighth trip, four trips of scale_axpy_bn_kernel's scalar arm, the
    second trip of se_tail_apply_kernel<false>, xm_div by 49 over the whole range"""
    _se_check(SE_BIG, train)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("shape", SE_LANE_SHAPES)
def test_se_tail_more_than_64_samples(gpu, shape, train):
    """N = 70: lanes 0 .. 5 of se_tail_finalize_kernel add a second plane"""
    _se_check(shape, train)


@pytest.mark.parametrize("off", [None, "u", "s", "x", "y", "dzdy", "y_out", "dz_out", "du_out"])
@pytest.mark.parametrize("shape", SE_GATE_SHAPES)
def test_se_tail_alignment_gates(gpu, shape, off):
    """H * W % 4 == 0: the float4 arms when every operand is aligned, the scalar arms as soon as ONE is not"""
    _se_check(shape, True, off)


# ============================================ softmax =========================================================================
def _logits(rng, shape, scale, col=0):
    """scale * randn, with +300 and -300 in one channel column (the last axis but one is the channel axis)"""
    x = O.F(rng.standard_normal(shape) * scale)
    C = shape[-2]
    x[..., 0, col] = 300.0
    x[..., C - 1, col] = -300.0
    return x


def np_softmaxt(x, T, axis):
    z = x.astype(np.float64) / T
    e = np.exp(z - z.max(axis, keepdims=True))
    return e / e.sum(axis, keepdims=True)


def np_softmaxt_backward(x, d, T, axis):
    y = np_softmaxt(x, T, axis)
    d = d.astype(np.float64)
    return y * (d - (d * y).sum(axis, keepdims=True)) / T


SOFTMAX_SHAPES = [(1, 1, C, N) for C in (1, 8, 64) for N in (128, 129)] + [(3, 5, 8, 9)]


@pytest.mark.parametrize("T", [0.25, 2.0])
@pytest.mark.parametrize("shape", SOFTMAX_SHAPES)
def test_softmaxt_block_edge_and_saturated_logits(gpu, shape, T):
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(shape[2] * 1000 + shape[3])
    x = _logits(rng, shape, 60, col=shape[3] - 1)
    dz = rnd(rng, *shape)
    xd = vl.from_numpy(x)
    y_ref = O.vl_nnsoftmaxt(x, T)
    assert np.isfinite(y_ref).all()
    close(vl.to_numpy(vl.vl_nnsoftmaxt(xd, temperature=T)), y_ref, 1e-6, "softmaxt")
    close(vl.to_numpy(vl.vl_nnsoftmaxt(xd, vl.from_numpy(dz), temperature=T)), O.vl_nnsoftmaxt_backward(x, dz, T), 1e-6,
          "softmaxt bwd")
    # the oracle against the restatement the dim != 3 cases use
    close(y_ref, np_softmaxt(x, T, 2), 1e-6, "oracle softmaxt")


@pytest.mark.parametrize("T", [0.25, 2.0])
@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_softmaxt_along_every_dim(gpu, dim, T):
    """'dim' through the (HW, C, N) view of a (6,8,5,4) tensor, forward and backward, against float64 numpy"""
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(dim)
    shape = (6, 8, 5, 4)
    x, dz = O.F(rng.standard_normal(shape) * 60), rnd(rng, *shape)
    x[0, 0, 0, 0], x[5, 7, 4, 3] = 300.0, -300.0
    xd = vl.from_numpy(x)
    close(vl.to_numpy(vl.vl_nnsoftmaxt(xd, temperature=T, dim=dim)), np_softmaxt(x, T, dim - 1), 1e-6, "softmaxt dim %d" % dim)
    close(vl.to_numpy(vl.vl_nnsoftmaxt(xd, vl.from_numpy(dz), temperature=T, dim=dim)), np_softmaxt_backward(x, dz, T, dim - 1),
          1e-6, "softmaxt bwd dim %d" % dim)


# ============================================ losses ==========================================================================
CELOSS_CASES = [(64, 257, 0.25, 60), (1, 3, 2.0, 3), (8, 513, 0.5, 200), (63, 256, 2.0, 3)]


@pytest.mark.parametrize("case", CELOSS_CASES)
def test_softmaxceloss_class_limits_and_saturated_logits(gpu, case):
    """vl_nnsoftmaxceloss forward and backward, logit and probability targets, with and without instanceWeights, at
    test_losses' 1e-6"""
    from mcncrossmodalemotions_amd import vl
    C, N, T, scale = case
    rng = np.random.default_rng(C * 1000 + N)
    x, p = _logits(rng, (1, 1, C, N), scale), O.F(rng.standard_normal((1, 1, C, N)) * scale)
    pr = O.vl_nnsoftmaxt(p, 1.0)
    w = O.F(rng.uniform(0.5, 2, (1, 1, 1, N)))
    xd = vl.from_numpy(x)
    for tgt, logit in ((p, True), (pr, False)):
        td = vl.from_numpy(tgt)
        for wt in (None, w):
            wd = None if wt is None else vl.from_numpy(wt)
            tag = "softmaxce %s targets%s" % ("logit" if logit else "probability", "" if wt is None else ", weights")
            ref = O.vl_nnsoftmaxceloss(x, tgt, temperature=T, logit_targets=logit, instance_weights=wt)
            assert np.isfinite(ref)
            got = vl.vl_nnsoftmaxceloss(xd, td, temperature=T, logitTargets=logit, instanceWeights=wd)
            close(vl.to_numpy(got).ravel()[0], ref, 1e-6, tag + " fwd")
            for dzdy in (1.0, 0.37):
                gref = O.vl_nnsoftmaxceloss(x, tgt, np.full(1, dzdy, np.float32), temperature=T, logit_targets=logit,
                                            instance_weights=wt)
                assert np.isfinite(gref).all()
                g = vl.vl_nnsoftmaxceloss(xd, td, dzdy, temperature=T, logitTargets=logit, instanceWeights=wd)
                close(vl.to_numpy(g), gref, 1e-6, tag + " bwd, dzdy %g" % dzdy)


def test_softmaxceloss_refuses_more_than_64_classes(gpu):
    """C = 65 does not fit the per-thread array: an error through _lib.check, and nothing is written"""
    import torch
    from mcncrossmodalemotions_amd import vl, _lib
    L = _lib.load()
    C, N = 65, 5
    rng = np.random.default_rng(65)
    xd, pd = vl.from_numpy(rnd(rng, 1, 1, C, N)), vl.from_numpy(rnd(rng, 1, 1, C, N))
    with pytest.raises(_lib.XmError):
        vl.vl_nnsoftmaxceloss(xd, pd, temperature=2, logitTargets=True)
    one = vl.from_numpy(np.ones((1, 1), np.float32))
    for dz in (None, one):
        y = torch.full((C * N,), 7.25, dtype=torch.float32, device=xd.device)
        rc = L.xm_nnsoftmaxceloss(vl._ptr(xd), vl._ptr(pd), C, N, 2.0, 1, None, vl._ptr(dz), vl._ptr(y), vl._stream())
        with pytest.raises(_lib.XmError):
            _lib.check(rc)
        torch.cuda.synchronize()
        assert bool((y == 7.25).all()), "the refused call wrote its output"
    # 64 is accepted by the same call
    y = torch.full((64 * N,), 7.25, dtype=torch.float32, device=xd.device)
    _lib.check(L.xm_nnsoftmaxceloss(vl._ptr(xd), vl._ptr(pd), 64, N, 2.0, 1, None, vl._ptr(one), vl._ptr(y), vl._stream()))
    assert bool((y != 7.25).all())


@pytest.mark.parametrize("N", [256, 257, 513])
@pytest.mark.parametrize("C", [1, 2, 8, 100])
def test_nnloss_ties_saturated_logits_and_labels_outside_the_classes(gpu, C, N):
    """vl_nnloss, softmaxlog and classerror, forward and backward at test_losses' 1e-6.  Ties: the first maximum is the
    prediction in kernel and oracle alike.  Labels 0, C + 1 and -3 are skipped (tests/test_oracle.py holds the oracle to a
    numpy restatement of that)."""
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(C * 1000 + N)
    x = _logits(rng, (1, 1, C, N), 60, col=7)
    lab = O.F(rng.integers(1, C + 1, (1, 1, 1, N)))
    if C >= 2:                                  # two equal maxima, the label on the second: an error
        x[0, 0, :, 10] = -1.0
        x[0, 0, 0, 10] = x[0, 0, C - 1, 10] = 5.0
        lab[0, 0, 0, 10] = C
        x[0, 0, :, 11] = x[0, 0, :, 10]         # ... the label on the first: none
        lab[0, 0, 0, 11] = 1
    if C >= 3:                                  # three equal maxima
        x[0, 0, :, 12] = -1.0
        x[0, 0, [1, 2, C - 1], 12] = 5.0
        lab[0, 0, 0, 12] = 3
        x[0, 0, :, 13] = x[0, 0, :, 12]
        lab[0, 0, 0, 13] = 2
    for n, v in ((0, 0), (N - 1, C + 1), (N // 2, -3)):
        lab[0, 0, 0, n] = v
    xd, ld = vl.from_numpy(x), vl.from_numpy(lab)
    for loss in ("softmaxlog", "classerror"):
        ref = O.vl_nnloss(x, lab, loss=loss)
        assert np.isfinite(ref)
        close(vl.to_numpy(vl.vl_nnloss(xd, ld, loss=loss)).ravel()[0], ref, 1e-6, loss)
        for dzdy in (1.0, 0.37):
            got = vl.to_numpy(vl.vl_nnloss(xd, ld, dzdy, loss=loss))
            close(got, O.vl_nnloss(x, lab, np.full(1, dzdy, np.float32), loss=loss), 1e-6, loss + " bwd")
            assert not got[0, 0, :, [0, N - 1, N // 2]].any(), "a skipped sample has a derivative"
    if C >= 3:      # the oracle's count on the four planted samples alone: 1 + 0 + 1 + 0
        errors = O.vl_nnloss(x[:, :, :, 10:14], lab[:, :, :, 10:14], loss="classerror")
        assert errors == 2
        assert vl.to_numpy(vl.vl_nnloss(vl.from_numpy(x[:, :, :, 10:14]), vl.from_numpy(lab[:, :, :, 10:14]),
                                        loss="classerror")).ravel()[0] == 2


@functools.lru_cache(maxsize=None)
def _reg_case(shape):
    rng = np.random.default_rng(shape[2])
    x, t = rnd(rng, *shape) * 3, rnd(rng, *shape) * 3
    # the two sides of Huber's knee at sigma = 0.5 (|d| > 1 / sigma^2 = 4): d = +-4, +-nextafter(4, 5), +-nextafter(4, 3)
    f4 = np.float32(4)
    knee = [f4, np.nextafter(f4, np.float32(5)), np.nextafter(f4, np.float32(3))]
    xf, tf = x.reshape(-1, order="F"), t.reshape(-1, order="F")
    last = xf.size - 1
    for k, v in enumerate(knee + [-v for v in knee]):
        for pos in (k, last - k):
            xf[pos], tf[pos] = v, 0.0
    x, t = O.F(xf.reshape(shape, order="F")), O.F(tf.reshape(shape, order="F"))
    w = O.F(rng.uniform(0.5, 2, (1, 1, 1, shape[3])))
    return x, t, w


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 4100, 257), (3, 2, 5, 7)])
def test_regression_losses_second_grid_trip_and_huber_knee(gpu, shape, weights):
    """vl_nneuclideanloss / vl_nnhuberloss at test_losses' 1e-6: a million-term forward sum in one block, a backward past
    4,096 blocks, E = 4100 and E = H W C = 30 elements per sample.  Huber's two arms meet with equal value and slope at the
    knee (2 and 1 at |d| = 4, sigma = 0.5), so the planted differences pin the loss and its derivative on both sides of it,
    not which arm `|d| > 1 / sigma^2` picks AT it"""
    from mcncrossmodalemotions_amd import vl
    x, t, w = _reg_case(shape)
    wt = w if weights else None
    xd, td, wd = vl.from_numpy(x), vl.from_numpy(t), (vl.from_numpy(w) if weights else None)
    close(vl.to_numpy(vl.vl_nneuclideanloss(xd, td, instanceWeights=wd)).ravel()[0],
          O.vl_nnregloss(x, t, kind="euclidean", instance_weights=wt), 1e-6, "euclid fwd")
    close(vl.to_numpy(vl.vl_nneuclideanloss(xd, td, 0.5, instanceWeights=wd)),
          O.vl_nnregloss(x, t, np.full(1, 0.5, np.float32), kind="euclidean", instance_weights=wt), 1e-6, "euclid bwd")
    for sg in (0.5, 0.7, 1.0):
        close(vl.to_numpy(vl.vl_nnhuberloss(xd, td, sigma=sg, instanceWeights=wd)).ravel()[0],
              O.vl_nnregloss(x, t, kind="huber", sigma=sg, instance_weights=wt), 1e-6, "huber fwd, sigma %g" % sg)
        close(vl.to_numpy(vl.vl_nnhuberloss(xd, td, 1.0, sigma=sg, instanceWeights=wd)),
              O.vl_nnregloss(x, t, np.ones(1, np.float32), kind="huber", sigma=sg, instance_weights=wt), 1e-6,
              "huber bwd, sigma %g" % sg)


# ============================================ batch provider ==================================================================
@pytest.mark.parametrize("W", [2, 3, 4, 5, 9])
@pytest.mark.parametrize("H", [1, 63, 64, 65, 130])
def test_spec_rownorm_partial_blocks(gpu, H, W):
    """rows past H in the last block of 64, and fewer / more columns than the four waves.  Every row is offset + amplitude *
    (+-(1 + 0.1 w)) + 0.1 * noise with amplitude >= 0.5: its standard deviation is of the order of its values, so the fp32
    mean and centred squares carry a few ulp (~1e-6) into the result, inside test_sgd_and_batch_math's 1e-5"""
    from mcncrossmodalemotions_amd import vl
    N = 3
    rng = np.random.default_rng(H * 10 + W)
    pat = ((-1.0) ** np.arange(W)) * (1 + 0.1 * np.arange(W))
    spec = O.F(rng.uniform(-1, 1, (H, 1, 1, N)) + rng.uniform(0.5, 2, (H, 1, 1, N)) * pat.reshape(1, W, 1, 1) +
               0.1 * rng.standard_normal((H, W, 1, N)))
    close(vl.to_numpy(vl.spec_rownorm(vl.from_numpy(spec))), O.spec_rownorm(spec), 1e-5, "rownorm")


@pytest.mark.parametrize("case", [(1, 1, 1), (31, 33, 2), (32, 32, 1), (33, 31, 3), (300, 512, 1)])
def test_spec_magnitude_partial_tiles(gpu, case):
    """xm_spec_magnitude called directly: out(b, j, n) = |reim(j, b, n) + i reim(j, B + b, n)| against np.hypot in float64,
    element by element within 1e-6 |ref| (sqrtf(re * re + im * im): four roundings at most, under 3 ulp)"""
    from mcncrossmodalemotions_amd import vl
    Wo, B, N = case
    reim = rnd(np.random.default_rng(Wo * 1000 + B), 1, Wo, 2 * B, N)
    ref = np.hypot(reim[0, :, :B, :].astype(np.float64), reim[0, :, B:, :].astype(np.float64)).transpose(1, 0, 2)
    got = vl.to_numpy(vl.spec_magnitude(vl.from_numpy(reim)))
    assert got.shape == (B, Wo, 1, N)
    err = np.abs(got[:, :, 0, :].astype(np.float64) - ref)
    assert (err <= 1e-6 * ref).all(), "worst relative error %.3e" % float((err / ref).max())


def np_peak(lg, first, last):
    """selectPeakLogit per segment: the row of the block holding its largest entry, the first one in column-major order"""
    out = []
    for f, l in zip(first, last):
        blk = lg[f - 1:min(l, lg.shape[0])]
        out.append(blk[int(np.argmax(blk.ravel(order="F"))) % blk.shape[0]])
    return np.stack(out, 1)


def test_aggregate_logits_three_blocks(gpu):
    """130 segments (blocks of 64, 64 and 2 threads) over 200 x 8 frame logits: single-row segments, segments that end past
    the last row (clamped by kernel and oracle alike), ties of the peak"""
    import torch
    from mcncrossmodalemotions_amd import vl
    Fr, E, N = 200, 8, 130
    rng = np.random.default_rng(130)
    lg = rnd(rng, Fr, E)
    first = rng.integers(1, Fr + 1, N)
    last = first + rng.integers(0, 12, N)
    last[::7] = first[::7]                               # single rows, n = 0 and n = 126 (the third block) among them
    first[5], last[5] = 50, 56
    first[6], last[6] = 101, 105
    first[128], last[128] = 195, 230                     # last > F
    first[129], last[129] = 200, 200                     # the last row alone, by the last thread
    assert (last > Fr).sum() >= 1 and (first == last).sum() >= 19
    # the maximum of segment 5 twice, in two rows and two columns: the lowest column wins, on the LATER row
    lg[49 + 5, 1] = lg[49 + 2, 6] = 50.0
    # ... of segment 6 twice in one column: the lowest row
    lg[100, 3] = lg[102, 3] = 40.0
    first, last = first.astype(np.int32), last.astype(np.int32)
    dl, df, dla = vl.from_numpy(lg), torch.from_numpy(first).cuda(), torch.from_numpy(last).cuda()
    for agg in ("max", "mean"):
        out, lab = vl.aggregate_logits(dl, df, dla, agg)
        ref = np.stack([O.aggregate_logits(lg, f, l, agg) for f, l in zip(first, last)], 1)
        close(vl.to_numpy(out).reshape(E, N, order="F"), ref, 1e-6, "aggregate " + agg)
        close(vl.to_numpy(lab).ravel(), ref.argmax(0) + 1, 0, "maxLabel " + agg)
    ref = np_peak(lg.astype(np.float64), first, last)
    assert np.array_equal(ref[:, 5], lg[54]) and np.array_equal(ref[:, 6], lg[100])
    out, lab = vl.aggregate_logits(dl, df, dla, "peak")
    close(vl.to_numpy(out).reshape(E, N, order="F"), ref, 0, "aggregate peak")
    close(vl.to_numpy(lab).ravel(), ref.argmax(0) + 1, 0, "maxLabel peak")


@pytest.mark.parametrize("C", [1, 8])
@pytest.mark.parametrize("N", [1, 64, 65, 129])
def test_max_label_block_edges(gpu, N, C):
    """[~, maxLabel] = max(x, [], 3): the first of equal maxima, as numpy's argmax"""
    from mcncrossmodalemotions_amd import vl
    x = rnd(np.random.default_rng(N * 10 + C), 1, 1, C, N)
    if C > 1:
        x[0, 0, [2, 5], 0] = 9.0                         # ties in the first and the last sample
        x[0, 0, [C - 2, C - 1], N - 1] = 9.0
    ref = x[0, 0].astype(np.float64).argmax(0) + 1
    if C > 1:
        assert ref[0] == 3 and ref[N - 1] == (C - 1 if N > 1 else 3)
    close(vl.to_numpy(vl.max_label(vl.from_numpy(x))).ravel(), ref, 0, "maxLabel")


def test_class_stats_many_classes(gpu):
    """C = 300, N = 513, two calls into the same counters; labels 0 and C + 1 count nowhere"""
    from mcncrossmodalemotions_amd import vl
    C, N = 300, 513
    rng = np.random.default_rng(300)
    correct, pop = vl.mat_zeros(C, 1), vl.mat_zeros(C, 1)
    ref_c, ref_p = np.zeros(C), np.zeros(C)
    for call in range(2):
        x = rnd(rng, 1, 1, C, N)
        lab = rng.integers(1, C + 1, N)
        pred = x[0, 0].astype(np.float64).argmax(0) + 1
        lab[:200] = pred[:200]                           # hits in classes past 256 as well
        lab[[0, 255, 256, 512]] = [0, C + 1, 0, C + 1]
        assert (lab[1:200] > 256).any()
        vl.class_stats(vl.from_numpy(x), vl.from_numpy(O.F(lab.reshape(1, 1, 1, N))), correct, pop)
        ok = (lab >= 1) & (lab <= C)
        ref_p += np.bincount(lab[ok] - 1, minlength=C)
        ref_c += np.bincount(lab[ok & (pred == lab)] - 1, minlength=C)
        assert ref_p.sum() == (call + 1) * (N - 4)
        close(vl.to_numpy(correct).ravel(), ref_c.astype(np.float32), 0, "correct")
        close(vl.to_numpy(pop).ravel(), ref_p.astype(np.float32), 0, "population")
