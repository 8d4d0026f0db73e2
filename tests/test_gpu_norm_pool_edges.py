"""GPU parity of csrc/norm_pool.hip at the edges of its launch arithmetic: shapes at which the sample splits are uneven, the
lane / grid-stride / plane-stride loops take a second step, the LDS-staged pooling kernel starts mid-quad, ends in its scalar
tail, cuts a plane into column groups or hands over to the one-thread-per-output kernel, and operands that are not 16-byte
aligned.  Every comparison is against the CPU oracle (fp64 accumulate for bnorm) or the numpy routing table of
tests/pool_routing.py (itself held to the oracle in tests/test_pool_routing_cpu.py), never against another HIP path alone.

Max pooling of a plain tensor copies inputs, its table is a pure function of the input, and DX adds the routed DZDY in the
oracle's own order (wo outer, ho inner, fp32, from 0): Y, the table and DX are compared BIT FOR BIT.  Average pooling and the
bnorm modes use the bounds of tests/test_gpu_ops.py (test_pool, test_bnorm, test_fused_bnorm_relu_pool).

The derived quantities beside each shape are the planning of csrc/norm_pool_plan.h (bn_splits, bn_dxsum_splits, bn_vec,
ew_grid, pool_launch, pool_lds_plan, pool_cover_2x2, bnpool_bwd_plan), which norm_pool.hip launches from; the library's
profiler hooks do not count these kernels, so tests/norm_pool_plan_check.cpp (run by tests/test_norm_pool_plan_cpu.py, no
GPU) asserts every one of them as a literal against that header: it is the evidence of which kernel and which branch a case
reaches, and it fails when a constant of the planning moves a case off its branch.

Kernel / template -> the case that reaches it, and through which condition:
  bn_stats_partial_kernel, bn_bwd_partial_kernel   S < N, uneven nper: (2,2,300,9) float4 arm, (3,1,300,9) scalar arm; run 2 and
                                                   run 1 (division by 1): (1,8,4100,3), (1,1,4100,3); unaligned x / dzdy / y
  bn_finalize_kernel, bn_bwd_finalize_kernel       S = 70 > 64 (second lane step): (3,3,8,70), (4,2,8,70)
  bn_apply_kernel<true>, bn_bwd_apply_kernel<true> 557,056 quads > 2,048 * 256 (second grid-stride trip): (64,64,32,17)
  bn_apply_kernel<false>, bn_bwd_apply_kernel<false>  HW % 4 == 0 with an unaligned operand (al == false), incl. (64,64,32,17)
  bn_bwd_apply_ch_kernel<true> / <false>           S2 = 6 != S = 3, uneven: (2,2,600,9); Sp = 70: (3,3,8,70), (4,2,8,70); <false> at
                                                   HW % 4 == 0 through an unaligned operand
  sum_partials_kernel                              S2 = 70 > 64: (3,3,8,70), (4,2,8,70)
  pool_fwd_lds_kernel<3, 3>                        plain and fused: cases a .. g1 (lead 1 .. 3: a, d, g1; tail load: a, d, g1; padding:
                                                   b, c, d; three groups: e; two groups: f; wob = 1 == Wo: g1)
  pool_fwd_kernel<3, 3>                            gate refusals g2 (maxcols < 3), g3 (wob < 4, != Wo), unaligned x, XM_NO_POOL_LDS
  pool_fwd_kernel<2, 2> / <5, 3> / <0, 0>          gy < planes / bz: (301,41) x 120 planes; bz = 4: (6,6) x 32,781 planes; <0, 0> also
                                                   with the 15 x 17 window (code 254)
  pool_bwd_kernel<true> / <false>                  the same shapes (2 x 2 / 1 -> <true>; 5 x 3 / 1, 4 x 3 / 1, 15 x 17 -> <false>)
  pool_global_kernel                               max and avg; float4 arm (8,8), (30,30); scalar arm (7,7), (1,3) and every unaligned view
  bnpool_bwd_partial_kernel, bnpool_bwd_apply_kernel    S = 2 < N = 3: (6,6,1500,3)
  bnpool_bwd_apply_patch_kernel<2,2,true> / <2,2,false> / <3,2,false>   pS = 2 < N = 3: (6,6,6000,3) / (7,6,6000,3) / (7,6,6000,3) 5 x 3 / (3,2)
  bnpool_bwd_partial_pooled_kernel                 S2 = 2 < N = 3, inverting and gathering channels: (6,6,700,3) with y_pool"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pool_routing as PR
from aligned_views import misaligned
from oracle import oracle as O
from test_gpu_ops import TOL, close, rnd, test_bnorm as _bnorm_sequence

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_pool_edges_worker.py")


def table_of(am, shape):
    return am.cpu().numpy().reshape(shape, order="F")


# ============================================ pooling =========================================================================
@functools.lru_cache(maxsize=None)
def _lds_ref(name):
    H, W, C, N, stride, pad = PR.LDS_CASES[name]
    x, dzdy = PR.lds_case_input(name)
    return {"y": O.vl_nnpool(x, PR.POOL3, stride=stride, pad=pad, method="max"),
            "am": PR.routing_table(x, PR.POOL3, stride, pad),
            "dx": O.vl_nnpool(x, PR.POOL3, dzdy, stride=stride, pad=pad, method="max")}


def _assert_bits(got, name, tag):
    ref = _lds_ref(name)
    for k, r in (("y", "y"), ("y2", "y"), ("am", "am"), ("dx", "dx"), ("dx2", "dx")):
        assert got[k].shape == ref[r].shape, (tag, name, k)
        bad = int((got[k] != ref[r]).sum())
        assert bad == 0, "%s, case %s: %s differs from the reference at %d of %d places" % (tag, name, k, bad, ref[r].size)


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("name", sorted(PR.LDS_CASES))
def test_pool3_lds_geometries(gpu, name, unaligned):
    """cases (a) .. (g3) of PR.LDS_CASES.  Aligned: pool_fwd_lds_kernel<3, 3> for a .. g1, pool_fwd_kernel<3, 3> for g2, g3 (the
    gate's two refusals).  From a view one float past a 16-byte boundary the gate must refuse all of them, and
    pool_fwd_kernel<3, 3> / pool_bwd_kernel<true> run with an offset base."""
    import _pool_edges_worker as worker
    from mcncrossmodalemotions_amd import vl
    got = worker.run_case(vl, name, misaligned if unaligned else None)
    _assert_bits(got, name, "unaligned view" if unaligned else "aligned")


def test_pool3_lds_geometries_with_the_lds_kernel_off(gpu, tmp_path):
    """the same cases in ONE fresh child process with XM_NO_POOL_LDS=1 (the selectors are read once per process): the
    one-thread-per-output kernel at the shapes of the LDS kernel, against the same references"""
    out = str(tmp_path / "pool_edges.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("XM_NO_")}
    env["XM_NO_POOL_LDS"] = "1"
    r = subprocess.run([sys.executable, WORKER, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    res = dict(np.load(out))
    for name in sorted(PR.LDS_CASES):
        _assert_bits({k: res[name + "_" + k] for k in ("y", "y2", "am", "dx", "dx2")}, name, "XM_NO_POOL_LDS=1")


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("name", sorted(PR.LDS_CASES))
def test_fused_bnorm_relu_pool_lds_geometries(gpu, name, train, unaligned):
    """vl.bnorm_relu_pool over the same geometries (the fused mode of the same two kernels) against the oracle's
    vl_nnpool(vl_nnrelu(vl_nnbnorm(x))): forward at TOL; the table equal to the table of the oracle's tensor except in windows
    whose two largest values differ by less than the forward bound -- counted, at most 0.1 % of the windows (the seeds keep
    the oracle's own fp32 arithmetic under that cap: tests/test_pool_routing_cpu.py)."""
    from mcncrossmodalemotions_amd import vl
    H, W, C, N, stride, pad = PR.LDS_CASES[name]
    x, g, b, mom = PR.fused_case_input(name, train)
    yb, mref = O.vl_nnbnorm(x, g, b, moments=mom, acc64=True)
    yr = np.maximum(yb, 0)
    yp = O.vl_nnpool(yr, PR.POOL3, stride=stride, pad=pad, method="max")
    xd = vl.from_numpy(x)
    if unaligned:
        xd = misaligned(xd)
    md = None if mom is None else vl.from_numpy(mom)
    y, am, mo = vl.bnorm_relu_pool(xd, vl.from_numpy(g.reshape(C, 1)), vl.from_numpy(b.reshape(C, 1)), PR.POOL3, stride=stride,
                                   pad=pad, moments=md)
    close(vl.to_numpy(y), yp, what="fused fwd")
    close(vl.to_numpy(mo), mref, what="fused moments")
    tie = PR.near_tie_windows(yr, PR.POOL3, stride, pad, TOL)
    print("case %s: %d near-tie windows of %d" % (name, int(tie.sum()), tie.size))
    assert tie.sum() <= 1e-3 * tie.size, (int(tie.sum()), tie.size)
    table, got = PR.routing_table(yr, PR.POOL3, stride, pad), table_of(am, yp.shape)
    bad = int((got[~tie] != table[~tie]).sum())
    assert bad == 0, "table differs in %d windows that are no near-ties" % bad


# pool_launch(rows, cols, planes) of csrc/norm_pool_plan.h (the figures below are asserted in tests/norm_pool_plan_check.cpp):
# bx = pow2 >= rows (<= 256), by = pow2 >= cols (<= 256 / bx), bz = 256 / (bx by);
# gx = ceil(cols / by), gz = ceil(rows / bx), gy = min(max(1, 8192 / (gx gz)), ceil(planes / bz)): a block strides over planes
# iff gy < ceil(planes / bz).  (301, 41) x 120 planes, stride 1 -- forward launch over the outputs, backward over the inputs:
#   2 x 2: Ho x Wo = 300 x 40: bx 256, by 1, bz 1, gx 40, gz 2 -> gy = 102 < 120    pool_fwd_kernel<2, 2>, pool_bwd_kernel<true>
#   5 x 3: 297 x 39: gx 39, gz 2 -> gy = 105 < 120                                  pool_fwd_kernel<5, 3>, pool_bwd_kernel<false>
#   4 x 3: 298 x 39: gy = 105 < 120                                                 pool_fwd_kernel<0, 0>, pool_bwd_kernel<false>
#   backward: rows x cols = 301 x 41: gx 41, gz 2 -> gy = 99 < 120
PLANE_STRIDE_SHAPE = (301, 41, 40, 3)
# tiny outputs: (6, 6) -> 5 x 5: bx 8, by 8, bz 4 (forward and backward alike), gx = gz = 1, gy = min(8192, ceil(32781 / 4) = 8196):
# blocks 0 .. 3 take a second step of 8192 * 4 planes, the last one with planes 32780 only (threadIdx.z 1 .. 3 past the end)
PACKED_SHAPE = (6, 6, 4683, 7)


@pytest.mark.parametrize("case", [(PLANE_STRIDE_SHAPE, (2, 2), "max"), (PLANE_STRIDE_SHAPE, (2, 2), "avg"),
                                  (PLANE_STRIDE_SHAPE, (5, 3), "max"), (PLANE_STRIDE_SHAPE, (5, 3), "avg"),
                                  (PLANE_STRIDE_SHAPE, (4, 3), "max"), (PLANE_STRIDE_SHAPE, (4, 3), "avg"),
                                  (PACKED_SHAPE, (2, 2), "max"), (PACKED_SHAPE, (2, 2), "avg")])
def test_pool_plane_stride_loops(gpu, case):
    """pool_fwd_kernel / pool_bwd_kernel with more planes than gridDim.y * blockDim.z: `plane += gridDim.y * blockDim.z`"""
    from mcncrossmodalemotions_amd import vl
    (H, W, C, N), pool, method = case
    x = PR.planted_input(H + C, H, W, C, N, pool)
    y_ref = O.vl_nnpool(x, pool, method=method)
    dzdy = rnd(np.random.default_rng(C), *y_ref.shape)
    dx_ref = O.vl_nnpool(x, pool, dzdy, method=method)
    xd, dd = vl.from_numpy(x), vl.from_numpy(dzdy)
    y = vl.to_numpy(vl.vl_nnpool(xd, pool, method=method))
    dx = vl.to_numpy(vl.vl_nnpool(xd, pool, dd, method=method))
    y2, am = vl.vl_nnpool(xd, pool, method=method, want_argmax=True)
    dx2 = vl.to_numpy(vl.vl_nnpool(xd, pool, dd, method=method, argmax=am))
    if method == "max":
        assert np.array_equal(y, y_ref) and np.array_equal(vl.to_numpy(y2), y_ref)
        assert np.array_equal(table_of(am, y_ref.shape), PR.routing_table(x, pool))
        assert np.array_equal(dx, dx_ref) and np.array_equal(dx2, dx_ref)
    else:
        assert am is None
        close(y, y_ref, 1e-6, "pool fwd")
        close(vl.to_numpy(y2), y_ref, 1e-6, "pool fwd (argmax variant)")
        close(dx, dx_ref, 1e-5, "pool bwd")
        close(dx2, dx_ref, 1e-5, "pool bwd (argmax variant)")


# pool_global_kernel (window = plane, no padding, no table): one wave per plane, 4 planes per block; float4 loads iff
# HW % 4 == 0 and the PLANE's address is 16-byte aligned
GLOBAL_SHAPES = [(7, 7, 5, 3),       # HW = 49: scalar arm; 15 planes: the last block holds 3
                 (8, 8, 6, 3),       # HW = 64: vector arm, 16 quads (lanes 16 .. 63 idle); scalar arm from the unaligned view
                 (1, 3, 7, 1),       # HW = 3 < 64: most lanes have nothing
                 (30, 30, 3, 3)]     # HW = 900: 225 quads, 4 steps of the lane loop (15 scalar steps unaligned)


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("method", ["max", "avg"])
@pytest.mark.parametrize("shape", GLOBAL_SHAPES)
def test_pool_global(gpu, shape, method, unaligned):
    from mcncrossmodalemotions_amd import vl
    H, W, C, N = shape
    rng = np.random.default_rng(H * 100 + W + C)
    x = rnd(rng, *shape)
    x[H - 1, W - 1, 0, 0] = 9.0            # a maximum in the last element of the first plane, one below zero in the last
    x[:, :, C - 1, N - 1] = -np.abs(x[:, :, C - 1, N - 1]) - 1
    y_ref = O.vl_nnpool(x, [H, W], method=method)
    xd = vl.from_numpy(x)
    if unaligned:
        xd = misaligned(xd)
    y = vl.to_numpy(vl.vl_nnpool(xd, [H, W], method=method))
    if method == "max":
        assert np.array_equal(y, y_ref)
    else:
        close(y, y_ref, 1e-6, "global avg")
    if H * W <= 255 or method == "avg":
        dzdy = rnd(rng, 1, 1, C, N)
        dx_ref = O.vl_nnpool(x, [H, W], dzdy, method=method)
        dx = vl.to_numpy(vl.vl_nnpool(xd, [H, W], vl.from_numpy(dzdy), method=method))
        if method == "max":
            assert np.array_equal(dx, dx_ref)
        else:
            close(dx, dx_ref, 1e-5, "global avg bwd")


def test_pool_window_limit_and_refusals(gpu):
    """the table is one byte per output: 255 window elements are the most it encodes"""
    from mcncrossmodalemotions_amd import vl, _lib
    rng = np.random.default_rng(15)
    x = PR.planted_input(3, 16, 18, 2, 2, (15, 17))
    x[14, 16, 0, 0] = 9.0                  # window (0, 0): its last tap, code 14 + 15 * 16 = 254
    x[15, 17, 1, 1] = 9.0                  # window (1, 1): again 254; windows (0, 1), (1, 0): 239 + ..., 253
    xd = vl.from_numpy(x)
    y_ref = O.vl_nnpool(x, [15, 17], method="max")
    table = PR.routing_table(x, [15, 17])
    assert table.max() == 254
    y, am = vl.vl_nnpool(xd, [15, 17], method="max", want_argmax=True)
    assert np.array_equal(vl.to_numpy(y), y_ref)
    assert np.array_equal(table_of(am, y_ref.shape), table)
    dzdy = rnd(rng, *y_ref.shape)
    dx_ref = O.vl_nnpool(x, [15, 17], dzdy, method="max")
    assert np.array_equal(vl.to_numpy(vl.vl_nnpool(xd, [15, 17], vl.from_numpy(dzdy), method="max")), dx_ref)
    assert np.array_equal(vl.to_numpy(vl.vl_nnpool(xd, [15, 17], vl.from_numpy(dzdy), method="max", argmax=am)), dx_ref)
    with pytest.raises(_lib.XmError):      # 256 elements
        vl.vl_nnpool(vl.from_numpy(rnd(rng, 16, 16, 2, 2)), [16, 16], method="max", want_argmax=True)
    # bnorm_relu_pool_backward reads at most 2 x 2 covering windows: ceil(5 / 2) = 3 is refused
    C = 3
    xb = vl.from_numpy(rnd(rng, 13, 9, C, 2))
    gd, bd = vl.from_numpy(O.F(np.ones((C, 1)))), vl.from_numpy(O.F(np.zeros((C, 1))))
    yp, am, mo = vl.bnorm_relu_pool(xb, gd, bd, [5, 3], stride=[2, 1])
    with pytest.raises(_lib.XmError):
        vl.bnorm_relu_pool_backward(xb, gd, bd, mo, am, vl.from_numpy(rnd(rng, *yp.shape)), [5, 3], stride=[2, 1])


# bnpool_bwd_plan of csrc/norm_pool_plan.h (the figures below are asserted in tests/norm_pool_plan_check.cpp):
# element kernels: bx = pow2 >= H, by = pow2 >= W (<= 256 / bx), S = min(N, 4096 / (C gx gz)); patch kernel
# (strides 2 x 2 and 3 x 2): KH = (H + pt + sy - 1) / sy, KW likewise, pS = min(N, 16384 / (C pgx pgz)); pooled sums (y_pool
# given): S2 = bn_splits = min(N, 2048 / C).  All planes here fit one block (gx = gz = pgx = pgz = 1), N = 3:
# (H, W, C, N, pool, stride, pad, with y_pool)
SPLIT_CASES = [
    # S = 4096 / 1500 = 2 < 3 in bnpool_bwd_partial_kernel (samples 0, 2 | 1); apply: patch <2, 2, true> with pS = 3
    (6, 6, 1500, 3, (3, 3), (2, 2), 0, False),
    # stride 1: no patch kernel -> bnpool_bwd_apply_kernel with S = 2 as well
    (6, 6, 1500, 3, (2, 2), (1, 1), (1, 0, 1, 0), False),
    # pS = 16384 / 6000 = 2 < 3 (S = 1): bnpool_bwd_apply_patch_kernel<2, 2, true> (H, pt even)
    (6, 6, 6000, 3, (3, 3), (2, 2), 0, False),
    # ... <2, 2, false>: odd H
    (7, 6, 6000, 3, (3, 3), (2, 2), 0, False),
    # ... <3, 2, false>: KH = KW = 3
    (7, 6, 6000, 3, (5, 3), (3, 2), 0, False),
    # S2 = 2048 / 700 = 2 < 3 in bnpool_bwd_partial_pooled_kernel, both of its arms (channel 0 gathers x)
    (6, 6, 700, 3, (3, 3), (2, 2), 0, True),
]


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("case", SPLIT_CASES)
def test_fused_backward_uneven_sample_splits(gpu, case, train):
    """vl.bnorm_relu_pool_backward where a block walks samples sp, sp + S, ... with S < N and N % S != 0, against the oracle
    composition of test_fused_bnorm_relu_pool at its tolerances, dxsum_out included"""
    from mcncrossmodalemotions_amd import vl
    H, W, C, N, pool, stride, pad, pooled = case
    rng = np.random.default_rng(H * 1000 + C + 7 * pool[0] + int(train))
    x = O.F(rng.standard_normal((H, W, C, N)) * 1.5 + 0.3)
    g, b = O.F(rng.uniform(0.5, 1.5, C) * rng.choice([-1, 1], C)), rnd(rng, C)
    g[0] = 1e-4 * np.sign(g[0])       # |b| > 100 |g|: the pooled-domain sums must gather x for this channel
    b[0] = 0.5
    mom = None if train else O.F(np.stack([rng.standard_normal(C) * 0.3, rng.uniform(0.5, 1.5, C)], 1))
    yb, mref = O.vl_nnbnorm(x, g, b, moments=mom, acc64=True)
    yr = np.maximum(yb, 0)
    yp = O.vl_nnpool(yr, pool, stride=stride, pad=pad, method="max")
    dz = rnd(rng, *yp.shape)
    dyr = O.vl_nnpool(yr, pool, dz, stride=stride, pad=pad, method="max")
    dx_ref, dg_ref, db_ref, _ = O.vl_nnbnorm(x, g, b, dyr * (yb > 0), moments=mom, acc64=True)
    xd, gd, bd = vl.from_numpy(x), vl.from_numpy(g.reshape(C, 1)), vl.from_numpy(b.reshape(C, 1))
    md = None if mom is None else vl.from_numpy(mom)
    y, am, mo = vl.bnorm_relu_pool(xd, gd, bd, pool, stride=stride, pad=pad, moments=md)
    close(vl.to_numpy(y), yp, what="fused fwd")
    close(vl.to_numpy(mo), mref, what="fused moments")
    dxs = vl.mat_zeros(C, 1)
    dx, dg, db = vl.bnorm_relu_pool_backward(xd, gd, bd, mo, am, vl.from_numpy(dz), pool, stride=stride, pad=pad, train=train,
                                             dxsum_out=dxs, y_pool=y if pooled else None)
    close(vl.to_numpy(dx), dx_ref, what="fused dx")
    close(vl.to_numpy(dxs).ravel(), dx_ref.astype(np.float64).sum((0, 1, 3)), 2e-4, what="fused dxsum")
    close(vl.to_numpy(dg).ravel(), dg_ref, what="fused dg")
    close(vl.to_numpy(db).ravel(), db_ref, what="fused db")


# ============================================ bnorm ===========================================================================
# S = bn_splits(C, N) = min(N, 2048 / C): block (c, s) reduces samples s, s + S, ...: nper = (N - s + S - 1) / S of them, walked
# as one flat index of nper * run positions, run = HW / 4 quads (HW % 4 == 0) or HW elements.  S2 = min(N, 4096 / C) blocks per
# channel in bn_bwd_apply_ch_kernel (dxsum path).  Finalize kernels: lane l adds partials l, l + 64, ...
BN_EDGE_SHAPES = [
    (2, 2, 300, 9),       # S = 6: nper = 2, 2, 2, 1, 1, 1 (uneven), vector arm, run = 1; S2 = 9
    (3, 1, 300, 9),       # the same on the scalar arm, run = 3
    (2, 2, 600, 9),       # S = 3 (nper = 3), S2 = 6 (nper = 2, 2, 2, 1, 1, 1): S and S2 differ, both below N
    (1, 8, 4100, 3),      # C > 4096: S = S2 = 1, nper = 3: the FC-shaped layers' run length of 2 quads
    (1, 1, 4100, 3),      # run length 1 on the scalar arm: the magic division by 1
    (3, 3, 8, 70),        # S = S2 = 70 > 64: lanes 0 .. 5 of the finalize / sum_partials loops take a second step; Sp = 70
    (4, 2, 8, 70),        # the same on the vector arm
    (64, 64, 32, 17),     # 557,056 quads > 2,048 blocks * 256: a second trip of the grid-stride loop in bn_apply_kernel<true> and
]                         # bn_bwd_apply_kernel<true> (the scalar arms: test_bnorm_unaligned_operands); S = S2 = 17


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", BN_EDGE_SHAPES)
def test_bnorm_launch_edges(gpu, shape, relu):
    """test_bnorm's whole sequence -- forward and moments, relu, train backward, backward with the forward's moments (bit-equal),
    the dxsum path, test mode -- with its tolerances, against oracle.vl_nnbnorm(acc64=True)"""
    _bnorm_sequence(gpu, shape, relu)


@functools.lru_cache(maxsize=None)
def _bn_case(shape):
    from mcncrossmodalemotions_amd import vl
    H, W, C, N = shape
    rng = np.random.default_rng(H * 1000 + W * 100 + C * 10 + N)
    x = O.F(rng.standard_normal(shape) * 2.0 + 3.0)
    g, b = O.F(rng.uniform(0.5, 1.5, C)), rnd(rng, C)
    dzdy = rnd(rng, *shape)
    y_ref, m_ref = O.vl_nnbnorm(x, g, b, acc64=True)
    y_ref = np.maximum(y_ref, 0)
    dx_ref, dg_ref, db_ref, _ = O.vl_nnbnorm(x, g, b, dzdy * (y_ref > 0), acc64=True)
    dev = {"x": vl.from_numpy(x), "g": vl.from_numpy(g.reshape(C, 1)), "b": vl.from_numpy(b.reshape(C, 1)),
           "dzdy": vl.from_numpy(dzdy)}
    dev["y"], dev["m"] = vl.vl_nnbnorm(dev["x"], dev["g"], dev["b"], relu=True)
    close(vl.to_numpy(dev["y"]), y_ref, what="bn fwd")
    close(vl.to_numpy(dev["m"]), m_ref, what="bn moments")
    base = _bn_backward_raw(dev, dict(dev, dx_out=vl.mat_empty(*shape)))
    close(base["dx"], dx_ref, what="bn dx")
    close(base["dx3"], dx_ref, what="bn dx (dxsum path)")
    close(base["dg"].ravel(), dg_ref, what="bn dg")
    close(base["db"].ravel(), db_ref, what="bn db")
    return dev, base, dx_ref


def _bn_backward_raw(dev, ops):
    """train-mode backward through the C ABI with every operand (DX included) supplied by the caller: the fused-relu entry with
    the forward's moments, then the dxsum entry"""
    from mcncrossmodalemotions_amd import vl, _lib
    L = _lib.load()
    H, W, C, N = [int(v) for v in ops["x"].shape]
    p = vl._ptr
    out = {}
    dg, db, mo, dxs = vl.mat_empty(C, 1), vl.mat_empty(C, 1), vl.mat_empty(C, 2), vl.mat_empty(C, 1)
    flags = 1 | 2          # XM_FUSE_RELU | XM_BN_BATCH_MOMENTS
    _lib.check(L.xm_nnbnorm_backward_fused(p(ops["x"]), p(ops["y"]), H, W, C, N, p(dev["g"]), p(dev["b"]), p(ops["dzdy"]), 1e-4,
                                           p(dev["m"]), p(ops["dx_out"]), p(dg), p(db), p(mo), flags, vl._stream()))
    out["dx"], out["dg"], out["db"] = vl.to_numpy(ops["dx_out"]), vl.to_numpy(dg), vl.to_numpy(db)
    ops["dx_out"].fill_(float("nan"))
    _lib.check(L.xm_nnbnorm_backward_dxsum(p(ops["x"]), p(ops["y"]), H, W, C, N, p(dev["g"]), p(dev["b"]), p(ops["dzdy"]), 1e-4,
                                           p(dev["m"]), p(ops["dx_out"]), p(dg), p(db), p(mo), p(dxs), flags, vl._stream()))
    out["dx3"], out["dg3"], out["db3"], out["dxs"] = (vl.to_numpy(ops["dx_out"]), vl.to_numpy(dg), vl.to_numpy(db),
                                                      vl.to_numpy(dxs))
    return out


@pytest.mark.parametrize("which", ["x", "dzdy", "y", "dx_out"])
@pytest.mark.parametrize("shape", [(2, 2, 300, 9), (4, 2, 8, 70), (64, 64, 32, 17)])
def test_bnorm_unaligned_operands(gpu, shape, which):
    """H * W % 4 == 0 with ONE operand one float past a 16-byte boundary: bn_apply_kernel<false>, bn_bwd_apply_kernel<false> and
    bn_bwd_apply_ch_kernel<false> at plane sizes that otherwise take the float4 arms (at (64, 64, 32, 17) with several trips of
    the grid-stride loop).  The reductions walk the same quads in the same order and both apply arms evaluate the same
    expression per element, so Y, the moments, DX, DG and DB must equal the aligned run bit for bit (and through it the
    oracle within TOL); the sum(DX) partials are cut differently between the two arms and keep test_bnorm's bounds."""
    from mcncrossmodalemotions_amd import vl
    H, W, C, N = shape
    dev, base, dx_ref = _bn_case(shape)
    ops = dict(dev, dx_out=vl.mat_empty(*shape))
    if which == "dx_out":
        ops["dx_out"] = misaligned(ops["dx_out"])
    else:
        ops[which] = misaligned(dev[which])
    if which == "x":
        y, m = vl.vl_nnbnorm(ops["x"], dev["g"], dev["b"], relu=True)
        assert np.array_equal(vl.to_numpy(y), vl.to_numpy(dev["y"])), "bn fwd from an unaligned x"
        assert np.array_equal(vl.to_numpy(m), vl.to_numpy(dev["m"])), "moments from an unaligned x"
        mom = O.F(np.stack([np.linspace(-1, 1, C), np.linspace(0.5, 1.5, C)], 1))
        yt, _ = vl.vl_nnbnorm(ops["x"], dev["g"], dev["b"], moments=vl.from_numpy(mom))
        yt0, _ = vl.vl_nnbnorm(dev["x"], dev["g"], dev["b"], moments=vl.from_numpy(mom))
        assert np.array_equal(vl.to_numpy(yt), vl.to_numpy(yt0)), "test-mode fwd from an unaligned x"
    got = _bn_backward_raw(dev, ops)
    for k in ("dx", "dg", "db", "dx3", "dg3", "db3"):
        bad = int((got[k] != base[k]).sum())
        assert bad == 0, "%s differs from the aligned run at %d places (%s unaligned)" % (k, bad, which)
    dxs = got["dxs"].ravel().astype(np.float64)
    scale = max(1.0, np.abs(dx_ref).max()) * np.sqrt(H * W * N)
    assert np.abs(dxs - got["dx3"].astype(np.float64).sum(axis=(0, 1, 3))).max() <= 1e-6 * scale
    assert np.abs(dxs - dx_ref.astype(np.float64).sum(axis=(0, 1, 3))).max() <= 1e-5 * scale
