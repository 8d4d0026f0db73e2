"""vl_nnconv from operands that are 4-byte aligned only.  include/xmodal.h asks no more of any xm_nnconv_* pointer, so every
access wider than 4 bytes to a caller-owned tensor hangs on a host-side gate that reads the low bits of the address.  Each
case below crosses one gate in both directions: (a) with aligned operands the wide arm runs, (b) with one operand one float
(ptr % 16 == 4; for the 8-byte gates also two floats, ptr % 16 == 8, which must still be accepted) past a 16-byte boundary
it does not, and (c) what runs then agrees with the fp64-accumulate oracle under test_gpu_ops.TOL.  Destinations the
binding would allocate itself (y, dx, df, db) are views into guarded buffers (aligned_views.Guarded: 64 sentinel floats on
either side, bit-identical afterwards) handed to the C entry points through ctypes.

Evidence for (a) / (b): the profiler's kernel names (prof.kernels_run), the sign of xm_debug_get("conv_last_combine"),
the read-only keys "stats_last_splits" / "dgrad_last_transpose" / "bias_grad_last_splits"; where a choice shows in none of
them the case names the host line that makes it.

Accesses wider than 4 bytes to caller-owned tensors (x, f, b, scale, shift, gate, resid, y, dzdy, dx, dx_accum, df, db,
moments_out), by kernel, with the gate that guarantees their alignment and the case that crosses it.  b, scale, shift,
gate, df, db and moments_out are only ever read / written 4 bytes at a time (bias_grad_finalize_kernel, reduce_splits_kernel,
conv_stem_wgrad_reduce_kernel, the epilogue constants, conv_stats_*_kernel's mom[c]); a strided residual and every gather
source of the implicit GEMM (x forward, dzdy in dgrad, x in wgrad) go through 4-byte buffer loads.
  forward
    conv_gemm_kernel / conv_gemm_multi_kernel / conv_halo_kernel / conv_stem*_kernel epilogue: 16-byte stores to y, 16-byte
        loads of resid                 forward_args: vecStore = Ho*Wo % 4 == 0 && ((y | resid) & 15) == 0
                                       test_forward_gemm[y / resid]; with conv_splits 3 the sign of conv_last_combine
    conv_splitk_epilogue_kernel<true>, conv_splitk_epilogue_stats_kernel: 16-byte slab loads, resid loads, y stores
                                       launch_gemm / launch_halo: vec = a.vecStore && ... && (slab & 15) == 0
                                       test_forward_gemm[splits 3]: +3 aligned, -3 with y or resid off
    conv_gemm_kernel, A operand (16-byte loads of filter rows): a.A = f only if !need_pad
                                       conv_forward: need_pad = R % 16 != 0 || (f & 15)  -> pad_filter_kernel's copy
                                       test_forward_gemm[f], test_forward_1x1_dma[f] (pad_filter_kernel is not profiled: the
                                       line is the evidence; the DMA case shows need_pad through dma_ok)
    conv_gemm_dma_kernel: 16-byte global -> LDS loads of x and f, 16-byte-store epilogue only
                                       conv_forward: dma_ok = !need_pad && ... && (x & 15) == 0 && (f & 15) == 0;
                                       forward_args: dmaOk = dma_ok && vecStore    test_forward_1x1_dma[x / f / y]
    conv_halo_kernel, 16-byte loads of a.A: halo_setup: (a.lda & 3) || (a.A & 15) -> refuse.  a.A is the caller's f only
                                       when f is aligned (need_pad otherwise: the aligned copy), in dgrad always scratch:
                                       no caller pointer can fail this gate; test_halo_from_unaligned_operands pins that
                                       the arm still runs, on the copy, and is right
    conv_stem_kernel: 16-byte loads of x; conv_stem3_kernel: 8-byte loads of x; both only the 16-byte-store epilogue
                                       stem_shape_can: (x & 15); stem3_can: (x & 7); stem_fwd_can / stem3_can: kEpiVecStore
                                       test_stem_forward, test_stem3_forward
    fc_skinny_kernel<A, true>, fc_skinny4_kernel<A>: 16-byte loads of x and f
                                       fc_skinny_forward: vec = HW == 1 && C % 4 == 0 && ((x | f) & 15) == 0
                                       test_skinny_fc (not profiled: that line is the evidence), test_skinny_dgrad
    bn_stats_partial_kernel (the pass over y when the epilogue cannot carry the statistics): 16-byte loads of y
                                       bn_stats_vec: HW % 4 == 0 && (x & 15) == 0   [was ungated: fixed with this file]
                                       test_forward_moments[y]
  dgrad
    transpose_filter_kernel: 16-byte loads of f, stores to the scratch operand
                                       dgrad_pure_transpose: ((f | Ag) & 15) == 0   test_dgrad_filter_operand, test_skinny_dgrad[f]
    the GEMM / halo / split-K epilogues: 16-byte stores to dx, loads of dx_accum
                                       dgrad_args: vecStore = stride 1 && H*W % 4 == 0 && ((dx | dx_accum) & 15) == 0
                                       test_dgrad_gemm[dx / dx_accum] (conv_last_combine), test_dgrad_merged_strided[dx]
    fc_skinny*_kernel as dX = W' dY: 16-byte loads of dzdy (and of the scratch operand)
                                       fc_skinny_forward's vec with x = dzdy       test_skinny_dgrad[dzdy]
    conv_dgrad_s2_kernel: 8-byte loads of dzdy, 8-byte stores to dx
                                       dgrad_s2_can: ((dzdy | dx) & 7) == 0        test_dgrad_s2
  wgrad and bias
    conv_wgrad_kernel<..., AV>: 16- / 8-byte loads of dzdy
                                       wgrad_av: HW % 4 == 0 && (dY & 15) == 0 -> 4; HW % 2 == 0 && (dY & 7) == 0 -> 2; else 1
                                       test_wgrad_vector_width
    conv_stem_wgrad_kernel: 16-byte loads of x and dzdy    stem_wgrad_can: (x & 15), (dzdy & 15)     test_stem_wgrad
    conv_wgrad_patch_kernel<30>, conv_wgrad_patch_s2_kernel<5, 2>: 8-byte loads of x and dzdy
                                       wgrad_patch_can / wgrad_patch_s2_can: ((x | dzdy) & 7) == 0
                                       test_wgrad_patch, test_wgrad_patch_s2
    bias_grad_partial_kernel: 16-byte loads of dzdy
                                       xm_nnconv_backward_accum: vec = HW % 4 == 0 && (dzdy & 15) == 0
                                       [was ungated: fixed with this file]        test_bias_derivative_unaligned_dzdy
  xm_nnconv_prepare_backward launches the filter kernels of dgrad only (f: the dgrad_pure_transpose gate above)."""
import ctypes as C
import functools

import numpy as np
import pytest

from aligned_views import Guarded, misaligned
from oracle import oracle as O
from test_gpu_ops import close, rnd

pytestmark = pytest.mark.gpu


# ---- the C entry points with every destination caller-owned ---------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pad4(pad):
    return (pad,) * 4 if np.isscalar(pad) else tuple(pad)


def conv_fwd(x, f, b, y, stride=1, pad=0, scale=None, shift=None, resid=None, relu=False, moments=None):
    """xm_nnconv_forward_fused (moments: xm_nnconv_forward_moments) into the caller's y"""
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    (H, W, Cc, N), (FH, FW, FC, K) = x.shape, f.shape
    geo = (stride, stride) + _pad4(pad) + (1, 1)
    if moments is not None:
        _lib.check(L.xm_nnconv_forward_moments(_p(x), H, W, Cc, N, _p(f), FH, FW, FC, K, _p(b), _p(y), *geo, 1e-4, _p(moments),
                                               _stream()))
    else:
        _lib.check(L.xm_nnconv_forward_fused(_p(x), H, W, Cc, N, _p(f), FH, FW, FC, K, _p(b), _p(y), *geo, _p(scale), _p(shift),
                                             _p(resid), 1 if relu else 0, _stream()))


def conv_bwd(xshape, fshape, dzdy, x=None, f=None, dx=None, df=None, db=None, accum=None, stride=1, pad=0):
    """xm_nnconv_backward_accum into the caller's dx / df / db (None: not asked for)"""
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    (H, W, Cc, N), (FH, FW, FC, K) = xshape, fshape
    s = stride if isinstance(stride, tuple) else (stride, stride)
    _lib.check(L.xm_nnconv_backward_accum(_p(x), H, W, Cc, N, _p(f), FH, FW, FC, K, _p(dzdy), _p(dx), _p(df), _p(db), *s,
                                          *_pad4(pad), 1, 1, _p(accum), _stream()))


def kernels(fn):
    """names of the profiled convolution kernels `fn` launched"""
    from mcncrossmodalemotions_amd import _lib, prof
    _, rows = prof.kernels_run(fn, _lib.load())
    return [r.name for r in rows]


def dev(a, offset=0):
    """numpy array -> device tensor, `offset` floats past a 16-byte boundary"""
    from mcncrossmodalemotions_amd import vl
    t = vl.from_numpy(a)
    return misaligned(t, offset) if offset else t


def col(v):
    return v.reshape(-1, 1)


def got(g):
    from mcncrossmodalemotions_amd import vl
    return vl.to_numpy(g.view)


class forced:
    """xm_debug_set switches for the length of a `with`, restored afterwards"""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        from mcncrossmodalemotions_amd import _lib
        L = _lib.load()
        for k, v in self.kv.items():
            self.old[k] = L.xm_debug_set(k.encode(), v)
        return L

    def __exit__(self, *exc):
        from mcncrossmodalemotions_amd import _lib
        L = _lib.load()
        for k, v in self.old.items():
            L.xm_debug_set(k.encode(), v)


def dbg(key):
    from mcncrossmodalemotions_amd import _lib
    return _lib.load().xm_debug_get(key.encode())


def off_of(which, name, offset=1):
    return offset if which == name else 0


# ---- forward / dgrad / wgrad of one 3 x 3 / pad 1 layer: Ho * Wo = 48 (% 4 == 0), R = 144 (% 16 == 0) ------------------------
GEMM = (8, 6, 16, 3, 24)   # H, W, C, N, K
GEMM_CFG = 4               # 64 x 64 tiles: conv_gemm_kernel<1, 1, 2, 2, MODE>


@functools.lru_cache(maxsize=None)
def gemm_ref():
    H, W, Cc, N, K = GEMM
    rng = np.random.default_rng(20261020)
    r = {"x": rnd(rng, H, W, Cc, N), "f": rnd(rng, 3, 3, Cc, K), "b": rnd(rng, K), "sc": O.F(rng.uniform(0.5, 1.5, K)),
         "sh": rnd(rng, K), "res": rnd(rng, H, W, K, N), "dzdy": rnd(rng, H, W, K, N), "acc": rnd(rng, H, W, Cc, N)}
    y = O.vl_nnconv(r["x"], r["f"], r["b"], pad=1, acc64=True)
    r["yf"] = np.maximum(y * r["sc"].reshape(1, 1, K, 1) + r["sh"].reshape(1, 1, K, 1) + r["res"], 0)
    r["dx"], r["df"], r["db"] = O.vl_nnconv(r["x"], r["f"], r["b"], r["dzdy"], pad=1, acc64=True)
    return r


@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("which", ["none", "y", "resid", "f", "x"])
def test_forward_gemm(gpu, which, splits):
    """the implicit GEMM with its fused epilogue.  y / resid off: the scalar-store epilogue (forward_args: a.vecStore), and with
    three forced slabs conv_splitk_epilogue_kernel<false> -- conv_last_combine goes from +3 to -3.  f off: conv_forward's
    need_pad sends the filter bank through pad_filter_kernel (an aligned copy with the same values).  x off: the gather reads
    4 bytes at a time, same kernel."""
    r = gemm_ref()
    H, W, Cc, N, K = GEMM
    x, f, res = dev(r["x"], off_of(which, "x")), dev(r["f"], off_of(which, "f")), dev(r["res"], off_of(which, "resid"))
    b, sc, sh = dev(col(r["b"])), dev(col(r["sc"])), dev(col(r["sh"]))
    y = Guarded((H, W, K, N), off_of(which, "y"), gpu)
    with forced(conv_cfg=GEMM_CFG, conv_splits=splits):
        names = kernels(lambda: conv_fwd(x, f, b, y.view, pad=1, scale=sc, shift=sh, resid=res, relu=True))
        combine = dbg("conv_last_combine")
    assert names == ["conv_gemm_kernel<1, 1, 2, 2, 1>"], names
    assert combine == (0 if splits == 0 else (-3 if which in ("y", "resid") else 3)), (which, splits, combine)
    y.assert_guards_untouched("y, %s off" % which)
    close(got(y), r["yf"], what="fused forward, %s off, splits %d" % (which, splits))


@pytest.mark.parametrize("which", ["none", "dzdy", "dx", "dx_accum"])
def test_dgrad_gemm(gpu, which):
    """stride 1, H * W % 4 == 0: dgrad_args' a.vecStore reads dx | dx_accum.  Three forced slabs: conv_last_combine +3 with both
    aligned (and with dzdy off: the gather source), -3 with either off."""
    r = gemm_ref()
    H, W, Cc, N, K = GEMM
    f, dzdy, acc = dev(r["f"]), dev(r["dzdy"], off_of(which, "dzdy")), dev(r["acc"], off_of(which, "dx_accum"))
    dx = Guarded((H, W, Cc, N), off_of(which, "dx"), gpu)
    with forced(conv_cfg=GEMM_CFG, conv_splits=3):
        names = kernels(lambda: conv_bwd((H, W, Cc, N), (3, 3, Cc, K), dzdy, f=f, dx=dx.view, accum=acc, pad=1))
        combine = dbg("conv_last_combine")
    assert names == ["conv_gemm_kernel<1, 1, 2, 2, 1>"], names
    assert combine == (-3 if which in ("dx", "dx_accum") else 3), (which, combine)
    dx.assert_guards_untouched("dx, %s off" % which)
    close(got(dx), r["dx"] + r["acc"], what="dgrad + accum, %s off" % which)


@pytest.mark.parametrize("cfg", [0, 4])
@pytest.mark.parametrize("which,offset,av", [("none", 0, 4), ("dzdy", 2, 2), ("dzdy", 1, 1), ("df", 1, 4), ("db", 1, 4)])
def test_wgrad_vector_width(gpu, which, offset, av, cfg):
    """Ho * Wo % 4 == 0: wgrad_av takes 4 pixels per load from a 16-byte aligned dzdy, 2 from an 8-byte aligned one, else 1 -- the
    last template argument of conv_wgrad_kernel's name.  df and db are written 4 bytes at a time: off, nothing changes."""
    r = gemm_ref()
    H, W, Cc, N, K = GEMM
    x, dzdy = dev(r["x"]), dev(r["dzdy"], off_of(which, "dzdy", offset))
    df, db = Guarded((3, 3, Cc, K), off_of(which, "df", offset), gpu), Guarded((K, 1), off_of(which, "db", offset), gpu)
    with forced(conv_cfg=cfg):
        names = kernels(lambda: conv_bwd((H, W, Cc, N), (3, 3, Cc, K), dzdy, x=x, df=df.view, db=db.view, pad=1))
    assert len(names) == 1 and names[0].startswith("conv_wgrad_kernel<") and names[0].endswith(", %d>" % av), names
    df.assert_guards_untouched("df")
    db.assert_guards_untouched("db")
    close(got(df), r["df"], what="wgrad, %s off by %d, cfg %d" % (which, offset, cfg))
    close(got(db).ravel(), r["db"].ravel(), what="dzdb next to it")


# ---- 1 x 1 layer eligible for the LDS-DMA configurations ---------------------------------------------------------------------
DMA = (28, 28, 64, 48, 3)   # H, W, C, K, N: the first geometry of test_gpu_ops.test_lds_dma_conv_configs


@functools.lru_cache(maxsize=None)
def dma_ref():
    H, W, Cc, K, N = DMA
    rng = np.random.default_rng(28064)
    r = {"x": rnd(rng, H, W, Cc, N), "f": O.F(rng.standard_normal((1, 1, Cc, K)) * 0.2), "b": rnd(rng, K)}
    r["y"] = O.vl_nnconv(r["x"], r["f"], r["b"], acc64=True)
    return r


@pytest.mark.parametrize("which", ["none", "x", "f", "y"])
def test_forward_1x1_dma(gpu, which):
    """every LDS-DMA configuration, forced: conv_gemm_dma_kernel with aligned operands; with x or f off (conv_forward's dma_ok) or y
    off (forward_args' dmaOk needs the 16-byte-store epilogue) its register-staged base runs and no DMA kernel appears"""
    from mcncrossmodalemotions_amd import _lib
    r = dma_ref()
    H, W, Cc, K, N = DMA
    x, f, b = dev(r["x"], off_of(which, "x")), dev(r["f"], off_of(which, "f")), dev(col(r["b"]))
    ncfg = _lib.load().xm_debug_get(b"num_conv_cfgs")
    for cfg in range(ncfg - 4, ncfg):
        y = Guarded((H, W, K, N), off_of(which, "y"), gpu)
        with forced(conv_cfg=cfg):
            names = kernels(lambda: conv_fwd(x, f, b, y.view))
        assert len(names) == 1, names
        if which == "none":
            assert names[0].startswith("conv_gemm_dma_kernel<"), (cfg, names)
        else:
            assert names[0].startswith("conv_gemm_kernel<") and "dma" not in names[0], (cfg, which, names)
        y.assert_guards_untouched("y, cfg %d" % cfg)
        close(got(y), r["y"], what="1 x 1 forward, cfg %d, %s off" % (cfg, which))


# ---- forward with batch moments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias_offset", [0.0, 25.0])
@pytest.mark.parametrize("which", ["none", "y"])
def test_forward_moments(gpu, which, bias_offset):
    """MOMENT_CASES' 320-pixel geometry.  y aligned: the statistics ride in the GEMM epilogue and forward_stats_reduce runs
    (stats_last_splits == 1).  y off: no 16-byte-store epilogue, FwdStats::ok is false, the moments come from
    bn_batch_moments' pass over y (stats_last_splits == 0) -- through bn_stats_partial_kernel's 4-byte arm, which the host now
    picks from y's address.  Bounds of test_gpu_ops.test_conv_forward_with_batch_moments."""
    H, W, Cc, N, K = 20, 16, 12, 3, 100
    rng = np.random.default_rng(H * 131 + W * 17 + K)
    xh, fh, bh = rnd(rng, H, W, Cc, N), rnd(rng, 3, 3, Cc, K), O.F(rng.standard_normal(K) + bias_offset)
    y_ref = O.vl_nnconv(xh, fh, bh, pad=1, acc64=True)
    _, m_ref = O.vl_nnbnorm(y_ref, O.F(np.ones(K)), O.F(np.zeros(K)), acc64=True)
    x, f, b = dev(xh), dev(fh), dev(col(bh))
    y, mo = Guarded((H, W, K, N), off_of(which, "y"), gpu), Guarded((K, 2), 0, gpu)
    conv_fwd(x, f, b, y.view, pad=1, moments=mo.view)
    assert dbg("stats_last_splits") == (1 if which == "none" else 0)
    y.assert_guards_untouched("y")
    mo.assert_guards_untouched("moments")
    close(got(y), y_ref, what="forward + moments, %s off" % which)
    m = got(mo)
    close(m[:, 0], m_ref[:, 0], what="mean, %s off" % which)
    err = float(np.abs(m[:, 1] / m_ref[:, 1] - 1).max())
    assert err <= 1e-4, (which, bias_offset, err)


# ---- skinny fully-connected layers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["none", "x", "f"])
@pytest.mark.parametrize("K", [32, 8])
def test_skinny_fc(gpu, K, which):
    """H * W == 1, C % 4 == 0: fc_skinny4_kernel (K >= 16) / fc_skinny_kernel<A, true> (K < 16) with x and f aligned,
    fc_skinny_kernel<A, false> with either off -- fc_skinny_forward's `vec` line decides; none of them is profiled, so the
    empty list of names shows only that no implicit GEMM ran in their place"""
    from mcncrossmodalemotions_amd import vl
    Cc, N = 64, 5
    rng = np.random.default_rng(K)
    xh, fh, bh = rnd(rng, 1, 1, Cc, N), O.F(rng.standard_normal((1, 1, Cc, K)) / np.sqrt(Cc)), rnd(rng, K)
    x, f, b = dev(xh, off_of(which, "x")), dev(fh, off_of(which, "f")), dev(col(bh))
    out = []
    names = kernels(lambda: out.append(vl.vl_nnconv(x, f, b)))
    assert names == [], names
    close(vl.to_numpy(out[0]), O.vl_nnconv(xh, fh, bh, acc64=True), what="skinny fc, K %d, %s off" % (K, which))


SKINNY_DGRAD = (512, 40, 256)   # C, N, K of CONV_CASES' (1, 1, 512, 40, 1, 1, 512, 256, ...)


@functools.lru_cache(maxsize=None)
def skinny_dgrad_ref():
    Cc, N, K = SKINNY_DGRAD
    rng = np.random.default_rng(51240)
    r = {"x": rnd(rng, 1, 1, Cc, N), "f": O.F(rng.standard_normal((1, 1, Cc, K)) / np.sqrt(K)), "dzdy": rnd(rng, 1, 1, K, N)}
    r["dx"], _, _ = O.vl_nnconv(r["x"], r["f"], None, r["dzdy"], acc64=True, no_der_filters=True)
    return r


@pytest.mark.parametrize("which", ["none", "f", "dzdy", "dx"])
def test_skinny_dgrad(gpu, which):
    """dX = W' dY of an FC layer as the skinny product over the transposed filter bank (dgrad_as_skinny_fc).  f off:
    dgrad_pure_transpose is false, prep_dgrad_filter_kernel builds the operand (dgrad_last_transpose 0) and the implicit GEMM
    runs.  dzdy off: the skinny product with `vec` false.  dx off: the skinny kernels store 4 bytes at a time."""
    r = skinny_dgrad_ref()
    Cc, N, K = SKINNY_DGRAD
    f, dzdy = dev(r["f"], off_of(which, "f")), dev(r["dzdy"], off_of(which, "dzdy"))
    dx = Guarded((1, 1, Cc, N), off_of(which, "dx"), gpu)
    names = kernels(lambda: conv_bwd((1, 1, Cc, N), (1, 1, Cc, K), dzdy, f=f, dx=dx.view))
    assert dbg("dgrad_last_transpose") == (0 if which == "f" else 1)
    if which == "f":
        assert names and all(n.startswith("conv_gemm_kernel<") for n in names), names
    else:
        assert names == [], names
    dx.assert_guards_untouched("dx")
    close(got(dx), r["dx"], what="FC dgrad, %s off" % which)


@pytest.mark.parametrize("case", [(1, 1, 100, 5, 1, 1, 100, 96), (9, 8, 24, 4, 9, 1, 24, 80)])
@pytest.mark.parametrize("f_offset", [0, 1])
def test_dgrad_filter_operand(gpu, case, f_offset):
    """CONV_CASES' two FC-shaped layers with K % 16 == 0 (1 x 1, and 9 x 1 folded into the GEMM rows): the dgrad operand is a
    plain transpose.  f aligned: transpose_filter_kernel; f off: the generic prep_dgrad_filter_kernel (dgrad_pure_transpose).
    Neither kernel is profiled: dgrad_last_transpose tells them apart."""
    H, W, Cc, N, FH, FW, FC, K = case
    rng = np.random.default_rng(H * 100 + K)
    xh, fh = rnd(rng, H, W, Cc, N), rnd(rng, FH, FW, FC, K)
    y = O.vl_nnconv(xh, fh, None)
    dh = rnd(rng, *y.shape)
    dx_ref, _, _ = O.vl_nnconv(xh, fh, None, dh, acc64=True, no_der_filters=True)
    f, dzdy, dx = dev(fh, f_offset), dev(dh), Guarded((H, W, Cc, N), 0, gpu)
    conv_bwd((H, W, Cc, N), (FH, FW, FC, K), dzdy, f=f, dx=dx.view)
    assert dbg("dgrad_last_transpose") == 1 - f_offset
    dx.assert_guards_untouched("dx")
    close(got(dx), dx_ref, what="dgrad, f off by %d" % f_offset)


def test_dgrad_merged_strided(gpu):
    """MERGED_DGRAD_CASES' stride 2 x 1 layer: both stride-parity classes in one conv_gemm_multi_kernel launch, whose stores are
    strided and 4 bytes wide (dgrad_args: vecStore needs unit stride) -- dx one float off is the same launch and the same
    values"""
    H, W, Cc, N, K, stride, pad = 260, 140, 4, 4, 6, (2, 1), (1, 0, 1, 1)
    rng = np.random.default_rng(260140)
    xh, fh = rnd(rng, H, W, Cc, N), rnd(rng, 3, 3, Cc, K)
    dh = rnd(rng, *O.vl_nnconv(xh, fh, None, stride=stride, pad=pad).shape)
    dx_ref, _, _ = O.vl_nnconv(xh, fh, None, dh, stride=stride, pad=pad, acc64=True, no_der_filters=True)
    f, dzdy = dev(fh), dev(dh)
    with forced(conv_halo=0):
        for offset in (0, 1):
            dx = Guarded((H, W, Cc, N), offset, gpu)
            names = kernels(lambda: conv_bwd((H, W, Cc, N), (3, 3, Cc, K), dzdy, f=f, dx=dx.view, stride=stride, pad=pad))
            assert names and all(n.startswith("conv_gemm_multi_kernel<") for n in names), names
            dx.assert_guards_untouched("dx")
            close(got(dx), dx_ref, what="merged strided dgrad, dx off by %d" % offset)


# ---- special-purpose kernels under their force hook --------------------------------------------------------------------------
OFFSETS = [("none", 0), ("x", 1), ("x", 2), ("y", 1), ("y", 2)]


@functools.lru_cache(maxsize=None)
def stem_ref():
    H, W, N, K = 256, 20, 2, 64                    # test_gpu_ops.STEM_CASES: 5 x 5 / stride 1 / pad 2
    rng = np.random.default_rng(256 + 60 + 64 + 5)
    r = {"x": rnd(rng, H, W, 1, N), "f": rnd(rng, 5, 5, 1, K), "b": rnd(rng, K), "dzdy": rnd(rng, H, W, K, N)}
    r["y"] = O.vl_nnconv(r["x"], r["f"], r["b"], pad=2, acc64=True)
    _, r["df"], _ = O.vl_nnconv(r["x"], r["f"], r["b"], r["dzdy"], pad=2, acc64=True, no_der_data=True)
    return r


@pytest.mark.parametrize("which,offset", OFFSETS)
def test_stem_forward(gpu, which, offset):
    """conv_stem_kernel forced: stem_shape_can refuses an x that is not 16-byte aligned (one float off, and two), stem_fwd_can a
    launch without the 16-byte-store epilogue (y off either way); the implicit GEMM runs then"""
    r = stem_ref()
    x, f, b = dev(r["x"], off_of(which, "x", offset)), dev(r["f"]), dev(col(r["b"]))
    y = Guarded(r["y"].shape, off_of(which, "y", offset), gpu)
    with forced(conv_stem=1):
        names = kernels(lambda: conv_fwd(x, f, b, y.view, pad=2))
    assert any(n.startswith("conv_stem_kernel") for n in names) == (which == "none"), names
    assert which == "none" or names[-1].startswith("conv_gemm_kernel<"), names
    y.assert_guards_untouched("y")
    close(got(y), r["y"], what="stem forward, %s off by %d" % (which, offset))


@pytest.mark.parametrize("which,offset", [("none", 0), ("x", 1), ("x", 2), ("dzdy", 1), ("dzdy", 2)])
def test_stem_wgrad(gpu, which, offset):
    """conv_stem_wgrad_kernel forced: stem_wgrad_can reads x & 15 and dzdy & 15; refused, conv_wgrad_kernel runs"""
    r = stem_ref()
    H, W, _, N = r["x"].shape
    K = r["f"].shape[3]
    x, dzdy = dev(r["x"], off_of(which, "x", offset)), dev(r["dzdy"], off_of(which, "dzdy", offset))
    df = Guarded((5, 5, 1, K), 0, gpu)
    with forced(conv_stem=1):
        names = kernels(lambda: conv_bwd((H, W, 1, N), (5, 5, 1, K), dzdy, x=x, df=df.view, pad=2))
    assert any(n.startswith("conv_stem_wgrad_kernel") for n in names) == (which == "none"), names
    assert which == "none" or names[-1].startswith("conv_wgrad_kernel<"), names
    df.assert_guards_untouched("df")
    close(got(df), r["df"], what="stem wgrad, %s off by %d" % (which, offset))


@functools.lru_cache(maxsize=None)
def stem3_ref():
    H, W, N, K = 134, 256, 1, 64                   # test_gpu_ops.test_conv_stem3_kernel's second case
    rng = np.random.default_rng(H + W + N)
    r = {"x": rnd(rng, H, W, 3, N), "f": O.F(rng.standard_normal((7, 7, 3, K)) * 0.1), "b": rnd(rng, K)}
    r["y"] = O.vl_nnconv(r["x"], r["f"], r["b"], stride=2, pad=3, acc64=True)
    return r


@pytest.mark.parametrize("which,offset", OFFSETS)
def test_stem3_forward(gpu, which, offset):
    """conv_stem3_kernel forced: stem3_can reads x & 7 -- one float off is refused, two are accepted (8-byte loads) -- and wants the
    16-byte-store epilogue: y off by one float or by two is refused"""
    r = stem3_ref()
    x, f, b = dev(r["x"], off_of(which, "x", offset)), dev(r["f"]), dev(col(r["b"]))
    y = Guarded(r["y"].shape, off_of(which, "y", offset), gpu)
    with forced(conv_stem3=1):
        names = kernels(lambda: conv_fwd(x, f, b, y.view, stride=2, pad=3))
    wide = which == "none" or (which == "x" and offset == 2)
    assert any(n.startswith("conv_stem3_kernel<") for n in names) == wide, names
    assert wide or names[-1].startswith("conv_gemm_kernel<"), names
    y.assert_guards_untouched("y")
    close(got(y), r["y"], what="stem3 forward, %s off by %d" % (which, offset))


def _patch_wgrad_case(gpu, key, kernel, shape, fshape, stride, pad, which, offset, seed):
    H, W, Cc, N = shape
    K = fshape[3]
    rng = np.random.default_rng(seed)
    xh, fh = rnd(rng, *shape), rnd(rng, *fshape)
    dh = rnd(rng, *O.vl_nnconv(xh, fh, None, stride=stride, pad=pad).shape)
    _, df_ref, _ = O.vl_nnconv(xh, fh, None, dh, stride=stride, pad=pad, acc64=True, no_der_data=True)
    x, dzdy = dev(xh, off_of(which, "x", offset)), dev(dh, off_of(which, "dzdy", offset))
    df = Guarded(fshape, 0, gpu)
    with forced(**{key: 1}):
        names = kernels(lambda: conv_bwd(shape, fshape, dzdy, x=x, df=df.view, stride=stride, pad=pad))
    assert (kernel in names) == (offset != 1), (which, offset, names)
    assert any(n.startswith("conv_wgrad_kernel<") for n in names) or offset != 1, names
    df.assert_guards_untouched("df")
    close(got(df), df_ref, what="%s, %s off by %d" % (kernel, which, offset))


WG_OFFSETS = [("none", 0), ("x", 1), ("x", 2), ("dzdy", 1), ("dzdy", 2)]


@pytest.mark.parametrize("which,offset", WG_OFFSETS)
def test_wgrad_patch(gpu, which, offset):
    """conv_wgrad_patch_kernel<30> forced, WGRAD_PATCH_CASES' first shape: wgrad_patch_can reads (x | dzdy) & 7 -- one float off is
    refused (conv_wgrad_kernel runs), two are accepted"""
    _patch_wgrad_case(gpu, "wgrad_patch", "conv_wgrad_patch_kernel<30>", (30, 17, 20, 5), (3, 3, 20, 70), 1, 1, which, offset, 3017)


@pytest.mark.parametrize("which,offset", WG_OFFSETS)
def test_wgrad_patch_s2(gpu, which, offset):
    """conv_wgrad_patch_s2_kernel<5, 2> forced, WGRAD_PATCH_S2_CASES' second shape: wgrad_patch_s2_can reads (x | dzdy) & 7"""
    _patch_wgrad_case(gpu, "wgrad_patch_s2", "conv_wgrad_patch_s2_kernel<5, 2>", (30, 21, 20, 8), (5, 5, 20, 130), 2, 1, which, offset,
                      3021)


@pytest.mark.parametrize("which,offset", [("none", 0), ("dzdy", 1), ("dzdy", 2), ("dx", 1), ("dx", 2)])
def test_dgrad_s2(gpu, which, offset):
    """conv_dgrad_s2_kernel forced, DGRAD_S2_CASES' second shape: dgrad_s2_can reads (dzdy | dx) & 7 -- one float off is refused (the
    stride-parity classes through the implicit GEMM), two are accepted (8-byte loads and stores)"""
    H, W, Cc, N, K = 30, 21, 20, 3, 24
    rng = np.random.default_rng(3021 + K)
    xh, fh = rnd(rng, H, W, Cc, N), rnd(rng, 5, 5, Cc, K)
    dh = rnd(rng, *O.vl_nnconv(xh, fh, None, stride=2, pad=1).shape)
    dx_ref, _, _ = O.vl_nnconv(xh, fh, None, dh, stride=2, pad=1, acc64=True, no_der_filters=True)
    f, dzdy = dev(fh), dev(dh, off_of(which, "dzdy", offset))
    dx = Guarded((H, W, Cc, N), off_of(which, "dx", offset), gpu)
    with forced(dgrad_s2=1):
        names = kernels(lambda: conv_bwd((H, W, Cc, N), (5, 5, Cc, K), dzdy, f=f, dx=dx.view, stride=2, pad=1))
    if offset != 1:
        assert names == ["conv_dgrad_s2_kernel<1>"], names
    else:
        assert names and not any("dgrad_s2" in n for n in names), names
    dx.assert_guards_untouched("dx")
    close(got(dx), dx_ref, what="dgrad 5 x 5 / 2, %s off by %d" % (which, offset))


@pytest.mark.parametrize("which", ["none", "f", "x", "y", "dx"])
def test_halo_from_unaligned_operands(gpu, which):
    """conv_halo_kernel forced, HALO_CASES' (12, 20, 16, 2, 24) without padding (Ho * Wo = 180, R = 144): halo_setup refuses an A operand that is not 16-byte aligned, but A is
    the caller's f only when f is aligned -- otherwise the copy of pad_filter_kernel (forward) or the scratch operand (dgrad).
    So the arm keeps running whichever operand is off: on the copy (f), with 4-byte patch loads (x), with the scalar-store
    epilogue (y, dx) -- and has to be right."""
    H, W, Cc, N, K = 12, 20, 16, 2, 24
    rng = np.random.default_rng(H * 7 + W * 3 + Cc + K)
    xh, fh, bh = rnd(rng, H, W, Cc, N), rnd(rng, 3, 3, Cc, K), rnd(rng, K)
    y_ref = O.vl_nnconv(xh, fh, bh, acc64=True)
    dh = rnd(rng, *y_ref.shape)
    dx_ref, _, _ = O.vl_nnconv(xh, fh, bh, dh, acc64=True, no_der_filters=True)
    x, f, b, dzdy = dev(xh, off_of(which, "x")), dev(fh, off_of(which, "f")), dev(col(bh)), dev(dh)
    y, dx = Guarded(y_ref.shape, off_of(which, "y"), gpu), Guarded((H, W, Cc, N), off_of(which, "dx"), gpu)
    with forced(conv_halo=1):
        names = kernels(lambda: conv_fwd(x, f, b, y.view))
        assert any(n.startswith("conv_halo_kernel<") for n in names), names
        names = kernels(lambda: conv_bwd((H, W, Cc, N), (3, 3, Cc, K), dzdy, f=f, dx=dx.view))
        assert any(n.startswith("conv_halo_kernel<") for n in names), names
    y.assert_guards_untouched("y")
    dx.assert_guards_untouched("dx")
    close(got(y), y_ref, what="halo forward, %s off" % which)
    close(got(dx), dx_ref, what="halo dgrad, %s off" % which)


# ---- bias derivative ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 2])
def test_bias_derivative_unaligned_dzdy(gpu, offset):
    """Ho * Wo = 1024 (% 4 == 0) over three samples: S = 3 sample splits.  bias_grad_partial_kernel used to take 16-byte loads
    whenever Ho * Wo % 4 == 0; xm_nnconv_backward_accum now passes vec = ... && (dzdy & 15) == 0 with the matching divisor,
    so dzdy one or two floats off is summed 4 bytes at a time (that line is the evidence: the kernel is not profiled)"""
    H, W, N, K = 32, 32, 3, 6
    rng = np.random.default_rng(323236)
    dh = rnd(rng, H, W, K, N)
    dzdy, db = dev(dh, offset), Guarded((K, 1), 0, gpu)
    conv_bwd((H, W, 1, N), (1, 1, 1, K), dzdy, db=db.view)
    assert dbg("bias_grad_last_splits") == 3
    db.assert_guards_untouched("db")
    _, _, db_ref = O.vl_nnconv(rnd(rng, H, W, 1, N), rnd(rng, 1, 1, 1, K), rnd(rng, K), dh, acc64=True, no_der_data=True,
                               no_der_filters=True)
    close(got(db).ravel(), db_ref.ravel(), what="dzdb, dzdy off by %d" % offset)
