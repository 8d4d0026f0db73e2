"""Host-side mirror of the MatConvNet / mcnExtraLayers operator API, over the HIP C ABI.

Same names, argument meaning and error behaviour as the MATLAB operators the reference's
graphs execute:

    y            = vl_nnconv(x, f, b, stride=.., pad=.., dilate=..)
    dx, df, db   = vl_nnconv(x, f, b, dzdy, ...)           # backward when dzdy is given
    y            = vl_nnpool(x, pool, stride=.., pad=.., method='max'|'avg')
    y[, moments] = vl_nnbnorm(x, g, b, epsilon=1e-4, moments=M)
    ...

Tensors are torch float32 CUDA tensors in MATLAB layout: logical shape (H, W, C, N) with
column-major strides (H fastest) -- create them with `mat_empty/mat_zeros/from_numpy`.
torch is used for device memory and streams only; every operator below is one or more
hand-written HIP kernels from libxmodal_hip.so.  There is no CPU / eager fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

# --------------------------------------------------------------------------------------------
# MATLAB-layout tensor helpers
# --------------------------------------------------------------------------------------------


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


XM_ENOTSUP = 5   # include/xmodal.h


def mat_empty(*shape, device=None):
    """uninitialised `single` array of MATLAB shape `shape` (column-major)."""
    shape = tuple(int(s) for s in (shape[0] if len(shape) == 1 and not np.isscalar(shape[0]) else shape))
    t = torch.empty(tuple(reversed(shape)), dtype=torch.float32, device=device or _dev())
    return t.permute(*reversed(range(len(shape))))


def mat_zeros(*shape, device=None):
    t = mat_empty(*shape, device=device)
    t.zero_()
    return t


def from_numpy(a, device=None):
    """numpy array (any order) -> device tensor with MATLAB (column-major) layout."""
    a = np.asarray(a, dtype=np.float32)
    ct = np.ascontiguousarray(a.transpose(*reversed(range(a.ndim))))
    t = torch.from_numpy(ct).to(device or _dev())
    return t.permute(*reversed(range(a.ndim)))


def to_numpy(t):
    """device tensor in MATLAB layout -> numpy Fortran-ordered array of the same shape."""
    c = t.permute(*reversed(range(t.dim()))).contiguous().cpu().numpy()
    return np.asfortranarray(c.transpose(*reversed(range(c.ndim))))


def is_mat(t):
    return t.permute(*reversed(range(t.dim()))).is_contiguous()


def _chk(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch tensor" % name)
    if t.dtype != torch.float32:
        raise TypeError("%s: expected single precision (float32), got %s" % (name, t.dtype))
    if not t.is_cuda:
        raise RuntimeError("%s: tensor is not on the GPU; this build has no CPU path" % name)
    if not is_mat(t):
        raise ValueError("%s: tensor is not in MATLAB column-major layout" % name)
    return t


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _shape4(t):
    s = tuple(t.shape) + (1,) * (4 - t.dim())
    if len(s) != 4:
        raise ValueError("expected an array with at most 4 dimensions, got %r" % (tuple(t.shape),))
    return [int(v) for v in s]


def _pair(v, name):
    if np.isscalar(v):
        return int(v), int(v)
    v = list(v)
    if len(v) == 1:
        return int(v[0]), int(v[0])
    if len(v) != 2:
        raise ValueError("%s must have 1 or 2 elements" % name)
    return int(v[0]), int(v[1])


def _pad4(pad):
    if np.isscalar(pad):
        return (int(pad),) * 4
    pad = list(pad)
    if len(pad) == 1:
        return (int(pad[0]),) * 4
    if len(pad) == 2:
        return int(pad[0]), int(pad[0]), int(pad[1]), int(pad[1])
    if len(pad) != 4:
        raise ValueError("PAD must have 1, 2 or 4 elements")
    return tuple(int(v) for v in pad)


def _L():
    return _lib.load()


def tune_save(path=None):
    """write the measured tile-configuration table next to the library (or to `path`); returns (total, new)"""
    tot, new = C.c_int(0), C.c_int(0)
    _lib.check(_L().xm_tune_entries(C.byref(tot), C.byref(new)))
    _lib.check(_L().xm_tune_save(path.encode() if path else None))
    return int(tot.value), int(new.value)


EXEC_SINGLE_STREAM = 1    # include/xmodal.h XM_EXEC_SINGLE_STREAM


def set_exec_hint(flags):
    """xm_set_exec_hint: tell the library HOW this host calls it (EXEC_SINGLE_STREAM: every operator call on one stream,
    MatConvNet's own sequence) -- kernel choice is a function of (shape, table, this hint), never of the call history.
    Returns the previous value."""
    old = int(_L().xm_get_exec_hint())
    _lib.check(_L().xm_set_exec_hint(int(flags)))
    return old


def out_size(n, pa, pb, f, d, s):
    return _L().xm_out_size(n, pa, pb, f, d, s)


# --------------------------------------------------------------------------------------------
# vl_nnconv
# --------------------------------------------------------------------------------------------


def vl_nnconv(x, f, b=None, dzdy=None, stride=1, pad=0, dilate=1, no_der_data=False,
              no_der_filters=False, no_der_biases=False, scale=None, shift=None, residual=None,
              relu=False, df_out=None, db_out=None, dx_accum=None, sigmoid=False, moments_out=None, epsilon=1e-4,
              gate=None, residual_stride=None, out_lattice=None, precision=None):
    """Y = VL_NNCONV(X, F, B) / [DX, DF, DB] = VL_NNCONV(X, F, B, DZDY).

    `gate` (forward, extension; 1 x 1 x K x N): per-(channel, sample) multiplier between scale / shift and the residual --
    the SE excite folded into the projection that produces its operand (xm_nnconv_forward_gated).
    `moments_out` (forward, extension; a K x 2 device matrix): also receives the batch moments [mean, sqrt(var +
    epsilon)] of Y -- the statistics pass of the train-mode vl_nnbnorm that follows (xm_nnconv_forward_moments).
    `scale/shift/residual/relu/sigmoid` select the fused forward epilogue (extension; see xmodal.h);
    `residual_stride=(sy, sx)` (forward, extension): RESIDUAL has an extent of its own, RH x RW x K x N, and is sampled at
    (oy * sy, ox * sx); Ho must equal floor((RH - 1) / sy) + 1, likewise Wo (xm_nnconv_forward_strided_residual);
    `out_lattice=(ly, lx)` (forward, extension; with scale / shift / relu only): Y keeps its full extent but only the pixels
    (ly * i, lx * j) are computed, with the bits of the full-extent call; the other elements of Y are unspecified
    (xm_nnconv_forward_lattice: what a layer whose only reader has stride (ly, lx) needs);
    `dx_accum` (backward, extension): DX = dgrad + dx_accum in the dgrad epilogue;
    `precision` (forward, extension): None / 'fp32' is the library's fp32 arithmetic; 'bf16x3' runs an unpadded, ungrouped
    1 x 1 layer on the bf16 matrix cores with both operands split in two bf16 halves (xm_nnconv_forward_split: error at
    most 3 * 2^-16 * sum |x||f| per output, bits independent of the batch) -- with scale / shift / gate / residual /
    residual_stride / relu, never with dzdy, moments_out, out_lattice or sigmoid."""
    if precision not in (None, "fp32", "bf16x3"):
        raise ValueError("vl_nnconv: unknown precision %r (None, 'fp32' or 'bf16x3')" % (precision,))
    if precision == "bf16x3":
        return _nnconv_split(x, f, b, dzdy, stride, pad, dilate, scale, shift, residual, relu, sigmoid, moments_out, gate,
                             residual_stride, out_lattice)
    x, f = _chk(x, "X"), _chk(f, "F")
    H, W, Cc, N = _shape4(x)
    FH, FW, FC, K = _shape4(f)
    sy, sx = _pair(stride, "STRIDE")
    dy, dx = _pair(dilate, "DILATE")
    pt, pb, pl, pr = _pad4(pad)
    bb = None
    if b is not None and b.numel() > 0:
        bb = _chk(b, "B")
        if bb.numel() != K:
            raise ValueError("vl_nnconv: B has %d elements, expected %d" % (bb.numel(), K))
    L = _L()
    Ho = L.xm_out_size(H, pt, pb, FH, dy, sy)
    Wo = L.xm_out_size(W, pl, pr, FW, dx, sx)
    if dzdy is None:
        y = mat_empty(max(Ho, 0), max(Wo, 0), K, N, device=x.device)
        fused = scale is not None or residual is not None or relu or sigmoid
        if out_lattice is not None:
            if residual is not None or gate is not None or sigmoid or moments_out is not None or residual_stride is not None:
                raise ValueError("vl_nnconv: out_lattice takes the scale / shift / relu epilogue only")
            lty, ltx = _pair(out_lattice, "OUT_LATTICE")
            _lib.check(L.xm_nnconv_forward_lattice(
                _ptr(x), H, W, Cc, N, _ptr(f), FH, FW, FC, K, _ptr(bb), _ptr(y), sy, sx, pt, pb, pl, pr, dy, dx,
                _ptr(scale), _ptr(shift), None, 1 if relu else 0, lty, ltx, _stream()))
        elif residual_stride is not None:
            if residual is None:
                raise ValueError("vl_nnconv: residual_stride without a residual")
            if moments_out is not None or sigmoid:
                raise ValueError("vl_nnconv: residual_stride cannot be combined with moments_out or sigmoid")
            rsy, rsx = _pair(residual_stride, "RESIDUAL_STRIDE")
            RH, RW, RK, RN = _shape4(_chk(residual, "RESIDUAL"))
            if [RK, RN] != [K, N]:
                raise ValueError("vl_nnconv: residual shape mismatch")
            gt = None
            if gate is not None:
                gt = _chk(gate, "GATE")
                if gt.numel() != K * N:
                    raise ValueError("vl_nnconv: GATE must be 1 x 1 x %d x %d" % (K, N))
            # (the extents are checked by the library: XM_EINVAL unless the sampled residual has the output's size)
            _lib.check(L.xm_nnconv_forward_strided_residual(
                _ptr(x), H, W, Cc, N, _ptr(f), FH, FW, FC, K, _ptr(bb), _ptr(y), sy, sx, pt, pb, pl, pr, dy, dx,
                _ptr(scale), _ptr(shift), _ptr(gt), _ptr(residual), RH, RW, rsy, rsx, 1 if relu else 0, _stream()))
        elif gate is not None:
            gt = _chk(gate, "GATE")
            if gt.numel() != K * N:
                raise ValueError("vl_nnconv: GATE must be 1 x 1 x %d x %d" % (K, N))
            if residual is not None and _shape4(_chk(residual, "RESIDUAL")) != [Ho, Wo, K, N]:
                raise ValueError("vl_nnconv: residual shape mismatch")
            _lib.check(L.xm_nnconv_forward_gated(
                _ptr(x), H, W, Cc, N, _ptr(f), FH, FW, FC, K, _ptr(bb), _ptr(y), sy, sx, pt, pb, pl, pr, dy, dx,
                _ptr(scale), _ptr(shift), _ptr(gt), _ptr(residual), (1 if relu else 0) | (4 if sigmoid else 0), _stream()))
        elif moments_out is not None:
            if fused:
                raise ValueError("vl_nnconv: moments_out cannot be combined with a fused epilogue")
            mo = _chk(moments_out, "MOMENTS")
            if mo.numel() != 2 * K:
                raise ValueError("vl_nnconv: moments_out must be %d x 2" % K)
            _lib.check(L.xm_nnconv_forward_moments(_ptr(x), H, W, Cc, N, _ptr(f), FH, FW, FC, K, _ptr(bb), _ptr(y),
                                                   sy, sx, pt, pb, pl, pr, dy, dx, float(epsilon), _ptr(mo),
                                                   _stream()))
        elif fused:
            if residual is not None:
                _chk(residual, "RESIDUAL")
                if _shape4(residual) != [Ho, Wo, K, N]:
                    raise ValueError("vl_nnconv: residual shape mismatch")
            _lib.check(L.xm_nnconv_forward_fused(
                _ptr(x), H, W, Cc, N, _ptr(f), FH, FW, FC, K, _ptr(bb), _ptr(y), sy, sx, pt, pb,
                pl, pr, dy, dx, _ptr(scale), _ptr(shift), _ptr(residual), (1 if relu else 0) | (4 if sigmoid else 0),
                _stream()))
        else:
            _lib.check(L.xm_nnconv_forward(_ptr(x), H, W, Cc, N, _ptr(f), FH, FW, FC, K, _ptr(bb),
                                           _ptr(y), sy, sx, pt, pb, pl, pr, dy, dx, _stream()))
        return y
    dzdy = _chk(dzdy, "DZDY")
    if _shape4(dzdy) != [Ho, Wo, K, N]:
        raise ValueError("vl_nnconv: DZDY is %r, expected %r" % (tuple(dzdy.shape), (Ho, Wo, K, N)))
    dxo = None if no_der_data else mat_empty(H, W, Cc, N, device=x.device)
    # df_out / db_out: caller-owned destinations (e.g. views of the flat gradient buffer)
    dfo = None if no_der_filters else (df_out if df_out is not None else mat_empty(FH, FW, FC, K, device=x.device))
    dbo = None if (no_der_biases or bb is None) else (db_out if db_out is not None else mat_empty(K, 1, device=x.device))
    acc = None
    if dx_accum is not None and dxo is not None:
        acc = _chk(dx_accum, "DX_ACCUM")
        if _shape4(acc) != [H, W, Cc, N]:
            raise ValueError("vl_nnconv: dx_accum must have the size of X")
    _lib.check(L.xm_nnconv_backward_accum(_ptr(x), H, W, Cc, N, _ptr(f), FH, FW, FC, K, _ptr(dzdy),
                                          _ptr(dxo), _ptr(dfo), _ptr(dbo), sy, sx, pt, pb, pl, pr, dy, dx,
                                          _ptr(acc), _stream()))
    return dxo, dfo, dbo


CONV_BF16X3 = 1    # include/xmodal.h XM_CONV_BF16X3


def conv_split_geometry(xshape, fshape, stride=1, pad=0, dilate=1, relu=False, sigmoid=False):
    """xm_nnconv_split_geometry (host only, no device call): dict(can, want, blocks, launches) of the bf16x3 arm for a
    layer of these shapes -- `can`: vl_nnconv(precision='bf16x3') would run it; `want`: a forward-only plan sends it there."""
    H, W, Cc, N = [int(v) for v in tuple(xshape) + (1,) * (4 - len(xshape))]
    FH, FW, FC, K = [int(v) for v in tuple(fshape) + (1,) * (4 - len(fshape))]
    sy, sx = _pair(stride, "STRIDE")
    dy, dx = _pair(dilate, "DILATE")
    pt, pb, pl, pr = _pad4(pad)
    out = [C.c_int(0) for _ in range(4)]
    _lib.check(_L().xm_nnconv_split_geometry(H, W, Cc, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx,
                                             (1 if relu else 0) | (4 if sigmoid else 0), *[C.byref(o) for o in out]))
    return dict(can=bool(out[0].value), want=bool(out[1].value), blocks=out[2].value, launches=out[3].value)


def _nnconv_split(x, f, b, dzdy, stride, pad, dilate, scale, shift, residual, relu, sigmoid, moments_out, gate,
                  residual_stride, out_lattice):
    """vl_nnconv(precision='bf16x3'): the forward direction of an unpadded 1 x 1 layer through xm_nnconv_forward_split"""
    for name, v in (("dzdy", dzdy), ("moments_out", moments_out), ("out_lattice", out_lattice), ("sigmoid", sigmoid or None)):
        if v is not None:
            raise ValueError("vl_nnconv: precision='bf16x3' is a forward mode and cannot be combined with %s" % name)
    x, f = _chk(x, "X"), _chk(f, "F")
    H, W, Cc, N = _shape4(x)
    FH, FW, FC, K = _shape4(f)
    sy, sx = _pair(stride, "STRIDE")
    dy, dx = _pair(dilate, "DILATE")
    pt, pb, pl, pr = _pad4(pad)
    bb = None
    if b is not None and b.numel() > 0:
        bb = _chk(b, "B")
        if bb.numel() != K:
            raise ValueError("vl_nnconv: B has %d elements, expected %d" % (bb.numel(), K))
    L = _L()
    Ho, Wo = L.xm_out_size(H, pt, pb, FH, dy, sy), L.xm_out_size(W, pl, pr, FW, dx, sx)
    for name, v in (("SCALE", scale), ("SHIFT", shift)):
        if v is not None and _chk(v, name).numel() != K:
            raise ValueError("vl_nnconv: %s has %d elements, expected %d" % (name, v.numel(), K))
    gt = None
    if gate is not None:
        gt = _chk(gate, "GATE")
        if gt.numel() != K * N:
            raise ValueError("vl_nnconv: GATE must be 1 x 1 x %d x %d" % (K, N))
    RH, RW, rsy, rsx = 0, 0, 1, 1
    if residual_stride is not None and residual is None:
        raise ValueError("vl_nnconv: residual_stride without a residual")
    if residual is not None:
        RH, RW, RK, RN = _shape4(_chk(residual, "RESIDUAL"))
        if residual_stride is not None:
            rsy, rsx = _pair(residual_stride, "RESIDUAL_STRIDE")
        if [RK, RN] != [K, N] or (residual_stride is None and [RH, RW] != [Ho, Wo]):
            raise ValueError("vl_nnconv: residual shape mismatch")
    y = mat_empty(max(Ho, 0), max(Wo, 0), K, N, device=x.device)
    _lib.check(L.xm_nnconv_forward_split(
        _ptr(x), H, W, Cc, N, _ptr(f), FH, FW, FC, K, _ptr(bb), _ptr(y), sy, sx, pt, pb, pl, pr, dy, dx,
        _ptr(scale), _ptr(shift), _ptr(gt), _ptr(residual), RH, RW, rsy, rsx, 1 if relu else 0, CONV_BF16X3, _stream()))
    return y


def conv_prepare_backward(x, f, stride=1, pad=0, dilate=1):
    """Extension: build the transposed filter operand of the DZDX GEMM now, on the current stream (see xmodal.h);
    the backward call of the same layer finds it as long as the parameters have not been updated in between."""
    H, W, Cc, N = _shape4(x)
    FH, FW, FC, K = _shape4(f)
    sy, sx = _pair(stride, "STRIDE")
    dy, dx = _pair(dilate, "DILATE")
    pt, pb, pl, pr = _pad4(pad)
    _lib.check(_L().xm_nnconv_prepare_backward(H, W, Cc, N, _ptr(f), FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx,
                                               _stream()))


def params_changed():
    """Extension: xm_params_changed -- every operand conv_prepare_backward built so far is stale.  sgd_update,
    solver_update and average_update say so themselves; call this after writing parameter values by any other means
    (a torch copy_ into a filter tensor, a checkpoint load) and after giving parameters new storage (a freed filter's
    address can be handed to the next tensor of its shape: the cache is keyed by address).  Host-side counter, no launch."""
    _lib.check(_L().xm_params_changed())


# --------------------------------------------------------------------------------------------
# vl_nnpool
# --------------------------------------------------------------------------------------------
_METHOD = {"max": 0, "avg": 1}


def vl_nnpool(x, pool, dzdy=None, stride=1, pad=0, method="max", argmax=None, want_argmax=False, dx_accum=None):
    """Y = VL_NNPOOL(X, POOL) / DX = VL_NNPOOL(X, POOL, DZDY).

    Extension for max pooling: `want_argmax=True` (forward) also returns the uint8 routing table
    of first maxima; pass it back as `argmax=` (backward) to skip the recomputation from X.
    Extension for global average pooling (POOL = the whole plane, the SE squeeze): `dx_accum` = the derivative another
    consumer of X already left; the result is DX + dx_accum in one pass (xm_nnpool_global_avg_backward_accum)."""
    x = _chk(x, "X")
    if method not in _METHOD:
        raise ValueError("vl_nnpool: unknown METHOD '%s'" % method)
    H, W, Cc, N = _shape4(x)
    ph, pw = _pair(pool, "POOL")
    sy, sx = _pair(stride, "STRIDE")
    pt, pb, pl, pr = _pad4(pad)
    L = _L()
    Ho = L.xm_out_size(H, pt, pb, ph, 1, sy)
    Wo = L.xm_out_size(W, pl, pr, pw, 1, sx)
    if dzdy is None:
        y = mat_empty(max(Ho, 0), max(Wo, 0), Cc, N, device=x.device)
        if want_argmax and method == "max":
            am = torch.empty(max(Ho, 0) * max(Wo, 0) * Cc * N, dtype=torch.uint8, device=x.device)
            _lib.check(L.xm_nnpool_forward_argmax(_ptr(x), H, W, Cc, N, ph, pw, sy, sx, pt, pb, pl, pr,
                                                  _ptr(y), C.c_void_p(am.data_ptr()), _stream()))
            return y, am
        _lib.check(L.xm_nnpool_forward(_ptr(x), H, W, Cc, N, ph, pw, sy, sx, pt, pb, pl, pr,
                                       _METHOD[method], _ptr(y), _stream()))
        return (y, None) if want_argmax else y
    dzdy = _chk(dzdy, "DZDY")
    if _shape4(dzdy) != [Ho, Wo, Cc, N]:
        raise ValueError("vl_nnpool: DZDY is %r, expected %r" % (tuple(dzdy.shape), (Ho, Wo, Cc, N)))
    dxo = mat_empty(H, W, Cc, N, device=x.device)
    if dx_accum is not None:
        if method != "avg" or (ph, pw) != (H, W) or (pt | pb | pl | pr) or _shape4(dx_accum) != [H, W, Cc, N]:
            raise ValueError("vl_nnpool: dx_accum is built for global average pooling only")
        _lib.check(L.xm_nnpool_global_avg_backward_accum(_ptr(dzdy), _ptr(_chk(dx_accum, "DX_ACCUM")), _ptr(dxo), H, W, Cc, N,
                                                         _stream()))
        return dxo
    if argmax is not None and method == "max":
        _lib.check(L.xm_nnpool_backward_argmax(C.c_void_p(argmax.data_ptr()), H, W, Cc, N, ph, pw, sy,
                                               sx, pt, pb, pl, pr, _ptr(dzdy), _ptr(dxo), _stream()))
    else:
        _lib.check(L.xm_nnpool_backward(_ptr(x), H, W, Cc, N, ph, pw, sy, sx, pt, pb, pl, pr,
                                        _METHOD[method], _ptr(dzdy), _ptr(dxo), _stream()))
    return dxo


# --------------------------------------------------------------------------------------------
# vl_nnbnorm
# --------------------------------------------------------------------------------------------


def vl_nnbnorm(x, g, b, dzdy=None, epsilon=1e-4, moments=None, relu=False, y=None, dg_out=None,
               db_out=None, moments_out=None, batch_moments=False, dxsum_out=None):
    """forward:  Y, MOMENTS = VL_NNBNORM(X, G, B);  backward: DX, DG, DB, MOMENTS = (..., DZDY).

    MOMENTS is C x 2 = [mean, sqrt(var + epsilon)].  `relu=True` fuses vl_nnrelu (forward) /
    its mask (backward; pass the fused forward output as `y`).  `batch_moments=True` (backward,
    extension): `moments` are the batch moments the forward call returned for this X -- train-mode
    derivative without recomputing them.  `dxsum_out` (backward, extension; C x 1): receives sum(DX) per channel =
    the DZDB of the vl_nnconv that produced X (xm_nnbnorm_backward_dxsum)."""
    x, g, b = _chk(x, "X"), _chk(g, "G"), _chk(b, "B")
    H, W, Cc, N = _shape4(x)
    if g.numel() != Cc or b.numel() != Cc:
        raise ValueError("vl_nnbnorm: G and B must have %d elements" % Cc)
    mi = None
    if moments is not None:
        mi = _chk(moments, "MOMENTS")
        if mi.numel() != 2 * Cc:
            raise ValueError("vl_nnbnorm: MOMENTS must be %d x 2" % Cc)
    L = _L()
    mo = moments_out if moments_out is not None else mat_empty(Cc, 2, device=x.device)
    if dzdy is None:
        yo = mat_empty(H, W, Cc, N, device=x.device)
        _lib.check(L.xm_nnbnorm_forward_fused(_ptr(x), H, W, Cc, N, _ptr(g), _ptr(b),
                                              float(epsilon), _ptr(mi), _ptr(yo), _ptr(mo),
                                              1 if relu else 0, _stream()))
        return yo, mo
    dzdy = _chk(dzdy, "DZDY")
    if _shape4(dzdy) != [H, W, Cc, N]:
        raise ValueError("vl_nnbnorm: DZDY shape mismatch")
    dxo = mat_empty(H, W, Cc, N, device=x.device)
    dg = dg_out if dg_out is not None else mat_empty(Cc, 1, device=x.device)
    db = db_out if db_out is not None else mat_empty(Cc, 1, device=x.device)
    if batch_moments and mi is None:
        raise ValueError("vl_nnbnorm: batch_moments needs the moments of the forward call")
    if dxsum_out is not None:
        if relu and y is None:
            raise ValueError("vl_nnbnorm: fused backward needs the forward output y")
        if _chk(dxsum_out, "DXSUM").numel() != Cc:
            raise ValueError("vl_nnbnorm: dxsum_out must have %d elements" % Cc)
        _lib.check(L.xm_nnbnorm_backward_dxsum(_ptr(x), _ptr(_chk(y, "Y")) if relu else None, H, W, Cc, N,
                                               _ptr(g), _ptr(b), _ptr(dzdy), float(epsilon), _ptr(mi),
                                               _ptr(dxo), _ptr(dg), _ptr(db), _ptr(mo), _ptr(dxsum_out),
                                               (1 if relu else 0) | (2 if batch_moments else 0), _stream()))
    elif relu or batch_moments:
        if relu and y is None:
            raise ValueError("vl_nnbnorm: fused backward needs the forward output y")
        _lib.check(L.xm_nnbnorm_backward_fused(_ptr(x), _ptr(_chk(y, "Y")) if relu else None, H, W, Cc, N,
                                               _ptr(g), _ptr(b), _ptr(dzdy), float(epsilon), _ptr(mi),
                                               _ptr(dxo), _ptr(dg), _ptr(db), _ptr(mo),
                                               (1 if relu else 0) | (2 if batch_moments else 0), _stream()))
    else:
        _lib.check(L.xm_nnbnorm_backward(_ptr(x), H, W, Cc, N, _ptr(g), _ptr(b), _ptr(dzdy),
                                         float(epsilon), _ptr(mi), _ptr(dxo), _ptr(dg), _ptr(db),
                                         _ptr(mo), _stream()))
    return dxo, dg, db, mo


def bnorm_relu_pool(x, g, b, pool, stride=1, pad=0, epsilon=1e-4, moments=None, moments_out=None):
    """Extension: vl_nnpool(vl_nnrelu(vl_nnbnorm(x, g, b)), pool, 'method', 'max') in one fused pass.
    Returns (y_pool, argmax_table, moments)."""
    x, g, b = _chk(x, "X"), _chk(g, "G"), _chk(b, "B")
    H, W, Cc, N = _shape4(x)
    ph, pw = _pair(pool, "POOL")
    sy, sx = _pair(stride, "STRIDE")
    pt, pb, pl, pr = _pad4(pad)
    L = _L()
    Ho, Wo = L.xm_out_size(H, pt, pb, ph, 1, sy), L.xm_out_size(W, pl, pr, pw, 1, sx)
    y = mat_empty(max(Ho, 0), max(Wo, 0), Cc, N, device=x.device)
    am = torch.empty(max(Ho, 0) * max(Wo, 0) * Cc * N, dtype=torch.uint8, device=x.device)
    mo = moments_out if moments_out is not None else mat_empty(Cc, 2, device=x.device)
    mi = None if moments is None else _chk(moments, "MOMENTS")
    _lib.check(L.xm_nnbnorm_relu_pool_forward(_ptr(x), H, W, Cc, N, _ptr(g), _ptr(b), float(epsilon),
                                              _ptr(mi), ph, pw, sy, sx, pt, pb, pl, pr, _ptr(y),
                                              C.c_void_p(am.data_ptr()), _ptr(mo), _stream()))
    return y, am, mo


def bnorm_relu_pool_backward(x, g, b, moments, argmax, dzdy, pool, stride=1, pad=0, train=True,
                             dg_out=None, db_out=None, need_dx=True, dxsum_out=None, y_pool=None):
    """Backward of bnorm_relu_pool: returns (dx, dg, db).  dxsum_out (optional, C x 1): receives
    sum(dx) per channel = the bias derivative of the convolution that produced x.  y_pool (optional): the
    forward's pooled output -- the per-channel sums then come from the pooled tensors alone."""
    x, g, b, dzdy = _chk(x, "X"), _chk(g, "G"), _chk(b, "B"), _chk(dzdy, "DZDY")
    H, W, Cc, N = _shape4(x)
    ph, pw = _pair(pool, "POOL")
    sy, sx = _pair(stride, "STRIDE")
    pt, pb, pl, pr = _pad4(pad)
    dx = mat_empty(H, W, Cc, N, device=x.device) if need_dx else None
    dg = dg_out if dg_out is not None else mat_empty(Cc, 1, device=x.device)
    db = db_out if db_out is not None else mat_empty(Cc, 1, device=x.device)
    _lib.check(_L().xm_nnbnorm_relu_pool_backward(
        _ptr(x), H, W, Cc, N, _ptr(g), _ptr(b), _ptr(_chk(moments, "MOMENTS")), 1 if train else 0, ph, pw,
        sy, sx, pt, pb, pl, pr, C.c_void_p(argmax.data_ptr()),
        None if y_pool is None else _ptr(_chk(y_pool, "Y_POOL")), _ptr(dzdy), _ptr(dx), _ptr(dg), _ptr(db),
        _ptr(dxsum_out), _stream()))
    return dx, dg, db


def conv_backward_filter_bnrelupool(x, filter_shape, y, g, b, moments, argmax, y_pool, dzdy, pool, stride=1, pad=0,
                                    dilate=1, pool_stride=1, pool_pad=0, train=True, df_out=None, dbias_out=None,
                                    dg_out=None, db_out=None, has_bias=True):
    """Extension (xm_nnconv_backward_filter_bnrelupool): [DZDF, DZDB] of the first-layer convolution Y = vl_nnconv(X, F, B)
    and [DG, DB] of the bnorm in  vl_nnpool(vl_nnrelu(vl_nnbnorm(Y, G, B)))  from the POOLED derivative `dzdy`: the
    bnorm's DZDX is never materialised.  Returns (df, dbias, dg, db), or None when the shapes are outside what the fused
    kernel covers (the caller then runs bnorm_relu_pool_backward + vl_nnconv backward)."""
    x, y, g, b, dzdy = _chk(x, "X"), _chk(y, "Y"), _chk(g, "G"), _chk(b, "B"), _chk(dzdy, "DZDY")
    H, W, Cc, N = _shape4(x)
    FH, FW, FC, K = (int(v) for v in filter_shape)
    sy, sx = _pair(stride, "STRIDE")
    dy, dx = _pair(dilate, "DILATE")
    pt, pb, pl, pr = _pad4(pad)
    ph, pw = _pair(pool, "POOL")
    psy, psx = _pair(pool_stride, "STRIDE")
    ppt, ppb, ppl, ppr = _pad4(pool_pad)
    df = df_out if df_out is not None else mat_empty(FH, FW, FC, K, device=x.device)
    dbias = (dbias_out if dbias_out is not None else mat_empty(K, 1, device=x.device)) if has_bias else None
    dg = dg_out if dg_out is not None else mat_empty(K, 1, device=x.device)
    db = db_out if db_out is not None else mat_empty(K, 1, device=x.device)
    rc = _L().xm_nnconv_backward_filter_bnrelupool(
        _ptr(x), H, W, Cc, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx, _ptr(y), _ptr(g), _ptr(b),
        _ptr(_chk(moments, "MOMENTS")), 1 if train else 0, ph, pw, psy, psx, ppt, ppb, ppl, ppr,
        C.c_void_p(argmax.data_ptr()), None if y_pool is None else _ptr(_chk(y_pool, "Y_POOL")), _ptr(dzdy), _ptr(df),
        _ptr(dbias), _ptr(dg), _ptr(db), _stream())
    if rc == XM_ENOTSUP:
        return None
    _lib.check(rc)
    return df, dbias, dg, db


def stem_gram(x, filter_shape, stride=1, pad=0):
    """Extension (xm_stem_gram): fp64 [64][64] Gram matrix of the im2col patches (+ ones) of a single-channel first
    layer; None when the geometry is not covered."""
    x = _chk(x, "X")
    H, W, Cc, N = _shape4(x)
    FH, FW = int(filter_shape[0]), int(filter_shape[1])
    sy, sx = _pair(stride, "STRIDE")
    pt, pb, pl, pr = _pad4(pad)
    if Cc != 1:
        return None
    gram = torch.empty(64 * 64, dtype=torch.float64, device=x.device)
    rc = _L().xm_stem_gram(_ptr(x), H, W, N, FH, FW, sy, sx, pt, pb, pl, pr, C.c_void_p(gram.data_ptr()), _stream())
    if rc == XM_ENOTSUP:
        return None
    _lib.check(rc)
    return gram


def stem_gram_moments(gram, f, b, epsilon=1e-4, moments_out=None):
    """Extension (xm_stem_gram_moments): vl_nnbnorm's MOMENTS of Y = vl_nnconv(X, F, B) from the Gram matrix of X."""
    f = _chk(f, "F")
    FH, FW, FC, K = _shape4(f)
    mo = moments_out if moments_out is not None else mat_empty(K, 2, device=f.device)
    _lib.check(_L().xm_stem_gram_moments(C.c_void_p(gram.data_ptr()), _ptr(f), _ptr(None if b is None else _chk(b, "B")),
                                         FH, FW, K, float(epsilon), _ptr(mo), _stream()))
    return mo


def conv_bnorm_relu_pool(x, f, bias, g, b, pool, stride=1, pad=0, dilate=1, pool_stride=1, pool_pad=0, epsilon=1e-4,
                         moments=None, moments_out=None, gram=None):
    """Extension (xm_nnconv_bnorm_relu_pool_forward): vl_nnpool(vl_nnrelu(vl_nnbnorm(vl_nnconv(x, f, bias), g, b))) for a
    single-channel first layer in one kernel -- the convolution's output is never written.  Returns
    (y_pool, argmax_table, moments, gram) or None when the shapes are not covered.  `moments` given = test mode (no Gram
    matrix); the table marks closed windows with 255 (include/xmodal.h)."""
    x, f, g, b = _chk(x, "X"), _chk(f, "F"), _chk(g, "G"), _chk(b, "B")
    H, W, Cc, N = _shape4(x)
    FH, FW, FC, K = _shape4(f)
    sy, sx = _pair(stride, "STRIDE")
    dy, dx = _pair(dilate, "DILATE")
    pt, pb, pl, pr = _pad4(pad)
    ph, pw = _pair(pool, "POOL")
    psy, psx = _pair(pool_stride, "STRIDE")
    ppt, ppb, ppl, ppr = _pad4(pool_pad)
    L = _L()
    Ho, Wo = L.xm_out_size(H, pt, pb, FH, dy, sy), L.xm_out_size(W, pl, pr, FW, dx, sx)
    pHo, pWo = L.xm_out_size(Ho, ppt, ppb, ph, 1, psy), L.xm_out_size(Wo, ppl, ppr, pw, 1, psx)
    if Ho <= 0 or Wo <= 0 or pHo <= 0 or pWo <= 0:
        return None
    y = mat_empty(pHo, pWo, K, N, device=x.device)
    am = torch.empty(pHo * pWo * K * N, dtype=torch.uint8, device=x.device)
    mi = None if moments is None else _chk(moments, "MOMENTS")
    mo = None
    if mi is None:
        mo = moments_out if moments_out is not None else mat_empty(K, 2, device=x.device)
        if gram is None:
            gram = torch.empty(64 * 64, dtype=torch.float64, device=x.device)
    rc = L.xm_nnconv_bnorm_relu_pool_forward(
        _ptr(x), H, W, Cc, N, _ptr(f), FH, FW, FC, K, None if bias is None else _ptr(_chk(bias, "B")), sy, sx, pt, pb, pl, pr,
        dy, dx, _ptr(g), _ptr(b), float(epsilon), _ptr(mi), ph, pw, psy, psx, ppt, ppb, ppl, ppr,
        None if gram is None else C.c_void_p(gram.data_ptr()), _ptr(y), C.c_void_p(am.data_ptr()), _ptr(mo), _stream())
    if rc == XM_ENOTSUP:
        return None
    _lib.check(rc)
    return y, am, (mi if mo is None else mo), gram


def conv_backward_filter_bnrelupool_gram(x, f, bias, g, moments, argmax, y_pool, dzdy, pool, stride=1, pad=0, dilate=1,
                                         pool_stride=1, pool_pad=0, train=True, gram=None, df_out=None, dbias_out=None,
                                         dg_out=None, db_out=None):
    """Extension (xm_nnconv_backward_filter_bnrelupool_gram): conv_backward_filter_bnrelupool without the convolution's
    output -- F / B take its place, the bnorm's sums and the normalisation's correction terms come from the Gram matrix of
    the input patches (include/xmodal.h).  Returns (df, dbias, dg, db) or None when the shapes are not covered."""
    x, f, g, dzdy = _chk(x, "X"), _chk(f, "F"), _chk(g, "G"), _chk(dzdy, "DZDY")
    H, W, Cc, N = _shape4(x)
    FH, FW, FC, K = _shape4(f)
    sy, sx = _pair(stride, "STRIDE")
    dy, dx = _pair(dilate, "DILATE")
    pt, pb, pl, pr = _pad4(pad)
    ph, pw = _pair(pool, "POOL")
    psy, psx = _pair(pool_stride, "STRIDE")
    ppt, ppb, ppl, ppr = _pad4(pool_pad)
    has_bias = bias is not None
    df = df_out if df_out is not None else mat_empty(FH, FW, FC, K, device=x.device)
    dbias = (dbias_out if dbias_out is not None else mat_empty(K, 1, device=x.device)) if has_bias else None
    dg = dg_out if dg_out is not None else mat_empty(K, 1, device=x.device)
    db = db_out if db_out is not None else mat_empty(K, 1, device=x.device)
    rc = _L().xm_nnconv_backward_filter_bnrelupool_gram(
        _ptr(x), H, W, Cc, N, _ptr(f), FH, FW, FC, K, _ptr(_chk(bias, "B")) if has_bias else None, sy, sx, pt, pb, pl, pr,
        dy, dx, _ptr(g), _ptr(_chk(moments, "MOMENTS")), 1 if train else 0, ph, pw, psy, psx, ppt, ppb, ppl, ppr,
        C.c_void_p(argmax.data_ptr()), None if y_pool is None else _ptr(_chk(y_pool, "Y_POOL")), _ptr(dzdy),
        None if gram is None else C.c_void_p(gram.data_ptr()), _ptr(df), _ptr(dbias), _ptr(dg), _ptr(db), _stream())
    if rc == XM_ENOTSUP:
        return None
    _lib.check(rc)
    return df, dbias, dg, db


# --------------------------------------------------------------------------------------------
# elementwise
# --------------------------------------------------------------------------------------------


def vl_nnrelu(x, dzdy=None, leak=0.0):
    x = _chk(x, "X")
    y = mat_empty(*x.shape, device=x.device)
    d = None if dzdy is None else _chk(dzdy, "DZDY")
    _lib.check(_L().xm_nnrelu(_ptr(x), x.numel(), float(leak), _ptr(d), _ptr(y), _stream()))
    return y


def nnnormalize_geometry():
    """(pixels_per_block, channels_per_pass, window_in_registers) of the vl_nnnormalize kernels (host only)"""
    v = [C.c_int(0) for _ in range(3)]
    _lib.check(_L().xm_nnnormalize_geometry(*[C.byref(t) for t in v]))
    return tuple(int(t.value) for t in v)


def vl_nnnormalize(x, param, dzdy=None, out=None):
    """Y = vl_nnnormalize(X, PARAM) / DZDX = vl_nnnormalize(X, PARAM, DZDY) [EXT], PARAM = [N KAPPA ALPHA BETA]: cross-channel
    normalisation Y = X .* (KAPPA + ALPHA * sum of X.^2 over N neighbouring channels).^(-BETA) (include/xmodal.h).
    `out` (extension): the array that receives the result; it may not overlap X or DZDY."""
    x = _chk(x, "X")
    param = [float(v) for v in np.asarray(param, dtype=np.float64).ravel()]
    if len(param) != 4:
        raise ValueError("PARAM must have four elements [N KAPPA ALPHA BETA]")
    if param[0] != int(param[0]):
        raise ValueError("PARAM(1) = N must be a positive integer")
    H, W, Cc, S = _shape4(x)
    y = mat_empty(*x.shape, device=x.device) if out is None else _chk(out, "OUT")
    if tuple(y.shape) != tuple(x.shape):
        raise ValueError("OUT and X do not have the same size")
    # (a window of 2^31 - 1 channels already covers every tensor the ABI's int C can describe)
    N, kappa, alpha, beta = min(int(param[0]), 2 ** 31 - 1), param[1], param[2], param[3]
    if dzdy is None:
        _lib.check(_L().xm_nnnormalize_forward(_ptr(x), H, W, Cc, S, N, kappa, alpha, beta, _ptr(y), _stream()))
        return y
    d = _chk(dzdy, "DZDY")
    if tuple(d.shape) != tuple(x.shape):
        raise ValueError("DZDY and X do not have the same size")
    _lib.check(_L().xm_nnnormalize_backward(_ptr(x), _ptr(d), H, W, Cc, S, N, kappa, alpha, beta, _ptr(y), _stream()))
    return y


def vl_nndropout(x, dzdy=None, rate=0.5, mask=None, seed=0, offset=0):
    """[Y, MASK] = vl_nndropout(X, 'rate', r) / Y = vl_nndropout(X, 'mask', M) / DZDX = vl_nndropout(X, DZDY, 'mask', M).
    Without a mask one is drawn from the library's stateless Philox stream (seed, offset: include/xmodal.h)."""
    x = _chk(x, "X")
    y = mat_empty(*x.shape, device=x.device)
    if dzdy is not None:
        if mask is None:
            raise ValueError("vl_nndropout: the backward call needs the forward call's mask")
        _lib.check(_L().xm_nndropout_apply(_ptr(_chk(dzdy, "DZDY")), _ptr(_chk(mask, "MASK")), x.numel(), _ptr(y), _stream()))
        return y
    if mask is not None:
        _lib.check(_L().xm_nndropout_apply(_ptr(x), _ptr(_chk(mask, "MASK")), x.numel(), _ptr(y), _stream()))
        return y, mask
    mask = mat_empty(*x.shape, device=x.device)
    _lib.check(_L().xm_nndropout_forward(_ptr(x), x.numel(), float(rate), int(seed), int(offset), _ptr(y), _ptr(mask),
                                         _stream()))
    return y, mask


def vl_nnsigmoid(x, dzdy=None):
    x = _chk(x, "X")
    y = mat_empty(*x.shape, device=x.device)
    d = None if dzdy is None else _chk(dzdy, "DZDY")
    _lib.check(_L().xm_nnsigmoid(_ptr(x), x.numel(), _ptr(d), _ptr(y), _stream()))
    return y


def sum2(a, b, relu=False):
    """dagnn.Sum over two inputs (+ optional fused vl_nnrelu)."""
    a, b = _chk(a, "A"), _chk(b, "B")
    if a.shape != b.shape:
        raise ValueError("dagnn.Sum: input sizes differ")
    y = mat_empty(*a.shape, device=a.device)
    _lib.check(_L().xm_sum2(_ptr(a), _ptr(b), a.numel(), 1 if relu else 0, _ptr(y), _stream()))
    return y


def scale_axpy(x, a, r=None, relu=False):
    """y = a .* x (+ r) (relu): the SE-block excite + residual of SENet50 (mcnExtraLayers)."""
    x, a = _chk(x, "X"), _chk(a, "A")
    H, W, Cc, N = _shape4(x)
    if a.numel() != Cc * N:
        raise ValueError("scale: A must be 1 x 1 x %d x %d" % (Cc, N))
    rr = None if r is None else _chk(r, "R")
    y = mat_empty(H, W, Cc, N, device=x.device)
    _lib.check(_L().xm_scale_axpy(_ptr(x), H * W, Cc * N, _ptr(a), _ptr(rr), 1 if relu else 0,
                                  _ptr(y), _stream()))
    return y


def se_squeeze_bn(u, g, b, moments):
    """gp = mean_hw(vl_nnbnorm(u, g, b, 'moments', moments)) without materialising the bnorm's output (xm_se_squeeze_bn)"""
    u = _chk(u, "U")
    H, W, Cc, N = _shape4(u)
    gp = mat_empty(1, 1, Cc, N, device=u.device)
    _lib.check(_L().xm_se_squeeze_bn(_ptr(u), H, W, Cc, N, _ptr(_chk(g, "G")), _ptr(_chk(b, "B")),
                                     _ptr(_chk(moments, "MOMENTS")), _ptr(gp), _stream()))
    return gp


def scale_axpy_bn(u, a, r, g, b, moments, relu=False):
    """y = [relu](a .* vl_nnbnorm(u, g, b, 'moments', moments) + r) (xm_scale_axpy_bn)"""
    u, a = _chk(u, "U"), _chk(a, "A")
    H, W, Cc, N = _shape4(u)
    if a.numel() != Cc * N:
        raise ValueError("scale: A must be 1 x 1 x %d x %d" % (Cc, N))
    y = mat_empty(H, W, Cc, N, device=u.device)
    _lib.check(_L().xm_scale_axpy_bn(_ptr(u), H, W, Cc, N, _ptr(a), _ptr(None if r is None else _chk(r, "R")),
                                     _ptr(_chk(g, "G")), _ptr(_chk(b, "B")), _ptr(_chk(moments, "MOMENTS")),
                                     1 if relu else 0, _ptr(y), _stream()))
    return y


def se_tail_backward_reduce(y, dzdy, u, g, b, moments):
    """first half of the fused SE-tail backward (xm_se_tail_backward_reduce): returns (da 1 x 1 x C x N, plane sums)"""
    y, dzdy, u = _chk(y, "Y"), _chk(dzdy, "DZDY"), _chk(u, "U")
    H, W, Cc, N = _shape4(u)
    da = mat_empty(1, 1, Cc, N, device=u.device)
    sums = torch.empty(3 * Cc * N, dtype=torch.float64, device=u.device)
    _lib.check(_L().xm_se_tail_backward_reduce(_ptr(y), _ptr(dzdy), _ptr(u), H, W, Cc, N, _ptr(_chk(g, "G")), _ptr(_chk(b, "B")),
                                               _ptr(_chk(moments, "MOMENTS")), _ptr(da), C.c_void_p(sums.data_ptr()), _stream()))
    return da, sums


def se_tail_backward_apply(y, dzdy, u, gate, dgp, g, moments, sums, train=True, dg_out=None, db_out=None):
    """second half (xm_se_tail_backward_apply): returns (dz = the shortcut's derivative, du, dg, db)"""
    y, dzdy, u = _chk(y, "Y"), _chk(dzdy, "DZDY"), _chk(u, "U")
    H, W, Cc, N = _shape4(u)
    dz = mat_empty(H, W, Cc, N, device=u.device)
    du = mat_empty(H, W, Cc, N, device=u.device)
    dg = dg_out if dg_out is not None else mat_empty(Cc, 1, device=u.device)
    db = db_out if db_out is not None else mat_empty(Cc, 1, device=u.device)
    _lib.check(_L().xm_se_tail_backward_apply(_ptr(y), _ptr(dzdy), _ptr(u), H, W, Cc, N, _ptr(_chk(gate, "A")),
                                              _ptr(_chk(dgp, "DGP")), _ptr(_chk(g, "G")), _ptr(_chk(moments, "MOMENTS")),
                                              1 if train else 0, C.c_void_p(sums.data_ptr()), _ptr(dz), _ptr(du), _ptr(dg),
                                              _ptr(db), _stream()))
    return dz, du, dg, db


def scale_backward(x, a, dzdy, need_dx=True):
    x, a, dzdy = _chk(x, "X"), _chk(a, "A"), _chk(dzdy, "DZDY")
    H, W, Cc, N = _shape4(x)
    dx = mat_empty(H, W, Cc, N, device=x.device) if need_dx else None
    da = mat_empty(1, 1, Cc, N, device=x.device)
    _lib.check(_L().xm_scale_backward(_ptr(x), H * W, Cc * N, _ptr(a), _ptr(dzdy), _ptr(dx),
                                      _ptr(da), _stream()))
    return dx, da


# --------------------------------------------------------------------------------------------
# losses
# --------------------------------------------------------------------------------------------


def vl_nnsoftmaxt(x, dzdy=None, temperature=1.0, dim=3):
    """Y = VL_NNSOFTMAXT(X, 'temperature', T, 'dim', d); DZDX = VL_NNSOFTMAXT(X, DZDY, ...).
    dim is 1-based as in MATLAB (student_stats.m:95 uses 'dim', 2)."""
    x = _chk(x, "X")
    shp = [int(s) for s in x.shape] + [1] * (4 - x.dim())
    d = int(dim) - 1
    HW = int(np.prod(shp[:d])) if d > 0 else 1
    Cc = shp[d]
    N = int(np.prod(shp[d + 1:])) if d < 3 else 1
    y = mat_empty(*x.shape, device=x.device)
    if dzdy is None:
        _lib.check(_L().xm_nnsoftmaxt(_ptr(x), HW, Cc, N, float(temperature), _ptr(y), _stream()))
        return y
    dzdy = _chk(dzdy, "DZDY")
    if tuple(dzdy.shape) != tuple(x.shape):
        raise ValueError("vl_nnsoftmaxt: DZDY must have the size of X")
    _lib.check(_L().xm_nnsoftmaxt_backward(_ptr(x), _ptr(dzdy), HW, Cc, N, float(temperature), _ptr(y),
                                           _stream()))
    return y


def vl_nnsoftmax(x, dzdy=None):
    """Y = VL_NNSOFTMAX(X); DZDX = VL_NNSOFTMAX(X, DZDY) -- channel softmax along dim 3."""
    return vl_nnsoftmaxt(x, dzdy, 1.0, 3)


def vl_nnsoftmaxceloss(x, p, dzdy=None, temperature=1.0, logitTargets=False, instanceWeights=None):
    """VL_NNSOFTMAXCELOSS(X, P [, DZDY], 'temperature', T, 'logitTargets', tf, ...)."""
    x, p = _chk(x, "X"), _chk(p, "P")
    H, W, Cc, N = _shape4(x)
    if H != 1 or W != 1:
        raise ValueError("vl_nnsoftmaxceloss: X must be 1 x 1 x C x N")
    if _shape4(p) != [1, 1, Cc, N]:
        raise ValueError("vl_nnsoftmaxceloss: P must have the size of X")
    w = None if instanceWeights is None else _chk(instanceWeights, "instanceWeights")
    if dzdy is None:
        y = mat_empty(1, 1, device=x.device)
        _lib.check(_L().xm_nnsoftmaxceloss(_ptr(x), _ptr(p), Cc, N, float(temperature),
                                           1 if logitTargets else 0, _ptr(w), None, _ptr(y),
                                           _stream()))
        return y
    if not isinstance(dzdy, torch.Tensor):
        dzdy = from_numpy(np.array([[float(dzdy)]], np.float32), device=x.device)
    y = mat_empty(1, 1, Cc, N, device=x.device)
    _lib.check(_L().xm_nnsoftmaxceloss(_ptr(x), _ptr(p), Cc, N, float(temperature),
                                       1 if logitTargets else 0, _ptr(w), _ptr(dzdy), _ptr(y),
                                       _stream()))
    return y


_LOSS = {"softmaxlog": 0, "classerror": 1}


def vl_nnloss(x, c, dzdy=None, loss="softmaxlog"):
    """VL_NNLOSS(X, c [, DZDY], 'loss', 'softmaxlog' | 'classerror'); c holds 1-based labels."""
    x, c = _chk(x, "X"), _chk(c, "C")
    H, W, Cc, N = _shape4(x)
    if H != 1 or W != 1:
        raise ValueError("vl_nnloss: X must be 1 x 1 x C x N")
    if loss not in _LOSS:
        raise ValueError("vl_nnloss: unknown loss '%s'" % loss)
    if c.numel() != N:
        raise ValueError("vl_nnloss: need one label per sample")
    if dzdy is None:
        y = mat_empty(1, 1, device=x.device)
        _lib.check(_L().xm_nnloss(_ptr(x), _ptr(c), Cc, N, _LOSS[loss], None, _ptr(y), _stream()))
        return y
    if not isinstance(dzdy, torch.Tensor):
        dzdy = from_numpy(np.array([[float(dzdy)]], np.float32), device=x.device)
    y = mat_empty(1, 1, Cc, N, device=x.device)
    _lib.check(_L().xm_nnloss(_ptr(x), _ptr(c), Cc, N, _LOSS[loss], _ptr(dzdy), _ptr(y), _stream()))
    return y


def _regloss(x, t, dzdy, kind, sigma, instanceWeights, name):
    x, t = _chk(x, "X"), _chk(t, "T")
    if tuple(x.shape) != tuple(t.shape):
        raise ValueError("%s: X and T must have the same size" % name)
    N = int(x.shape[3]) if x.dim() > 3 else 1
    E = int(x.numel()) // N
    w = None if instanceWeights is None else _chk(instanceWeights, "instanceWeights")
    if w is not None and int(w.numel()) != N:
        raise ValueError("%s: need one instance weight per sample" % name)
    if dzdy is None:
        y = mat_empty(1, 1, device=x.device)
        _lib.check(_L().xm_nnregloss(_ptr(x), _ptr(t), E, N, kind, float(sigma), _ptr(w), None, _ptr(y),
                                     _stream()))
        return y
    if not isinstance(dzdy, torch.Tensor):
        dzdy = from_numpy(np.array([[float(dzdy)]], np.float32), device=x.device)
    y = mat_empty(*x.shape, device=x.device)
    _lib.check(_L().xm_nnregloss(_ptr(x), _ptr(t), E, N, kind, float(sigma), _ptr(w), _ptr(dzdy), _ptr(y),
                                 _stream()))
    return y


def vl_nneuclideanloss(x, t, dzdy=None, instanceWeights=None):
    """VL_NNEUCLIDEANLOSS(X, T [, DZDY], 'instanceWeights', w) -- mcnExtraLayers (emoVoxZoo.m:139)."""
    return _regloss(x, t, dzdy, 0, 1.0, instanceWeights, "vl_nneuclideanloss")


def vl_nnhuberloss(x, t, dzdy=None, sigma=1.0, instanceWeights=None):
    """VL_NNHUBERLOSS(X, T [, DZDY], 'sigma', s, 'instanceWeights', w) -- mcnExtraLayers (emoVoxZoo.m:147)."""
    if not sigma > 0:
        raise ValueError("vl_nnhuberloss: sigma must be positive")
    return _regloss(x, t, dzdy, 1, sigma, instanceWeights, "vl_nnhuberloss")


# --------------------------------------------------------------------------------------------
# optimiser / parameter server
# --------------------------------------------------------------------------------------------


def sgd_update(w, m, der, lr, momentum=0.9, weight_decay=5e-4, batch=1.0):
    """in-place accumulateGradients step of cnn_train_dag (trainMethod 'gradient')."""
    _lib.check(_L().xm_sgd_update(_ptr(w), _ptr(m), _ptr(der), w.numel(), float(lr),
                                  float(momentum), float(weight_decay), float(batch), _stream()))


# cnn_train_dag's 'solver' / 'solverOpts' (MatConvNet +solver [EXT]) and the nesterovUpdate arm of its default solver:
# name -> (XM_SOLVER_* kind, option defaults, uses the second state)
SOLVERS = {
    "adagrad": (0, {"epsilon": 1e-10, "rho": 1.0}, False),
    "rmsprop": (1, {"epsilon": 1e-8, "rho": 0.99}, False),
    "adadelta": (2, {"epsilon": 1e-6, "rho": 0.9}, True),
    "adam": (3, {"beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8}, True),
    "nesterov": (4, {"momentum": 0.9}, False),
}


def solver_opts(kind, solverOpts=None):
    """the solver's options with its defaults filled in; unknown solver or option names raise ValueError"""
    if kind not in SOLVERS:
        raise ValueError("unknown solver %r (one of %s)" % (kind, ", ".join(sorted(SOLVERS))))
    defaults = SOLVERS[kind][1]
    unknown = sorted(set(solverOpts or {}) - set(defaults))
    if unknown:
        raise ValueError("solver %r has no option %s (its options: %s)" %
                         (kind, ", ".join(map(repr, unknown)), ", ".join(sorted(defaults))))
    return dict(defaults, **{k: float(v) for k, v in (solverOpts or {}).items()})


def solver_coef(kind, lr, t=1, **solverOpts):
    """the four coefficient slots of xm_solver_update (include/xmodal.h) as float32.  Formed in double and rounded once, as
    MATLAB does with a double scalar expression that meets a single array: 1 - beta2 is float32(0.001), not
    1 - float32(0.999).  `t` (adam): updates so far, this one included."""
    o = solver_opts(kind, solverOpts)
    if kind == "adagrad":
        c = [o["epsilon"], o["rho"], 0.0, 0.0]
    elif kind in ("rmsprop", "adadelta"):
        c = [o["epsilon"], o["rho"], 1.0 - o["rho"], 0.0]
    elif kind == "adam":
        t = int(t)
        if t < 1:
            raise ValueError("solver 'adam': t counts the updates from 1")
        lr_t = float(lr) * np.sqrt(1.0 - o["beta2"] ** t) / (1.0 - o["beta1"] ** t)
        c = [o["epsilon"], 1.0 - o["beta1"], 1.0 - o["beta2"], lr_t]
    else:
        c = [o["momentum"], 0.0, 0.0, 0.0]
    return np.asarray(c, np.float64).astype(np.float32)


def solver_update(kind, w, s1, s2, der, lr, weight_decay, batch, t=1, **solverOpts):
    """in-place accumulateGradients step of cnn_train_dag with 'solver', @solver.<kind> (or, kind 'nesterov', with
    'nesterovUpdate'): one launch of xm_solver_update.  s1: g_sqr / adam's m / the momentum; s2: adadelta's delta_sqr /
    adam's v (None for the other kinds).  `t`: adam's update count, this update included (the caller keeps it)."""
    coef = solver_coef(kind, lr, t, **solverOpts)
    _lib.check(_L().xm_solver_update(SOLVERS[kind][0], _ptr(w), _ptr(s1), _ptr(s2), _ptr(der), w.numel(), float(lr),
                                     float(weight_decay), float(batch),
                                     coef.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float)), _stream()))


def scale_(x, a):
    """x <- a * x in place (worker-batch weighting of the BN moments before the ParameterServer exchange)."""
    _lib.check(_L().xm_scale_f32(_ptr(x), x.numel(), float(a), _stream()))


def average_update(w, der, lr, nworkers=1.0):
    """in-place trainMethod 'average' update (BN moments): w <- (1-lr) w + lr der / nworkers (denominator: 1 for a
    single worker, the GLOBAL batch size when der = sum over workers of moments * worker batch size)."""
    _lib.check(_L().xm_average_update(_ptr(w), _ptr(der), w.numel(), float(lr), float(nworkers),
                                      _stream()))


# --------------------------------------------------------------------------------------------
# batch-provider arithmetic
# --------------------------------------------------------------------------------------------


def spec_rownorm(spec):
    """getBatchEmoVoxCeleb.m:164-169 on the device; spec is H x W x 1 x N."""
    spec = _chk(spec, "SPEC")
    H, W, Cc, N = _shape4(spec)
    out = mat_empty(*spec.shape, device=spec.device)
    _lib.check(_L().xm_spec_rownorm(_ptr(spec), H, W, Cc * N, _ptr(out), _stream()))
    return out


def spec_magnitude(reim):
    """|Re + i Im| of the framing convolution's output: 1 x Wo x 2B x N -> B x Wo x 1 x N."""
    reim = _chk(reim, "REIM")
    H, Wo, C2, N = _shape4(reim)
    if H != 1 or C2 % 2:
        raise ValueError("spec_magnitude: expected a 1 x Wo x 2B x N tensor")
    out = mat_empty(C2 // 2, Wo, 1, N, device=reim.device)
    _lib.check(_L().xm_spec_magnitude(_ptr(reim), Wo, C2 // 2, N, _ptr(out), _stream()))
    return out


def resample(x, h, p, q, delay, Ly):
    """y = upfirdn(x, h, p, q) without the filter delay, Ly samples (xm_resample); x, h: 1-D device tensors."""
    y = torch.empty(int(Ly), dtype=torch.float32, device=x.device)
    _lib.check(_L().xm_resample(_ptr(x), int(x.numel()), _ptr(h), int(h.numel()), int(p), int(q), int(delay), _ptr(y),
                                int(Ly), _stream()))
    return y


WAV_MAX_RATIO = 1 << 20   # p, q of a wav_batch descriptor (xm_wav_batch resamples anything beyond to zeros)


def wav_batch(wav, noise, desc, ratio, L):
    """The L x N sample matrix of a batch (xm_wav_batch; getBatchEmoVoxCeleb.m:102-135) from the device banks `wav` /
    `noise` (1-D; `noise` may be None when no clip mixes any).  desc: N x 6 int64 HOST array {src, len, p, q, nsrc, nlen}
    per clip, ratio: N float32 HOST array -- checked here (ranges inside the banks, len >= 0, p, q in 1 .. 2^20,
    0 <= nlen <= L; ValueError otherwise) and sent up in ONE pinned, non-blocking upload."""
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    ratio = np.ascontiguousarray(ratio, dtype=np.float32).reshape(-1)
    L = int(L)
    if desc.ndim != 2 or desc.shape[1] != 6 or ratio.size != desc.shape[0]:
        raise ValueError("wav_batch: DESC must be N x 6 and RATIO must have N elements")
    if L <= 0:
        raise ValueError("wav_batch: L must be positive")
    for t, name in ((wav, "WAV"), (noise, "NOISE")):
        if t is not None and (_chk(t, name).dim() != 1 or not t.is_contiguous()):
            raise ValueError("wav_batch: %s must be a contiguous 1-D bank" % name)
    if wav is None:
        raise ValueError("wav_batch: WAV is required")
    N, wav_len, noise_len = int(desc.shape[0]), int(wav.numel()), 0 if noise is None else int(noise.numel())
    src, ln, p, q, nsrc, nlen = (desc[:, i] for i in range(6))
    if N and not ((ln >= 0).all() and (src >= 0).all() and (src + ln <= wav_len).all()):
        raise ValueError("wav_batch: a clip's [src, src + len) leaves the waveform bank")
    if N and not ((p >= 1).all() and (q >= 1).all() and (p <= WAV_MAX_RATIO).all() and (q <= WAV_MAX_RATIO).all()):
        raise ValueError("wav_batch: p, q must be in 1 .. 2^20")
    if N and not ((nlen >= 0).all() and (nlen <= L).all()):
        raise ValueError("wav_batch: nlen must be in 0 .. L")
    mixed = nlen > 0
    if N and not ((nsrc[mixed] >= 0).all() and (nsrc[mixed] + nlen[mixed] <= noise_len).all()):
        raise ValueError("wav_batch: a clip's [nsrc, nsrc + nlen) leaves the noise bank")
    z = torch.empty((N, L), dtype=torch.float32, device=wav.device)      # storage of the L x N mat
    if N:
        host = torch.empty(52 * N, dtype=torch.uint8, pin_memory=True)   # [desc | ratio]
        raw = host.numpy()
        raw[:48 * N].view(np.int64)[:] = desc.reshape(-1)
        raw[48 * N:].view(np.float32)[:] = ratio
        up = host.to(wav.device, non_blocking=True)
        _lib.check(_L().xm_wav_batch(_ptr(wav), wav_len, _ptr(noise), noise_len, C.c_void_p(up.data_ptr()),
                                     C.c_void_p(up.data_ptr() + 48 * N), N, _ptr(z), L, _stream()))
    return z.t()


def spec_bucket_batch(wav, desc, rsize, audio=None):
    """The 512 x rsize x 1 x N input of the student for N whole clips of one width bucket (xm_spec_bucket_batch;
    compute_audio_feats.m:160-185): runSpec of every clip, its rows normalised by their mean / std over ALL T frames of
    the clip, the rsize frames from f0 on.  wav: the 1-D device bank; desc: N x 3 int64 HOST array {src, len, f0} per
    clip -- checked here ([src, src + len) inside the bank, 0 <= f0, f0 + rsize <= T = floor((len - Nw) / Ns) + 1;
    ValueError otherwise) and sent up in ONE pinned, non-blocking upload.  `audio` as for batch.runSpec; both use the
    same device filter bank."""
    from . import batch as xbatch
    a = dict(fs=16000, Tw=25, Ts=10, alpha=0.97)
    a.update({k: v for k, v in (audio or {}).items() if k in a})
    Nw, Ns = int(round(1e-3 * a["Tw"] * a["fs"])), int(round(1e-3 * a["Ts"] * a["fs"]))
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    rsize = int(rsize)
    if desc.ndim != 2 or desc.shape[1] != 3:
        raise ValueError("spec_bucket_batch: DESC must be N x 3")
    if rsize <= 0:
        raise ValueError("spec_bucket_batch: RSIZE must be positive")
    if wav is None or _chk(wav, "WAV").dim() != 1 or not wav.is_contiguous():
        raise ValueError("spec_bucket_batch: WAV must be a contiguous 1-D bank")
    N, wav_len = int(desc.shape[0]), int(wav.numel())
    src, ln, f0 = (desc[:, i] for i in range(3))
    if N and not ((ln >= 0).all() and (src >= 0).all() and (src + ln <= wav_len).all()):
        raise ValueError("spec_bucket_batch: a clip's [src, src + len) leaves the waveform bank")
    T = np.where(ln >= Nw, (ln - Nw) // Ns + 1, 0)
    if N and not ((f0 >= 0).all() and (f0 + rsize <= T).all()):
        raise ValueError("spec_bucket_batch: a clip's frames [f0, f0 + rsize) leave its spectrogram")
    nfft = 1024
    bank = xbatch._spec_filter_bank(a["fs"], a["Tw"], a["Ts"], a["alpha"], nfft, wav.device)
    out = mat_empty(nfft // 2, rsize, 1, N, device=wav.device)
    if N:
        host = torch.empty(3 * N, dtype=torch.int64, pin_memory=True)
        host.numpy()[:] = desc.reshape(-1)
        up = host.to(wav.device, non_blocking=True)
        _lib.check(_L().xm_spec_bucket_batch(_ptr(wav), wav_len, C.c_void_p(up.data_ptr()), N, rsize, _ptr(bank), Nw + 1, Ns,
                                             nfft // 2, _ptr(out), _stream()))
    return out


_AGG = {"max": 0, "mean": 1, "peak": 2}   # XM_AGG_MAX / XM_AGG_MEAN / XM_AGG_PEAK


def aggregate_logits(frame_logits, first, last, agg="max"):
    """frame_logits F x E (column-major), first/last int32 device vectors (1-based, inclusive).
    agg: "max" | "mean" (getBatchEmoVoxCeleb.m:179-188) | "peak" (selectPeakLogit, run_cross_val.m:149-155: the row
    of the block holding its largest entry).  Returns (logitTarget 1 x 1 x E x N, maxLabel 1 x 1 x 1 x N)."""
    fl = _chk(frame_logits, "LOGITS")
    Fr, E = int(fl.shape[0]), int(fl.shape[1])
    N = int(first.numel())
    out = mat_empty(1, 1, E, N, device=fl.device)
    lab = mat_empty(1, 1, 1, N, device=fl.device)
    if agg not in _AGG:
        raise ValueError("unreccognised aggregator %s" % agg)
    _lib.check(_L().xm_aggregate_logits(_ptr(fl), Fr, E, C.c_void_p(first.data_ptr()),
                                        C.c_void_p(last.data_ptr()), N, _AGG[agg],
                                        _ptr(out), _ptr(lab), _stream()))
    return out, lab


def window_targets(logits, first, last, agg="max", numPredEmotions=None):
    """(logitTarget 1 x 1 x P x N, maxLabel 1 x 1 x 1 x N) of N windows straight from the teacher's 1 x 1 x E x n output
    (getBatchEmoVoxCeleb.m:30-32,145-158,179-188; xm_window_targets): what aggregate_logits on the transposed n x E
    copy, lgo(:,:,1:P,:) and max_label give, bit for bit, in one launch.  first / last: int32 device vectors, 1-based
    inclusive rows into the n frames.  agg: "max" | "mean"; numPredEmotions P defaults to E."""
    lg = _chk(logits, "LOGITS")
    one, one_, E, n = _shape4(lg)
    if one != 1 or one_ != 1:
        raise ValueError("window_targets: expected the teacher's 1 x 1 x E x n logits")
    if agg not in ("max", "mean"):
        raise ValueError("unreccognised aggregator %s" % agg)
    P = E if numPredEmotions is None else int(numPredEmotions)
    N = int(first.numel())
    for t, name in ((first, "first"), (last, "last")):
        if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or int(t.numel()) != N:
            raise ValueError("window_targets: %s must be a contiguous int32 device vector of N entries" % name)
    if not 1 <= P <= E:
        raise ValueError("window_targets: numPredEmotions %d outside 1 .. %d" % (P, E))
    out = mat_empty(1, 1, P, N, device=lg.device)
    lab = mat_empty(1, 1, 1, N, device=lg.device)
    _lib.check(_L().xm_window_targets(_ptr(lg), E, n, C.c_void_p(first.data_ptr()), C.c_void_p(last.data_ptr()), N,
                                      _AGG[agg], P, _ptr(out), _ptr(lab), _stream()))
    return out, lab


# xm_mnrfit status codes (include/xmodal.h)
MNR_CONVERGED, MNR_ITERLIMIT, MNR_NOTPD, MNR_BADINPUT = 0, 1, 2, 3


def _features(X):
    """p x n single features in MATLAB layout (p x n, or the 1 x 1 x p x n output of aggregate_logits) -> (p, n)."""
    X = _chk(X, "X")
    if X.dim() < 2 or any(int(d) != 1 for d in X.shape[:-2]):
        raise ValueError("X: expected p x n (or 1 x 1 x p x n) features")
    return int(X.shape[-2]), int(X.shape[-1])


def _labels(labels, n, device):
    if not isinstance(labels, torch.Tensor):
        raise TypeError("LABELS: expected a torch tensor")
    if not labels.is_cuda:
        raise RuntimeError("LABELS: tensor is not on the GPU; this build has no CPU path")
    if labels.numel() != n:
        raise ValueError("LABELS: %d labels for %d samples" % (labels.numel(), n))
    return labels.reshape(-1).to(device=device, dtype=torch.int32).contiguous()


def _csr(sets, device):
    """list of 1-based index lists -> (offsets int32[G+1], rows int32[nnz]) on the device, offsets on the host."""
    sets = [np.asarray(s, dtype=np.int64).reshape(-1) for s in sets]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    if offs[-1] >= 2 ** 31:
        raise ValueError("too many rows")
    rows = np.concatenate(sets).astype(np.int32) if offs[-1] else np.zeros(1, np.int32)
    return (torch.from_numpy(offs.astype(np.int32)).to(device), torch.from_numpy(rows).to(device), offs)


def mnrfit(X, labels, train_sets, k, maxIter=100, tolX=1e-6):
    """coefficients = mnrfit(double(X(:, train)'), labels(train)) for every index set in `train_sets` (1-based sample
    indices), one launch (xm_mnrfit, fp64 Newton-Raphson).  X: p x n single device features, labels: n device labels
    in 1..k.  Returns device tensors (B, status, iters, dev): B is (p+1) x (k-1) x G double in MATLAB layout (B[:, :, g]
    is the problem's `coefficients`), status (MNR_*), iters int32 and the deviance double, G each."""
    p, n = _features(X)
    lab = _labels(labels, n, X.device)
    k, G = int(k), len(train_sets)
    offs, rows, h_offs = _csr(train_sets, X.device)
    B = torch.empty(G, k - 1, p + 1, dtype=torch.float64, device=X.device).permute(2, 1, 0)
    status = torch.empty(G, dtype=torch.int32, device=X.device)
    iters = torch.empty(G, dtype=torch.int32, device=X.device)
    dev = torch.empty(G, dtype=torch.float64, device=X.device)
    _lib.check(_L().xm_mnrfit(_ptr(X), p, n, _ptr(lab), k, _ptr(offs), _ptr(rows), int(h_offs[-1]), G, int(maxIter),
                              float(tolX), _ptr(B), _ptr(dev), _ptr(iters), _ptr(status), _stream()))
    return B, status, iters, dev


def mnrval(B, X, val_sets, labels=None):
    """preds = mnrval(B(:, :, g), double(X(:, val)')) for every index set of `val_sets`, one launch (xm_mnrval).
    B: (p+1) x (k-1) x G double device coefficients (what mnrfit returns), X: p x n single device features,
    labels (optional): n device labels.  Returns (probs, preds, conf): per problem an n_g x k double tensor and an
    n_g int32 tensor of 1-based classes (first maximum wins), and conf = G x k x k int32 counts
    [true label - 1, predicted - 1] as confusionmat(..., 'Order', 1:k) (None without labels)."""
    p, n = _features(X)
    if not isinstance(B, torch.Tensor) or B.dtype != torch.float64:
        raise TypeError("B: expected a double-precision torch tensor")
    if not B.is_cuda:
        raise RuntimeError("B: tensor is not on the GPU; this build has no CPU path")
    Bm = B.reshape(B.shape[0], B.shape[1], -1) if B.dim() >= 2 else B
    if Bm.dim() != 3 or int(Bm.shape[0]) != p + 1 or not Bm.permute(2, 1, 0).is_contiguous():
        raise ValueError("B: expected (p+1) x (k-1) x G coefficients in MATLAB layout")
    k, G = int(Bm.shape[1]) + 1, int(Bm.shape[2])
    if G != len(val_sets):
        raise ValueError("mnrval: %d coefficient sets for %d index sets" % (G, len(val_sets)))
    lab = None if labels is None else _labels(labels, n, X.device)
    offs, rows, h_offs = _csr(val_sets, X.device)
    nnz = int(h_offs[-1])
    probs = torch.empty(max(nnz, 1), k, dtype=torch.float64, device=X.device)
    preds = torch.empty(max(nnz, 1), dtype=torch.int32, device=X.device)
    conf = None if lab is None else torch.empty(G, k, k, dtype=torch.int32, device=X.device)
    _lib.check(_L().xm_mnrval(_ptr(Bm), _ptr(X), p, n, k, _ptr(offs), _ptr(rows), nnz, G, _ptr(lab), _ptr(probs),
                              _ptr(preds), _ptr(conf), _stream()))
    sl = [slice(int(h_offs[g]), int(h_offs[g + 1])) for g in range(G)]
    return ([probs[s] for s in sl], [preds[s] for s in sl],
            None if conf is None else conf.transpose(1, 2))


# xm_roc status codes (include/xmodal.h)
ROC_OK, ROC_NAN, ROC_BADINPUT = 0, 1, 2


def roc_sets(sets, n, device):
    """index sets (1-based rows of an n-row score matrix) checked on the host and uploaded once: the tuple can be
    passed to roc() as `sets` any number of times."""
    sets = [np.asarray(s, dtype=np.int64).reshape(-1) for s in sets]
    for g, s in enumerate(sets):
        if s.size and (s.min() < 1 or s.max() > n):
            raise ValueError("roc: set %d holds a row outside 1..%d" % (g + 1, n))
    return _csr(sets, device)


def roc_geometry():
    """(tile, wave_span, threads, hist_classes_max) of the xm_roc / xm_label_hist kernels (xm_roc_geometry; no device call)"""
    v = [C.c_int(0) for _ in range(4)]
    _lib.check(_L().xm_roc_geometry(*[C.byref(t) for t in v]))
    return tuple(int(t.value) for t in v)


def roc(scores, cls, sets, want_curve=False):
    """[~, ~, info] = vl_roc(labels, scores) (vlfeat, default options; student_stats.m:109-115) for every index set of
    `sets` (1-based rows, or the tuple roc_sets() made of them) and every column of `scores`, one call of xm_roc.
    scores: n x E single device scores, cls: n device classes (1-based); problem (g, c) labels a row +1 where cls == c + 1 and -1 elsewhere.
    Returns a dict of device tensors: auc (G x E double), area (G x E int64: S, auc = S / (p n)), p, n, retrieved and
    status (G x E int32, ROC_*), offsets (the host CSR offsets of the sets) and, with want_curve, perm and tp
    (E x nnz int32: row c holds, set after set, the rows by descending score and the positives among the first
    i + 1 of them)."""
    scores = _chk(scores, "SCORES")
    if scores.dim() != 2:
        raise ValueError("SCORES: expected n x E scores")
    n, E = int(scores.shape[0]), int(scores.shape[1])
    lab = _labels(cls, n, scores.device)
    offs, rows, h_offs = sets if isinstance(sets, tuple) else roc_sets(sets, n, scores.device)
    G, nnz = len(h_offs) - 1, int(h_offs[-1])
    dev = scores.device
    auc = torch.empty(G, E, dtype=torch.float64, device=dev)
    area = torch.empty(G, E, dtype=torch.int64, device=dev)
    counts = torch.empty(G, E, 3, dtype=torch.int32, device=dev)
    status = torch.empty(G, E, dtype=torch.int32, device=dev)
    perm = tp = None
    if want_curve:
        perm = torch.empty(E, max(nnz, 1), dtype=torch.int32, device=dev)
        tp = torch.empty(E, max(nnz, 1), dtype=torch.int32, device=dev)
    _lib.check(_L().xm_roc(_ptr(scores), n, E, _ptr(lab), _ptr(offs), _ptr(rows), nnz, G, _ptr(auc), _ptr(area),
                           _ptr(counts), _ptr(status), _ptr(perm), _ptr(tp), _stream()))
    out = {"auc": auc, "area": area, "p": counts[:, :, 0], "n": counts[:, :, 1], "retrieved": counts[:, :, 2],
           "status": status, "offsets": h_offs}
    if want_curve:
        out["perm"], out["tp"] = perm[:, :nnz], tp[:, :nnz]
    return out


def vl_roc(labels, scores):
    """[TPR, TNR, INFO] = VL_ROC(LABELS, SCORES) of vlfeat for one problem (default options): labels in {-1, 0, +1}
    (host or device), scores a device vector.  A 0 label is ignored: counted in neither p nor n and it advances
    neither cumulative sum -- those rows are left out of the index set, the others keep their relative order.
    Returns (tpr, tnr, info) as numpy doubles of retrieved + 1 points and info = {'auc', 'p', 'n', 'status'};
    info.eer and the plotting branch are not provided (student_stats.m reads info.auc only)."""
    if not isinstance(scores, torch.Tensor):
        raise TypeError("SCORES: expected a torch tensor")
    if not scores.is_cuda:
        raise RuntimeError("SCORES: tensor is not on the GPU; this build has no CPU path")
    lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    lab = lab.reshape(-1)
    s = scores.reshape(-1).to(torch.float32).contiguous()[:, None]
    if lab.size != s.shape[0]:
        raise ValueError("vl_roc: %d labels for %d scores" % (lab.size, s.shape[0]))
    if lab.size == 0:
        z = np.zeros(1)
        return z, 1 - z, {"auc": 0.0, "p": 0, "n": 0, "status": ROC_OK}
    cls = torch.from_numpy(np.where(lab > 0, 1, 2).astype(np.int32)).to(s.device)
    r = roc(s, cls, [np.nonzero(lab != 0)[0] + 1], want_curve=True)
    p, n, ret = (int(r[k][0, 0]) for k in ("p", "n", "retrieved"))
    tp = np.concatenate([[0], r["tp"][0, :ret].cpu().numpy().astype(np.float64)])
    fp = np.arange(ret + 1, dtype=np.float64) - tp
    tpr, fpr = tp / max(p, 1e-10), fp / max(n, 1e-10)
    return tpr, 1 - fpr, {"auc": float(r["auc"][0, 0]), "p": p, "n": n, "status": int(r["status"][0, 0])}


def label_hist(x, dim=None, bins=None):
    """histcounts(labels, 0.5:E+0.5) with [~, labels] = max(x, [], dim): exact int64 counts of the first maximum per
    sample, one launch (xm_label_hist).  x: N x E (dim = 2, the default for 2-D input: vertcat(wavLogits{:}),
    student_stats.m:65, teacher_stats.m:28-29) or 1 x 1 x E x N (dim = 3, as max_label).  `bins` (E int64 device
    counts) is added to when given, so blocks of frames can be streamed through."""
    x = _chk(x, "X")
    if dim is None:
        dim = 2 if x.dim() == 2 else 3
    if dim == 2 and x.dim() == 2:
        N, E, sample_major = int(x.shape[0]), int(x.shape[1]), 1
    elif dim == 3:
        H, W, E, N = _shape4(x)
        if H != 1 or W != 1:
            raise ValueError("label_hist: X must be 1 x 1 x E x N for dim = 3")
        sample_major = 0
    else:
        raise ValueError("label_hist: dim = 2 needs an N x E array, dim = 3 a 1 x 1 x E x N array")
    if bins is None:
        bins = torch.zeros(E, dtype=torch.int64, device=x.device)
    elif bins.dtype != torch.int64 or not bins.is_cuda or bins.numel() != E or not bins.is_contiguous():
        raise ValueError("label_hist: bins must be E contiguous int64 device counts")
    _lib.check(_L().xm_label_hist(_ptr(x), N, E, sample_major, _ptr(bins), _stream()))
    return bins


def max_label(lgo):
    """[~, maxLabel] = max(lgo, [], 3) -- getBatchEmoVoxCeleb.m:32; lgo is 1 x 1 x C x N."""
    lgo = _chk(lgo, "LGO")
    H, W, Cc, N = _shape4(lgo)
    lab = mat_empty(1, 1, 1, N, device=lgo.device)
    _lib.check(_L().xm_max_label(_ptr(lgo), Cc, N, _ptr(lab), _stream()))
    return lab


def class_stats(x, labels, correct, population):
    """dagnn.ErrorStats bookkeeping: correct[c] / population[c] += ... for the samples of this batch
    (x: 1 x 1 x C x N scores, labels: 1-based, correct / population: C-element device arrays)."""
    x, labels = _chk(x, "X"), _chk(labels, "LABELS")
    H, W, Cc, N = _shape4(x)
    if H != 1 or W != 1 or labels.numel() != N:
        raise ValueError("class_stats: X must be 1 x 1 x C x N with one label per sample")
    if correct.numel() != Cc or population.numel() != Cc:
        raise ValueError("class_stats: counters must have C elements")
    _lib.check(_L().xm_class_stats(_ptr(x), _ptr(labels), Cc, N, _ptr(correct), _ptr(population), _stream()))


# --------------------------------------------------------------------------------------------
# teacher logits per track (fetch_emovoxceleb_imdb.m:119-148, sample_audio.m:69-74)
# --------------------------------------------------------------------------------------------


def _ivec(t, name, count=None):
    """contiguous int32 device vector (no CPU path, as _chk)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s: tensor is not on the GPU; this build has no CPU path" % name)
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise TypeError("%s: expected a contiguous int32 tensor" % name)
    if count is not None and t.numel() != count:
        raise ValueError("%s: %d entries, expected %d" % (name, t.numel(), count))
    return t.reshape(-1)


def group_rows(ids, keys, key_max=None):
    """wavLogits{ii} = logits(denseFramesWavIds == images.id(ii), :) for every ii at once, as index sets
    (fetch_emovoxceleb_imdb.m:140-148; xm_group_rows).  ids: int32 device vector, the wav id of each frame, in any
    order; keys: the T distinct ids (host sequence) that own a group, each in 0 < key <= key_max (default max(keys)).
    Returns device tensors (offsets int32[T + 1], rows int32[n] -- 1-based, stable, the first nnz entries --, nnz
    int32[1]); no result is downloaded.  The keys are uploaded from pageable memory on every call, a copy that makes
    the host wait for the stream: call it after a loop, not inside one.  Duplicate keys raise XmError(XM_EINVAL)."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1)
    T = int(keys.size)
    if key_max is None:
        key_max = int(keys.max()) if T else 0
    if T and (keys.min() < 1 or keys.max() > key_max):
        raise _lib.XmError(1, "group_rows: keys must lie in 1..key_max")
    if np.unique(keys).size != T:
        raise _lib.XmError(1, "group_rows: duplicate keys")
    ids = _ivec(ids, "IDS")
    n = int(ids.numel())
    dkeys = torch.from_numpy(keys.astype(np.int32)).to(ids.device)
    offsets = torch.empty(T + 1, dtype=torch.int32, device=ids.device)
    rows = torch.empty(max(n, 1), dtype=torch.int32, device=ids.device)
    nnz = torch.empty(1, dtype=torch.int32, device=ids.device)
    _lib.check(_L().xm_group_rows(_ptr(ids), n, _ptr(dkeys), T, int(key_max), _ptr(offsets), _ptr(rows), _ptr(nnz),
                                  _stream()))
    return offsets, rows[:n], nnz


def _logit_matrix(mat, name):
    mat = _chk(mat, name)
    if mat.dim() != 2:
        raise ValueError("%s: expected an F x E matrix" % name)
    return mat, int(mat.shape[0]), int(mat.shape[1])


def gather_rows(mat, rows=None, row0=0, n=None):
    """F x E column-major matrix -> 1 x 1 x E x n (xm_gather_rows): sample i is matrix row rows[i] (1-based int32 device
    list) or, without a list, row row0 + i + 1 for i < n."""
    mat, F, E = _logit_matrix(mat, "MAT")
    if rows is not None:
        rows = _ivec(rows, "ROWS")
        n = int(rows.numel())
    elif n is None:
        n = F - int(row0)
    out = mat_empty(1, 1, E, max(int(n), 0), device=mat.device)
    _lib.check(_L().xm_gather_rows(_ptr(mat), F, E, int(row0), _ptr(rows), int(n), _ptr(out), _stream()))
    return out


def scatter_rows(packed, mat, rows=None, row0=0):
    """logits(batch, :) = out' (fetch_emovoxceleb_imdb.m:130-131; xm_scatter_rows): the 1 x 1 x E x n output of a network
    into rows row0 + 1 .. row0 + n of the F x E column-major matrix `mat` (in place), or into the rows of a 1-based int32
    device list.  Returns mat."""
    packed = _chk(packed, "PACKED")
    mat, F, E = _logit_matrix(mat, "MAT")
    H, W, Cc, n = _shape4(packed)
    if H != 1 or W != 1 or Cc != E:
        raise ValueError("scatter_rows: PACKED must be 1 x 1 x %d x n" % E)
    if rows is not None:
        rows = _ivec(rows, "ROWS", n)
    _lib.check(_L().xm_scatter_rows(_ptr(packed), n, E, _ptr(mat), F, int(row0), _ptr(rows), _stream()))
    return mat


def track_peaks(logits, offsets, rows=None):
    """sample_audio.m:69-74 for every track in one launch (xm_track_peaks): [~, m] = max(x(:)), [frameIdx, tag] =
    ind2sub(size(x), m) and max(x, [], 1) of the groups rows[offsets[t] : offsets[t + 1]] (1-based rows; rows = None:
    the contiguous rows offsets[t] + 1 .. offsets[t + 1]) of the F x E matrix.  offsets: int32 device vector of T + 1.
    Returns (frame_idx int32[T], tag int32[T], maxed 1 x 1 x E x T), all on the device; ties go to the lowest emotion,
    then the lowest position; an empty group gives 0, 0, -Inf.  With a row list the largest offset is read back to
    check it against the list (one device synchronisation); without one nothing is synchronised."""
    logits, F, E = _logit_matrix(logits, "LOGITS")
    offsets = _ivec(offsets, "OFFSETS")
    T = int(offsets.numel()) - 1
    if T < 0:
        raise ValueError("track_peaks: OFFSETS needs at least one entry")
    if rows is not None:
        rows = _ivec(rows, "ROWS")
        if T and int(offsets.max()) > int(rows.numel()):
            raise ValueError("track_peaks: OFFSETS reach past the %d listed rows" % int(rows.numel()))
    frame_idx = torch.empty(max(T, 1), dtype=torch.int32, device=logits.device)
    tag = torch.empty(max(T, 1), dtype=torch.int32, device=logits.device)
    maxed = mat_empty(1, 1, E, T, device=logits.device)
    _lib.check(_L().xm_track_peaks(_ptr(logits), F, E, _ptr(offsets), _ptr(rows), T, _ptr(frame_idx), _ptr(tag),
                                   _ptr(maxed), _stream()))
    return frame_idx[:T], tag[:T], maxed


def crop_resize_face(src, average_image, image_size=(224, 224), crop=1 / 1.6):
    """getImageBatch of fetch_emovoxceleb_imdb.m:152-193 from decoded frames (Hin x Win x 3 x N, values
    0..255): centre crop 1/1.6 -> bilinear resize -> uint8 -> grey -> x3 -> minus averageImage, fused."""
    src = _chk(src, "SRC")
    Hin, Win, c3, N = _shape4(src)
    if c3 != 3:
        raise ValueError("crop_resize_face: expected Hin x Win x 3 x N")
    avg = (C.c_float * 3)(*[float(v) for v in np.ravel(average_image)[:3]])
    out = mat_empty(int(image_size[0]), int(image_size[1]), 3, N, device=src.device)
    _lib.check(_L().xm_crop_resize_face(_ptr(src), Hin, Win, N, float(crop), int(image_size[0]),
                                        int(image_size[1]), avg, _ptr(out), _stream()))
    return out


def normalize_face(rgb, average_image):
    """fetch_emovoxceleb_imdb.m:176-193: grey -> x3 -> minus averageImage; rgb H x W x 3 x N."""
    rgb = _chk(rgb, "RGB")
    H, W, c3, N = _shape4(rgb)
    if c3 != 3:
        raise ValueError("normalize_face: expected H x W x 3 x N")
    avg = (C.c_float * 3)(*[float(v) for v in np.ravel(average_image)[:3]])
    out = mat_empty(H, W, 3, N, device=rgb.device)
    _lib.check(_L().xm_normalize_face(_ptr(rgb), H, W, N, avg, _ptr(out), _stream()))
    return out


# --------------------------------------------------------------------------------------------
# vl_nnaffinegrid / vl_nnbilinearsampler and the fused FER+ batch (getBatchFerPlus, ferplus_baselines.m:153-221)
# --------------------------------------------------------------------------------------------


def vl_nnaffinegrid(A, sz, dzdy=None):
    """GRID = vl_nnaffinegrid(A, [Ho Wo]) / DA = vl_nnaffinegrid(A, [Ho Wo], DZDY).  A is 1 x 1 x 6 x N, GRID
    2 x Ho x Wo x N: GRID(1) = c1 y + c3 x + c5, GRID(2) = c2 y + c4 x + c6 over linspace(-1, 1, Ho / Wo)
    (include/xmodal.h; parity with MatConvNet unpinned)."""
    A = _chk(A, "A")
    Ho, Wo = _pair(sz, "SZ")
    N = int(A.numel()) // 6
    if A.numel() != 6 * N or N < 1:
        raise ValueError("vl_nnaffinegrid: A must be 1 x 1 x 6 x N")
    if dzdy is not None:
        d = _chk(dzdy, "DZDY")
        if d.numel() != 2 * Ho * Wo * N:
            raise ValueError("vl_nnaffinegrid: DZDY must be 2 x Ho x Wo x N")
        dA = mat_empty(1, 1, 6, N, device=A.device)
        _lib.check(_L().xm_nnaffinegrid_backward(_ptr(d), N, Ho, Wo, _ptr(dA), _stream()))
        return dA
    grid = mat_empty(2, Ho, Wo, N, device=A.device)
    _lib.check(_L().xm_nnaffinegrid(_ptr(A), N, Ho, Wo, _ptr(grid), _stream()))
    return grid


def vl_nnbilinearsampler(X, grid, dzdy=None):
    """Y = vl_nnbilinearsampler(X, GRID) / [DX, DGRID] = vl_nnbilinearsampler(X, GRID, DZDY).  X is H x W x C x N,
    GRID 2 x Ho x Wo x No with No a multiple of N (output image m reads input image m // (No / N)); zero padding.
    DX is accumulated with float atomics (its last bits depend on scheduling); DGRID has fixed bits."""
    X, grid = _chk(X, "X"), _chk(grid, "GRID")
    H, W, Cc, N = _shape4(X)
    two, Ho, Wo, No = _shape4(grid)
    if two != 2:
        raise ValueError("vl_nnbilinearsampler: GRID must be 2 x Ho x Wo x No")
    if No % N:
        raise ValueError("vl_nnbilinearsampler: %d grids for %d images (must be a multiple)" % (No, N))
    if dzdy is not None:
        d = _chk(dzdy, "DZDY")
        if tuple(_shape4(d)) != (Ho, Wo, Cc, No):
            raise ValueError("vl_nnbilinearsampler: DZDY must be Ho x Wo x C x No")
        dX = mat_empty(H, W, Cc, N, device=X.device)
        dG = mat_empty(2, Ho, Wo, No, device=X.device)
        _lib.check(_L().xm_nnbilinearsampler_backward(_ptr(X), H, W, Cc, N, _ptr(grid), Ho, Wo, No, _ptr(d), _ptr(dX),
                                                      _ptr(dG), _stream()))
        return dX, dG
    Y = mat_empty(Ho, Wo, Cc, No, device=X.device)
    _lib.check(_L().xm_nnbilinearsampler(_ptr(X), H, W, Cc, N, _ptr(grid), Ho, Wo, No, _ptr(Y), _stream()))
    return Y


def ferplus_batch(grey, transforms, flips, average_image, image_size=(224, 224)):
    """the data path of getBatchFerPlus (ferplus_baselines.m:182-213) in one kernel: grey H x W x 1 x N (0..255) ->
    fliplr where flips[n] -> x3 minus averageImage -> affine grid of `transforms` (1 x 1 x 6 x N) -> bilinear sampler
    at image_size.  `flips`: int32 device tensor of N entries, or None.  Returns Ho x Wo x 3 x N."""
    grey, transforms = _chk(grey, "GREY"), _chk(transforms, "TRANSFORMS")
    H, W, c1, N = _shape4(grey)
    if c1 != 1:
        raise ValueError("ferplus_batch: expected H x W x 1 x N greyscale images")
    if transforms.numel() != 6 * N:
        raise ValueError("ferplus_batch: TRANSFORMS must be 1 x 1 x 6 x N")
    if flips is not None:
        if not (isinstance(flips, torch.Tensor) and flips.is_cuda):
            raise RuntimeError("FLIPS: tensor is not on the GPU; this build has no CPU path")
        if flips.dtype != torch.int32 or flips.numel() != N or not flips.is_contiguous():
            raise ValueError("ferplus_batch: FLIPS must be a contiguous int32 tensor of N entries")
    Ho, Wo = _pair(image_size, "IMAGE_SIZE")
    avg = (C.c_float * 3)(*[float(v) for v in np.ravel(average_image)[:3]])
    out = mat_empty(Ho, Wo, 3, N, device=grey.device)
    _lib.check(_L().xm_ferplus_batch(_ptr(grey), H, W, N, _ptr(flips), _ptr(transforms), Ho, Wo, avg, _ptr(out),
                                     _stream()))
    return out


# --------------------------------------------------------------------------------------------
# vl_imreadjpeg (fetch_emovoxceleb_imdb.m:160-172, compute_visual_feats.m:130-143): baseline JPEG decode on the device,
# progressive files too with progressive=True
# --------------------------------------------------------------------------------------------
JPEG_DESC, JPEG_LANE, JPEG_QT_BYTES, JPEG_HT_BYTES = 24, 4, 128, 1024          # include/xmodal.h XM_JPEG_*
JPEG_OK, JPEG_TRUNCATED, JPEG_BADCODE = 0, 1, 2
JPEG_SCAN = 24                                                                  # XM_JPEG_SCAN: int64 per scan row


def jpeg_plan(files, stage=None, progressive=False):
    """The host side of imreadjpeg (xm_jpeg_plan; touches no device): `files` is a list of bytes.  Lays one staging
    buffer out as [file bytes | desc | lanes | tables] (16-byte aligned parts), parses every header into it and returns
    (stage, plan): `stage` a uint8 numpy array (`stage(nbytes)`, when given, allocates it -- imreadjpeg hands out
    pinned memory) and plan = dict(N, nbytes, desc, lanes, tables: (offset, used bytes) in the buffer, sizes: the
    eight int64 of xm_jpeg_plan).  An unsupported or malformed file raises _lib.XmError naming its index.
    progressive=True plans with xm_jpeg_plan_prog instead, which also accepts progressive (SOF2) files: the buffer is
    [file bytes | desc | scans | lanes | tables], the plan has `scans` too and the eleven sizes of xm_jpeg_plan_prog, and
    jpeg_decode runs it through xm_jpeg_decode_batch_prog."""
    N = len(files)
    lens = np.array([len(f) for f in files], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    up = lambda v: (int(v) + 15) & ~15
    nbytes = int(offsets[-1])
    lanes_cap = N + 1024
    scans_cap = 16 * N if progressive else 0
    tab_cap = N * (3 * JPEG_QT_BYTES + (24 if progressive else 6) * JPEG_HT_BYTES)
    while True:
        o_desc = up(nbytes + 1)
        o_scans = up(o_desc + 8 * JPEG_DESC * N)
        o_lanes = up(o_scans + 8 * JPEG_SCAN * scans_cap)
        o_tab = up(o_lanes + 8 * JPEG_LANE * lanes_cap)
        total = up(o_tab + tab_cap)
        buf = stage(total) if stage is not None else np.empty(total, np.uint8)
        for f, o in zip(files, offsets):
            buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
        buf[nbytes:o_desc] = 0
        sizes = np.zeros(11 if progressive else 8, np.int64)
        base = buf.ctypes.data
        if progressive:
            rc = _L().xm_jpeg_plan_prog(C.c_void_p(base), C.c_void_p(offsets.ctypes.data), N, C.c_void_p(base + o_desc),
                                        C.c_void_p(base + o_scans), scans_cap, C.c_void_p(base + o_lanes), lanes_cap,
                                        C.c_void_p(base + o_tab), tab_cap, C.c_void_p(sizes.ctypes.data))
            if rc == 2 and (int(sizes[8]) > scans_cap or int(sizes[6]) > lanes_cap or int(sizes[0]) > tab_cap):
                scans_cap, lanes_cap, tab_cap = (max(scans_cap, int(sizes[8])), max(lanes_cap, int(sizes[6])),
                                                 max(tab_cap, int(sizes[0])))          # XM_ENOMEM: the need is reported
                continue
        else:
            rc = _L().xm_jpeg_plan(C.c_void_p(base), C.c_void_p(offsets.ctypes.data), N, C.c_void_p(base + o_desc),
                                   C.c_void_p(base + o_lanes), lanes_cap, C.c_void_p(base + o_tab), tab_cap,
                                   C.c_void_p(sizes.ctypes.data))
            if rc == 2 and int(sizes[6]) > lanes_cap:          # XM_ENOMEM: more restart intervals than assumed
                lanes_cap = int(sizes[6])
                continue
        _lib.check(rc)
        break
    plan = dict(N=N, nbytes=nbytes, sizes=sizes, desc=(o_desc, 8 * JPEG_DESC * N),
                lanes=(o_lanes, 8 * JPEG_LANE * int(sizes[6])), tables=(o_tab, int(sizes[0])), total=total)
    if progressive:
        plan["scans"] = (o_scans, 8 * JPEG_SCAN * int(sizes[8]))
    return buf, plan


def jpeg_split_geometry():
    """(segments per pass, launches) of the segment-parallel entropy decode (xm_jpeg_split_geometry; no device call)"""
    spp, launches = C.c_int(0), C.c_int(0)
    _lib.check(_L().xm_jpeg_split_geometry(C.byref(spp), C.byref(launches)))
    return spp.value, launches.value


def jpeg_decode(buf, plan, *, want_pixels=True, resize=None, crop=1.0, average_image=None, device=None, split=None,
                return_rounds=False):
    """uploads a planned staging buffer (non-blocking, three slices of the one pinned buffer) and enqueues
    xm_jpeg_decode_batch.  Returns (pixels ragged float32 | None, faces Ho x Wo x 3 x N | None, status int32[N], desc
    numpy N x 24).  Nothing is synchronised.  split=seg_bytes (a multiple of 16 in 16 .. 65536) decodes the entropy data
    segment-parallel (xm_jpeg_decode_batch_split): the same pixels, faces and status bit for bit; return_rounds=True then
    appends the int32 device vector of decode rounds per lane.  A plan made with progressive=True goes through
    xm_jpeg_decode_batch_prog (one entropy launch per level of the batch's scans; no split)."""
    prog = "scans" in plan
    if prog and split is not None:
        raise ValueError("jpeg_decode: split does not apply to a progressive plan")
    if split is None and return_rounds:
        raise ValueError("jpeg_decode: return_rounds needs split")
    if split is not None and (int(split) != split or not 16 <= split <= 65536 or split % 16):
        raise ValueError("jpeg_decode: split must be a multiple of 16 in 16 .. 65536 (got %r)" % (split,))
    device = device or _dev()
    N, sizes = plan["N"], plan["sizes"]
    host = torch.from_numpy(buf) if isinstance(buf, np.ndarray) else buf
    dev = torch.empty(plan["total"], dtype=torch.uint8, device=device)
    head = plan["desc"][0] + plan["desc"][1]
    with torch.cuda.device(device):
        dev[:head].copy_(host[:head], non_blocking=True)
        for o, n in (plan["lanes"], plan["tables"]) + ((plan["scans"],) if prog else ()):
            dev[o:o + n].copy_(host[o:o + n], non_blocking=True)
        pixels = torch.empty(int(sizes[5]), dtype=torch.float32, device=device) if want_pixels else None
        faces, avg, Ho, Wo = None, None, 0, 0
        if resize is not None:
            Ho, Wo = _pair(resize, "RESIZE")
            faces = mat_empty(Ho, Wo, 3, N, device=device)
            if average_image is not None:
                avg = (C.c_float * 3)(*[float(v) for v in np.ravel(average_image)[:3]])
        status = torch.empty(N, dtype=torch.int32, device=device)
        p = dev.data_ptr()
        args = [C.c_void_p(p), plan["nbytes"], C.c_void_p(p + plan["desc"][0]), N, C.c_void_p(p + plan["lanes"][0]),
                int(sizes[6]), C.c_void_p(p + plan["tables"][0]), int(sizes[1]), int(sizes[2]), int(sizes[3]), int(sizes[4]),
                int(sizes[5]), _ptr(pixels), _ptr(faces), float(crop), Ho, Wo, avg, _ptr(status)]
        rounds = None
        if prog:
            _lib.check(_L().xm_jpeg_decode_batch_prog(*args, C.c_void_p(p + plan["scans"][0]), int(sizes[8]), int(sizes[9]),
                                                      int(sizes[10]), _stream()))
        elif split is None:
            _lib.check(_L().xm_jpeg_decode_batch(*args, _stream()))
        else:
            if return_rounds:
                rounds = torch.empty(int(sizes[6]), dtype=torch.int32, device=device)
            _lib.check(_L().xm_jpeg_decode_batch_split(*args, int(split), _ptr(rounds), _stream()))
    desc = np.array(buf[plan["desc"][0]:plan["desc"][0] + plan["desc"][1]]).view(np.int64).reshape(N, JPEG_DESC)
    return (pixels, faces, status, desc, rounds) if return_rounds else (pixels, faces, status, desc)


def _pinned(nbytes):
    return torch.empty(int(nbytes), dtype=torch.uint8, pin_memory=True).numpy()


def imreadjpeg(files, resize=None, crop_size=None, crop_location="center", interpolation="bilinear", pack=True,
               num_threads=None, *, prefetch=False, average_image=None, device=None, return_status=False, split=None,
               progressive=False):
    """vl_imreadjpeg (fetch_emovoxceleb_imdb.m:160-172, compute_visual_feats.m:130-143) for baseline JPEG files, decoded
    on the device: `files` is a list of bytes or of paths.  Option names follow vl_imreadjpeg; `num_threads` is accepted
    and ignored (there are no decoder threads), only 'center' and 'bilinear' exist, `prefetch` raises.
      no resize                    a list of H x W x 3 device tensors (single, 0..255), one per file
      resize, average_image        the teacher's input Ho x Wo x 3 x N: centre crop of relative size crop_size, bilinear
                                   resize, uint8 rounding, rgb2gray, x3, minus average_image -- per image bit for bit
                                   crop_resize_face of its decoded pixels
      resize alone                 the resized R, G, B pack Ho x Wo x 3 x N (the same resampler)
    The bytes, descriptors and tables go up through one pinned staging buffer with non-blocking copies and the call does
    not synchronise; return_status=True also returns the int32 device vector of JPEG_OK / JPEG_TRUNCATED / JPEG_BADCODE
    bits.  Progressive, arithmetic-coded, 12-bit, multi-scan, CMYK files and unusual sampling factors raise before
    anything is launched, with the index of the file; there is no host decode to fall back to.  split=seg_bytes: the
    segment-parallel entropy decode of jpeg_decode, for files without restart markers; the same result bit for bit.
    progressive=True also reads progressive (SOF2) files, as vl_imreadjpeg does: every scan script T.81 allows, files that
    end after any scan; a baseline file in such a batch gives what it gives without the option.  A scan script libjpeg
    would only warn about raises.  The option excludes split=."""
    if progressive and split is not None:
        raise ValueError("imreadjpeg: progressive=True and split= exclude each other (progressive scans are not decoded "
                         "segment-parallel)")
    if prefetch:
        raise ValueError("imreadjpeg: 'Prefetch' is not supported: the call already returns without waiting")
    if str(crop_location).lower() != "center":
        raise ValueError("imreadjpeg: only CropLocation 'center' exists (got %r)" % (crop_location,))
    if str(interpolation).lower() != "bilinear":
        raise ValueError("imreadjpeg: only Interpolation 'bilinear' exists (got %r)" % (interpolation,))
    if not torch.cuda.is_available():
        raise RuntimeError("imreadjpeg needs a GPU; this build has no CPU path")
    if resize is None and (crop_size is not None or average_image is not None):
        raise ValueError("imreadjpeg: crop_size and average_image need resize")
    datas = []
    for f in files:
        if isinstance(f, (bytes, bytearray, memoryview)):
            datas.append(bytes(f))
        else:
            with open(f, "rb") as fh:
                datas.append(fh.read())
    if not datas:
        return ([], None) if return_status else []
    buf, plan = jpeg_plan(datas, stage=_pinned, progressive=progressive)
    pixels, faces, status, desc = jpeg_decode(buf, plan, want_pixels=resize is None, resize=resize,
                                              crop=1.0 if crop_size is None else float(crop_size),
                                              average_image=average_image, device=device, split=split)
    if resize is not None:
        out = faces
    else:
        out = []
        for d in desc:
            H, W, o = int(d[2]), int(d[3]), int(d[21])
            out.append(pixels[o:o + 3 * H * W].view(3, W, H).permute(2, 1, 0))
    return (out, status) if return_status else out


# --------------------------------------------------------------------------------------------
# vl_imreadjpeg with MatConvNet's crop, flip, filter and colour options [EXT; DESIGN section 24 is the specification]: one
# device stage (xm_imread_transform_batch) behind the decoders above.  imreadjpeg itself stays the narrow path.
# --------------------------------------------------------------------------------------------
IMREAD_ROW, IMREAD_OPTS, IMREAD_DRAWS, IMREAD_SIZES = 44, 24, 10, 8             # include/xmodal.h XM_IMREAD_*
IMREAD_FILTERS = {"box": 0, "bilinear": 1, "bicubic": 2}
_IMREAD_FLAGS = ("pack", "flip", "gpu", "verbose", "prefetch")
_IMREAD_VALUED = ("resize", "cropsize", "cropanisotropy", "croplocation", "interpolation", "subtractaverage", "brightness",
                  "contrast", "saturation", "numthreads")


def imread_options(options):
    """MatConvNet's option list ('Pack', 'Resize', [224 224], 'Flip', 'CropSize', [0.35 1] ...) -> dict keyed by the
    lower-case names; names are matched without regard to case (vl_argparse).  'Pack', 'Flip', 'Gpu', 'Verbose' and
    'Prefetch' are flags (a bool may follow); 'Prefetch' raises; an unknown option raises with its name."""
    out, i, options = {}, 0, list(options)
    while i < len(options):
        name = options[i]
        if not isinstance(name, str):
            raise ValueError("vl_imreadjpeg: expected an option name at position %d, got %r" % (i, name))
        key = name.lower()
        i += 1
        if key in _IMREAD_FLAGS:
            val = True
            if i < len(options) and isinstance(options[i], (bool, np.bool_)):
                val = bool(options[i])
                i += 1
        elif key in _IMREAD_VALUED:
            if i >= len(options):
                raise ValueError("vl_imreadjpeg: option '%s' needs a value" % name)
            val = options[i]
            i += 1
        else:
            raise ValueError("vl_imreadjpeg: unknown option '%s'" % name)
        out[key] = val
    if out.get("prefetch"):
        raise ValueError("vl_imreadjpeg: 'Prefetch' is not supported: the call already returns without waiting")
    return out


def imread_opts_vector(opt, antialias=False):
    """the XM_IMREAD_OPTS doubles of xm_imread_plan from a dict of imread_options, and the SubtractAverage array or None"""
    v = np.zeros(IMREAD_OPTS, np.float64)
    if opt.get("resize") is not None:
        r = np.ravel(np.asarray(opt["resize"], np.float64))
        if r.size == 1:
            v[0], v[1] = 2, r[0]
        elif r.size == 2:
            v[0], v[1], v[2] = 1, r[0], r[1]
        else:
            raise ValueError("vl_imreadjpeg: 'Resize' takes S or [Ho Wo]")
    a = np.ravel(np.asarray(opt.get("cropanisotropy", [0, 0]), np.float64))
    v[3], v[4] = (a[0], a[0]) if a.size == 1 else (a[0], a[1])
    s = np.ravel(np.asarray(opt.get("cropsize", 1.0), np.float64))
    v[5], v[6] = (s[0], s[0]) if s.size == 1 else (s[0], s[1])
    loc = str(opt.get("croplocation", "center")).lower()
    if loc not in ("center", "random"):
        raise ValueError("vl_imreadjpeg: CropLocation must be 'center' or 'random' (got %r)" % (opt["croplocation"],))
    v[7] = loc == "random"
    v[8] = bool(opt.get("flip", False))
    name = str(opt.get("interpolation", "bilinear")).lower()
    if name not in IMREAD_FILTERS:
        raise ValueError("vl_imreadjpeg: Interpolation must be 'box', 'bilinear' or 'bicubic' (got %r)" % (opt["interpolation"],))
    v[9] = IMREAD_FILTERS[name]
    v[10] = bool(antialias)
    v[11] = float(opt.get("contrast", 0.0))
    v[12] = float(opt.get("saturation", 0.0))
    B = np.asarray(opt.get("brightness", 0.0), np.float64)
    if B.size == 1:
        B = np.eye(3) * float(B.ravel()[0])
    elif B.size == 3:
        B = np.diag(B.ravel())
    elif B.shape != (3, 3):
        raise ValueError("vl_imreadjpeg: 'Brightness' takes a scalar, 3 values or a 3 x 3 matrix")
    v[13:22] = B.reshape(-1)
    avg = opt.get("subtractaverage")
    if avg is not None:
        if isinstance(avg, torch.Tensor):
            avg = to_numpy(avg) if avg.dim() > 1 else avg.detach().cpu().numpy()
        avg = np.asarray(avg, np.float32)
        if avg.size == 3:
            avg, v[22] = avg.reshape(3), 1
        elif avg.ndim == 3 and avg.shape[2] == 3:
            v[22] = 2
        else:
            raise ValueError("vl_imreadjpeg: 'SubtractAverage' takes 3 values or an Ho x Wo x 3 array")
    return v, avg


def imread_random(v):
    """whether the options vector asks for anything drawn"""
    return bool(v[3] != v[4] or v[5] != v[6] or v[7] or v[8] or v[11] > 0 or v[12] > 0 or np.any(v[13:22] != 0))


def imread_draws(rng, N):
    """the draws of a batch: U = rng.random((N, 7)) and then G = rng.standard_normal((N, 3)), always both and in that order"""
    U = rng.random((N, 7))
    G = rng.standard_normal((N, 3))
    return np.ascontiguousarray(np.concatenate([U, G], 1))


def imread_plan(hw, opts, draws=None):
    """xm_imread_plan (host only): hw N x 3 (H, W, pixel offset), opts from imread_opts_vector, draws N x 10 or None ->
    (rows N x 44 float64, sizes int64[8]); a refusal raises _lib.XmError"""
    hw = np.ascontiguousarray(hw, np.int64).reshape(-1, 3)
    N = int(hw.shape[0])
    opts = np.ascontiguousarray(opts, np.float64)
    rows = np.zeros((max(N, 1), IMREAD_ROW), np.float64)
    sizes = np.zeros(IMREAD_SIZES, np.int64)
    d = None if draws is None else np.ascontiguousarray(draws, np.float64)
    if d is not None and d.shape != (N, IMREAD_DRAWS):
        raise ValueError("imread_plan: draws must be N x %d" % IMREAD_DRAWS)
    _lib.check(_L().xm_imread_plan(C.c_void_p(hw.ctypes.data), N, C.c_void_p(opts.ctypes.data),
                                   None if d is None else C.c_void_p(d.ctypes.data), C.c_void_p(rows.ctypes.data),
                                   C.c_void_p(sizes.ctypes.data)))
    return rows[:N], sizes


def imread_geometry():
    """(launches, launches with Contrast, LDS tile rows, LDS tile columns) of the stage (xm_imread_geometry; no device call)"""
    g = [C.c_int(0) for _ in range(4)]
    _lib.check(_L().xm_imread_geometry(*[C.byref(x) for x in g]))
    return tuple(x.value for x in g)


def imread_transform(pixels, rows, sizes, avg=None, device=None):
    """enqueues xm_imread_transform_batch on decoded `pixels` (the ragged float32 buffer of jpeg_decode): returns the flat
    float32 output of sizes[0] values; image n is Ho x Wo x 3 (MATLAB layout) at rows[n, 5].  No synchronisation."""
    device = device or pixels.device
    N = int(rows.shape[0])
    rows = np.ascontiguousarray(rows, np.float64)
    kind = int(rows[0, 40]) if N else 0
    want = {0: None, 1: (3,), 2: (int(rows[0, 3]), int(rows[0, 4]), 3) if N else None}[kind]
    if (None if avg is None else tuple(np.shape(avg))) != want:
        raise ValueError("imread_transform: the rows were planned for an average of shape %r, got %r"
                         % (want, None if avg is None else tuple(np.shape(avg))))
    with torch.cuda.device(device):
        host = torch.empty(rows.shape, dtype=torch.float64, pin_memory=True)
        host.numpy()[...] = rows
        desc = host.to(device, non_blocking=True)
        avg_dev = None
        if avg is not None:
            avg_dev = from_numpy(avg, device) if np.ndim(avg) == 3 else torch.from_numpy(np.asarray(avg, np.float32)).to(device)
        out = torch.empty(int(sizes[0]), dtype=torch.float32, device=device)
        _lib.check(_L().xm_imread_transform_batch(_ptr(pixels), _ptr(desc), N, C.c_void_p(rows.ctypes.data), _ptr(avg_dev),
                                                  _ptr(out), _stream()))
    return out


def uint8_round(x):
    """min(max(floor(x + 1/2), 0), 255) on the device (xm_imread_round_u8): the uint8 values imreadjpeg's resampler rounds
    to, from vl_imreadjpeg's unrounded ones; same shape and layout"""
    x = _chk(x, "X")
    y = torch.empty_like(x)
    _lib.check(_L().xm_imread_round_u8(_ptr(x), int(x.numel()), _ptr(y), _stream()))
    return y


def vl_imreadjpeg(files, *options, rng=None, antialias=False, device=None, split=None, progressive=False,
                  return_status=False):
    """vl_imreadjpeg(files, 'Pack', 'Resize', [224 224], 'Flip', 'CropSize', [0.35 1], ...) with MatConvNet's option list
    [EXT], decoded, cropped, mirrored, resampled and colour-jittered on the device (DESIGN section 24 holds the
    definitions).  `files`: bytes or paths.  Options: Resize (S | [Ho Wo]), CropSize, CropAnisotropy, CropLocation
    ('center' | 'random'), Flip, Interpolation ('box' | 'bilinear' | 'bicubic'), SubtractAverage (3 values | Ho x Wo x 3),
    Brightness, Contrast, Saturation, Pack; NumThreads, Gpu and Verbose are accepted and ignored, Prefetch raises.
    `antialias` (ours): widen the kernel by the reduction ratio.  `rng`: the numpy Generator every random option draws
    from (rng.random((N, 7)), then rng.standard_normal((N, 3)), whatever options are on).  Returns single values that are
    never rounded to uint8: with Pack an Ho x Wo x 3 x N tensor (all outputs must have one size), otherwise a list of
    Ho x Wo x 3 tensors.  split / progressive: imreadjpeg's; return_status as there.  The call does not synchronise."""
    if progressive and split is not None:
        raise ValueError("vl_imreadjpeg: progressive=True and split= exclude each other (progressive scans are not decoded "
                         "segment-parallel)")
    opt = imread_options(options)
    v, avg = imread_opts_vector(opt, antialias)
    if rng is None and imread_random(v):
        raise ValueError("vl_imreadjpeg: a random option (CropSize or CropAnisotropy range, CropLocation 'random', Flip, "
                         "Brightness, Contrast, Saturation) needs rng")
    datas = _file_bytes(files)
    N = len(datas)
    pack = bool(opt.get("pack", False))
    if not datas:
        return ([], None) if return_status else []
    buf, plan = jpeg_plan(datas, stage=_pinned if torch.cuda.is_available() else None, progressive=progressive)
    jdesc = np.array(buf[plan["desc"][0]:plan["desc"][0] + plan["desc"][1]]).view(np.int64).reshape(N, JPEG_DESC)
    draws = imread_draws(rng, N) if rng is not None else None
    rows, sizes = imread_plan(jdesc[:, [2, 3, 21]], v, draws)
    if pack and not sizes[5]:
        raise ValueError("vl_imreadjpeg: 'Pack' needs outputs of one size; these are ragged (give 'Resize' [Ho Wo])")
    if avg is not None and v[22] == 2 and tuple(avg.shape[:2]) != (int(rows[0, 3]), int(rows[0, 4])):
        raise ValueError("vl_imreadjpeg: 'SubtractAverage' is %d x %d, the outputs are %d x %d"
                         % (avg.shape[0], avg.shape[1], rows[0, 3], rows[0, 4]))
    if not torch.cuda.is_available():
        raise RuntimeError("vl_imreadjpeg needs a GPU; this build has no CPU path")
    pixels, _, status, _ = jpeg_decode(buf, plan, want_pixels=True, device=device, split=split)
    flat = imread_transform(pixels, rows, sizes, avg)
    if pack:
        Ho, Wo = int(rows[0, 3]), int(rows[0, 4])
        out = flat.view(N, 3, Wo, Ho).permute(3, 2, 1, 0)
    else:
        out = []
        for r in rows:
            Ho, Wo, o = int(r[3]), int(r[4]), int(r[5])
            out.append(flat[o:o + 3 * Ho * Wo].view(3, Wo, Ho).permute(2, 1, 0))
    return (out, status) if return_status else out


# --------------------------------------------------------------------------------------------
# audioinfo / audioread (getBatchEmoVoxCeleb.m:79,97-117,126, compute_audio_feats.m:173-175): WAV decode on the device
# --------------------------------------------------------------------------------------------
WAV_DESC = 16                                                                   # include/xmodal.h XM_WAV_*
WAV_U8, WAV_S16, WAV_S24, WAV_S32, WAV_F32, WAV_F64 = range(6)
WAV_OK, WAV_TRUNCATED = 0, 1


def _file_bytes(files):
    datas = []
    for f in files:
        if isinstance(f, (bytes, bytearray, memoryview)):
            datas.append(bytes(f))
        else:
            with open(f, "rb") as fh:
                datas.append(fh.read())
    return datas


def wav_plan(files, ranges=None, channel=None, out_base=0, stage=None, fs=None):
    """The host side of audioread (xm_wav_plan; touches no device): `files` is a list of bytes.  Lays one staging buffer
    out as [file bytes | desc] (16-byte aligned parts), parses every header into it and returns (stage, plan): `stage` a
    uint8 numpy array (`stage(nbytes)`, when given, allocates it -- audioread hands out pinned memory) and plan =
    dict(N, nbytes, desc: (offset, bytes) in the buffer, rows: the N x 16 int64 view of it, floats, total).
    ranges: None, one [first last] pair for every file, or N pairs (1-based inclusive, last = -1 or inf: to the end);
    channel: None for all channels or the 0-based channel to keep; out_base: first float of the batch in the bank.
    An unsupported or malformed file raises _lib.XmError naming its index.
    fs: None, or the rate every file is resampled to (xm_wav_plan_fs): rows[:, 14:16] then hold p, q = fs / SampleRate
    reduced, rows[:, 11], `floats` and plan["out_frames"] (per file and channel written) count floats at rate fs, and
    plan["fs"] records the rate; such rows go to xm_wav_decode_resample_batch.  A ratio beyond 16 either way raises too."""
    N = len(files)
    lens = np.array([len(f) for f in files], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nbytes = int(offsets[-1])
    up = lambda v: (int(v) + 15) & ~15
    o_desc = up(nbytes + 1)
    total = up(o_desc + 8 * WAV_DESC * N + 1)
    buf = stage(total) if stage is not None else np.empty(total, np.uint8)
    for f, o in zip(files, offsets):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    buf[nbytes:o_desc] = 0
    rng = None
    if ranges is not None:
        r = np.asarray(ranges, np.float64)
        r = np.where(np.isinf(r), -1, r)
        if r.ndim == 1 and r.size == 2:
            r = np.tile(r, (N, 1))
        if r.shape != (N, 2):
            raise ValueError("wav_plan: RANGES must be [first last] or N x 2")
        rng = np.ascontiguousarray(r, np.int64)
    sizes = np.zeros(2, np.int64)
    base = buf.ctypes.data
    args = (C.c_void_p(base), C.c_void_p(offsets.ctypes.data), N, C.c_void_p(rng.ctypes.data) if rng is not None else None,
            -1 if channel is None else int(channel))
    tail = (int(out_base), C.c_void_p(base + o_desc), C.c_void_p(sizes.ctypes.data))
    if fs is None:
        _lib.check(_L().xm_wav_plan(*args, *tail))
    else:
        _lib.check(_L().xm_wav_plan_fs(*args, int(fs), *tail))
    rows = buf[o_desc:o_desc + 8 * WAV_DESC * N].view(np.int64).reshape(N, WAV_DESC)
    plan = dict(N=N, nbytes=nbytes, desc=(o_desc, 8 * WAV_DESC * N), rows=rows, floats=int(sizes[0]), total=total,
                out_base=int(out_base))
    if fs is not None:
        plan.update(fs=int(fs), out_frames=_wav_out_frames(rows))
    return buf, plan


def _wav_out_frames(rows):
    """ceil(frames decoded * p / q) of every row of xm_wav_plan_fs"""
    return -(-rows[:, 8] * rows[:, 14] // rows[:, 15])


def wav_resample_geometry():
    """(tile, launches) of xm_wav_decode_resample_batch: the output floats of one tile, the launches of one call."""
    t, n = C.c_int(), C.c_int()
    _lib.check(_L().xm_wav_resample_geometry(C.byref(t), C.byref(n)))
    return t.value, n.value


def _wav_info(rows, resampled=False):
    info = [dict(SampleRate=int(d[2]), TotalSamples=int(d[6]), NumChannels=int(d[3]), BitsPerSample=int(d[4]),
                 Duration=float(d[6]) / float(d[2]), Truncated=bool(int(d[12]) & WAV_TRUNCATED)) for d in rows]
    if resampled:
        for i, n in zip(info, _wav_out_frames(rows)):
            i["ResampledSamples"] = int(n)
    return info


def audioinfo(files, fs=None):
    """info = audioinfo(file) for a list of WAV files (bytes or paths): a list of dicts with SampleRate, TotalSamples
    (frames), NumChannels, BitsPerSample, Duration (and Truncated: the data chunk claimed more than the file holds).
    With fs, ResampledSamples = ceil(TotalSamples fs / SampleRate) is added: the length audioread(fs=fs) gives the file.
    Host only -- the parse of xm_wav_plan / xm_wav_plan_fs; no device call."""
    datas = _file_bytes(files)
    if not datas:
        return []
    return _wav_info(wav_plan(datas, fs=fs)[1]["rows"], fs is not None)


def audioread(files, ranges=None, *, channel=None, out=None, out_base=0, device=None, return_info=False, fs=None):
    """[y, Fs] = audioread(file) / audioread(file, [first last]) for a batch of WAV files (bytes or paths), decoded on
    the device into one waveform bank: returns (bank, offsets), `bank` a 1-D float32 device tensor and `offsets` int64
    numpy with N + 1 entries -- file i is bank[offsets[i]:offsets[i + 1]], a frames x channels matrix in MATLAB layout
    (channel c at + c * frames; mono files and channel=c are plain vectors).  PCM 8 / 16 / 24 / 32 and float 32 / 64, also
    as WAVE_FORMAT_EXTENSIBLE; values are single(audioread's double), bit for bit.  `out` / `out_base` decode into a
    slice of an existing bank starting at float out_base.  One pinned staging buffer, one non-blocking upload, one
    launch, no wait.  return_info=True appends the audioinfo dicts.  Anything else (companded, compressed, RF64 ...)
    raises before anything is launched, with the index of the file; there is no host decode to fall back to.
    fs: None, or the rate of the bank -- every file is decoded and resampled in one pass (xm_wav_decode_resample_batch,
    two launches), file i becoming resample(audioread(file_i, range_i), fs, SampleRate_i) column by column: `offsets`
    then count floats at rate fs, a file at fs already is copied bit for bit, and the info dicts keep the file's own
    SampleRate and TotalSamples and gain ResampledSamples.  A range is cut from the file BEFORE resampling."""
    if not torch.cuda.is_available():
        raise RuntimeError("audioread needs a GPU; this build has no CPU path")
    datas = _file_bytes(files)
    out_base = int(out_base)
    if out is None and out_base:
        raise ValueError("audioread: out_base needs out")
    if out is not None:
        _chk(out, "OUT")
        if out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous():
            raise ValueError("audioread: OUT must be a contiguous 1-D float32 device tensor")
        device = out.device
    device = device or _dev()
    if not datas:
        bank = out if out is not None else torch.empty(0, dtype=torch.float32, device=device)
        res = (bank, np.array([out_base], np.int64))
        return res + ([],) if return_info else res
    held = []

    def stage(n):
        held.append(torch.empty(int(n), dtype=torch.uint8, pin_memory=True))
        return held[-1].numpy()

    buf, plan = wav_plan(datas, ranges, channel, out_base, stage=stage, fs=fs)
    rows, floats = plan["rows"], plan["floats"]
    if out is None:
        out = torch.empty(floats, dtype=torch.float32, device=device)
    elif out_base + floats > out.numel():
        raise ValueError("audioread: %d floats from %d on do not fit OUT of %d" % (floats, out_base, out.numel()))
    offsets = np.concatenate([rows[:, 11], [out_base + floats]]).astype(np.int64)
    if floats:
        with torch.cuda.device(device):
            dev = torch.empty(plan["total"], dtype=torch.uint8, device=device)
            dev.copy_(held[-1], non_blocking=True)
            p = dev.data_ptr()
            decode = _L().xm_wav_decode_batch if fs is None else _L().xm_wav_decode_resample_batch
            _lib.check(decode(C.c_void_p(p), plan["nbytes"], C.c_void_p(p + plan["desc"][0]), plan["N"], _ptr(out), out.numel(),
                              _stream()))
    res = (out, offsets)
    return res + (_wav_info(rows, fs is not None),) if return_info else res


# --------------------------------------------------------------------------------------------
# The pixel column of the FER2013 CSV (getFerPlusImdb(opts.dataDir), ferplus_baselines.m:103-110): parsed on the device
# --------------------------------------------------------------------------------------------
PIX_DESC = 8                                                                    # include/xmodal.h XM_PIX_*
PIX_BADCHAR, PIX_RANGE, PIX_COUNT, PIX_NOFIT = 1, 2, 4, 8
PIX_USAGE = ("Training", "PublicTest", "PrivateTest")


def _pix_bytes(data):
    """bytes-like, a uint8 numpy array or a path -> a contiguous uint8 numpy array (no copy where there is none to make)"""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise TypeError("pixcsv: expected a 1-D uint8 array")
        return np.ascontiguousarray(data)
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, np.uint8)
    return np.fromfile(data, np.uint8)


def pixcsv_geometry():
    """(bytes per pass, launches) of the pixel-field decode (xm_pixcsv_geometry; no device call)"""
    bpp, launches = C.c_int(0), C.c_int(0)
    _lib.check(_L().xm_pixcsv_geometry(C.byref(bpp), C.byref(launches)))
    return bpp.value, launches.value


def pixcsv_plan(data):
    """The host side of pixcsv_decode (xm_pixcsv_plan; touches no device): `data` is the CSV as bytes, a uint8 array or a
    path.  Returns plan = dict(N, nbytes, rows: N x 8 int64 -- byte range of the pixel field, emotion, usage code (index
    into PIX_USAGE or -1), 1-based line, output image index (preset to the row's ordinal; overwrite it to place or, with
    -1, skip a row), two zeros --, longest: the longest pixel field in bytes, data: the uint8 array).  A malformed file
    raises _lib.XmError naming the line."""
    buf = _pix_bytes(data)
    sizes = np.zeros(2, np.int64)
    p = C.c_void_p(buf.ctypes.data) if buf.size else None
    _lib.check(_L().xm_pixcsv_plan(p, buf.size, None, 0, C.c_void_p(sizes.ctypes.data)))
    N = int(sizes[0])
    rows = np.zeros((N, PIX_DESC), np.int64)
    _lib.check(_L().xm_pixcsv_plan(p, buf.size, C.c_void_p(rows.ctypes.data), N, C.c_void_p(sizes.ctypes.data)))
    return dict(N=N, nbytes=int(buf.size), rows=rows, longest=int(sizes[1]), data=buf)


def _pix_chunks(rows, chunk_bytes):
    """consecutive row ranges [a, b) whose bytes -- from the 16-byte boundary at or below the first field to the end of
    the last -- stay within chunk_bytes where a single row allows it.  Rows must ascend in the file."""
    N = len(rows)
    if chunk_bytes is None:
        return [(0, N)] if N else []
    cuts, a = [], 0
    while a < N:
        start = int(rows[a, 0]) & ~15
        b = a + 1
        while b < N and int(rows[b, 1]) - start <= chunk_bytes:
            b += 1
        cuts.append((a, b))
        a = b
    return cuts


def pixcsv_decode(data, plan, size=(48, 48), transpose=True, out=None, image_base=0, *, strict=True, chunk_bytes=None,
                  device=None):
    """Decodes the pixel fields of a planned CSV on the device (xm_pixcsv_decode_batch): the row whose output index is j
    becomes image image_base + j.  Returns (images, status): `images` the H x W x 1 x M device view (MATLAB layout) of
    `out` -- a contiguous 1-D float32 device tensor of M * H * W floats, allocated (and zeroed, so that an image no row
    names is defined) when not given, M then being image_base + 1 + the largest index --, `status` the N x 2 int32 host
    array [count of numbers, XM_PIX_* flags].  transpose=True reads a field as a row-major image (FER2013) and stores
    the MATLAB H x W array; False stores the numbers in file order.  Rows with a negative index are skipped.
    chunk_bytes cuts the upload at row boundaries: one pinned staging buffer, one upload and one launch per chunk,
    whatever the number of rows in it; the images never exist on the host.  A row with a status flag raises
    _lib.XmError naming the CSV line unless strict=False.  An index whose image does not fit `out` raises before
    anything is launched."""
    if not torch.cuda.is_available():
        raise RuntimeError("pixcsv_decode needs a GPU; this build has no CPU path")
    buf = _pix_bytes(data)
    H, W = _pair(size, "SIZE")
    if H * W <= 0:
        raise ValueError("pixcsv_decode: SIZE must be positive (got %r)" % (size,))
    rows = np.array(plan["rows"], np.int64, copy=True).reshape(-1, PIX_DESC)
    N, image_base = len(rows), int(image_base)
    if image_base < 0:
        raise ValueError("pixcsv_decode: image_base must not be negative")
    if N and (rows[:, 0].min() < 0 or rows[:, 1].max() > buf.size or (rows[:, 1] < rows[:, 0]).any()):
        raise ValueError("pixcsv_decode: the plan's byte ranges do not lie inside DATA")
    live = rows[:, 5] >= 0
    rows[live, 5] += image_base
    need = int(rows[live, 5].max()) + 1 if live.any() else image_base
    if out is None:
        device = device or _dev()
        out = torch.zeros(need * H * W, dtype=torch.float32, device=device)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("pixcsv_decode: OUT must be a contiguous 1-D float32 device tensor")
        device = out.device
        if need * H * W > out.numel():
            bad = int(np.nonzero(live & ((rows[:, 5] + 1) * H * W > out.numel()))[0][0])
            raise _lib.XmError(1, "pixcsv_decode: line %d: image %d of %d x %d does not fit OUT of %d floats"
                               % (rows[bad, 4], rows[bad, 5], H, W, out.numel()))
    M = out.numel() // (H * W)
    status = torch.zeros((N, 2), dtype=torch.int32, device=device)
    up = lambda v: (int(v) + 15) & ~15
    with torch.cuda.device(device):
        for a, b in _pix_chunks(rows, chunk_bytes):
            if not live[a:b].any():              # nothing but skipped rows: their status is (0, 0) already
                continue
            start, end = int(rows[a:b, 0].min()) & ~15, int(rows[a:b, 1].max())
            nb = end - start
            o_desc = up(nb + 1)
            total = o_desc + 8 * PIX_DESC * (b - a)
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            stage = host.numpy()
            stage[:nb] = buf[start:end]
            stage[nb:o_desc] = 0
            d = stage[o_desc:].view(np.int64).reshape(b - a, PIX_DESC)
            d[:] = rows[a:b]
            d[:, 0:2] -= start
            dev = torch.empty(total, dtype=torch.uint8, device=device)
            dev.copy_(host, non_blocking=True)
            p = dev.data_ptr()
            _lib.check(_L().xm_pixcsv_decode_batch(C.c_void_p(p), nb, C.c_void_p(p + o_desc), b - a, H, W, int(bool(transpose)),
                                                   _ptr(out), out.numel(), C.c_void_p(status.data_ptr() + 8 * a), _stream()))
    st = status.cpu().numpy()
    if strict and N and st[:, 1].any():
        i = int(np.nonzero(st[:, 1])[0][0])
        f = int(st[i, 1])
        what = [w for bit, w in ((PIX_BADCHAR, "a byte that is not a digit, a space or a tab"),
                                 (PIX_RANGE, "a number above 255 or of more than three digits"),
                                 (PIX_COUNT, "%d numbers where %d x %d = %d are expected" % (st[i, 0], H, W, H * W)),
                                 (PIX_NOFIT, "an image index outside the output")) if f & bit]
        raise _lib.XmError(1, "pixcsv_decode: line %d: %s (%d rows flagged)" % (rows[i, 4], "; ".join(what), int((st[:, 1] != 0).sum())))
    return out[:M * H * W].view(M, 1, W, H).permute(3, 2, 1, 0), st
