"""GPU: the bf16x3 arm of 1 x 1 layers (xm_nnconv_forward_split, vl_nnconv(precision='bf16x3')) against an fp64 numpy
evaluation of its formula from the same fp32 inputs:

  y = act( ((sum_c x f + b) scale + shift) gate + residual )

Bound per element, with S = sum_c |x||f| + |b_k|:

  |got - ref| <= (3 * 2^-16 + (C + 8) * 2^-24) * S * |scale_k gate| + 8 * 2^-24 * (largest magnitude among the epilogue's
                                                                                   intermediates and the result)

The first term is the DERIVED split error (x_lo f_lo + r_x f + x r_f dropped per product) plus the worst-case fp32
accumulation of C products in any order; the second is the fp32 epilogue.  Nothing is tuned to the kernel;
tests/test_conv_split_plan_cpu.py pins by emulation that a kernel which forgot one cross term cannot meet it."""
import ctypes as C

import numpy as np
import pytest

from aligned_views import Guarded, misaligned

pytestmark = pytest.mark.gpu

SPLIT_NAME = "conv_split_kernel"


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(a):
    return np.asfortranarray(np.asarray(a, np.float32))


def reference(x, f, b=None, scale=None, shift=None, gate=None, resid=None, stride=(1, 1), rstride=(1, 1), relu=False):
    """(ref, bound) in fp64 from the fp32 operands (numpy, MATLAB shapes)"""
    H, W, Cc, N = x.shape
    K = f.shape[3]
    xs = x[::stride[0], ::stride[1]].astype(np.float64)
    F = f.reshape(Cc, K).astype(np.float64)
    dot = np.einsum("hwcn,ck->hwkn", xs, F)
    S = np.einsum("hwcn,ck->hwkn", np.abs(xs), np.abs(F))
    kk = (1, 1, K, 1)
    v = dot.copy()
    mags = [np.abs(v)]
    if b is not None:
        v = v + b.astype(np.float64).reshape(kk)
        S = S + np.abs(b.astype(np.float64)).reshape(kk)
        mags.append(np.abs(v))
    amp = np.ones(kk)
    if scale is not None:
        v = v * scale.astype(np.float64).reshape(kk)
        mags.append(np.abs(v))
        v = v + shift.astype(np.float64).reshape(kk)
        mags.append(np.abs(v))
        amp = amp * np.abs(scale.astype(np.float64)).reshape(kk)
    if gate is not None:
        g = gate.astype(np.float64).reshape(1, 1, K, N)
        v = v * g
        mags.append(np.abs(v))
        amp = amp * np.abs(g)
    if resid is not None:
        r = resid[::rstride[0], ::rstride[1]].astype(np.float64)
        mags.append(np.abs(r))
        v = v + r
        mags.append(np.abs(v))
    if relu:
        v = np.maximum(v, 0.0)
    big = np.max(np.stack([np.broadcast_to(m, v.shape) for m in mags]), axis=0)
    bound = (3 * 2.0 ** -16 + (Cc + 8) * 2.0 ** -24) * S * amp + 8 * 2.0 ** -24 * big
    return v, bound


def split_call(gpu, x, f, b=None, scale=None, shift=None, gate=None, resid=None, stride=(1, 1), rstride=None, relu=False):
    """vl_nnconv(precision='bf16x3') from numpy operands -> numpy"""
    from mcncrossmodalemotions_amd import vl
    dev = lambda a: None if a is None else vl.from_numpy(_f32(a), device=gpu)
    y = vl.vl_nnconv(dev(x), dev(f), dev(b), stride=stride, scale=dev(scale), shift=dev(shift), gate=dev(gate),
                     residual=dev(resid), residual_stride=rstride, relu=relu, precision="bf16x3")
    return vl.to_numpy(y)


def check(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    print("%s: worst error / bound = %.3f (max |ref| %.3g)" % (what, float((err / np.maximum(bound, 1e-300)).max()),
                                                              float(np.abs(ref).max())))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(err <= bound), "%s: %d of %d elements over the bound, worst ratio %.3f" % (
        what, int((err > bound).sum()), err.size, float((err / np.maximum(bound, 1e-300)).max()))


def operands(rng, H, W, Cc, N, K, epi, stride=(1, 1)):
    x = _f32(rng.standard_normal((H, W, Cc, N)))
    f = _f32(rng.standard_normal((1, 1, Cc, K)))
    Ho, Wo = (H - 1) // stride[0] + 1, (W - 1) // stride[1] + 1
    kw = {}
    if "b" in epi:
        kw["b"] = _f32(rng.standard_normal((K, 1)))
    if "s" in epi:
        kw["scale"], kw["shift"] = _f32(rng.uniform(0.5, 2.0, (K, 1))), _f32(rng.standard_normal((K, 1)))
    if "g" in epi:
        kw["gate"] = _f32(rng.uniform(0.0, 1.0, (1, 1, K, N)))
    if "r" in epi:
        kw["resid"] = _f32(rng.standard_normal((Ho, Wo, K, N)) * 3)
    kw["relu"] = "R" in epi
    return x, f, kw


# (H, W, C, N, K, stride, epilogue): b bias, s scale + shift, g gate, r residual, R relu
CASES = [
    (1, 1, 1, 1, 1, (1, 1), ""),              # every extent 1
    (5, 7, 15, 3, 31, (1, 1), "b"),           # reduction tail below one step; a 128-pixel tile that holds three samples
    (9, 4, 16, 1, 32, (1, 1), "sR"),          # exactly one step, exactly one accumulator of channels
    (5, 7, 17, 3, 33, (1, 1), "bsrR"),        # one element into the second step / the second accumulator
    (9, 4, 24, 3, 40, (1, 1), "sgrR"),        # tail inside the second step
    (3, 3, 2048, 1, 33, (1, 1), ""),          # the deep chain of the teachers' last stage
    (12, 11, 40, 3, 70, (1, 1), "bsgrR"),     # four pixel tiles x two channel tiles, two LDS stages, samples inside tiles
    (7, 5, 17, 3, 40, (2, 2), "b"),
    (7, 5, 17, 3, 40, (2, 1), "bsR"),
    (7, 5, 17, 3, 40, (1, 3), "r"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%dx%d-K%d-s%d%d-%s" % (c[:5] + c[5] + (c[6] or "plain",)))
def test_split_against_fp64(gpu, case):
    H, W, Cc, N, K, stride, epi = case
    x, f, kw = operands(np.random.default_rng(1), H, W, Cc, N, K, epi, stride)
    got = split_call(gpu, x, f, stride=stride, **kw)
    ref, bound = reference(x, f, stride=stride, **kw)
    check(got, ref, bound, str(case))


def test_split_strided_residual_of_a_pruned_stage_end(gpu):
    """the conv runs with stride 2 over its 7 x 5 input; the shortcut keeps the 7 x 5 extent and is sampled with stride 2"""
    rng = np.random.default_rng(2)
    x, f, kw = operands(rng, 7, 5, 24, 3, 33, "sgR")
    kw["resid"] = _f32(rng.standard_normal((7, 5, 33, 3)) * 3)
    got = split_call(gpu, x, f, stride=(2, 2), rstride=(2, 2), **kw)
    ref, bound = reference(x, f, stride=(2, 2), rstride=(2, 2), **kw)
    assert got.shape == (4, 3, 33, 3)
    check(got, ref, bound, "strided residual")


def test_split_every_operand_one_float_off(gpu):
    """operands need 4-byte alignment only: every tensor starts one float past a 16-byte boundary, y sits between guards"""
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    L = _lib.load()
    rng = np.random.default_rng(3)
    H, W, Cc, N, K = 5, 7, 24, 3, 33
    x, f, kw = operands(rng, H, W, Cc, N, K, "bsgrR")
    d = {k: misaligned(vl.from_numpy(v, device=gpu)) for k, v in dict(x=x, f=f, **{k: v for k, v in kw.items() if k != "relu"}).items()}
    y = Guarded((H, W, K, N), 1, gpu)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.xm_nnconv_forward_split(_p(d["x"]), H, W, Cc, N, _p(d["f"]), 1, 1, Cc, K, _p(d["b"]), _p(y.view), 1, 1, 0, 0, 0, 0, 1, 1,
                                         _p(d["scale"]), _p(d["shift"]), _p(d["gate"]), _p(d["resid"]), H, W, 1, 1, 1, 1, st))
    torch.cuda.synchronize()
    y.assert_guards_untouched("conv_split_kernel")
    ref, bound = reference(x, f, **kw)
    check(vl.to_numpy(y.view), ref, bound, "unaligned operands")


def test_split_is_exact_on_small_integers(gpu):
    """x, f integers in -4 .. 4, C = 300: every lo half is zero, every partial sum an integer below 2^24 -- the output equals
    numpy's bit for bit in any summation order; a wrong index shows as a wrong integer"""
    rng = np.random.default_rng(4)
    H, W, Cc, N, K = 5, 7, 300, 3, 33
    x = _f32(rng.integers(-4, 5, (H, W, Cc, N)))
    f = _f32(rng.integers(-4, 5, (1, 1, Cc, K)))
    want = np.einsum("hwcn,ck->hwkn", x.astype(np.float64), f.reshape(Cc, K).astype(np.float64)).astype(np.float32)
    for stride in ((1, 1), (2, 3)):
        got = split_call(gpu, x, f, stride=stride)
        assert np.array_equal(got, want[::stride[0], ::stride[1]]), stride


def fixed_mantissa(rng, shape):
    """(1 + 2^-8 - 2^-17 + j 2^-23) 2^e, j in 0..3, e in -3..2: hi rounds down and lo carries nearly half a bf16 ulp, with one
    sign throughout -- the dropped-term error does not cancel, so a missing cross term cannot pass"""
    j, e = rng.integers(0, 4, shape), rng.integers(-3, 3, shape)
    return _f32((1 + 2.0 ** -8 - 2.0 ** -17 + j * 2.0 ** -23) * 2.0 ** e)


@pytest.mark.parametrize("Cc", [64, 2048])
def test_split_fixed_mantissa_operands(gpu, Cc):
    rng = np.random.default_rng(5)
    x, f = fixed_mantissa(rng, (3, 3, Cc, 2)), fixed_mantissa(rng, (1, 1, Cc, 8))
    got = split_call(gpu, x, f)
    ref, bound = reference(x, f)
    check(got, ref, bound, "fixed mantissa C=%d" % Cc)


def test_split_bits_depend_on_an_outputs_own_operands_only(gpu):
    rng = np.random.default_rng(6)
    x, f, kw = operands(rng, 7, 5, 40, 3, 33, "bsR")
    a, b = split_call(gpu, x, f, **kw), split_call(gpu, x, f, **kw)
    assert np.array_equal(a, b)                                                   # two calls
    one = split_call(gpu, x[..., :1], f, **kw)
    assert np.array_equal(a[..., :1], one)                                        # sample 0 of N = 3 == the N = 1 call
    strided = split_call(gpu, x, f, stride=(2, 2), **kw)
    presampled = split_call(gpu, _f32(x[::2, ::2]), f, **kw)
    assert np.array_equal(strided, presampled) and np.array_equal(strided, a[::2, ::2])


def test_split_launches_show_under_their_own_name(gpu):
    from mcncrossmodalemotions_amd import prof
    rng = np.random.default_rng(7)
    x, f, kw = operands(rng, 9, 4, 24, 3, 40, "bsR")
    _, rows = prof.kernels_run(lambda: (split_call(gpu, x, f, **kw), split_call(gpu, x, f, stride=(2, 2), **kw)))
    assert [(r.name, r.launches) for r in rows] == [(SPLIT_NAME, 2)], rows
    assert all(r.key >= 2500 for r in rows)


def test_split_refuses_what_it_is_not_built_for(gpu):
    from mcncrossmodalemotions_amd import _lib, vl
    x = vl.from_numpy(_f32(np.ones((6, 6, 4, 2))), device=gpu)
    with pytest.raises(_lib.XmError, match="larger than 1 x 1") as e:
        vl.vl_nnconv(x, vl.from_numpy(_f32(np.ones((3, 3, 4, 5))), device=gpu), precision="bf16x3")
    assert e.value.code == 5
    with pytest.raises(_lib.XmError, match="padding"):
        vl.vl_nnconv(x, vl.from_numpy(_f32(np.ones((1, 1, 4, 5))), device=gpu), pad=1, precision="bf16x3")
    with pytest.raises(_lib.XmError, match="filter groups"):
        vl.vl_nnconv(x, vl.from_numpy(_f32(np.ones((1, 1, 2, 6))), device=gpu), precision="bf16x3")
