"""GPU parity of vl.vl_nnconv(..., residual=R, residual_stride=(s, s)) -- xm_nnconv_forward_strided_residual -- against the
CPU oracle: y = act(((conv + b) .* scale + shift) [.* gate] + R(oy * s, ox * s)).

The expected value is the oracle's unit-stride convolution, scale / shift, gate, FULL-SIZE residual and ReLU composed in numpy,
then [::s, ::s] (a 1 x 1 convolution of a sampled tensor is the sampled convolution).  Allowance: the one of the fused-epilogue
cases of test_gpu_ops.py, |hip - oracle| <= 1e-4 * max(1, max|oracle|) against the fp64-accumulate oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4


def close(a, b, tol=TOL, what=""):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    err = float(np.abs(a - b).max()) if b.size else 0.0
    assert err <= tol * scale, "%s: max err %.3e > %.1e * %.3g" % (what, err, tol, scale)


def rnd(rng, *shape):
    return O.F(rng.standard_normal(shape))


# (H, W, C, K, N, s, gate)
CASES = [
    (8, 8, 16, 32, 2, 2, True),      # 16-byte stores, pixel quads inside one output column
    (28, 28, 16, 32, 1, 2, False),   # 16-byte stores, Ho = 14: quads straddle output columns
    (14, 14, 16, 32, 3, 2, True),    # 7 x 7 = 49 outputs per plane: scalar stores, quads straddle samples
    (7, 7, 16, 32, 2, 2, False),     # odd extent -> 4 x 4: the last row and column are sampled at the edge
    (5, 9, 16, 32, 2, 2, False),     # -> 3 x 5, scalar stores, both edges
    (8, 8, 16, 40, 2, 2, False),     # row-tile tail
    (8, 8, 20, 32, 2, 2, False),     # C no multiple of the reduction depth per stage: padded-filter mode
    (9, 9, 16, 32, 2, 3, False),     # stride 3 -> 3 x 3
]


class Problem:
    """operands of one case on the device and the expected values, computed once and shared (never modified)"""

    def __init__(self, case):
        from mcncrossmodalemotions_amd import vl
        H, W, Cc, K, N, s, gated = case
        rng = np.random.default_rng(1000 * H + 100 * W + Cc + K + N + s)
        x, f, b = rnd(rng, H, W, Cc, N), rnd(rng, 1, 1, Cc, K), rnd(rng, K)
        sc, sh = O.F(rng.uniform(0.5, 1.5, K)), rnd(rng, K)
        res = rnd(rng, H, W, K, N)
        gate = O.F(rng.uniform(0.0, 1.0, (1, 1, K, N))) if gated else None
        y0 = O.vl_nnconv(x, f, b, acc64=True)
        full = y0 * sc.reshape(1, 1, K, 1) + sh.reshape(1, 1, K, 1)
        self.s = s
        self.ref = {}
        for g_ in ((False, True) if gated else (False,)):
            for relu in (False, True):
                v = (full * gate if g_ else full) + res
                self.ref[(g_, relu)] = (np.maximum(v, 0) if relu else v)[::s, ::s]
        self.x, self.f, self.b = vl.from_numpy(x), vl.from_numpy(f), vl.from_numpy(b.reshape(K, 1))
        self.kw = dict(scale=vl.from_numpy(sc.reshape(K, 1)), shift=vl.from_numpy(sh.reshape(K, 1)),
                       residual=vl.from_numpy(res), residual_stride=(s, s))
        self.gate = vl.from_numpy(gate) if gated else None

    def run(self, gated, relu, **conv):
        from mcncrossmodalemotions_amd import vl
        conv.setdefault("stride", self.s)
        return vl.vl_nnconv(self.x, self.f, self.b, relu=relu, gate=self.gate if gated else None, **self.kw, **conv)

    def check(self, what, **conv):
        from mcncrossmodalemotions_amd import vl
        for (gated, relu), ref in self.ref.items():
            close(vl.to_numpy(self.run(gated, relu, **conv)), ref,
                  what="%s%s%s" % (what, ", gate" if gated else "", ", relu" if relu else ""))


_problems = {}


def problem(case):
    if case not in _problems:
        _problems[case] = Problem(case)
    return _problems[case]


def _kernels_run(L, fn):
    from mcncrossmodalemotions_amd import prof
    out, rows = prof.kernels_run(fn, L)
    return out, [r.name for r in rows]


def _only_the_implicit_gemm(names):
    assert names and not any(w in n for n in names for w in ("halo", "stem", "dma")), names


@pytest.mark.parametrize("case", CASES)
def test_strided_residual(gpu, case):
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    p = problem(case)
    p.check("strided residual %r" % (case,))
    _, names = _kernels_run(L, lambda: p.run(False, True))
    _only_the_implicit_gemm(names)


@pytest.mark.parametrize("case", [CASES[0], CASES[2]])
def test_strided_residual_every_tile_configuration(gpu, case):
    """every tile configuration asked for by hand (an LDS-DMA one falls back to its register-staged base: the strided
    residual keeps the call off that kernel)"""
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    p = problem(case)
    try:
        for cfg in range(L.xm_debug_num_conv_cfgs()):
            L.xm_debug_force_conv_cfg(cfg)
            p.check("cfg %d" % cfg)
            _, names = _kernels_run(L, lambda: p.run(False, True))
            _only_the_implicit_gemm(names)
    finally:
        L.xm_debug_force_conv_cfg(-1)


# the 8 x 8 and the 14 x 14 case with a reduction deep enough to be split: C = 64 is four stages of kBK = 16 (with C = 16 a
# forced split is one stage and the launch stores through its own epilogue)
SPLIT_CASES = [((8, 8, 64, 32, 2, 2, True), 2),      # 16 outputs per plane: conv_splitk_epilogue_kernel<true>, 16-byte form
               ((14, 14, 64, 32, 3, 2, True), -2)]   # 49 outputs per plane: conv_splitk_epilogue_kernel<false>, scalar form


@pytest.mark.parametrize("case, combine", SPLIT_CASES)
def test_strided_residual_split_k(gpu, case, combine):
    """forced split-K: the launch leaves two partial slabs and the combine kernel applies the epilogue with the sampled
    residual -- its 16-byte form and its scalar form; the library's record of the last launch proves which one ran"""
    from mcncrossmodalemotions_amd import vl, _lib
    L = _lib.load()
    p = problem(case)
    p.check("unsplit")
    assert L.xm_debug_get(b"conv_last_combine") == 0          # an automatic strided-residual launch never splits
    old = L.xm_debug_force_conv_splits(2)
    try:
        for (gated, relu), ref in p.ref.items():
            y = p.run(gated, relu)
            assert L.xm_debug_get(b"conv_last_combine") == combine
            close(vl.to_numpy(y), ref, what="split-K%s%s" % (", gate" if gated else "", ", relu" if relu else ""))
    finally:
        L.xm_debug_force_conv_splits(old)


def test_strided_residual_stays_off_the_dma_kernel(gpu):
    """a unit-stride 1 x 1 convolution over 4 x 4 maps is a plain GEMM in memory, the LDS-DMA kernel's case -- but not
    with a residual of 8 x 8 sampled at every second pixel"""
    from mcncrossmodalemotions_amd import vl, _lib
    L = _lib.load()
    rng = np.random.default_rng(5)
    H, Cc, K, N = 4, 64, 64, 8
    x, f = rnd(rng, H, H, Cc, N), rnd(rng, 1, 1, Cc, K)
    res = rnd(rng, 2 * H, 2 * H, K, N)
    ref = np.maximum(O.vl_nnconv(x, f, None, acc64=True) + res[::2, ::2], 0)
    xd, fd, rd = vl.from_numpy(x), vl.from_numpy(f), vl.from_numpy(res)
    y, names = _kernels_run(L, lambda: vl.vl_nnconv(xd, fd, None, residual=rd, residual_stride=2, relu=True))
    _only_the_implicit_gemm(names)
    close(vl.to_numpy(y), ref, what="1 x 1 / stride 1 with a sampled residual")
    try:
        for cfg in range(L.xm_debug_num_conv_cfgs() - 4, L.xm_debug_num_conv_cfgs()):      # the LDS-DMA configurations
            L.xm_debug_force_conv_cfg(cfg)
            y, names = _kernels_run(L, lambda: vl.vl_nnconv(xd, fd, None, residual=rd, residual_stride=2, relu=True))
            _only_the_implicit_gemm(names)
            close(vl.to_numpy(y), ref, what="forced cfg %d" % cfg)
    finally:
        L.xm_debug_force_conv_cfg(-1)


def test_strided_residual_stays_off_the_halo_kernel(gpu):
    """3 x 3 / pad 1 / unit stride is the halo-patch kernel's case; with a sampled residual the call stays on the
    implicit-GEMM kernel even when the halo kernel is asked for by hand"""
    from mcncrossmodalemotions_amd import vl, _lib
    L = _lib.load()
    rng = np.random.default_rng(6)
    H, Cc, K, N = 8, 16, 32, 2
    x, f, b = rnd(rng, H, H, Cc, N), rnd(rng, 3, 3, Cc, K), rnd(rng, K)
    res = rnd(rng, 2 * H - 1, 2 * H, K, N)          # 15 rows: floor(14 / 2) + 1 = 8
    ref = O.vl_nnconv(x, f, b, pad=1, acc64=True) + res[::2, ::2]
    xd, fd, bd, rd = vl.from_numpy(x), vl.from_numpy(f), vl.from_numpy(b.reshape(K, 1)), vl.from_numpy(res)
    old = L.xm_debug_force_conv_halo(1)
    try:
        _, names = _kernels_run(L, lambda: vl.vl_nnconv(xd, fd, bd, pad=1))
        assert any("halo" in n for n in names), names               # (the shape IS the halo kernel's)
        y, names = _kernels_run(L, lambda: vl.vl_nnconv(xd, fd, bd, pad=1, residual=rd, residual_stride=2))
        _only_the_implicit_gemm(names)
        close(vl.to_numpy(y), ref, what="3 x 3 with a sampled residual")
    finally:
        L.xm_debug_force_conv_halo(old)


def test_unit_stride_is_the_plain_residual(gpu):
    """residual_stride=(1, 1) with the residual at output extent is the older entry point: same kernels, same bits"""
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(7)
    x, f, res = rnd(rng, 8, 8, 16, 2), rnd(rng, 1, 1, 16, 32), rnd(rng, 8, 8, 32, 2)
    xd, fd, rd = vl.from_numpy(x), vl.from_numpy(f), vl.from_numpy(res)
    a = vl.to_numpy(vl.vl_nnconv(xd, fd, None, residual=rd, relu=True))
    b = vl.to_numpy(vl.vl_nnconv(xd, fd, None, residual=rd, residual_stride=1, relu=True))
    assert np.array_equal(a, b)


def test_inconsistent_residual_extent_is_rejected(gpu):
    from mcncrossmodalemotions_amd import vl, _lib
    rng = np.random.default_rng(8)
    xd, fd = vl.from_numpy(rnd(rng, 8, 8, 16, 2)), vl.from_numpy(rnd(rng, 1, 1, 16, 32))
    for shape, rs in (((8, 8, 32, 2), 3), ((9, 8, 32, 2), 2), ((8, 10, 32, 2), 2), ((4, 4, 32, 2), 2)):
        with pytest.raises(_lib.XmError, match="does not give") as e:
            vl.vl_nnconv(xd, fd, None, stride=2, residual=vl.from_numpy(rnd(rng, *shape)), residual_stride=rs)
        assert e.value.code == 1           # XM_EINVAL
    res = vl.from_numpy(rnd(rng, 8, 8, 32, 2))
    with pytest.raises(ValueError, match="without a residual"):
        vl.vl_nnconv(xd, fd, None, stride=2, residual_stride=2)
    with pytest.raises(ValueError, match="cannot be combined"):
        vl.vl_nnconv(xd, fd, None, stride=2, residual=res, residual_stride=2, sigmoid=True)
    with pytest.raises(ValueError, match="cannot be combined"):
        vl.vl_nnconv(xd, fd, None, stride=2, residual=res, residual_stride=2, moments_out=vl.mat_empty(32, 2, device=xd.device))
    with pytest.raises(ValueError, match="residual shape mismatch"):
        vl.vl_nnconv(xd, fd, None, stride=2, residual=vl.from_numpy(rnd(rng, 8, 8, 16, 2)), residual_stride=2)
    L = _lib.load()
    rc = L.xm_nnconv_forward_strided_residual(C.c_void_p(xd.data_ptr()), 8, 8, 16, 2, C.c_void_p(fd.data_ptr()), 1, 1, 16, 32,
                                              None, C.c_void_p(xd.data_ptr()), 2, 2, 0, 0, 0, 0, 1, 1, None, None, None,
                                              C.c_void_p(xd.data_ptr()), 8, 8, 0, 2, 0, None)
    assert rc == 1 and b"does not give" in L.xm_last_error()
