"""GPU: xm_nnconv_forward_lattice against the full-extent vl.vl_nnconv forward with the folded epilogue (bias, scale / shift,
ReLU): BIT equality at the lattice pixels (ly i, lx j), and the sentinel the output tensor was filled with before the call
everywhere else.

The reference is the library's own full-extent launch, not the oracle: what the lattice call promises is the bits of that
launch (the frozen teacher's logits are the student's targets).  The bits follow the structure of the reduction, so there is
one case per structure, the tile configuration named by hand (`conv_cfg`: then neither call measures anything and no
halo-patch kernel competes) and the split left to the library:
  * one accumulator chain, unsplit;
  * automatic split-K (few tiles, a deep reduction): the lattice has a quarter of the tiles and must not split further;
  * the two chains of the 1 x 1 wave tiles (configurations 4, 5, 6);
  * a hybrid launch (784 tiles of 64 x 128 on 768 slots: the last 16 tiles are two-way sums): the lattice pixels below the
    cut unsplit, the others as a split launch with the same cut points;
  * a 1 x 1 layer whose full-extent launch is an LDS-DMA kernel (configurations 8 ... 11: one chain each, also 11, whose
    register-staged base is the two-chain 4): the lattice runs a register-staged configuration with one chain.
A layer with filter groups stays at full extent.
prof.kernels_run names the kernel and counts its launches; xm_debug_get("conv_last_combine") tells how many slabs the last
launch left to the combine kernel (positive: its 16-byte form, negative: its scalar form), "conv_last_lattice" that the call
computed the lattice only."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.0)


class Problem:
    """k x k / pad (k - 1) / 2 / stride 1 layer H x W x C x N -> K (in `groups` filter groups) on the device; full-extent
    results are computed on request"""

    def __init__(self, H, W, Cc, N, K, k=3, groups=1, seed=0):
        from mcncrossmodalemotions_amd import vl
        rng = np.random.default_rng(seed + 1000 * H + 100 * W + Cc + K + N)
        self.shape = (H, W, Cc, N, K)
        self.x = vl.from_numpy(rng.standard_normal((H, W, Cc, N)).astype(np.float32))
        self.k, self.pad, self.FC = k, (k - 1) // 2, Cc // groups
        self.f = vl.from_numpy(rng.standard_normal((k, k, self.FC, K)).astype(np.float32))
        self.b = vl.from_numpy(rng.standard_normal((K, 1)).astype(np.float32))
        self.sc = vl.from_numpy(rng.uniform(0.5, 1.5, (K, 1)).astype(np.float32))
        self.sh = vl.from_numpy(rng.standard_normal((K, 1)).astype(np.float32))

    def full(self, folded=True, relu=True):
        from mcncrossmodalemotions_amd import vl
        kw = dict(scale=self.sc, shift=self.sh) if folded else {}
        return vl.vl_nnconv(self.x, self.f, self.b, pad=self.pad, relu=relu, **kw)

    def lattice(self, L, ly, lx, folded=True, relu=True, misalign=0):
        """(the whole output tensor as numpy H x W x K x N, filled with SENTINEL before the call)"""
        H, W, Cc, N, K = self.shape
        buf = torch.full((H * W * K * N + 4,), float(SENTINEL), dtype=torch.float32, device=self.x.device)
        y = buf[misalign:misalign + H * W * K * N]
        assert (y.data_ptr() & 15) == 4 * misalign
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        k, pd = self.k, self.pad
        rc = L.xm_nnconv_forward_lattice(p(self.x), H, W, Cc, N, p(self.f), k, k, self.FC, K, p(self.b), p(y), 1, 1, pd, pd, pd, pd, 1, 1,
                                         p(self.sc) if folded else None, p(self.sh) if folded else None, None,
                                         1 if relu else 0, ly, lx, stream)
        assert rc == 0, L.xm_last_error()
        torch.cuda.synchronize()
        assert float(buf[:misalign].min() if misalign else SENTINEL) == SENTINEL and bool((buf[misalign + y.numel():] == SENTINEL).all())
        return y.cpu().numpy().reshape(N, K, W, H).transpose(3, 2, 1, 0)


def same_bits_on_the_lattice(got, full, ly, lx, what):
    from mcncrossmodalemotions_amd import vl
    ref = vl.to_numpy(full)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    on = np.zeros(ref.shape, bool)
    on[::ly, ::lx] = True
    a, b = np.ascontiguousarray(got[::ly, ::lx]).view(np.uint32), np.ascontiguousarray(ref[::ly, ::lx]).view(np.uint32)
    assert a.shape[0] == (ref.shape[0] - 1) // ly + 1 and a.shape[1] == (ref.shape[1] - 1) // lx + 1
    assert np.array_equal(a, b), "%s: %d of %d lattice values differ in their bits, largest difference %.3e" % (
        what, int((a != b).sum()), a.size, float(np.abs(got[::ly, ::lx] - ref[::ly, ::lx]).max()))
    assert np.all(got[~on] == SENTINEL), "%s: %d elements off the lattice were written" % (what, int((got[~on] != SENTINEL).sum()))
    assert float(np.abs(ref).max()) > 0 and np.any(ref[::ly, ::lx] != 0)


def both(L, prob, cfg, ly=2, lx=2, dma=False, **kw):
    """full-extent and lattice call under one forced configuration -> (gemm rows of the full call, its combine, rows of the
    lattice call, its combine); asserts the bits"""
    from mcncrossmodalemotions_amd import prof
    mis = kw.pop("misalign", 0)
    L.xm_debug_force_conv_cfg(cfg)
    try:
        full, rows_f = prof.kernels_run(lambda: prob.full(**kw), L)
        comb_f = L.xm_debug_get(b"conv_last_combine")
        got, rows_l = prof.kernels_run(lambda: prob.lattice(L, ly, lx, misalign=mis, **kw), L)
        comb_l = L.xm_debug_get(b"conv_last_combine")
        assert L.xm_debug_get(b"conv_last_lattice") == 1
    finally:
        L.xm_debug_force_conv_cfg(-1)
    same_bits_on_the_lattice(got, full, ly, lx, "%r cfg %d lattice [%d %d] %r" % (prob.shape, cfg, ly, lx, kw))
    gemm = lambda rows: [(r.name, r.launches) for r in rows if "conv_gemm_kernel" in r.name]   # noqa: E731
    assert all("halo" not in r.name for r in rows_f + rows_l) and all("dma" not in r.name for r in rows_l)
    assert any("dma" in r.name for r in rows_f) == dma, [r.name for r in rows_f]
    return gemm(rows_f), comb_f, gemm(rows_l), comb_l, rows_f, rows_l


_problems = {}


def problem(*shape, **kw):
    key = shape + tuple(sorted(kw.items()))
    if key not in _problems:
        _problems[key] = Problem(*shape, **kw)
    return _problems[key]


@pytest.fixture
def L(gpu):
    from mcncrossmodalemotions_amd import _lib
    return _lib.load()


ONE_CHAIN = "conv_gemm_kernel<1, 2, 2, 2, 1>"      # configuration 3: 64 x 128 tiles


@pytest.mark.parametrize("shape", [(12, 10, 16, 3, 32), (12, 10, 16, 1, 32), (13, 11, 16, 3, 32), (13, 11, 16, 1, 32)])
def test_one_chain_unsplit(L, shape):
    p = problem(*shape)
    gf, cf, gl, cl, rows_f, rows_l = both(L, p, 3)
    assert gf == [(ONE_CHAIN, 1)] and gl == [(ONE_CHAIN, 1)] and cf == 0 and cl == 0
    # the profiler is told the work of the pixels that were computed
    H, W, Cc, N, K = shape
    npl = ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * N
    assert [r.flops for r in rows_l if ONE_CHAIN in r.name] == [2.0 * K * npl * 9 * Cc]
    assert [r.flops for r in rows_f if ONE_CHAIN in r.name] == [2.0 * K * H * W * N * 9 * Cc]


def test_epilogue_variants_and_other_lattices(L):
    p = problem(13, 11, 16, 3, 32)
    both(L, p, 3, folded=False, relu=False)
    both(L, p, 3, folded=True, relu=False)
    both(L, p, 3, folded=False, relu=True)
    both(L, p, 3, ly=3, lx=3)
    both(L, p, 3, ly=2, lx=3)
    both(L, p, 0, ly=1, lx=2)


@pytest.mark.parametrize("shape", [(12, 10, 16, 3, 32), (13, 11, 16, 1, 32)])
def test_misaligned_output(L, shape):
    """y four bytes past a 16-byte boundary (the full-extent reference is the aligned call: alignment never changes what is
    computed)"""
    gf, cf, gl, cl, _, _ = both(L, problem(*shape), 3, misalign=1)
    assert gl == [(ONE_CHAIN, 1)] and cl == 0
    both(L, problem(14, 14, 32, 2, 64), 0, misalign=3)


def test_automatic_split_k(L):
    """392 pixels x 64 rows are 4 tiles of 128 x 128 over 18 reduction stages: the library splits them two ways.  The 98 lattice
    pixels are one tile and keep the two slabs of nine stages"""
    gf, cf, gl, cl, _, _ = both(L, problem(14, 14, 32, 2, 64), 0)
    name = "conv_gemm_kernel<2, 2, 2, 2, 1>"
    assert gf == [(name, 1)] and gl == [(name, 1)]
    assert cf == 2 and cl == -2          # the full extent stores 16 bytes wide, the lattice one float at a time


@pytest.mark.parametrize("cfg, name", [(4, "conv_gemm_kernel<1, 1, 2, 2, 1>"), (5, "conv_gemm_kernel<1, 1, 4, 1, 1>"),
                                       (6, "conv_gemm_kernel<1, 1, 1, 4, 1>")])
def test_two_chain_configurations(L, cfg, name):
    gf, cf, gl, cl, _, _ = both(L, problem(13, 11, 16, 3, 32), cfg)
    assert gf == [(name, 1)] and gl == [(name, 1)] and cf == 0 and cl == 0
    gf, cf, gl, cl, _, _ = both(L, problem(14, 14, 32, 2, 64), cfg)      # ... and split two ways
    assert gf == [(name, 1)] and gl == [(name, 1)] and cf == 2 and cl == -2


@pytest.mark.parametrize("cfg, name", [(3, ONE_CHAIN), (5, "conv_gemm_kernel<1, 1, 4, 1, 1>")])
def test_hybrid_remainder(L, cfg, name):
    """100352 pixels x 64 rows: 784 tiles of 64 x 128 (3136 of 128 x 32) on 768 slots -- the full-extent launch computes the
    pixels from 98304 on (column 19, row 24 of the last sample) as two-way sums of nine stages.  On the lattice those are the
    pixels from column 20 of the last sample on: one unsplit launch below them, one split launch from that sample's start
    whose combine begins at the cut"""
    gf, cf, gl, cl, _, _ = both(L, problem(56, 56, 32, 32, 64), cfg)
    assert gf == [(name, 1)] and cf == 2
    assert gl == [(name, 2)] and cl == -2


# LDS-DMA configuration -> (its kernel, the register-staged kernel the lattice runs: the base of the same tile shape, but the
# one-chain <1, 2, 2, 2> for 11, whose base <1, 1, 2, 2> has two chains)
DMA = {8: ("conv_gemm_dma_kernel<2, 2, 2, 2,", "conv_gemm_kernel<2, 2, 2, 2, 0>"),
       9: ("conv_gemm_dma_kernel<2, 2, 1, 4,", "conv_gemm_kernel<2, 2, 1, 4, 0>"),
       10: ("conv_gemm_dma_kernel<1, 2, 2, 2,", "conv_gemm_kernel<1, 2, 2, 2, 0>"),
       11: ("conv_gemm_dma_kernel<1, 1, 2, 2,", "conv_gemm_kernel<1, 2, 2, 2, 0>")}


@pytest.mark.parametrize("cfg", sorted(DMA))
def test_a_1x1_layer_whose_full_extent_launch_is_an_lds_dma_kernel(L, cfg):
    """1 x 1 / unit stride / no padding over maps of H W % 4 == 0 pixels, aligned operands, C a multiple of 16: the full-extent
    launch is the LDS-DMA kernel asked for.  Unsplit (12 x 10 x 32 x 3 -> 32: two reduction stages) and split two ways
    (14 x 14 x 256 x 2 -> 64: 392 pixels, sixteen stages)"""
    dma_name, lat_name = DMA[cfg]
    for shape, comb in (((12, 10, 32, 3, 32), 0), ((14, 14, 256, 2, 64), 2)):
        _, cf, gl, cl, rows_f, _ = both(L, problem(*shape, k=1), cfg, dma=True)
        assert [r.launches for r in rows_f if dma_name in r.name] == [1], [r.name for r in rows_f]
        assert gl == [(lat_name, 1)] and cf == comb and cl == -comb


def test_a_grouped_layer_stays_at_full_extent(L):
    from mcncrossmodalemotions_amd import vl
    p = problem(12, 10, 32, 3, 32, groups=2)
    L.xm_debug_force_conv_cfg(3)
    try:
        full = vl.to_numpy(p.full())
        got = p.lattice(L, 2, 2)
        assert L.xm_debug_get(b"conv_last_lattice") == 0
    finally:
        L.xm_debug_force_conv_cfg(-1)
    assert np.array_equal(got.view(np.uint32), full.view(np.uint32))


def test_a_halo_patch_layer_stays_at_full_extent(L):
    """a full-extent selection that is no implicit-GEMM launch (here the halo-patch kernel, asked for by hand) has another
    summation order: the call computes the layer at full extent instead of other bits"""
    from mcncrossmodalemotions_amd import prof, vl
    p = problem(12, 10, 16, 3, 32)
    old = L.xm_debug_force_conv_halo(1)
    try:
        full, rows = prof.kernels_run(lambda: p.full(), L)
        assert any("halo" in r.name for r in rows), [r.name for r in rows]
        got, rows = prof.kernels_run(lambda: p.lattice(L, 2, 2), L)
        assert any("halo" in r.name for r in rows), [r.name for r in rows]
        assert L.xm_debug_get(b"conv_last_lattice") == 0
    finally:
        L.xm_debug_force_conv_halo(old)
    assert np.array_equal(got.view(np.uint32), vl.to_numpy(full).view(np.uint32))


def test_vl_nnconv_out_lattice(L):
    from mcncrossmodalemotions_amd import vl
    p = problem(13, 11, 16, 3, 32)
    L.xm_debug_force_conv_cfg(3)
    try:
        full = vl.to_numpy(p.full())
        y = vl.vl_nnconv(p.x, p.f, p.b, pad=1, relu=True, scale=p.sc, shift=p.sh, out_lattice=(2, 2))
        assert L.xm_debug_get(b"conv_last_lattice") == 1
    finally:
        L.xm_debug_force_conv_cfg(-1)
    got = vl.to_numpy(y)
    assert got.shape == full.shape and np.array_equal(got[::2, ::2].view(np.uint32), full[::2, ::2].view(np.uint32))
    with pytest.raises(ValueError, match="out_lattice"):
        vl.vl_nnconv(p.x, p.f, p.b, pad=1, residual=y, out_lattice=2)
