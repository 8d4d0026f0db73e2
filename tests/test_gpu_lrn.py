"""GPU parity of vl_nnnormalize (csrc/lrn.hip) against the fp64 restatement tests/lrn_ref.py, forward and backward, under the
project's rule |hip - ref| <= 1e-4 * max(1, max |ref|) (tests/test_gpu_ops.py).

The cases stand on the kernels' own edges, read from xm_nnnormalize_geometry:
  window edges    windows that clip at the first / last channel, at both, that cover every channel, even N (the adjoint
                  window is the mirrored one) and N past window_in_registers (the general arm), under KAPPA = ALPHA = 1,
                  where a mirrored window moves the result by 0.4 (tests/test_lrn_cpu.py)
  pixel edges     planes of 1 pixel, odd planes (the 4-byte arm), multiples of four (the 16-byte arm), one pixel short of /
                  exactly / one past a block's pixels, two blocks and one pixel; one and three samples
  channel edges   3 x 3 planes, where the channel axis is split into chunks of channels_per_pass: one short of / exactly /
                  one past a chunk, two chunks and one channel, many chunks; both arms at the switch between them
  alignment gate  x, dzdy or the output one float past a 16-byte boundary inside a guarded buffer"""
import functools

import numpy as np
import pytest

import lrn_ref as R
from test_gpu_misc_edges import guarded, guards_intact
from test_gpu_ops import close

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def geometry():
    from mcncrossmodalemotions_amd import vl
    return vl.nnnormalize_geometry()


@functools.lru_cache(maxsize=None)
def reference(shape, param, seed):
    x, d = R.case(shape, seed)
    return x, d, R.forward(x, list(param)), R.backward(x, list(param), d)


def check(shape, param, seed=0):
    from mcncrossmodalemotions_amd import vl
    x, d, y, dx = reference(tuple(shape), tuple(param), seed)
    xd, dd = vl.from_numpy(x), vl.from_numpy(d)
    got_y, got_dx = vl.to_numpy(vl.vl_nnnormalize(xd, param)), vl.to_numpy(vl.vl_nnnormalize(xd, param, dd))
    print("%s %s: forward %.3e of %.3g, backward %.3e of %.3g" % (shape, param, np.abs(got_y - y).max(), np.abs(y).max(),
                                                                  np.abs(got_dx - dx).max(), np.abs(dx).max()))
    close(got_y, y, R.TOL, "forward %s %s" % (shape, param))
    close(got_dx, dx, R.TOL, "backward %s %s" % (shape, param))


# ------------------------------------------------------------------------------------------------------- window edges
@pytest.mark.parametrize("C,N", R.WINDOW_CASES)
def test_window_edges(gpu, C, N):
    check((5, 13, C, 2), R.strong(N), seed=C * 100 + N)


@pytest.mark.parametrize("beta", [0.5, 1.0])
@pytest.mark.parametrize("C,N", [(6, 5), (6, 4), (40, 5)])
def test_window_edges_other_exponents(gpu, C, N, beta):
    check((5, 13, C, 2), R.strong(N, beta), seed=C * 100 + N)


# -------------------------------------------------------------------------------------------------------- pixel edges
def _planes():
    return [(1, 1), (7, 9), (8, 8), (5, 13), (16, 16), (257, 1), (3, 349), "ppb-1", "ppb", "ppb+1", "2ppb+1"]


def _plane(p):
    ppb = geometry()[0]
    return {"ppb-1": (ppb - 1, 1), "ppb": (ppb, 1), "ppb+1": (1, ppb + 1), "2ppb+1": (2 * ppb + 1, 1)}.get(p, p)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("plane", _planes(), ids=str)
def test_pixel_edges(gpu, plane, S):
    H, W = _plane(plane)
    check((H, W, 6, S), R.strong(5), seed=H * 7 + W)


# ------------------------------------------------------------------------------------------------------ channel edges
def _channels(c):
    cpp = geometry()[1]
    return {"cpp-1": cpp - 1, "cpp": cpp, "cpp+1": cpp + 1, "2cpp+1": 2 * cpp + 1}.get(c, c)


@pytest.mark.parametrize("N", [4, 5])
@pytest.mark.parametrize("C", [130, 513, "cpp-1", "cpp", "cpp+1", "2cpp+1"], ids=str)
def test_channel_edges(gpu, C, N):
    C = _channels(C)
    assert C >= 1, "the kernel splits the channel axis: channels_per_pass > 1"
    check((3, 3, C, 2), R.strong(N), seed=C + N)


@pytest.mark.parametrize("past", [0, 1])
@pytest.mark.parametrize("C", [130, "cpp+1"], ids=str)
def test_switch_between_the_arms(gpu, C, past):
    wir = geometry()[2]
    assert wir >= 1, "the kernel has two arms"
    C = _channels(C)
    check((3, 3, C, 2), R.strong(wir + past), seed=C + wir + past)


# ----------------------------------------------------------------------------------------------------- alignment gate
def _view(flat_view, shape):
    return flat_view.view(*reversed(shape)).permute(*reversed(range(len(shape))))


@pytest.mark.parametrize("N", [5, 4])
@pytest.mark.parametrize("which", ["x", "dzdy", "out"])
def test_operands_one_float_off_a_16_byte_boundary(gpu, which, N):
    """8 x 8 planes: the aligned call takes the 16-byte arm, a view one float off takes the 4-byte one -- the gate looks at
    the addresses it is given.  Same arithmetic per element: the results agree to a few ulps, and nothing outside the
    tensor is written"""
    from mcncrossmodalemotions_amd import vl
    shape, param = (8, 8, 6, 2), R.strong(N)
    x, d, y, dx = reference(shape, tuple(param), 77)
    n = x.size
    off = {k: (1 if k == which else 4) for k in ("x", "dzdy", "out")}
    fx, vx = guarded(x.ravel(order="F"), off["x"])
    fd, vd = guarded(d.ravel(order="F"), off["dzdy"])
    xd, dd = _view(vx, shape), _view(vd, shape)
    aligned_y = vl.to_numpy(vl.vl_nnnormalize(vl.from_numpy(x), param))
    aligned_dx = vl.to_numpy(vl.vl_nnnormalize(vl.from_numpy(x), param, vl.from_numpy(d)))
    for dz, ref, aligned in ((None, y, aligned_y), (dd, dx, aligned_dx)):
        fo, vo = guarded(np.zeros(n, np.float32), off["out"])
        got = vl.vl_nnnormalize(xd, param, dz, out=_view(vo, shape))
        assert got.data_ptr() == vo.data_ptr()
        got = vl.to_numpy(got)
        close(got, ref, R.TOL, "%s one float off" % which)
        assert np.abs(got - aligned).max() <= 1e-6 * max(1.0, np.abs(aligned).max())
        assert guards_intact(fo, off["out"], n)
    assert guards_intact(fx, off["x"], n) and guards_intact(fd, off["dzdy"], n)
    assert np.array_equal(vx.cpu().numpy(), x.ravel(order="F")) and np.array_equal(vd.cpu().numpy(), d.ravel(order="F"))


# ------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("N", [5, 11])
def test_all_zero_input(gpu, N):
    from mcncrossmodalemotions_amd import vl
    shape, param = (7, 9, 6, 2), [N, 2.0, 1e-4, 0.75]
    _, d = R.case(shape, 5)
    x = vl.mat_zeros(*shape)
    assert not vl.to_numpy(vl.vl_nnnormalize(x, param)).any()
    close(vl.to_numpy(vl.vl_nnnormalize(x, param, vl.from_numpy(d))), d.astype(np.float64) * 2.0 ** -0.75, R.TOL, "dx at x = 0")


def test_vgg_m_parameters(gpu):
    check((27, 27, 12, 2), R.VGG_M_PARAM, seed=1)


def test_empty_tensor_and_bad_param(gpu):
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    e = torch.empty((0, 3, 4, 4), device="cuda").permute(3, 2, 1, 0)
    assert tuple(vl.vl_nnnormalize(e, [5, 1, 1, 0.75]).shape) == (4, 4, 3, 0)
    x = vl.mat_zeros(2, 2, 3, 1)
    with pytest.raises(_lib.XmError, match="positive integer"):
        vl.vl_nnnormalize(x, [0, 1, 1, 0.75])
    with pytest.raises(ValueError, match="four elements"):
        vl.vl_nnnormalize(x, [5, 1, 1])
