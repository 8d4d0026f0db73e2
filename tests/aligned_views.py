"""Device tensors at a chosen distance from a 16-byte boundary, and guarded destinations, for the tests that hand the C entry
points operands that are 4-byte aligned only (tests/test_gpu_norm_pool_edges.py, tests/test_gpu_conv_alignment.py)."""
import numpy as np

GUARD = 64                       # sentinel floats on either side of a guarded destination (256 bytes: keeps the alignment)
SENTINEL = 0x7FC5A5A5            # a quiet NaN with a recognisable payload: an element the call did not write stays NaN


def _mat_view(flat, shape):
    """the flat buffer seen as a MATLAB-layout (column-major) tensor of `shape`"""
    return flat.view(*reversed(shape)).permute(*reversed(range(len(shape))))


def misaligned(t, offset=1):
    """copy of the MATLAB-layout device tensor `t` that starts `offset` floats past a 16-byte boundary: buf[offset:] of a flat
    buffer, reshaped and permuted to MATLAB layout (what a sample slice x[..., k:] of a tensor with an odd plane size looks
    like).  offset 1: ptr % 16 == 4, refused by the 16- and the 8-byte gates; offset 2: ptr % 16 == 8, passes the 8-byte gates
    and fails the 16-byte ones; offset 0: an aligned copy."""
    import torch
    assert 0 <= offset < 4
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = _mat_view(flat[offset:offset + t.numel()], tuple(t.shape))
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * offset
    return v


class Guarded:
    """a destination of MATLAB shape `shape` that starts `offset` floats past a 16-byte boundary inside a buffer with GUARD
    sentinel floats in front of it and at least GUARD behind; the destination itself starts out as sentinels too (NaN)"""

    def __init__(self, shape, offset, device):
        import torch
        assert 0 <= offset < 4
        self.n = int(np.prod(shape))
        self.lo = GUARD + offset
        self.flat = torch.empty(self.n + 2 * GUARD + 4, dtype=torch.float32, device=device)
        self.flat.view(torch.int32).fill_(SENTINEL)
        self.view = _mat_view(self.flat[self.lo:self.lo + self.n], tuple(int(s) for s in shape))
        assert self.view.data_ptr() % 16 == 4 * offset

    def assert_guards_untouched(self, what=""):
        import torch
        bits = self.flat.view(torch.int32).cpu().numpy()
        front, back = bits[:self.lo], bits[self.lo + self.n:]
        assert front.size >= GUARD and back.size >= GUARD
        assert int((front != SENTINEL).sum()) == 0, "%s: wrote in front of the destination" % what
        assert int((back != SENTINEL).sum()) == 0, "%s: wrote behind the destination" % what
