"""The numpy routing table of tests/pool_routing.py against the CPU oracle (no GPU): scattering DZDY through the table must
reproduce O.vl_nnpool(x, pool, dzdy, ...) EXACTLY -- same first-maximum rule, same order of the fp32 additions -- on every
geometry tests/test_gpu_norm_pool_edges.py uses, on planted plateaus, constant inputs and -inf.  The GPU file then holds the
kernels' uint8 tables against this one."""
import numpy as np
import pytest

import pool_routing as PR
from oracle import oracle as O

# geometries beyond PR.LDS_CASES that the GPU file runs: (H, W, C, N, pool, stride, pad)
OTHER_GEOMETRIES = [
    (13, 11, 5, 3, (3, 3), (2, 2), 0),
    (9, 8, 6, 2, (5, 3), (3, 2), 0),
    (12, 12, 4, 2, (3, 3), (2, 2), (0, 1, 0, 1)),
    (10, 9, 3, 2, (2, 2), (1, 1), (1, 0, 1, 0)),
    (31, 21, 3, 2, (2, 2), (1, 1), 0),          # the plane-stride shapes, scaled down (same windows and strides)
    (31, 21, 3, 2, (5, 3), (1, 1), 0),
    (31, 21, 3, 2, (4, 3), (1, 1), 0),
    (6, 6, 7, 3, (2, 2), (1, 1), 0),
    (16, 18, 2, 2, (15, 17), (1, 1), 0),        # the largest window the table can encode (codes up to 254)
    (16, 18, 2, 2, (15, 17), (1, 1), (14, 3, 16, 5)),
    (7, 7, 5, 3, (7, 7), (1, 1), 0),            # global
    (8, 8, 6, 3, (8, 8), (1, 1), 0),
    (1, 3, 7, 1, (1, 3), (1, 1), 0),
    (7, 6, 4, 3, (5, 3), (3, 2), 0),
]


def _check(x, pool, stride, pad, seed=0):
    x = O.F(x)
    H, W = x.shape[:2]
    code = PR.routing_table(x, pool, stride, pad)
    y_ref = O.vl_nnpool(x, pool, stride=stride, pad=pad, method="max")
    assert code.shape == y_ref.shape
    dzdy = O.F(np.random.default_rng(seed).standard_normal(y_ref.shape))
    dx_ref = O.vl_nnpool(x, pool, dzdy, stride=stride, pad=pad, method="max")
    dx = PR.scatter(code, dzdy, H, W, pool, stride, pad)
    assert np.array_equal(dx, dx_ref), "routing differs at %d elements" % int((dx != dx_ref).sum())
    # the table names the maximum itself: gathering x at the recorded tap gives Y
    g = PR.Geo(H, W, pool, stride, pad)
    xp = g.embed(x, -np.inf)
    got = np.full(y_ref.shape, -np.inf, np.float32)
    for dw in range(g.pw):
        for dh in range(g.ph):
            m = code == dh + g.ph * dw
            got[m] = xp[g.tap(dh, dw)][m]
    assert np.array_equal(got, y_ref)
    return code


@pytest.mark.parametrize("name", sorted(PR.LDS_CASES))
def test_table_reproduces_the_oracle_on_the_lds_geometries(name):
    H, W, C, N, stride, pad = PR.LDS_CASES[name]
    x, _ = PR.lds_case_input(name)
    code = _check(x, PR.POOL3, stride, pad)
    assert code.max() <= 8
    # the plateau: a window that lies wholly inside it routes to its first tap
    g = PR.Geo(H, W, PR.POOL3, stride, pad)
    assert (x[min(5, H - 3):min(5, H - 3) + 3, min(4, W - 3):min(4, W - 3) + 3, 0, 0] == 4.0).all()
    # all-zero windows (post-ReLU ties) exist and route to their first in-tensor tap
    y = O.vl_nnpool(x, PR.POOL3, stride=stride, pad=pad, method="max")
    zero = y == 0
    assert zero.any()
    ho, wo = np.nonzero(zero)[:2]
    first = np.maximum(g.pt - ho * g.sy, 0) + g.ph * np.maximum(g.pl - wo * g.sx, 0)
    assert np.array_equal(code[zero], first.astype(np.uint8))


@pytest.mark.parametrize("geom", OTHER_GEOMETRIES)
def test_table_reproduces_the_oracle_on_the_other_geometries(geom):
    H, W, C, N, pool, stride, pad = geom
    _check(PR.planted_input(H * 31 + W, H, W, C, N, pool, stride, pad), pool, stride, pad)


@pytest.mark.parametrize("name", sorted(PR.LDS_CASES))
def test_plateaus_constant_and_minus_inf(name):
    H, W, C, N, stride, pad = PR.LDS_CASES[name]
    H, W = min(H, 40), W                      # the same strides and padding; rows beyond 40 add nothing here
    rng = np.random.default_rng(7)
    # plateaus: a 7 x 7 block of equal maxima holds whole windows and straddles its neighbours; two more touch the borders
    x = np.maximum(rng.standard_normal((H, W, C, N)), 0).astype(np.float32)
    hb, wb = min(7, H), min(7, W)
    x[3:3 + hb, :wb] = 5.0
    x[H - 2:, :, 0] = 6.0
    x[:, W - 1:, -1] = 6.0
    code = _check(x, PR.POOL3, stride, pad)
    g = PR.Geo(H, W, PR.POOL3, stride, pad)
    # all equal: every window routes to its first in-tensor tap
    for v in (0.0, -3.5):
        code = _check(np.full((H, W, C, N), v, np.float32), PR.POOL3, stride, pad)
        ho, wo = np.meshgrid(np.arange(g.Ho), np.arange(g.Wo), indexing="ij")
        first = np.maximum(g.pt - ho * g.sy, 0) + g.ph * np.maximum(g.pl - wo * g.sx, 0)
        assert np.array_equal(code[:, :, 0, 0], first.astype(np.uint8))
    # -inf: a window of nothing but -inf has no maximum, the oracle routes it nowhere
    code = _check(np.full((H, W, C, N), -np.inf, np.float32), PR.POOL3, stride, pad)
    assert (code == PR.NO_MAX).all()
    x = np.maximum(rng.standard_normal((H, W, C, N)), 0).astype(np.float32)
    x[rng.random(x.shape) < 0.7] = -np.inf
    x[:6, :3] = -np.inf
    code = _check(x, PR.POOL3, stride, pad)
    assert (code == PR.NO_MAX).any() and (code != PR.NO_MAX).any()


@pytest.mark.parametrize("name", sorted(PR.LDS_CASES))
@pytest.mark.parametrize("train", [True, False])
def test_fused_seeds_keep_near_ties_under_the_cap(name, train):
    """The fused GPU test exempts windows whose two largest values of the oracle's relu(bnorm(x)) differ by less than the
    forward bound, and caps them at 0.1 % of the windows.  The seeds are chosen so that the oracle alone -- its plain fp32
    arithmetic against its fp64-accumulate arithmetic -- agrees on the table outside such windows and stays under the cap."""
    H, W, C, N, stride, pad = PR.LDS_CASES[name]
    x, g, b, mom = PR.fused_case_input(name, train)
    y64, _ = O.vl_nnbnorm(x, g, b, moments=mom, acc64=True)
    y32, _ = O.vl_nnbnorm(x, g, b, moments=mom, acc64=False)
    y64, y32 = np.maximum(y64, 0), np.maximum(y32, 0)
    t64, t32 = PR.routing_table(y64, PR.POOL3, stride, pad), PR.routing_table(y32, PR.POOL3, stride, pad)
    tie = PR.near_tie_windows(y64, PR.POOL3, stride, pad)
    assert np.array_equal(t64[~tie], t32[~tie])
    assert tie.sum() <= 1e-3 * tie.size, (int(tie.sum()), tie.size)
