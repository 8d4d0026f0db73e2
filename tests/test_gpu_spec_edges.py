"""GPU: xm_spec_bucket_batch (csrc/spec.hip) where a block of spec_gemm_kernel owns many tiles and several clips, and
at the edges of its entry point -- against the float64 restatement O.spec_rownorm(O.run_spec(clip)) cropped at f0, with
frames of the crop outside [0, T) filled as include/xmodal.h says (magnitude 0).

Block g of G owns the tiles [g q, (g + 1) q) of the flat (clip, tile) list, q = ceil(tiles / G); G is 2 x CUs, so an
input small enough for a test has q = 1 and never carries statistics from tile to tile, never flushes them when the
clip changes, never skips a clip without a tile.  xm_debug_set("spec_blocks", v) forces G; every test that sets it
restores it in a `finally` (`forced`).  The tables, the float64 reference, the allowances and a CPU restatement of the
launch geometry that asserts what each table covers are in tests/test_spec_edges_cpu.py.

Allowances: TOL = 1e-3 of tests/test_gpu_spec_bucket.py against the reference, max(TOL, 8 * 2^-24 * kappa) for clips of
fewer than 31 frames (kappa = max over the bins of mu / sd); 2^-22 (kappa + max |out|) between two groupings of the
same clip, which differ in the order of fp64 merges only (`regroup_bound`)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import test_spec_edges_cpu as E
from test_gpu_spec_bucket import TOL, close, err_of

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
XM_ENOTSUP = 5


@contextlib.contextmanager
def forced(G):
    """spec_gemm_kernel on G blocks (0: the default, CUs x 2) for the body; the previous setting comes back whatever
    happens"""
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    old = L.xm_debug_force_spec_blocks(G)
    try:
        assert L.xm_debug_get(b"spec_blocks") == G
        yield
    finally:
        L.xm_debug_force_spec_blocks(old)


def _vl_run(gpu, bank, desc, rsize, audio=None):
    """N x B x rsize through vl.spec_bucket_batch"""
    import torch
    from mcncrossmodalemotions_amd import vl
    got = vl.to_numpy(vl.spec_bucket_batch(torch.from_numpy(bank).to(gpu), desc, rsize, audio=audio))
    return np.ascontiguousarray(got[:, :, 0, :].transpose(2, 0, 1))


def _c_run(gpu, bank, desc, rsize, fs=16000, Tw=25, Ts=10):
    """(status, N x B x rsize) through the C entry, which takes descriptors vl.spec_bucket_batch refuses; `out` is
    prefilled with SENTINEL"""
    import torch
    from mcncrossmodalemotions_amd import _lib, batch as xbatch, vl
    L = _lib.load()
    N = len(desc)
    nw, ns = int(round(1e-3 * Tw * fs)), int(round(1e-3 * Ts * fs))
    w = torch.from_numpy(bank).to(gpu)
    d = torch.from_numpy(np.ascontiguousarray(desc, np.int64).reshape(-1)).to(gpu)
    fb = xbatch._spec_filter_bank(fs, Tw, Ts, 0.97, 1024, gpu)
    out = torch.full((N * rsize * 512,), SENTINEL, dtype=torch.float32, device=gpu)
    rc = L.xm_spec_bucket_batch(C.c_void_p(w.data_ptr()), w.numel(), C.c_void_p(d.data_ptr()), N, rsize,
                                C.c_void_p(fb.data_ptr()), nw + 1, ns, 512, C.c_void_p(out.data_ptr()), vl._stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().reshape(N, rsize, 512).transpose(0, 2, 1)


class Worst:
    """the figures a group of tests reports: worst error against the reference, worst regrouping difference as a
    fraction of its bound, worst err / (2^-24 kappa) over the clips of fewer than 31 frames"""

    def __init__(self, what):
        self.what, self.err, self.regroup, self.short = what, 0.0, 0.0, 0.0

    def report(self):
        print("%s: worst err vs float64 %.3e; worst regrouping difference %.3f of its bound; worst err / (2^-24 kappa) "
              "at T < 31: %.3f" % (self.what, self.err, self.regroup, self.short))


def check_clips(got, refs, T, what, worst, base=None):
    """every clip of `got` (N x B x rsize) against its reference and, with `base` (the output under the default G),
    within the regrouping bound of it.  Figures first, assertions after."""
    bad = []
    for n, (ref, kappa) in enumerate(refs):
        if ref is None:
            if not np.isnan(got[n]).all():
                bad.append("%s clip %d (T = %d): not NaN everywhere" % (what, n, T[n]))
            continue
        err, tol = err_of(got[n], ref), E.allowance(T[n], kappa)
        worst.err = max(worst.err, err)
        if T[n] < 31:
            worst.short = max(worst.short, err / (E.EPS * kappa))
        if not err <= tol:
            bad.append("%s clip %d (T = %d): err %.3e > %.3e" % (what, n, T[n], err, tol))
        if base is not None:
            diff, bound = float(np.abs(got[n].astype(np.float64) - base[n]).max()), E.regroup_bound(ref, kappa)
            worst.regroup = max(worst.regroup, diff / bound)
            if not diff <= bound:
                bad.append("%s clip %d (T = %d): %.3e from the default grouping > %.3e" % (what, n, T[n], diff, bound))
    worst.report()
    assert not bad, "\n".join(bad)


# ---- (a) many tiles per block, blocks across clips ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_a(gpu):
    bank, desc = E.table_a()
    refs = E.reference(bank, desc, E.RSIZE_A)
    with forced(0):
        base = _vl_run(gpu, bank, desc, E.RSIZE_A)
    return bank, desc, refs, base


def test_default_grid(gpu, case_a):
    bank, desc, refs, base = case_a
    assert base.shape == (len(desc), 512, E.RSIZE_A)
    check_clips(base, refs, E.frames_of(desc[:, 1]), "(a) default G", Worst("(a) default G"))


@pytest.mark.parametrize("G", E.FORCED_A)
def test_many_tiles_per_block(gpu, case_a, G):
    bank, desc, refs, base = case_a
    with forced(G):
        got = _vl_run(gpu, bank, desc, E.RSIZE_A)
    check_clips(got, refs, E.frames_of(desc[:, 1]), "(a) G = %d" % G, Worst("(a) G = %d" % G), base)


# ---- (d) a clip does not see its neighbours or its position ------------------------------------------------------------
@pytest.mark.parametrize("G", E.FORCED_D + [0])
def test_position_in_the_table(gpu, case_a, G):
    bank, desc = E.table_d()
    ref, kappa = case_a[2][E.D_CLIP]
    with forced(G):
        got = _vl_run(gpu, bank, desc, E.RSIZE_A)
    bound, worst = E.regroup_bound(ref, kappa), 0.0
    for i in E.D_AT:
        close(got[i], ref, TOL, "(d) G = %d, copy at %d" % (G, i))
        for j in E.D_AT:
            worst = max(worst, float(np.abs(got[i].astype(np.float64) - got[j]).max()))
    print("(d) G = %d: copies differ by %.3e, %.3f of the regrouping bound %.3e" % (G, worst, worst / bound, bound))
    assert worst <= bound
    # the clips between the copies are the ones of (a), each still its own
    rest = [i for i in range(len(desc)) if i not in E.D_AT]
    for i, k in zip(rest, range(len(rest))):
        assert float(np.abs(got[i].astype(np.float64) - case_a[3][k]).max()) <= E.regroup_bound(*case_a[2][k]), (i, k)


# ---- (b) short, empty and overhanging clips through the C entry --------------------------------------------------------
@pytest.fixture(scope="module")
def case_b(gpu):
    bank, desc = E.table_b()
    refs = E.reference(bank, desc, E.RSIZE_B)
    with forced(0):
        rc, base = _c_run(gpu, bank, desc, E.RSIZE_B)
    assert rc == 0
    return bank, desc, refs, base


@pytest.mark.parametrize("G", E.FORCED_B + [0])
def test_short_empty_overhanging(gpu, case_b, G):
    bank, desc, refs, base = case_b
    T = E.frames_of(desc[:, 1])
    with forced(G):
        rc, got = _c_run(gpu, bank, desc, E.RSIZE_B)
    assert rc == 0
    assert not (got == SENTINEL).any(), "elements never written: clips %s" % sorted(set(np.nonzero(got == SENTINEL)[0]))
    for n in np.nonzero(T < 2)[0]:
        assert np.isnan(got[n]).all(), (n, T[n])
    for n in np.nonzero(T >= 2)[0]:
        assert np.isfinite(got[n]).all(), (n, T[n])
    check_clips(got, refs, T, "(b) G = %d" % G, Worst("(b) G = %d" % G), base)


@pytest.mark.parametrize("G", [1, 3, 0])
def test_no_clip_has_a_frame(gpu, G):
    """total = 0 tiles: every block of the gemm kernel returns at once, and the finish kernel never divides by q"""
    bank, offs = E.bank_of(E.TABLE_B0, 3)
    desc = np.stack([offs[:-1], E.TABLE_B0, [0, -2, 0, 1, 5]], 1)
    with forced(G):
        rc, got = _c_run(gpu, bank, desc, E.RSIZE_B)
    assert rc == 0 and got.shape == (5, 512, E.RSIZE_B)
    assert not (got == SENTINEL).any() and np.isnan(got).all()


# ---- (c) other framings --------------------------------------------------------------------------------------------------
FRAMINGS = [(8000, 25, 10, 201, 80, [(65, 0), (130, 79)]),            # two clips of two and three tiles
            (16000, 20, 5, 321, 80, [(70, 1), (33, 0), (129, 79)]),   # floor(k / hop) reaches 4
            (22050, 25, 10, 552, 220, [(65, 219), (100, 0)])]         # Nw = 551: even taps, no padding tap
RSIZE_C = 16


@pytest.mark.parametrize("fs,Tw,Ts,taps,hop,frames_r", FRAMINGS)
def test_other_framings(gpu, fs, Tw, Ts, taps, hop, frames_r):
    audio = dict(fs=fs, Tw=Tw, Ts=Ts)
    nw, ns = int(round(1e-3 * Tw * fs)), int(round(1e-3 * Ts * fs))
    assert (nw + 1, ns) == (taps, hop)
    lengths = [nw + ns * (t - 1) + r for t, r in frames_r]
    bank, offs = E.bank_of(lengths, fs + Tw)
    T = E.frames_of(lengths, nw, ns)
    assert T.tolist() == [t for t, _ in frames_r]
    f0 = [(0, (t - RSIZE_C) // 2, t - RSIZE_C)[(i + 1) % 3] for i, t in enumerate(T.tolist())]
    desc = np.stack([offs[:-1], lengths, f0], 1).astype(np.int64)
    refs = E.reference(bank, desc, RSIZE_C, **audio)
    with forced(0):
        base = _vl_run(gpu, bank, desc, RSIZE_C, audio)
    what = "(c) %d Hz, %d / %d ms" % (fs, Tw, Ts)
    check_clips(base, refs, T, what + ", default G", Worst(what + ", default G"))
    with forced(2):
        got = _vl_run(gpu, bank, desc, RSIZE_C, audio)
    check_clips(got, refs, T, what + ", G = 2", Worst(what + ", G = 2"), base)


def test_span_beyond_the_lds_is_refused(gpu):
    """16000 Hz, 10 ms frames every 25 ms: hop 400 > taps 161, and 64 frames span about 101 KB"""
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    bank, offs = E.bank_of([160 + 400 * 69], 9)
    desc = np.array([[0, bank.size, 0]], np.int64)
    for G in (2, 0):
        with forced(G):
            rc, got = _c_run(gpu, bank, desc, 8, 16000, 10, 25)
            assert rc == XM_ENOTSUP and (got == SENTINEL).all()                   # before any launch
            with pytest.raises(_lib.XmError, match="64-frame sample span") as e:
                _lib.check(rc)
            assert e.value.code == XM_ENOTSUP
            with pytest.raises(_lib.XmError, match="64-frame sample span"):
                vl.spec_bucket_batch(torch.from_numpy(bank).to(gpu), desc, 8, audio=dict(fs=16000, Tw=10, Ts=25))


# ---- (e) more clips than spec_plan_kernel has threads --------------------------------------------------------------------
def test_more_clips_than_plan_threads(gpu):
    import torch
    bank, desc = E.table_e()
    T = E.frames_of(desc[:, 1])
    G = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count
    q = E.plan(T, G)[1]
    print("(e): N = %d, default G = %d, q = %d" % (len(desc), G, q))
    assert q >= 2
    refs = E.reference(bank, desc, E.RSIZE_E)
    with forced(0):
        rc, got = _c_run(gpu, bank, desc, E.RSIZE_E)
    assert rc == 0 and not (got == SENTINEL).any()
    check_clips(got, refs, T, "(e)", Worst("(e)"))


def test_switch_values(gpu):
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    assert L.xm_debug_get(b"spec_blocks") == 0
    try:
        assert L.xm_debug_force_spec_blocks(7) == 0 and L.xm_debug_get(b"spec_blocks") == 7
        assert L.xm_debug_force_spec_blocks(-3) == 7 and L.xm_debug_get(b"spec_blocks") == 0
    finally:
        L.xm_debug_force_spec_blocks(0)
