"""The prepared dgrad filter operand (csrc/conv.hip: g_prep, PrepKey, g_param_version, dgrad_filter_operand) -- the one
thing the library remembers between calls that can change a RESULT.  vl.conv_prepare_backward builds the transposed /
parity-split filter bank into a persistent buffer keyed by the filter's address and part of the geometry; a later
backward call takes it when the parameter version it was stamped with is still current.  Wrong bookkeeping there is a
silent wrong dX, so every test compares dX with O.vl_nnconv(acc64=True) under test_gpu_ops.close / TOL (the project's
bound for dX, unchanged) and reads from xm_debug_get("dgrad_last_prepared") whether the call took the cached operand
(1), built its own (0) or went a route without one (-1).

A prepared and an unprepared call of one geometry run the same GEMM on the same operand bits: their results are compared
bit for bit, after warm-up calls that leave the tuning entries of the shape behind.

The cache is keyed by address and never evicted, and the caching allocator hands a freed filter's address to the next
tensor of its size: every test starts with vl.params_changed() (the `stale_cache` fixture), so that no entry of an
earlier test answers for a tensor of this one.

What the tests leave behind (entries are never freed; counted from the shapes, not measured: per entry the sum over the
stride classes of 4 * FC [* FH] * Rp * G bytes, each rounded up to 256): a) 669,440 bytes, 524,288 of them the skinny
case's; b) 9 entries of 1,280; c) 1,024 + 6,144 + 2,816 + 2,048; d) the filters behind the first layer of the 1/8-width
student, 1,041,920 bytes and their padding, for each of the two nets that prepare -- at most 2.8 MB in all, less where
the allocator gives two tests' filters one address (one buffer per distinct address and key)."""
import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_ops import CONV_CASES, DGRAD_S2_CASES, MERGED_DGRAD_CASES, TOL, close, rnd

pytestmark = pytest.mark.gpu


def dbg(key):
    from mcncrossmodalemotions_amd import _lib
    return _lib.load().xm_debug_get(key.encode())


@pytest.fixture(autouse=True)
def stale_cache(gpu):
    from mcncrossmodalemotions_amd import vl
    vl.params_changed()


class Layer:
    """one convolution on the device: operands from a seed, dX through vl with the key the call left, and the oracle's dX"""

    def __init__(self, case, seed, f=None, fd=None):
        from mcncrossmodalemotions_amd import vl
        self.case = case
        H, W, C, N, FH, FW, FC, K, self.stride, self.pad, self.dil = case
        rng = np.random.default_rng(seed)
        self.x = rnd(rng, H, W, C, N)
        self.f = rnd(rng, FH, FW, FC, K) if f is None else f
        y = O.vl_nnconv(self.x, self.f, None, stride=self.stride, pad=self.pad, dilate=self.dil)
        self.dzdy, self.acc = rnd(rng, *y.shape), rnd(rng, H, W, C, N)
        self.xd, self.dd, self.ad = vl.from_numpy(self.x), vl.from_numpy(self.dzdy), vl.from_numpy(self.acc)
        self.fd = vl.from_numpy(self.f) if fd is None else fd
        self.kw = dict(stride=self.stride, pad=self.pad, dilate=self.dil)

    def ref(self, f=None, accum=False):
        dx, _, _ = O.vl_nnconv(self.x, self.f if f is None else f, None, self.dzdy, acc64=True, no_der_filters=True, **self.kw)
        return dx + self.acc if accum else dx

    def prepare(self, stream=None):
        import torch
        from mcncrossmodalemotions_amd import vl
        if stream is None:
            vl.conv_prepare_backward(self.xd, self.fd, **self.kw)
            return
        stream.wait_stream(torch.cuda.current_stream())      # as DagNN.eval orders its side stream behind the main one
        with torch.cuda.stream(stream):
            vl.conv_prepare_backward(self.xd, self.fd, **self.kw)

    def backward(self, accum=False):
        """(dX on the host, dgrad_last_prepared) of one backward call on the current stream"""
        from mcncrossmodalemotions_amd import vl
        dx, _, _ = vl.vl_nnconv(self.xd, self.fd, None, self.dd, no_der_filters=True, dx_accum=self.ad if accum else None,
                                **self.kw)
        how = dbg("dgrad_last_prepared")
        return vl.to_numpy(dx), how


# ---- a. every operand family ------------------------------------------------------------------------------------------
# (name, geometry (test_gpu_ops.CONV_CASES layout), prepare on a second stream)
FAMILIES = [
    ("1x1 pure transpose", CONV_CASES[13], True),            # (1,1,100,5), 1x1x100x96: transpose_filter_kernel
    ("FHx1 folded into the rows", CONV_CASES[12], False),     # (9,8,24,4), 9x1x24x80
    ("3x3 stride 1 pad 1", CONV_CASES[0], True),
    ("5x5 stride 2 pad 1", CONV_CASES[2], False),             # four parity classes, launched one by one
    ("merged multi-class launch", MERGED_DGRAD_CASES[1], True),
    ("1x1 stride 2", CONV_CASES[14], False),                  # three of four pixel classes get no gradient
    ("two filter groups", CONV_CASES[9], False),
    ("dilation 2", CONV_CASES[8], False),
    ("asymmetric stride and pad", CONV_CASES[7], True),       # (11,10,4,2), 3x2, stride (2,3), pad (0,1,2,0)
    ("skinny dgrad", CONV_CASES[15], False),                  # (1,1,512,40), K = 256: fc_skinny4_kernel (plain dX only)
]


def test_families_name_the_geometries_meant():
    """the indices above are the geometries the names say"""
    g = {n: c for n, c, _ in FAMILIES}
    assert g["1x1 pure transpose"][:8] == (1, 1, 100, 5, 1, 1, 100, 96)
    assert g["FHx1 folded into the rows"][:8] == (9, 8, 24, 4, 9, 1, 24, 80)
    assert g["3x3 stride 1 pad 1"][4:6] == (3, 3) and g["3x3 stride 1 pad 1"][8:] == ((1, 1), (1, 1, 1, 1), (1, 1))
    assert g["5x5 stride 2 pad 1"][4:6] == (5, 5) and g["5x5 stride 2 pad 1"][8:10] == ((2, 2), (1, 1, 1, 1))
    assert g["1x1 stride 2"][4:6] == (1, 1) and g["1x1 stride 2"][8] == (2, 2)
    assert g["two filter groups"][2] == 2 * g["two filter groups"][6]
    assert g["dilation 2"][10] == (2, 2)
    assert g["asymmetric stride and pad"] == (11, 10, 4, 2, 3, 2, 4, 6, (2, 3), (0, 1, 2, 0), (1, 1))
    assert g["skinny dgrad"][:8] == (1, 1, 512, 40, 1, 1, 512, 256)


@pytest.mark.parametrize("name,case,side", FAMILIES, ids=[n for n, _, _ in FAMILIES])
def test_prepared_equals_unprepared_equals_oracle(gpu, name, case, side):
    """Without a prepare the call builds its operand (key 0), after one it takes the cached operand (key 1), also when the
    prepare ran on a second stream; the two results are the same bits and both are the oracle's -- plain and with
    dx_accum in the epilogue."""
    import torch
    L = Layer(case, 1000 + len(name))
    ref = {False: L.ref(), True: L.ref(accum=True)}
    for accum in (False, True):              # warm-up: the tuning entries of both calls exist from here on
        L.backward(accum)
    plain = {}
    for accum in (False, True):
        plain[accum], how = L.backward(accum)
        assert how == 0, (name, accum)
        close(plain[accum], ref[accum], what="%s, unprepared, accum %d" % (name, accum))
    L.prepare(torch.cuda.Stream() if side else None)
    for accum in (False, True):
        dx, how = L.backward(accum)
        assert how == 1, (name, accum)
        close(dx, ref[accum], what="%s, prepared, accum %d" % (name, accum))
        assert np.array_equal(dx, plain[accum]), (name, accum)
    torch.cuda.synchronize()


def test_dgrad_s2_route_has_nothing_to_prepare(gpu):
    """conv_dgrad_s2_kernel lays its filter operand out inside the call: with the route forced a prepare is a no-op (the
    next call of the generic route finds nothing), the key reads -1 and dX is the oracle's.  The same key for a call
    with no stride class that holds a tap: a 1 x 1 / stride 2 filter whose only input row sits in the tapless class."""
    from mcncrossmodalemotions_amd import _lib
    lib = _lib.load()
    H, W, C, N, K, pad = DGRAD_S2_CASES[1]                    # (30, 21, 20, 3, 24)
    L = Layer((H, W, C, N, 5, 5, C, K, (2, 2), pad, (1, 1)), 77)
    ref = L.ref()
    old = lib.xm_debug_set(b"dgrad_s2", 1)
    try:
        L.prepare()
        dx, how = L.backward()
        assert how == -1
        close(dx, ref, what="dgrad_s2 route")
        lib.xm_debug_set(b"dgrad_s2", 0)
        dx, how = L.backward()
        assert how == 0                                        # the prepare above left no entry
        close(dx, ref, what="generic route after a no-op prepare")
    finally:
        lib.xm_debug_set(b"dgrad_s2", old)
    E = Layer((1, 5, 8, 2, 1, 1, 8, 16, (2, 2), (1, 0, 0, 0), (1, 1)), 78)
    E.prepare()
    dx, how = E.backward()
    assert how == -1
    assert not dx.any() and not E.ref().any()
    dx, how = E.backward(accum=True)
    assert how == -1 and np.array_equal(dx, E.acc)


# ---- b. every updater invalidates -------------------------------------------------------------------------------------
UPD_CASE = CONV_CASES[0]      # 3x3 / stride 1 / pad 1 on 12 x 9 x 5 x 2, 7 filters


def _updaters():
    """name -> callable(w): changes the filter tensor `w` in place through one of the package's update paths.  der is
    standard normal, the states start at zero, weight decay is 0 and batch 1; the steps move every filter value by a few
    tenths (the test asserts the effect on dX on the CPU and does not model the updater)."""
    import torch
    from mcncrossmodalemotions_amd import vl

    def operands(w):
        g = torch.Generator(device="cpu").manual_seed(9)
        der = torch.randn(w.numel(), generator=g).to(w.device)
        return der, torch.zeros_like(der), torch.zeros_like(der)

    def sgd(w):
        der, m, _ = operands(w)
        vl.sgd_update(w, m, der, 0.5, momentum=0.9, weight_decay=0.0, batch=1.0)

    def average(w):
        der, _, _ = operands(w)
        vl.average_update(w, der, 0.5)

    def solver(kind, lr, **opts):
        def run(w):
            der, s1, s2 = operands(w)
            vl.solver_update(kind, w, s1, s2 if vl.SOLVERS[kind][2] else None, der, lr, 0.0, 1.0, t=1, **opts)
        return run

    def torch_write(w):
        w.mul_(-0.5)
        vl.params_changed()

    return {"sgd": sgd, "average": average, "adagrad": solver("adagrad", 0.5), "rmsprop": solver("rmsprop", 0.05),
            "adadelta": solver("adadelta", 0.5, epsilon=1.0), "adam": solver("adam", 0.5),
            "nesterov": solver("nesterov", 0.3, momentum=0.9), "torch": torch_write}


UPDATERS = ["sgd", "average", "adagrad", "rmsprop", "adadelta", "adam", "nesterov", "torch"]


@pytest.mark.parametrize("how_updated", UPDATERS)
def test_every_updater_invalidates(gpu, how_updated):
    """prepare, update the filters, backward: the call must build its operand anew (key 0) and give the dX of the filter
    values read back after the update; the old and the new filters' dX differ by >= 100 x the tolerance bound (asserted
    on the CPU), so an operand left over from before the update cannot pass.  A new prepare is a hit again, and right."""
    from mcncrossmodalemotions_amd import vl
    L = Layer(UPD_CASE, 31)
    ref_old = L.ref()
    L.backward()                                               # warm-up
    L.prepare()
    dx, how = L.backward()
    assert how == 1
    close(dx, ref_old, what="prepared, before the update")
    _updaters()[how_updated](L.fd)
    dx_new, how = L.backward()
    f_new = vl.to_numpy(L.fd)
    ref_new = L.ref(f_new)
    assert np.abs(ref_new - ref_old).max() >= 100 * TOL * max(1.0, np.abs(ref_new).max(), np.abs(ref_old).max())
    assert how == 0, how_updated
    close(dx_new, ref_new, what="after %s" % how_updated)
    L.prepare()
    dx, how = L.backward()
    assert how == 1
    close(dx, ref_new, what="prepared again after %s" % how_updated)
    assert np.array_equal(dx, dx_new)


def test_torch_write_without_params_changed_is_the_documented_hazard(gpu):
    """include/xmodal.h: a host that changes the filters by other means calls xm_params_changed.  Without it the library
    cannot know: the next backward still takes the prepared operand (only that is asserted); after vl.params_changed()
    it builds a new one and is right."""
    from mcncrossmodalemotions_amd import vl
    L = Layer(UPD_CASE, 32)
    L.prepare()
    L.fd.mul_(-0.5)
    _, how = L.backward()
    assert how == 1
    vl.params_changed()
    dx, how = L.backward()
    assert how == 0
    close(dx, L.ref(vl.to_numpy(L.fd)), what="after params_changed")


# ---- c. the key -------------------------------------------------------------------------------------------------------
KEY_BASE = (12, 9, 4, 2, 3, 3, 4, 6, (1, 1), (1, 1, 1, 1), (1, 1))


def _variant(**ch):
    names = ["H", "W", "C", "N", "FH", "FW", "FC", "K", "stride", "pad", "dil"]
    return tuple(ch.get(n, v) for n, v in zip(names, KEY_BASE))


# (what changed between prepare and backward, geometry of the backward, expected dgrad_last_prepared)
KEY_VARIANTS = [
    ("nothing", KEY_BASE, 1),
    ("batch size 2 -> 3", _variant(N=3), 1),
    ("pb and pr (Ho, Wo differ)", _variant(pad=(1, 2, 1, 0)), 1),
    ("pt", _variant(pad=(2, 1, 1, 1)), 0),
    ("pl", _variant(pad=(1, 1, 0, 1)), 0),
    ("stride", _variant(stride=(2, 2)), 0),
    ("dilation", _variant(dil=(2, 2)), 0),
    ("H", _variant(H=13), 0),
    ("W", _variant(W=10), 0),
]


def test_key_shares_what_it_may_and_separates_what_it_must(gpu):
    """One filter tensor, prepared once at KEY_BASE: a backward call with another batch size or other bottom / right
    padding may take the operand (it does not depend on them) and must still be right; one with other top / left
    padding, stride, dilation or input extent must not take it."""
    P = Layer(KEY_BASE, 40)
    P.prepare()
    for k, (what, case, expect) in enumerate(KEY_VARIANTS + [KEY_VARIANTS[0]]):
        V = Layer(case, 41 + k, f=P.f, fd=P.fd)
        dx, how = V.backward()
        assert how == expect, what
        close(dx, V.ref(), what="prepared at the base geometry, changed: " + what)
        dx, how = V.backward(accum=True)
        assert how == expect, what
        close(dx, V.ref(accum=True), what="prepared at the base geometry, accum, changed: " + what)


GROUP_CASES = [(4, 8), (8, 4), (4, 16), (16, 4)]      # C of the prepare, C of the backward; the filters are 3 x 3 x 4 x 8


@pytest.mark.parametrize("c_prep,c_run", GROUP_CASES)
def test_key_separates_filter_groups(gpu, c_prep, c_run):
    """The same 3 x 3 x 4 x 8 filter tensor serves X of 4, 8 or 16 channels as 1, 2 or 4 filter groups; the operand holds
    K / G filters per group (Rp = 80, 48, 32 columns a row), so one prepared for another group count must not be taken --
    the key carries G.  (320 / 384 / 512 floats: in the (8, 4) and (16, 4) cases the buffer is large enough for the
    size guard to let a foreign operand through.)"""
    P = Layer((10, 9, c_prep, 2, 3, 3, 4, 8, (1, 1), (1, 1, 1, 1), (1, 1)), 60)
    V = Layer((10, 9, c_run, 2, 3, 3, 4, 8, (1, 1), (1, 1, 1, 1), (1, 1)), 61, f=P.f, fd=P.fd)
    P.prepare()
    dx, how = V.backward()
    assert how == 0
    close(dx, V.ref(), what="prepared for %d groups, run with %d" % (c_prep // 4, c_run // 4))
    dx, how = P.backward()
    assert how == 1
    close(dx, P.ref(), what="the prepared geometry itself")


def test_one_tensor_small_then_large_operand(gpu):
    """One filter tensor prepared for a small operand (one group, 320 floats) and then for a larger one (two groups, 384
    floats): each geometry finds its own operand, also the first after the second was built, and every result is right.
    (Every field the operand's size depends on is part of the key, so the two are separate entries and the `bytes >= abytes`
    guard of the lookup has no entry to replace; an entry that the larger prepare overwrote would show here as a wrong
    dX of the small geometry.)"""
    S = Layer((10, 9, 4, 2, 3, 3, 4, 8, (1, 1), (1, 1, 1, 1), (1, 1)), 70)
    B = Layer((10, 9, 8, 3, 3, 3, 4, 8, (1, 1), (1, 1, 1, 1), (1, 1)), 71, f=S.f, fd=S.fd)
    S.prepare()
    dx, how = S.backward()
    assert how == 1
    close(dx, S.ref(), what="small operand")
    B.prepare()
    dx, how = B.backward()
    assert how == 1
    close(dx, B.ref(), what="large operand")
    dx, how = S.backward()
    assert how == 1
    close(dx, S.ref(), what="small operand after the large one was built")


def test_two_filters_of_one_shape_do_not_answer_for_each_other(gpu):
    A = Layer(KEY_BASE, 50)
    B = Layer(KEY_BASE, 51)
    assert A.fd.data_ptr() != B.fd.data_ptr()
    assert np.abs(A.ref() - Layer.ref(A, B.f)).max() >= 100 * TOL * max(1.0, np.abs(A.ref()).max())
    A.prepare()
    B.prepare()
    for L in (A, B, A):
        dx, how = L.backward()
        assert how == 1
        close(dx, L.ref(), what="two prepared filters")
    # B's filters under A's input and output derivative: B's operand, not A's
    X = Layer(KEY_BASE, 50, f=B.f, fd=B.fd)
    dx, how = X.backward()
    assert how == 1
    close(dx, X.ref(), what="the other filter, same geometry")


# ---- d. Python flows --------------------------------------------------------------------------------------------------
def _student(seed):
    from mcncrossmodalemotions_amd import zoo
    from mcncrossmodalemotions_amd import dagnn
    net = zoo.emoVoxZoo(numSeconds=1, width_mult=0.125, seed=seed)
    net.pack_params()
    # network inputs get no derivative; the first variable dgrad writes is the input of the second convolution
    convs = [l for l in net.layers if isinstance(l.block, dagnn.Conv)]
    net.vars[convs[1].inputs[0]].precious = True
    return net, convs[1].inputs[0]


def _ders(net, var, inputs):
    """one eval with derivatives -> (every parameter derivative, the derivative of `var`), cloned"""
    import torch
    net.eval(inputs, ["objective", 1])
    torch.cuda.synchronize()
    return net._flat.der.clone(), net.vars[var].der.clone()


def _flow_inputs():
    from mcncrossmodalemotions_amd import vl
    rng = np.random.default_rng(5)
    xd = vl.from_numpy(O.F(rng.standard_normal((512, 100, 1, 4))))
    lgd = vl.from_numpy(O.F(rng.standard_normal((1, 1, 8, 4)) * 3))
    return ["data", xd, "logitTarget", lgd, "maxLabel", vl.max_label(lgd)]


def test_load_checkpoint_after_a_prepared_step(gpu, tmp_path):
    """A net whose last eval prepared its operands (wgradStream set, no update after it) takes other parameter values from
    a checkpoint -- written in place, at the addresses the operands are keyed by -- and then runs a backward pass for which
    nothing is prepared (wgradStream None).  Every parameter derivative and the first data derivative are the bits of a
    fresh net loaded from the same file that never prepared anything."""
    import torch
    from mcncrossmodalemotions_amd import train
    inputs = _flow_inputs()
    net, var = _student(1)
    net.wgradStream = torch.cuda.Stream()
    assert net.prepareBackward
    _ders(net, var, inputs)                                    # prepares every convolution's operand, no update
    other, _ = _student(2)
    path = str(tmp_path / "other.pt")
    train.save_checkpoint(other, path, {}, 1)
    train.load_checkpoint(net, path)
    net.wgradStream = None
    got = _ders(net, var, inputs)
    fresh, _ = _student(3)
    train.load_checkpoint(fresh, path)
    want = _ders(fresh, var, inputs)
    assert torch.equal(net._flat.val, fresh._flat.val) and torch.equal(net._flat.val, other._flat.val)
    assert torch.equal(got[1], want[1]), "derivative of %s" % var
    assert torch.equal(got[0], want[0]), "parameter derivatives"


def test_pack_params_after_a_prepared_step(gpu, tmp_path):
    """pack_params on a prepared net gives the parameters new storage and frees the old: the addresses the operands are
    keyed by go to the next tensors of that size -- here the flat buffers of a second net with other values.  Both nets'
    derivatives (nothing prepared for either: wgradStream None) are the bits of a net that never met a prepared operand."""
    import torch
    inputs = _flow_inputs()
    ref_net, var = _student(2)
    want2 = _ders(ref_net, var, inputs)                        # before any operand of these shapes was prepared
    ref_net1, _ = _student(1)
    want1 = _ders(ref_net1, var, inputs)
    net, _ = _student(1)
    net.wgradStream = torch.cuda.Stream()
    _ders(net, var, inputs)
    net.pack_params()
    net.wgradStream = None
    got1 = _ders(net, var, inputs)
    assert torch.equal(got1[1], want1[1]) and torch.equal(got1[0], want1[0])
    second, _ = _student(2)                                    # its flat buffers may sit where the first net's were
    got2 = _ders(second, var, inputs)
    assert torch.equal(got2[1], want2[1]) and torch.equal(got2[0], want2[0])
